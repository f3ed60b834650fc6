"""GPU tests of event-triggered holding among scripted obstacles (mpc_rollout_held, mpc_obstacle_trigger,
mpc_closed_loop_obstacles_event; BatchedMPC.rollout_held / obstacle_trigger / closed_loop_obstacles_event).  The rollout
is compared bit for bit with mpc_rollout on the shifted plan, the rule bit for bit with the numpy restatement of
tests/obstacles_event_common.py, the loop bit for bit with the loops it reduces to and with the host loop of the public
calls it is made of, and -- within the project's bars between two correct solvers -- with the mirror loop on the CPU
checker recorded in tests/golden/obstacles_event_reference.npz (tests/golden/make_obstacles_event_golden.py).  The measured
figures behind STATE_BOUND and CLEAR_MARGIN are in profiles/r22_obstacles_event.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from agent_tables_common import T
from conftest import GOLDEN, synthetic_states

import discs_common as D
import obstacles_common as OC
import obstacles_event_common as OE

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402
from model_predictive_control_amd.tracks import stadium_track  # noqa: E402

DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)   # tests/test_gpu_agent_discs.py
# States of the loop against the recorded mirror loop, 48 steps at TIGHT: measured on an MI355X 3.08e-7, at step 40
# (profiles/r22_obstacles_event.txt); four times that (the solver-path differences between builds), and below the
# cap of 1e-4
STATE_BOUND = 1.24e-6
# min_t traj_clear (d^2 - r^2) of the loop at the handle's default tolerances against the recorded mirror loop's, per car:
# measured on an MI355X, the loop is at most 5.07e-9 lower; four times that (profiles/r22_obstacles_event.txt)
CLEAR_MARGIN = 2.1e-8
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def engine(dev, model, N, mode=mp.CONSTR_DISCS, **kw):
    return mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, **kw), dev)


def arange32(B, dev):
    return torch.arange(B, dtype=torch.int32, device=dev)


def i32(a, dev):
    return T(a, dev, torch.int32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def shifted(U, held, N):
    """the in-place shift of the trigger in torch: stage j <- stage min(j + k, N - 1), k = min(max(held, 0), N - 1)"""
    B = U.shape[0]
    src = torch.clamp(torch.arange(N, device=U.device)[None, :] + torch.clamp(held, min=0, max=N - 1)[:, None].long(), max=N - 1)
    return torch.gather(U.view(B, N, 2), 1, src[:, :, None].expand(B, N, 2)).reshape(B, 2 * N).contiguous()


def tracks(eng, obs_h, dev):
    W = _lib.obstacle_width(eng.cfg)
    return T(_lib.obstacle_tracks(eng.cfg, centres=obs_h[..., :2], radii=obs_h[..., 2]) if W == 3
             else _lib.obstacle_tracks(eng.cfg, sources=obs_h), dev)


# ----------------------------------------------------------------------------- 1. rollout_held
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_rollout_held_is_rollout_of_the_shifted_plan_bit_for_bit(dev, model, N, table):
    """Fails on a library without the entry point.  B = 130: a partial last workgroup.  held cycles through
    -1, 0, 1, N - 2, N - 1, N + 3; held <= 0 is rollout itself."""
    B = 130
    eng = engine(dev, model, N, mode=mp.CONSTR_NONE)
    rng = np.random.default_rng(5 + model)
    x = T(synthetic_states(model, B, seed=3), dev)
    U = T(np.stack([rng.uniform(-1, 1, (B, N)), rng.uniform(-.32, .32, (B, N))], 2).reshape(B, 2 * N), dev)
    held = i32(np.array([-1, 0, 1, N - 2, N - 1, N + 3])[np.arange(B) % 6], dev)
    if table:
        P = 7
        base = _lib.default_params(eng.cfg)
        kw = dict(accel=base[22] * rng.uniform(.75, 1.25, P), friction=base[23] * rng.uniform(.7, 1.3, P)) if model == 0 else {}
        if model == 1:
            veh = np.tile(base[:22], (P, 1))
            veh[:, 7] *= rng.uniform(.9, 1.1, P); veh[:, 8] *= rng.uniform(.9, 1.1, P)
            kw = dict(veh=veh)
        eng.set_agent_params(T(_lib.param_rows(eng.cfg, P, **kw), dev), i32(rng.integers(0, P, B), dev))
    X = eng.rollout_held(x, U, held)
    want = eng.rollout(x, shifted(U, held, N))
    assert X.shape == (B, N, eng.nx) and torch.equal(X, want)
    plain = eng.rollout(x, U)
    low = (held <= 0)
    assert torch.equal(X[low], plain[low]) and not torch.equal(X[~low], plain[~low])
    if table:                                              # the rows matter: without the table the states differ
        eng.clear_agent_params()
        assert not torch.equal(eng.rollout_held(x, U, held), X)
    eng.close()


# ----------------------------------------------------------------------------- 2. the obstacle rule
# (W, N, B, G, K, which): `which` picks the window of obstacles_common.selection_window -- 1 clamps at the script's end,
# 2 and 4 wrap.  N = 33: three chunks of the kernel's 16 stages.  (128, 64, 64): Kp = 64, four passes.
TRIGGER_CASES = [(3, 20, 12, 3, 2, 1), (3, 20, 12, 3, 2, 2), (8, 20, 12, 3, 2, 4), (3, 20, 128, 64, 64, 2),
                 (8, 20, 128, 64, 64, 1), (3, 33, 12, 3, 2, 4), (8, 33, 130, 5, 3, 2)]


@pytest.mark.parametrize("W,N,B,G,K,which", TRIGGER_CASES)
def test_obstacle_trigger_is_the_restatement_bit_for_bit(dev, W, N, B, G, K, which):
    """sel_chk, clear_chk, why and fire against tests/obstacles_event_common.py at every watch.  The case is
    obstacles_common.selection_case: exact ties, absent samples (15 %) and non-finite plan stages inside the windows.
    Held counts put N - k_b at 1, 16, 17 and N (the chunk edge) and anywhere between; held <= 0 never fires a rule."""
    eng = engine(dev, 0, N, mode=mp.CONSTR_DISCS if W == 3 else mp.CONSTR_NONE)
    assert _lib.obstacle_width(eng.cfg) == W
    X, obs, ti, wrap = OC.selection_case(4, W, N, G, K, B, which, seed=2)
    rng = np.random.default_rng(1000 * N + B)
    held = np.array([N - 1, N - 16, N - 17, 0, -1, 1, N + 3] + list(rng.integers(1, N, 5)))[np.arange(B) % 12].astype(np.int32)
    nst = np.array([N - OE.held_start(h, N) for h in held])
    assert {1, 16, 17, N} <= set(nst.tolist())
    sel_plan = rng.integers(-1, K, (B, 2)).astype(np.int32)
    fire_in = (rng.uniform(size=B) < 0.3).astype(np.int32)
    reach = OC.SELECTION_REACH
    sel_w, clear_w, _ = OE.held_selection(X, held, G, obs, ti, reach, wrap)
    _, full_clear, _ = OC.select_obstacles(X, G, obs, ti, reach, wrap)
    assert not np.array_equal(bits(full_clear), bits(clear_w))      # the held window is not the full one
    seen = {}
    Xt, ot, ht, pt = T(X, dev), T(obs, dev), i32(held, dev), i32(sel_plan, dev)
    for clear_thr in (0.5, -0.05):
        for watch in range(4):
            for fin in (None, fire_in):
                why_w = OE.why_bits(held, sel_w, clear_w, sel_plan, clear_thr, watch, fin)
                fire, why, sel, clear = eng.obstacle_trigger(Xt, ht, pt, G, ot, ti, reach, clear_thr, watch,
                                                             fire=None if fin is None else i32(fin, dev), wrap=wrap)
                assert np.array_equal(sel.cpu().numpy(), sel_w), np.argwhere(sel.cpu().numpy() != sel_w)[:5]
                assert np.array_equal(bits(clear.cpu().numpy()), bits(clear_w))
                assert np.array_equal(why.cpu().numpy(), why_w), (watch, np.argwhere(why.cpu().numpy() != why_w)[:5])
                assert np.array_equal(fire.cpu().numpy(), (why_w != 0).astype(np.int32))
                if fin is None:
                    assert not (why_w & (7 ^ (2 * (watch & 1) | 4 * (watch >> 1)))).any() and not why_w[held <= 0].any()
                    seen[watch] = seen.get(watch, 0) | int(np.bitwise_or.reduce(why_w))
    assert seen == {0: 0, 1: 2, 2: 4, 3: 6}, seen                   # both rules fire somewhere, each under its own bit alone
    X_bad = ~np.isfinite(X[:, :, :2]).all(2)
    Lt, key = obs.shape[2], 2 if W == 3 else 4
    absent_inside = sum(obs[b // G, o, OC.sample_index(ti + k, Lt, wrap), key] == 0.0
                        for b in range(B) for o in sel_w[b] if o >= 0 for k in range(nst[b]))
    inside = X_bad & (np.arange(N)[None, :] < nst[:, None])
    print(f"W {W} N {N} B {B}: non-finite stages inside a held window {int(inside.sum())}, behind one {int((X_bad & ~inside).sum())}; "
          f"absent samples inside the held window of a selected track {absent_inside}; slots in use {int((sel_w >= 0).sum())} of {sel_w.size}")
    assert inside.any() and absent_inside > 0
    eng.close()


# ----------------------------------------------------------------------------- the loop's cases
W4 = np.ones(4)


def loop_case(dev, model, N, B, G, K, Lt, seed, tables=False, **cfg):
    mode = mp.CONSTR_DISCS if model == 0 else mp.CONSTR_LANE
    eng = engine(dev, model, N, mode=mode, Sigma0=10.0, max_total_inner=1500, **cfg)
    W = _lib.obstacle_width(eng.cfg)
    X0, v_ref, obs_h = OC.loop_scene(model, B, G, K, Lt, W, seed=seed)
    rates = None
    if tables:
        eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=v_ref), dev), arange32(B, dev))
        rates = T(_lib.rate_rows(np.linspace(0.0, 0.2, B), 0.05), dev)
        eng.set_agent_rates(rates, arange32(B, dev))
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    return eng, T(X0, dev), T(D.line_centerline(), dev), U0, tracks(eng, obs_h, dev), obs_h, rates


# ----------------------------------------------------------------------------- 3. reductions
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_threshold_zero_is_closed_loop_obstacles_bit_for_bit(dev, model, N):
    """thr = 0 fires everybody at every step: rollout_held at held = 1 is the rollout of the shifted plan, the masked gather
    writes every row.  U returns as last solved where closed_loop_obstacles returns it shifted."""
    B, G, K, Tn = 12, 3, 2, 5
    eng, x0, cl, U0, obs, _, _ = loop_case(dev, model, N, B, G, K, Tn + N - 3, seed=11 + model)
    want = eng.closed_loop_obstacles(x0, cl, U0, Tn, G, obs, 0.6, shift=True)
    wtable = want.table.clone()
    want.table.fill_(3.0)
    res = eng.closed_loop_obstacles_event(x0, cl, U0, Tn, G, obs, np.ones(eng.nx), 0.0, 3, reach=0.6, clear_thr=-1e-3, watch=3,
                                          shift=True, table=want.table)
    for name in ("x", "lam", "traj_x", "traj_u", "failures", "stats", "traj_sel", "traj_clear"):
        a, b = getattr(res, name), getattr(want, name)
        assert (a is None and b is None) or torch.equal(a, b), name
    assert torch.equal(shifted(res.U, res.held, N), want.U) and torch.equal(res.table, wtable)
    assert bool((res.solved == 1).all()) and bool((res.solve_count == Tn).all()) and bool((res.held == 1).all())
    assert bool((res.traj_why & 1).all()) and torch.equal(res.sel_plan, res.traj_sel[:, -1])
    assert bool((res.traj_sel >= 0).any())
    eng.close()


@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_all_samples_absent_is_closed_loop_event_on_a_zero_table(dev, model, N):
    B, G, K, Tn = 12, 3, 2, 9
    eng, x0, cl, U0, _, obs_h, _ = loop_case(dev, model, N, B, G, K, 9, seed=3)
    W = obs_h.shape[3]
    obs_h[..., 2 if W == 3 else 4] = 0.0                       # everything else stays: junk behind the zero
    table = torch.zeros(B, 2 * W * N, dtype=torch.float64, device=dev)
    (eng.set_agent_discs if W == 3 else eng.set_agent_fields)(table, arange32(B, dev))
    rng = np.random.default_rng(4)
    dist = T(rng.normal(0, 0.004, (B, Tn, eng.nx)) * (rng.uniform(size=(B, Tn, 1)) < 0.3), dev)
    w = np.ones(eng.nx)
    want = eng.closed_loop_event(x0, cl, U0, Tn, w, 0.01, 4, shift=True, disturbance=dist)
    res = eng.closed_loop_obstacles_event(x0, cl, U0, Tn, G, T(obs_h, dev), w, 0.01, 4, clear_thr=0.3, watch=3, shift=True,
                                          table=table, disturbance=dist)
    for name in mp.solver.EventLoopResult._fields:
        a, b = getattr(res, name), getattr(want, name)
        assert (a is None and b is None) or torch.equal(a, b), name
    assert not bool((res.traj_why & 6).any()) and torch.equal(res.traj_why, res.solved)
    assert 0 < int(res.solved.sum()) < B * Tn                   # some agents held, some fired by deviation or the hold limit
    assert bool((res.traj_sel == -1).all()) and bool(torch.isposinf(res.traj_clear).all()) and not bool(table.any())
    eng.close()


def test_watch_zero_fires_by_deviation_and_hold_alone(dev):
    B, G, K, Tn, N = 12, 3, 2, 8, 20
    eng, x0, cl, U0, obs, _, _ = loop_case(dev, 0, N, B, G, K, Tn + N, seed=11)
    res = eng.closed_loop_obstacles_event(x0, cl, U0, Tn, G, obs, W4, INF, 4, reach=0.6, clear_thr=0.3, watch=0, shift=True)
    want = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    want[:, ::4] = 1
    assert torch.equal(res.traj_why, want) and torch.equal(res.solved, want)
    both = eng.closed_loop_obstacles_event(x0, cl, U0, Tn, G, obs, W4, INF, 4, reach=0.6, clear_thr=0.3, watch=3, shift=True,
                                           table=res.table)
    assert bool((both.traj_why & 6).any())                      # the same scene with the rules on: they do fire
    eng.close()


# ----------------------------------------------------------------------------- 4. the loop is the host loop
def host_loop(eng, x, cl, U, Tn, G, obs, w, thr, max_hold, reach, clear_thr, watch, shift, table, t0=0, wrap=False, dist=None,
              rates=None, trk=None, ci=None):
    """the loop written with the public calls, one by one; plan shift, the copy of the firing agents' rows into the bound
    table and the sel_plan update in torch"""
    B, N, dev = x.shape[0], eng.N, x.device
    x, U = x.clone(), U.clone()
    gather = eng.discs_from_obstacles if _lib.obstacle_width(eng.cfg) == 3 else eng.fields_from_obstacles
    lam = torch.zeros(B, eng.m, dtype=torch.float64, device=dev) if eng.m else None
    held = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sel_plan = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    xhat = torch.zeros_like(x)
    stats = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    tx, tu = torch.zeros(B, Tn, eng.nx, dtype=torch.float64, device=dev), torch.zeros(B, Tn, 2, dtype=torch.float64, device=dev)
    tsel = torch.zeros(B, Tn, 2, dtype=torch.int32, device=dev)
    tclear = torch.zeros(B, Tn, dtype=torch.float64, device=dev)
    twhy = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    solved = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    fails = torch.zeros(B, dtype=torch.int32, device=dev)
    ar = torch.arange(B, device=dev)
    for t in range(Tn):
        ti = t0 + t + 1
        _, fire_dev = eng.trigger_eval(x, xhat, held, w, thr, max_hold)
        X = eng.rollout_held(x, U, held)
        fire, why, _, _ = eng.obstacle_trigger(X, held, sel_plan, G, obs, ti, reach, clear_thr, watch, fire=fire_dev, wrap=wrap)
        fb = fire != 0
        if shift:
            U = torch.where(fb[:, None], shifted(U, held, N), U)
        if trk is not None:
            ci, _ = eng.track_select(x, trk, ci, active=fire)
        sel, _ = eng.obstacles_select(X, G, obs, ti, reach, wrap)
        rows = gather(sel, G, obs, ti, wrap)
        table[fb] = rows[fb]
        sel_plan = torch.where(fb[:, None], sel, sel_plan)
        U, lam, stats, n = eng.solve_active(x, cl, U, fire, lam=lam, cl_index=ci, stats=stats)
        assert n == int(fb.sum())
        fails += (fb & (stats[:, 0] != 1)).to(torch.int32)
        held = torch.where(fb, torch.zeros_like(held), held)
        xhat = torch.where(fb[:, None], x, xhat)
        u = U.view(B, N, 2)[ar, held.long()].contiguous()
        if rates is not None:
            rates[:, 2:4] = u
        xn = eng.rollout(x, u)[:, 0]
        x = ((xn + dist[:, t]) if dist is not None else xn).contiguous()
        xhat = eng.rollout(xhat, u)[:, 0].contiguous()
        held = held + 1
        tx[:, t], tu[:, t], tsel[:, t], twhy[:, t], solved[:, t] = x, u, sel, why, fb.to(torch.uint8)
        count += fb.to(torch.int32)
        tclear[:, t] = eng.obstacles_select(x, G, obs, ti, INF, wrap)[1][:, 0]
    return mp.ObstacleEventLoopResult(x, U, lam, tx, tu, fails, stats, tsel, tclear, table, ci, solved, count, held, sel_plan, twhy)


def same(got, want):
    for name, a, b in zip(mp.ObstacleEventLoopResult._fields, got, want):
        assert (a is None and b is None) or torch.equal(a, b), name


@pytest.mark.parametrize("model,N,tables", [(0, 20, False), (0, 20, True), (1, 12, False)])
def test_the_loop_is_the_host_loop_bit_for_bit(dev, model, N, tables):
    """T = 6, B = 12, a disturbance that makes some agents fire by deviation; tables: a parameter and a rate table bound.
    And two calls of 3 steps, the second with t0 = 3 and what the first returned, are one call of 6."""
    B, G, K, Tn = 12, 3, 3, 6
    eng, x0, cl, U0, obs, _, rates = loop_case(dev, model, N, B, G, K, Tn + N - 3, seed=11 + model, tables=tables)
    first = None if rates is None else rates.clone()
    x0_in = x0.clone()
    rng = np.random.default_rng(7)
    dist = T(rng.normal(0, 0.01, (B, Tn, eng.nx)) * (rng.uniform(size=(B, Tn, 1)) < 0.25), dev)
    w = np.ones(eng.nx)
    args = dict(reach=0.6, clear_thr=-1e-3 if model == 0 else 0.02, watch=3, shift=True)
    res = eng.closed_loop_obstacles_event(x0, cl, U0, Tn, G, obs, w, 0.02, 5, disturbance=dist, **args)
    got = [None if t is None else t.clone() for t in res]
    if tables:
        assert torch.equal(rates[:, 2:], res.traj_u[:, -1])
        rates.copy_(first)
    res.table.zero_()                                             # (a held agent's row is never written: both start from zeros)
    want = host_loop(eng, x0, cl, U0, Tn, G, obs, w, 0.02, 5, args["reach"], args["clear_thr"], 3, True, res.table, dist=dist,
                     rates=rates)
    same(got, want)
    why = got[15]
    print(f"model {model}: solves {int(got[11].sum())} of {B * Tn}; why bits seen: car {int((why & 1).bool().sum())}, clearance "
          f"{int((why & 2).bool().sum())}, new obstacle {int((why & 4).bool().sum())}; failures {int(got[5].sum())}")
    assert 0 < int(got[11].sum()) < B * Tn and bool((why[:, 1:] & 1).any()) and bool((why & 6).any())
    assert torch.equal(x0, x0_in) and not bool(U0.any())          # the arguments are not written
    # two calls of 3 steps
    if tables:
        rates.copy_(first)
    res.table.zero_()
    a = eng.closed_loop_obstacles_event(x0, cl, U0, 3, G, obs, w, 0.02, 5, disturbance=dist[:, :3].contiguous(), table=res.table, **args)
    b = eng.closed_loop_obstacles_event(a.x, cl, a.U, 3, G, obs, w, 0.02, 5, disturbance=dist[:, 3:].contiguous(), table=res.table,
                                        t0=3, held=a.held, sel_plan=a.sel_plan, lam=a.lam, stats=a.stats, **args)
    F = mp.ObstacleEventLoopResult._fields
    for name in ("x", "U", "lam", "stats", "table", "held", "sel_plan"):
        i = F.index(name)
        assert (b[i] is None and got[i] is None) or torch.equal(b[i], got[i]), name
    for name in ("traj_x", "traj_u", "traj_sel", "traj_clear", "solved", "traj_why"):
        i = F.index(name)
        assert torch.equal(torch.cat([a[i], b[i]], 1), got[i]), name
    assert torch.equal(a.failures + b.failures, got[5]) and torch.equal(a.solve_count + b.solve_count, got[12])
    eng.close()


def test_the_loop_on_a_track_is_the_host_loop_with_track_select_of_the_firing_agents(dev):
    """lap driving on a small stadium among one periodic obstacle per scene; the firing agents alone re-select their window"""
    N, B, G, Tn = 20, 12, 4, 6
    eng = engine(dev, 0, N, Sigma0=10.0, max_total_inner=300)
    track = stadium_track(10, 3, 0.1)
    trk = eng.track_windows(T(track, dev), 4, 10, True)
    L = track.size // 2
    rng = np.random.default_rng(31)
    at = rng.integers(0, L, B)
    tx, ty = track[(at + 1) % L] - track[at], track[L + (at + 1) % L] - track[L + at]
    X0 = np.stack([track[at], track[L + at] + rng.uniform(-.05, .05, B), np.arctan2(ty, tx), rng.uniform(.6, 1.0, B)], 1)
    Lt = L // 8
    obs_h = np.zeros((B // G, 1, Lt, 3))
    for s in range(B // G):
        i = (at[s * G] + 4 + 8 * np.arange(Lt)) % L
        obs_h[s, 0, :, 0], obs_h[s, 0, :, 1], obs_h[s, 0, :, 2] = track[i], track[L + i] + 0.03, 0.12
    obs = tracks(eng, obs_h, dev)
    x0 = T(X0, dev)
    U0 = T(np.tile([1., 0.], (B, N)), dev)
    ci0 = eng.track_locate(x0, trk)
    t0 = Lt - 2                                                   # the windows wrap around the script's end
    dist = T(rng.normal(0, 0.01, (B, Tn, 4)) * (rng.uniform(size=(B, Tn, 1)) < 0.25), dev)
    res = eng.closed_loop_obstacles_event(x0, None, U0, Tn, G, obs, W4, 0.02, 5, reach=0.8, clear_thr=-1e-3, watch=3, t0=t0,
                                          wrap=True, cl_index=ci0, shift=True, track_obj=trk, disturbance=dist)
    got = [t.clone() for t in res]
    res.table.zero_()
    want = host_loop(eng, x0, trk.win, U0, Tn, G, obs, W4, 0.02, 5, 0.8, -1e-3, 3, True, res.table, t0=t0, wrap=True, dist=dist,
                     trk=trk, ci=ci0)
    same(got, want)
    assert 0 < int(got[11].sum()) < B * Tn and bool((got[7] >= 0).any())
    assert torch.equal(ci0, eng.track_locate(x0, trk))            # the argument is not written
    eng.close()


# ----------------------------------------------------------------------------- 5. the mirror loop
@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "obstacles_event_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    return ref


def script_loop(dev, ref, watch, Tn, **cfg):
    B = ref["X0"].shape[0]
    eng = engine(dev, 0, OE.SCRIPT_N, **cfg)
    eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=ref["v_ref"]), dev), arange32(B, dev))
    res = eng.closed_loop_obstacles_event(T(ref["X0"], dev), T(D.line_centerline(), dev), T(ref["U0"], dev), Tn, 1, T(ref["obs"], dev),
                                          OE.SCRIPT_W, OE.SCRIPT_THR, OE.SCRIPT_MAX_HOLD, reach=OE.SCRIPT_REACH,
                                          clear_thr=OE.SCRIPT_CLEAR_THR, watch=watch, shift=True)
    eng.close()
    return res


def test_mirror_loop(dev):
    """48 steps of the 16 recorded scenes at discs_common's tight tolerances against the mirror loop on the CPU checker: the
    same solves, reasons and selection step for step, the first controls within DU_METRIC, the states within STATE_BOUND.
    Fails for a loop that watches the car alone: the recording re-plans at step 1 for the obstacle's sake."""
    ref = reference()
    Tn = OE.SCRIPT_T
    res = script_loop(dev, ref, 3, Tn, **TIGHT)
    u, uref = res.traj_u.cpu().numpy(), ref["traj_u"]
    du0 = np.abs(u[:, 0] - uref[:, 0]).max(1) / np.maximum(1.0, np.abs(uref[:, 0]).max(1))
    dx = np.abs(res.traj_x.cpu().numpy() - ref["traj_x"])
    print(f"mirror loop: failures {int(res.failures.sum())}; du(step 0) {du0.max():.3e}; dx max {dx.max():.3e} at step "
          f"{int(dx.max((0, 2)).argmax())}; solves per car {res.solve_count.tolist()}")
    assert int(res.failures.sum()) == 0
    assert np.array_equal(res.solved.cpu().numpy(), ref["solved"])
    assert np.array_equal(res.traj_why.cpu().numpy(), ref["traj_why"])
    assert np.array_equal(res.traj_sel.cpu().numpy(), ref["traj_sel"])
    assert (ref["traj_why"][:, 1] & 6).all()
    assert du0.max() <= DU_METRIC
    assert STATE_BOUND <= 1e-4 and dx.max() <= STATE_BOUND


# ----------------------------------------------------------------------------- 6. end to end
def test_the_held_plan_and_the_new_obstacle_end_to_end(dev):
    """The recorded scenes at the handle's default tolerances.  The loop that watches the car alone (watch = 0) holds the
    plan of step 0 through the sample at which the second obstacle appears and drives through it: deeper than half r^2
    inside.  With the rules on it re-plans at the recorded step, its smallest realised clearance is no lower than the
    recorded mirror loop's minus CLEAR_MARGIN, and it still holds elsewhere."""
    ref = reference()
    r2 = OE.SCRIPT_NEW[2] ** 2
    blind = script_loop(dev, ref, 0, OE.SCRIPT_T_BLIND)
    res = script_loop(dev, ref, 3, OE.SCRIPT_T)
    cb, clear = blind.traj_clear.cpu().numpy(), res.traj_clear.cpu().numpy()
    diff = ref["traj_clear"].min(1) - clear.min(1)
    print(f"end to end: watch 0 min clear per car max {cb.min(1).max():.6f} (-0.5 r^2 = {-0.5 * r2:.6f}; recorded "
          f"{ref['blind_traj_clear'].min(1).max():.6f}); watch 3 min clear {clear.min():.3e}, mirror {ref['traj_clear'].min():.3e}; "
          f"mirror - loop per car: max {diff.max():.3e} min {diff.min():.3e}; solves per car {res.solve_count.tolist()}; failures "
          f"{int(res.failures.sum())}")
    assert (ref["blind_traj_clear"].min(1) < -0.5 * r2).all()
    assert (cb.min(1) < -0.5 * r2).all() and not bool((blind.traj_why & 6).any()) and bool((blind.solve_count == 1).all())
    assert np.array_equal(res.solved.cpu().numpy(), ref["solved"]) and bool((res.traj_why[:, 1] & 6).bool().all())
    assert (clear.min(1) >= ref["traj_clear"].min(1) - CLEAR_MARGIN).all()
    assert bool((res.solve_count < OE.SCRIPT_T).all())


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals(dev):
    """each MPC_E_ARG (-1) in the library's words, nothing launched: the outputs keep their sentinel"""
    N, B, G, K, Lt = 20, 12, 3, 2, 30
    X0, _, obs_h = OC.loop_scene(0, B, G, K, Lt, 3, seed=2)
    x0, cl, obs = T(X0, dev), T(D.line_centerline(), dev), T(obs_h, dev)
    fobs = torch.zeros(B // G, K, Lt, 8, dtype=torch.float64, device=dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    lam = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
    ftable = torch.zeros(B, 16 * N, dtype=torch.float64, device=dev)
    held = torch.full((B,), 2, dtype=torch.int32, device=dev)
    plan = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
    X = torch.ones(B, N, 4, dtype=torch.float64, device=dev)
    sel = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
    clear = torch.full((B, 2), 77.0, dtype=torch.float64, device=dev)
    why = torch.full((B,), 77, dtype=torch.uint8, device=dev)
    fire = torch.full((B,), 77, dtype=torch.int32, device=dev)
    tsel = torch.full((B, 1, 2), 77, dtype=torch.int32, device=dev)
    twhy = torch.full((B, 1), 77, dtype=torch.uint8, device=dev)
    Xout = torch.full((B, N, 4), 77.0, dtype=torch.float64, device=dev)
    wv = (C.c_double * 4)(1, 1, 1, 1)
    big = 2 ** 31 - 1

    def loop(eng, B=B, Tn=1, G=G, K=K, Lt=Lt, t0=0, obs=obs, reach=1.0, clear_thr=0.0, watch=3, max_hold=4, table=table,
             plan=plan, held=held, thr=0.1):
        return eng.lib.mpc_closed_loop_obstacles_event(
            eng._h, B, Tn, 1, wv, thr, max_hold, G, K, Lt, 0, t0, p(obs), float(reach), float(clear_thr), watch, p(x0), p(cl), None,
            p(U0), p(lam), p(held), p(plan), p(table), None, None, None, p(tsel), None, p(twhy), None, None, None, None, eng._stream(),
            None)

    def trig(eng, B=B, G=G, K=K, Lt=Lt, ti=0, X=X, obs=obs, reach=1.0, clear_thr=0.0, watch=3, held=held, plan=plan, sel=sel,
             fire=fire):
        return eng.lib.mpc_obstacle_trigger(eng._h, B, G, K, Lt, 0, ti, p(X), p(obs), float(reach), p(held), p(plan), float(clear_thr),
                                            watch, None, p(sel), p(clear), p(why), p(fire), eng._stream())

    def held_roll(eng, B=B, x=x0, U=U0, held=held, X=Xout):
        return eng.lib.mpc_rollout_held(eng._h, B, p(x), p(U), p(held), p(X), eng._stream())

    def refused(rc, who, words):
        msg = _lib.load().mpc_last_error().decode()
        assert rc == -1 and msg.startswith(who + ": ") and words in msg, (rc, msg)

    def untouched():
        torch.cuda.synchronize()
        assert bool((sel == 77).all()) and bool((clear == 77.0).all()) and bool((why == 77).all()) and bool((fire == 77).all())
        assert bool((tsel == 77).all()) and bool((twhy == 77).all()) and bool((plan == 77).all()) and bool((Xout == 77.0).all())
        assert bool((held == 2).all()) and not bool(table.any()) and not bool(ftable.any()) and not bool(U0.any())
    LOOP, TRIG, ROLL = "mpc_closed_loop_obstacles_event", "mpc_obstacle_trigger", "mpc_rollout_held"
    # a disc table on a field handle, a field table on a disc handle
    other = engine(dev, 0, N, mode=mp.CONSTR_LANE, max_total_inner=300)
    other.set_agent_fields(ftable, arange32(B, dev))
    refused(loop(other, obs=fobs, table=table), LOOP, "must be the field table that is bound (mpc_set_agent_fields)")
    other.close()
    eng = engine(dev, 0, N, max_total_inner=300)
    refused(loop(eng), LOOP, "no disc table is bound (mpc_set_agent_discs)")
    half = torch.zeros(B // 2, 6 * N, dtype=torch.float64, device=dev)
    eng.set_agent_discs(half, T(np.arange(B) // 2, dev, torch.int32))
    refused(loop(eng, table=half), LOOP, "has 6 rows, the loop needs one per agent")
    eng.set_agent_discs(table, arange32(B, dev))
    refused(loop(eng, table=ftable), LOOP, "must be the disc table that is bound")
    refused(loop(eng, table=table.clone()), LOOP, "must be the disc table that is bound")
    refused(loop(eng, table=None), LOOP, "must be the disc table that is bound")
    for fn, who in ((loop, LOOP), (trig, TRIG)):
        refused(fn(eng, clear_thr=1.0 + 1e-9), who, "clear_thr must be a number <= reach^2")
        refused(fn(eng, clear_thr=float("nan")), who, "clear_thr must be a number <= reach^2")
        refused(fn(eng, watch=4), who, "watch must be in [0, 3]")
        refused(fn(eng, watch=-1), who, "watch must be in [0, 3]")
        refused(fn(eng, plan=None), who, "null")
        refused(fn(eng, held=None), who, "null")
        for r in (-0.5, float("nan")):
            refused(fn(eng, reach=r), who, "reach must be >= 0")
        for kw, words in ((dict(G=5), "B % G"), (dict(G=0), "scene size G"), (dict(K=65), "obstacles K"), (dict(Lt=0), "Lt must be >= 1"),
                          (dict(obs=None), "null obs"), (dict(B=6, G=3), "the bound disc table is for a batch of 12 agents, this call has 6")):
            refused(fn(eng, **kw), who, words)
    refused(loop(eng, max_hold=N + 1), LOOP, "max_hold must be in [1, N]")
    refused(loop(eng, max_hold=0), LOOP, "max_hold must be in [1, N]")
    refused(loop(eng, thr=-1.0), LOOP, "thr must be >= 0")
    refused(loop(eng, Tn=-1), LOOP, "negative T")
    refused(loop(eng, t0=-1), LOOP, "t0 must be >= 0")
    refused(loop(eng, t0=big - N, Tn=1), LOOP, "does not fit an int32")      # the window of the last step, no wrap
    refused(trig(eng, ti=big - N + 1), TRIG, "does not fit an int32")
    refused(trig(eng, X=None), TRIG, "null X")
    refused(trig(eng, sel=None), TRIG, "null X")
    refused(trig(eng, fire=None), TRIG, "null X")
    refused(held_roll(eng, held=None), ROLL, "null buffer")
    refused(held_roll(eng, X=None), ROLL, "null buffer")
    six = engine(dev, 0, N, mode=mp.CONSTR_NONE)
    six.set_agent_params(T(_lib.param_rows(six.cfg, 6), dev), arange32(6, dev))
    refused(held_roll(six), ROLL, "the bound parameter table is for a batch of 6 agents, this call has 12")
    six.close()
    # a rate table with P != B
    eng.set_agent_rates(T(_lib.rate_rows(0.1, 0.1), dev), torch.zeros(B, dtype=torch.int32, device=dev))
    refused(loop(eng), LOOP, "the bound rate table has 1 rows")
    eng.clear_agent_rates()
    untouched()
    # the front end
    for kw in (dict(max_hold=N + 1), dict(thr=-1.0), dict(G=5), dict(reach=-1.0), dict(t0=-1), dict(obs=obs[:3].contiguous())):
        with pytest.raises(ValueError):
            eng.closed_loop_obstacles_event(x0, cl, U0, 1, **{**dict(G=G, obs=obs, w=W4, thr=0.1, max_hold=4, reach=1.0, table=table), **kw})
    with pytest.raises(mp.MpcError, match="clear_thr must be a number <= reach"):
        eng.closed_loop_obstacles_event(x0, cl, U0, 1, G, obs, W4, 0.1, 4, reach=1.0, clear_thr=2.0, table=table)
    with pytest.raises(mp.MpcError, match="watch must be in"):
        eng.obstacle_trigger(X, held, torch.zeros_like(plan), G, obs, 0, 1.0, 0.0, 4)
    with pytest.raises((ValueError, TypeError)):
        eng.rollout_held(x0, U0, held.long())
    # while solve_async is in flight
    wait = eng.solve_async(x0, cl, U0)
    refused(loop(eng), LOOP, "a solve of this handle is in flight")
    refused(trig(eng), TRIG, "a solve of this handle is in flight")
    refused(held_roll(eng), ROLL, "a solve of this handle is in flight")
    wait()
    untouched()
    assert held_roll(eng) == 0 and trig(eng) == 0 and loop(eng) == 0          # ... and afterwards all are served
    torch.cuda.synchronize()
    assert not bool((Xout == 77.0).any()) and not bool((fire == 77).any()) and bool((twhy != 77).all())
    eng.close()
