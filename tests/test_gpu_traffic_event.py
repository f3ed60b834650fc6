"""GPU tests of event-triggered holding in traffic (mpc_opponent_trigger, mpc_closed_loop_traffic_event;
BatchedMPC.opponent_trigger / closed_loop_traffic_event).  The rule is compared bit for bit with the numpy restatement of
tests/traffic_event_common.py, the loop bit for bit with the loops it reduces to and with the host loop of the public calls
it is made of, and -- within the project's bars between two correct solvers -- with the mirror loop on the CPU checker
recorded in tests/golden/traffic_event_reference.npz (tests/golden/make_traffic_event_golden.py).  The measured figures
behind STATE_BOUND and CLEAR_MARGIN are in profiles/r23_traffic_event.txt.  Every test fails on a library without the two
entry points."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from agent_tables_common import T
from conftest import GOLDEN

import discs_common as D
import traffic_common as TC
import traffic_event_common as TE

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402

DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)   # tests/test_gpu_agent_discs.py
# States of the loop against the recorded mirror loop, 24 steps at TIGHT: measured on an MI355X 1.825e-7, at step 7
# (profiles/r23_traffic_event.txt); four times that (the solver-path differences between builds), and below the
# cap of 1e-4
STATE_BOUND = 7.3e-7
# min_t traj_clear (d^2 - r^2) of the loop at the handle's default tolerances against the recorded mirror loop's, per car:
# measured on an MI355X, the loop is at most 7.058e-7 lower (and at most 7.63e-7 higher, which the assertion does not bound);
# four times the former (profiles/r23_traffic_event.txt)
CLEAR_MARGIN = 2.83e-6
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


# ----------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("N", [20, 40])
def test_opponent_trigger_is_the_restatement_bit_for_bit(dev, N):
    """opp_chk, clear_chk, why and fire against tests/traffic_event_common.py at every watch, two thresholds, with and
    without the caller's fire.  The cases are traffic_common.selection_case at SELECTION_SHAPES: exact ties, non-finite
    positions, scenes that straddle waves and workgroups; N = 40 takes two LDS chunks of 32 stages.  Held counts put
    n_b = N - k_b at 1, N and anywhere between (N = 40: 32 and 33, the chunk edge) and include held = 0, -1 and N + 3;
    held <= 0 never fires a rule."""
    eng = engine(dev, 0, N)
    reach = TC.SELECTION_REACH
    seen, differs, inside_n, behind_n = {}, 0, 0, 0
    for G, B in TC.SELECTION_SHAPES:
        X, radius = TC.selection_case(4, N, G, B, seed=2)
        rng = np.random.default_rng(1000 * N + B)
        edge = [N - n for n in (1, 32, 33, N) if 1 <= n <= N]
        held = np.array(edge + [0, -1, 1, N + 3] + list(rng.integers(1, N, 5)))[np.arange(B) % (len(edge) + 9)].astype(np.int32)
        nst = np.array([N - TE.held_start(h, N) for h in held])
        assert {n for n in (1, 32, 33, N) if n <= N} <= set(nst.tolist()) and {0, -1, N + 3} <= set(held.tolist())
        opp_plan = np.where(rng.uniform(size=(B, 2)) < 0.3, -1, (np.arange(B)[:, None] // G) * G + rng.integers(0, G, (B, 2))).astype(np.int32)
        fire_in = (rng.uniform(size=B) < 0.3).astype(np.int32)
        opp_w, clear_w, _ = TE.held_selection(X, held, G, radius, reach, want_margin=False)
        _, full_clear, _ = TE.held_selection(X, np.zeros(B, dtype=np.int32), G, radius, reach, want_margin=False)
        differs += not np.array_equal(bits(full_clear), bits(clear_w))
        Xt, rt, ht, pt = T(X, dev), T(radius, dev), i32(held, dev), i32(opp_plan, dev)
        full_opp, full_c = eng.opponents_from_plans(Xt, G, rt, reach)
        assert np.array_equal(bits(full_c.cpu().numpy()), bits(full_clear))       # held <= 0 everywhere is the plain selection
        for clear_thr in (0.5, -0.05):
            for watch in range(4):
                for fin in (None, fire_in):
                    why_w = TE.why_bits(held, opp_w, clear_w, opp_plan, clear_thr, watch, fin)
                    fire, why, opp, clear = eng.opponent_trigger(Xt, ht, pt, G, rt, reach, clear_thr, watch,
                                                                 fire=None if fin is None else i32(fin, dev))
                    assert np.array_equal(opp.cpu().numpy(), opp_w), (G, B, np.argwhere(opp.cpu().numpy() != opp_w)[:5])
                    assert np.array_equal(bits(clear.cpu().numpy()), bits(clear_w)), (G, B)
                    assert np.array_equal(why.cpu().numpy(), why_w), (G, B, watch, np.argwhere(why.cpu().numpy() != why_w)[:5])
                    assert np.array_equal(fire.cpu().numpy(), (why_w != 0).astype(np.int32))
                    if fin is None:
                        assert not (why_w & (7 ^ (2 * (watch & 1) | 4 * (watch >> 1)))).any() and not why_w[held <= 0].any()
                        seen[watch] = seen.get(watch, 0) | int(np.bitwise_or.reduce(why_w))
        on = opp_w >= 0
        assert (opp_w[on] // G == np.broadcast_to(np.arange(B)[:, None] // G, opp_w.shape)[on]).all()   # global indices, own scene
        X_bad = ~np.isfinite(X[:, :, :2]).all(2)
        inside = X_bad & (np.arange(N)[None, :] < nst[:, None])
        inside_n, behind_n = inside_n + int(inside.sum()), behind_n + int((X_bad & ~inside).sum())
    print(f"N {N}: shapes whose held selection differs from the full one {differs} of {len(TC.SELECTION_SHAPES)}; non-finite "
          f"stages inside a held window {inside_n}, behind one {behind_n}; why bits seen per watch {seen}")
    assert differs >= 3                                             # the held window is not the full one
    assert seen == {0: 0, 1: 2, 2: 4, 3: 6}, seen                   # both rules fire somewhere, each under its own bit alone
    assert inside_n > 0 and behind_n > 0
    eng.close()


# ----------------------------------------------------------------------------- the loop's cases
def loop_case(dev, model, N, B, G, seed, tables=False, **cfg):
    """(engine, x0, centerline, U0, radius, shape or None, rate table or None): kinematic on discs, Pacejka on a LANE handle
    with risk fields"""
    mode = mp.CONSTR_DISCS if model == 0 else mp.CONSTR_LANE
    eng = engine(dev, model, N, mode=mode, **{**dict(Sigma0=10.0, max_total_inner=1500), **cfg})
    X0, v_ref, radius, shape = TE.loop_scene(model, B, G, seed)
    rates = None
    if tables:
        eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=v_ref), dev), arange32(B, dev))
        rates = T(_lib.rate_rows(np.linspace(0.0, 0.2, B), 0.05), dev)
        eng.set_agent_rates(rates, arange32(B, dev))
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    return eng, T(X0, dev), T(D.line_centerline(), dev), U0, T(radius, dev), (None if model == 0 else T(shape, dev)), rates


def plain_traffic(eng, x0, cl, U0, Tn, G, radius, shape, reach, **kw):
    if shape is None:
        return eng.closed_loop_traffic(x0, cl, U0, Tn, G, radius, reach, **kw)
    return eng.closed_loop_traffic_field(x0, cl, U0, Tn, G, radius, shape, reach, **kw)


# ----------------------------------------------------------------------------- 2. reductions
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_threshold_zero_is_the_traffic_loop_bit_for_bit(dev, model, N):
    """thr = 0 fires everybody at every step: rollout_held at held = 1 is the rollout of the shifted plan, the masked gather
    writes every row.  U returns as last solved where the traffic loop returns it shifted."""
    B, G, Tn = 12, 3, 5
    eng, x0, cl, U0, radius, shape, _ = loop_case(dev, model, N, B, G, seed=11 + model)
    want = plain_traffic(eng, x0, cl, U0, Tn, G, radius, shape, 0.6, shift=True)
    wtable = want.table.clone()
    want.table.fill_(3.0)
    res = eng.closed_loop_traffic_event(x0, cl, U0, Tn, G, radius, np.ones(eng.nx), 0.0, 3, shape=shape, reach=0.6, clear_thr=-1e-3,
                                        watch=3, shift=True, table=want.table)
    for name in ("x", "lam", "traj_x", "traj_u", "failures", "stats", "traj_opp", "traj_clear"):
        a, b = getattr(res, name), getattr(want, name)
        assert (a is None and b is None) or torch.equal(a, b), name
    assert torch.equal(shifted(res.U, res.held, N), want.U) and torch.equal(res.table, wtable)
    assert bool((res.solved == 1).all()) and bool((res.solve_count == Tn).all()) and bool((res.held == 1).all())
    assert bool((res.traj_why & 1).all()) and torch.equal(res.opp_plan, res.traj_opp[:, -1])
    assert bool((res.traj_opp >= 0).any()) and bool(wtable.any())
    eng.close()


@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_scenes_of_one_are_closed_loop_event_on_a_zero_table(dev, model, N):
    B, Tn = 12, 9
    eng, x0, cl, U0, radius, shape, _ = loop_case(dev, model, N, B, 3, seed=3)
    W = 3 if model == 0 else 8
    table = torch.zeros(B, 2 * W * N, dtype=torch.float64, device=dev)
    (eng.set_agent_discs if W == 3 else eng.set_agent_fields)(table, arange32(B, dev))
    rng = np.random.default_rng(4)
    dist = T(rng.normal(0, 0.004, (B, Tn, eng.nx)) * (rng.uniform(size=(B, Tn, 1)) < 0.3), dev)
    w = np.ones(eng.nx)
    want = eng.closed_loop_event(x0, cl, U0, Tn, w, 0.01, 4, shift=True, disturbance=dist)
    res = eng.closed_loop_traffic_event(x0, cl, U0, Tn, 1, radius, w, 0.01, 4, shape=shape, clear_thr=0.3, watch=3, shift=True,
                                        table=table, disturbance=dist)
    for name in mp.solver.EventLoopResult._fields:
        a, b = getattr(res, name), getattr(want, name)
        assert (a is None and b is None) or torch.equal(a, b), name
    assert not bool((res.traj_why & 6).any()) and torch.equal(res.traj_why, res.solved)
    assert 0 < int(res.solved.sum()) < B * Tn                   # some agents held, some fired by deviation or the hold limit
    assert bool((res.traj_opp == -1).all()) and bool(torch.isposinf(res.traj_clear).all()) and not bool(table.any())
    assert bool((res.opp_plan == -1).all())
    eng.close()


def test_watch_zero_fires_by_deviation_and_hold_alone(dev):
    B, G, Tn, N = 12, 3, 8, 20
    eng, x0, cl, U0, radius, _, _ = loop_case(dev, 0, N, B, G, seed=11)
    res = eng.closed_loop_traffic_event(x0, cl, U0, Tn, G, radius, np.ones(4), INF, 4, reach=0.6, clear_thr=0.3, watch=0, shift=True)
    want = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    want[:, ::4] = 1
    assert torch.equal(res.traj_why, want) and torch.equal(res.solved, want)
    both = eng.closed_loop_traffic_event(x0, cl, U0, Tn, G, radius, np.ones(4), INF, 4, reach=0.6, clear_thr=0.3, watch=3, shift=True,
                                         table=res.table)
    assert bool((both.traj_why & 6).any())                      # the same scene with the rules on: they do fire
    eng.close()


# ----------------------------------------------------------------------------- 3. the loop is the host loop
def host_loop(eng, x, cl, U, Tn, G, radius, shape, w, thr, max_hold, reach, clear_thr, watch, shift, table, dist=None, rates=None):
    """the loop written with the public calls, one by one; plan shift, the copy of the firing agents' rows into the bound
    table and the opp_plan update in torch"""
    B, N, dev = x.shape[0], eng.N, x.device
    x, U = x.clone(), U.clone()
    gather = (lambda X, opp: eng.discs_from_plans(X, opp, radius)) if shape is None else (lambda X, opp: eng.fields_from_plans(X, opp, shape))
    lam = torch.zeros(B, eng.m, dtype=torch.float64, device=dev) if eng.m else None
    held = torch.full((B,), -1, dtype=torch.int32, device=dev)
    opp_plan = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    xhat = torch.zeros_like(x)
    stats = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    tx, tu = torch.zeros(B, Tn, eng.nx, dtype=torch.float64, device=dev), torch.zeros(B, Tn, 2, dtype=torch.float64, device=dev)
    topp = torch.zeros(B, Tn, 2, dtype=torch.int32, device=dev)
    tclear = torch.zeros(B, Tn, dtype=torch.float64, device=dev)
    twhy = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    solved = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    fails = torch.zeros(B, dtype=torch.int32, device=dev)
    ar = torch.arange(B, device=dev)
    for t in range(Tn):
        _, fire_dev = eng.trigger_eval(x, xhat, held, w, thr, max_hold)
        X = eng.rollout_held(x, U, held)
        fire, why, _, _ = eng.opponent_trigger(X, held, opp_plan, G, radius, reach, clear_thr, watch, fire=fire_dev)
        fb = fire != 0
        if shift:
            U = torch.where(fb[:, None], shifted(U, held, N), U)
        opp, _ = eng.opponents_from_plans(X, G, radius, reach)
        rows = gather(X, opp)
        table[fb] = rows[fb]
        opp_plan = torch.where(fb[:, None], opp, opp_plan)
        U, lam, stats, n = eng.solve_active(x, cl, U, fire, lam=lam, stats=stats)
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
        tx[:, t], tu[:, t], topp[:, t], twhy[:, t], solved[:, t] = x, u, opp, why, fb.to(torch.uint8)
        count += fb.to(torch.int32)
        tclear[:, t] = eng.opponents_from_plans(x, G, radius)[1][:, 0]
    return mp.TrafficEventLoopResult(x, U, lam, tx, tu, fails, stats, topp, tclear, table, solved, count, held, opp_plan, twhy)


@pytest.mark.parametrize("model,N,tables", [(0, 20, False), (0, 20, True), (1, 12, False)])
def test_the_loop_is_the_host_loop_bit_for_bit(dev, model, N, tables):
    """T = 6 (Pacejka: 4, and solves cut short at 500 inner iterations -- its disturbed solves are the slow part, and the
    comparison is of bits), B = 12, a sparse disturbance that makes some agents fire by deviation; tables: a parameter and a
    rate table bound.  And two calls of T / 2 steps, the second with what the first returned, are one call of T."""
    B, G, Tn = 12, 3, 6 if model == 0 else 4
    eng, x0, cl, U0, radius, shape, rates = loop_case(dev, model, N, B, G, seed=11 + model, tables=tables,
                                                      **({} if model == 0 else dict(max_total_inner=500)))
    first = None if rates is None else rates.clone()
    x0_in = x0.clone()
    rng = np.random.default_rng(7)
    dist = T(rng.normal(0, 0.004, (B, Tn, eng.nx)) * (rng.uniform(size=(B, Tn, 1)) < 0.3), dev)
    w = np.ones(eng.nx)
    # clear_thr: the cars of a row start at c = d^2 - r^2 of 0.02 .. 0.06 from each other, so the clearance rule fires for them
    args = dict(shape=shape, reach=0.6, clear_thr=0.05, watch=3, shift=True)
    res = eng.closed_loop_traffic_event(x0, cl, U0, Tn, G, radius, w, 0.01, 5, disturbance=dist, **args)
    got = [None if t is None else t.clone() for t in res]
    F = mp.TrafficEventLoopResult._fields
    if tables:
        assert torch.equal(rates[:, 2:], res.traj_u[:, -1])
        rates.copy_(first)
    res.table.zero_()                                             # (a held agent's row is never written: both start from zeros)
    want = host_loop(eng, x0, cl, U0, Tn, G, radius, shape, w, 0.01, 5, args["reach"], args["clear_thr"], 3, True, res.table, dist=dist,
                     rates=rates)
    for name, a, b in zip(F, got, want):
        assert (a is None and b is None) or torch.equal(a, b), name
    why, solved = got[F.index("traj_why")], got[F.index("solved")]
    print(f"model {model}: solves {int(solved.sum())} of {B * Tn}; why bits seen: car {int((why & 1).bool().sum())}, clearance "
          f"{int((why & 2).bool().sum())}, new opponent {int((why & 4).bool().sum())}; failures {int(got[5].sum())}")
    assert 0 < int(solved.sum()) < B * Tn and bool((why[:, 1:] & 1).any()) and bool((why & 6).any())
    assert torch.equal(x0, x0_in) and not bool(U0.any())          # the arguments are not written
    # two calls of T / 2 steps
    if tables:
        rates.copy_(first)
    res.table.zero_()
    h = Tn // 2
    a = eng.closed_loop_traffic_event(x0, cl, U0, h, G, radius, w, 0.01, 5, disturbance=dist[:, :h].contiguous(), table=res.table, **args)
    b = eng.closed_loop_traffic_event(a.x, cl, a.U, h, G, radius, w, 0.01, 5, disturbance=dist[:, h:].contiguous(), table=res.table,
                                      held=a.held, opp_plan=a.opp_plan, lam=a.lam, stats=a.stats, **args)
    for name in ("x", "U", "lam", "stats", "table", "held", "opp_plan"):
        i = F.index(name)
        assert (b[i] is None and got[i] is None) or torch.equal(b[i], got[i]), name
    for name in ("traj_x", "traj_u", "traj_opp", "traj_clear", "solved", "traj_why"):
        i = F.index(name)
        assert torch.equal(torch.cat([a[i], b[i]], 1), got[i]), name
    assert torch.equal(a.failures + b.failures, got[5]) and torch.equal(a.solve_count + b.solve_count, got[F.index("solve_count")])
    eng.close()


# ----------------------------------------------------------------------------- 4. the mirror loop
@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "traffic_event_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    return ref


def event_loop(dev, ref, watch, Tn, **cfg):
    B = ref["X0"].shape[0]
    eng = engine(dev, 0, TE.EVENT_N, **cfg)
    eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=ref["v_ref"]), dev), arange32(B, dev))
    res = eng.closed_loop_traffic_event(T(ref["X0"], dev), T(D.line_centerline(), dev), T(ref["U0"], dev), Tn, 3, T(ref["radius"], dev),
                                        TE.EVENT_W, TE.EVENT_THR, TE.EVENT_MAX_HOLD, reach=TE.EVENT_REACH, clear_thr=TE.EVENT_CLEAR_THR,
                                        watch=watch, shift=True)
    eng.close()
    return res


def test_mirror_loop(dev):
    """24 steps of the 16 recorded scenes at discs_common's tight tolerances against the mirror loop on the CPU checker: the
    same solves, reasons and opponents step for step, the first controls within DU_METRIC, the states within STATE_BOUND.
    Fails for a loop that watches the car alone: the recording re-plans at step 1 for the other car's sake."""
    ref = reference()
    Tn = TE.EVENT_T
    res = event_loop(dev, ref, 3, Tn, **TIGHT)
    u, uref = res.traj_u.cpu().numpy(), ref["traj_u"]
    du0 = np.abs(u[:, 0] - uref[:, 0]).max(1) / np.maximum(1.0, np.abs(uref[:, 0]).max(1))
    dx = np.abs(res.traj_x.cpu().numpy() - ref["traj_x"])
    print(f"mirror loop: failures {int(res.failures.sum())}; du(step 0) {du0.max():.3e}; dx max {dx.max():.3e} at step "
          f"{int(dx.max((0, 2)).argmax())}; solves per car {res.solve_count.tolist()}")
    assert int(res.failures.sum()) == 0
    assert np.array_equal(res.solved.cpu().numpy(), ref["solved"])
    assert np.array_equal(res.traj_why.cpu().numpy(), ref["traj_why"])
    assert np.array_equal(res.traj_opp.cpu().numpy(), ref["traj_opp"])
    assert (ref["traj_why"][0::3, 1] & 6).all()
    assert du0.max() <= DU_METRIC
    assert STATE_BOUND <= 1e-4 and dx.max() <= STATE_BOUND


# ----------------------------------------------------------------------------- 5. end to end
def test_the_held_plan_and_the_other_car_end_to_end(dev):
    """The recorded scenes at the handle's default tolerances.  The loop that watches the car alone (watch = 0) holds the
    plans of step 0, which were solved against nobody, up to the hold limit, and the rear car drives into the slower one:
    deeper than half r^2 inside.  With the rules on it re-plans at the recorded step, every car's smallest realised clearance
    is no lower than the recorded mirror loop's minus CLEAR_MARGIN, and it still holds elsewhere."""
    ref = reference()
    r2 = TE.EVENT_RADIUS ** 2
    blind = event_loop(dev, ref, 0, TE.EVENT_T_BLIND)
    res = event_loop(dev, ref, 3, TE.EVENT_T)
    cb, clear = blind.traj_clear.cpu().numpy(), res.traj_clear.cpu().numpy()
    diff = ref["traj_clear"].min(1) - clear.min(1)
    print(f"end to end: watch 0 rear cars' last clear max {cb[0::3, -1].max():.6f} (-0.5 r^2 = {-0.5 * r2:.6f}; recorded "
          f"{ref['blind_traj_clear'][0::3, -1].max():.6f}); watch 3 min clear {clear.min():.3e}, mirror {ref['traj_clear'].min():.3e}; "
          f"mirror - loop per car: max {diff.max():.3e} min {diff.min():.3e}; solves per car {res.solve_count.tolist()}; failures "
          f"{int(res.failures.sum())}")
    assert (ref["blind_traj_clear"][0::3, -1] < -0.5 * r2).all()
    assert (cb[0::3, -1] < -0.5 * r2).all() and not bool((blind.traj_why & 6).any()) and bool((blind.solve_count == 1).all())
    assert np.array_equal(res.solved.cpu().numpy(), ref["solved"]) and bool((res.traj_why[0::3, 1] & 6).bool().all())
    assert (clear.min(1) >= ref["traj_clear"].min(1) - CLEAR_MARGIN).all()
    assert bool((res.solve_count < TE.EVENT_T).all())


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    """each MPC_E_ARG (-1) in the library's words, nothing launched: the outputs keep their sentinel"""
    N, B, G = 20, 12, 3
    X0, _, radius_h, shape_h = TE.loop_scene(0, B, G, seed=2)
    x0, cl, radius, shape = T(X0, dev), T(D.line_centerline(), dev), T(radius_h, dev), T(shape_h, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    lam = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
    ftable = torch.zeros(B, 16 * N, dtype=torch.float64, device=dev)
    held = torch.full((B,), 2, dtype=torch.int32, device=dev)
    plan = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
    X = torch.ones(B, N, 4, dtype=torch.float64, device=dev)
    chk = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
    clear = torch.full((B, 2), 77.0, dtype=torch.float64, device=dev)
    why = torch.full((B,), 77, dtype=torch.uint8, device=dev)
    fire = torch.full((B,), 77, dtype=torch.int32, device=dev)
    topp = torch.full((B, 1, 2), 77, dtype=torch.int32, device=dev)
    twhy = torch.full((B, 1), 77, dtype=torch.uint8, device=dev)
    wv = (C.c_double * 4)(1, 1, 1, 1)

    def loop(eng, B=B, Tn=1, G=G, radius=radius, shape=None, reach=1.0, clear_thr=0.0, watch=3, max_hold=4, table=table, plan=plan,
             held=held, thr=0.1):
        return eng.lib.mpc_closed_loop_traffic_event(
            eng._h, B, Tn, 1, wv, thr, max_hold, G, p(radius), p(shape), float(reach), float(clear_thr), watch, p(x0), p(cl), None,
            p(U0), p(lam), p(held), p(plan), p(table), None, None, None, p(topp), None, p(twhy), None, None, None, None, eng._stream())

    def trig(eng, B=B, G=G, X=X, radius=radius, reach=1.0, clear_thr=0.0, watch=3, held=held, plan=plan, chk=chk, fire=fire):
        return eng.lib.mpc_opponent_trigger(eng._h, B, G, p(X), p(radius), float(reach), p(held), p(plan), float(clear_thr), watch, None,
                                            p(chk), p(clear), p(why), p(fire), eng._stream())

    def refused(rc, who, words):
        msg = _lib.load().mpc_last_error().decode()
        assert rc == -1 and msg.startswith(who + ": ") and words in msg, (rc, msg)

    def untouched():
        torch.cuda.synchronize()
        assert bool((chk == 77).all()) and bool((clear == 77.0).all()) and bool((why == 77).all()) and bool((fire == 77).all())
        assert bool((topp == 77).all()) and bool((twhy == 77).all()) and bool((plan == 77).all())
        assert bool((held == 2).all()) and not bool(table.any()) and not bool(ftable.any()) and not bool(U0.any())
    LOOP, TRIG = "mpc_closed_loop_traffic_event", "mpc_opponent_trigger"
    # a field handle: the field table and a shape; a disc handle: the disc table and no shape
    other = engine(dev, 0, N, mode=mp.CONSTR_LANE, max_total_inner=300)
    other.set_agent_fields(ftable, arange32(B, dev))
    refused(loop(other, table=ftable), LOOP, "null shape")
    refused(loop(other, shape=shape, table=table), LOOP, "must be the field table that is bound (mpc_set_agent_fields)")
    other.close()
    eng = engine(dev, 0, N, max_total_inner=300)
    refused(loop(eng), LOOP, "no disc table is bound (mpc_set_agent_discs)")
    half = torch.zeros(B // 2, 6 * N, dtype=torch.float64, device=dev)
    eng.set_agent_discs(half, T(np.arange(B) // 2, dev, torch.int32))
    refused(loop(eng, table=half), LOOP, "has 6 rows, the loop needs one per agent")
    eng.set_agent_discs(table, arange32(B, dev))
    refused(loop(eng, shape=shape), LOOP, "shape must be NULL")
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
        for kw, words in ((dict(G=5), "B % G"), (dict(G=0), "scene size G"), (dict(G=65), "scene size G"), (dict(radius=None), "null radius"),
                          (dict(B=6, G=3), "the bound disc table is for a batch of 12 agents, this call has 6")):
            refused(fn(eng, **kw), who, words)
    refused(loop(eng, max_hold=N + 1), LOOP, "max_hold must be in [1, N]")
    refused(loop(eng, max_hold=0), LOOP, "max_hold must be in [1, N]")
    refused(loop(eng, thr=-1.0), LOOP, "thr must be >= 0")
    refused(loop(eng, Tn=-1), LOOP, "negative T")
    refused(trig(eng, X=None), TRIG, "null X")
    refused(trig(eng, chk=None), TRIG, "null X")
    refused(trig(eng, fire=None), TRIG, "null X")
    # a rate table with P != B
    eng.set_agent_rates(T(_lib.rate_rows(0.1, 0.1), dev), torch.zeros(B, dtype=torch.int32, device=dev))
    refused(loop(eng), LOOP, "the bound rate table has 1 rows")
    eng.clear_agent_rates()
    untouched()
    # the front end
    ok = dict(G=G, radius=radius, w=np.ones(4), thr=0.1, max_hold=4, reach=1.0, table=table)
    zero_plan = torch.zeros_like(plan)
    for kw in (dict(max_hold=N + 1), dict(thr=-1.0), dict(G=5), dict(reach=-1.0), dict(shape=shape), dict(radius=radius[:6].contiguous()),
               dict(opp_plan=plan), dict(opp_plan=zero_plan - 2), dict(held=held.long())):
        with pytest.raises((ValueError, TypeError)):
            eng.closed_loop_traffic_event(x0, cl, U0, 1, **{**ok, **kw})
    with pytest.raises(mp.MpcError, match="clear_thr must be a number <= reach"):
        eng.closed_loop_traffic_event(x0, cl, U0, 1, G, radius, np.ones(4), 0.1, 4, reach=1.0, clear_thr=2.0, table=table)
    with pytest.raises(mp.MpcError, match="watch must be in"):
        eng.opponent_trigger(X, held, zero_plan, G, radius, 1.0, 0.0, 4)
    with pytest.raises(ValueError):
        eng.opponent_trigger(X, held, plan, G, radius, 1.0, 0.0, 3)           # 77 is no agent of a batch of 12
    # while solve_async is in flight
    wait = eng.solve_async(x0, cl, U0)
    refused(loop(eng), LOOP, "a solve of this handle is in flight")
    refused(trig(eng), TRIG, "a solve of this handle is in flight")
    wait()
    untouched()
    plan.fill_(-1)
    assert trig(eng) == 0 and loop(eng) == 0                      # ... and afterwards both are served
    torch.cuda.synchronize()
    assert not bool((fire == 77).any()) and bool((twhy != 77).all()) and bool((topp != 77).all())
    eng.close()
