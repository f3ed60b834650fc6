"""GPU tests of the scripted obstacles (mpc_obstacles_select, mpc_discs_from_obstacles / mpc_fields_from_obstacles,
mpc_closed_loop_obstacles; BatchedMPC.obstacles_select / discs_from_obstacles / fields_from_obstacles /
closed_loop_obstacles).  Selection and gathers are compared bit for bit with the numpy restatement of
tests/obstacles_common.py, the loop bit for bit with the host loop of the public calls it is made of, and -- within the
project's bars between two correct solvers -- with the mirror loop on the CPU checker recorded in
tests/golden/obstacles_reference.npz (tests/golden/make_obstacles_golden.py).  The measured figures behind the two bounds
that were measured (STATE_BOUND, CLEAR_MARGIN) are in profiles/r18_obstacles.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from agent_tables_common import T
from conftest import GOLDEN

import discs_common as D
import obstacles_common as OC

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402
from model_predictive_control_amd.tracks import stadium_track  # noqa: E402

DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)   # tests/test_gpu_agent_discs.py
# States of the loop against the recorded mirror loop, 8 steps at TIGHT: measured on an MI355X 1.66e-6, at the seventh step
# (profiles/r18_obstacles.txt); four times that (the solver-path differences between builds), and below the
# cap of 1e-4
STATE_BOUND = 6.7e-6
# min_t traj_clear (d^2 - r^2) of the loop at the handle's default tolerances against the recorded mirror loop's, per car:
# measured on an MI355X, the loop is at most 1.89e-8 lower; four times that (profiles/r18_obstacles.txt)
CLEAR_MARGIN = 7.6e-8
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def engine(dev, model, N, mode=mp.CONSTR_DISCS, **kw):
    return mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, **kw), dev)


def arange32(B, dev):
    return torch.arange(B, dtype=torch.int32, device=dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------- 1. selection and gathers
def check_selection(eng, dev, X, G, obs, ti, reach, wrap, tot):
    B, K, Lt = X.shape[0], obs.shape[1], obs.shape[2]
    want_sel, want_clear, info = OC.select_obstacles(X, G, obs, ti, reach, wrap)
    for k in tot:
        tot[k] += info[k]
    Xt, ot = T(X, dev), T(obs, dev)
    sel, clear = eng.obstacles_select(Xt, G, ot, ti, reach, wrap)
    assert np.array_equal(sel.cpu().numpy(), want_sel), (G, K, B, np.argwhere(sel.cpu().numpy() != want_sel)[:5])
    assert np.array_equal(bits(clear.cpu().numpy()), bits(want_clear)), (G, K, B)
    # clear = NULL is accepted and changes nothing
    sel2 = torch.full((B, 2), 7, dtype=torch.int32, device=dev)
    assert eng.lib.mpc_obstacles_select(eng._h, B, G, K, Lt, int(wrap), ti, X.shape[1], p(Xt), p(ot), float(reach), p(sel2), None,
                                        eng._stream()) == 0
    assert np.array_equal(sel2.cpu().numpy(), want_sel)
    return sel, ot, want_sel


def check_gather(eng, dev, sel, G, ot, obs, ti, wrap, want_sel):
    """every word of a table pre-filled with 3.0 is rewritten, and equals the restatement's"""
    B, W = sel.shape[0], obs.shape[3]
    gather = eng.discs_from_obstacles if W == 3 else eng.fields_from_obstacles
    out = torch.full((B, 2 * W * eng.N), 3.0, dtype=torch.float64, device=dev)
    assert gather(sel, G, ot, ti, wrap, out=out) is out
    want = OC.gather_rows(want_sel, G, obs, ti, eng.N, wrap).reshape(B, -1)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (G, B)
    # slots outside [0, K) give zeros
    off = sel.clone()
    off[::2, 0], off[1::2, 1] = obs.shape[1], -5
    got = gather(off, G, ot, ti, wrap).cpu().numpy().reshape(B, eng.N, 2, W)
    assert not got[::2, :, 0].any() and not got[1::2, :, 1].any()
    assert np.array_equal(bits(got[1::2, :, 0]), bits(want.reshape(B, eng.N, 2, W)[1::2, :, 0]))


@pytest.mark.parametrize("nx", [4, 6])
def test_selection_and_gathers_are_the_restatement_bit_for_bit(dev, nx):
    """Fails on a library without the entry points.  nx = 4: a disc handle (W = 3); nx = 6: a handle without constraints
    (W = 8).  Every Nst of obstacles_common.SELECTION_STAGES (17 and 37 cross the kernel's chunk of 16 stages) on every
    shape; the gathers where the case's window is the horizon's."""
    eng = engine(dev, 0, 20) if nx == 4 else engine(dev, 1, 12, mode=mp.CONSTR_NONE)
    W = _lib.obstacle_width(eng.cfg)
    assert eng.nx == nx and W == (3 if nx == 4 else 8)
    for Nst in OC.SELECTION_STAGES:
        tot = dict(ties=0, short=0, nonfinite=0, absent=0)
        for which, (G, K, B) in enumerate(OC.SELECTION_SHAPES):
            X, obs, ti, wrap = OC.selection_case(nx, W, Nst, G, K, B, which)
            sel, ot, want_sel = check_selection(eng, dev, X, G, obs, ti, OC.SELECTION_REACH, wrap, tot)
            if Nst in (12, 20):
                check_gather(eng, dev, sel, G, ot, obs, ti, wrap, want_sel)
        print(f"nx {nx}, Nst {Nst}: {tot}")
        assert tot["ties"] >= 20 and tot["short"] >= 20 and tot["nonfinite"] >= 5, tot
        assert tot["absent"] >= 20 or Nst == 1, tot       # (a window of one absent sample makes its obstacle no candidate)
    # reach = +inf (every obstacle with a present sample is a candidate) and the states as they are now ([B, nx])
    X, obs, ti, wrap = OC.selection_case(nx, W, 20, 17, 64, 255, 2)
    check_selection(eng, dev, X, 17, obs, ti, INF, wrap, dict(ties=0))
    x = np.ascontiguousarray(X[:, 0])
    s1, c1 = eng.obstacles_select(T(x, dev), 17, T(obs, dev), ti, OC.SELECTION_REACH, wrap)
    w1, wc1, _ = OC.select_obstacles(x, 17, obs, ti, OC.SELECTION_REACH, wrap)
    assert np.array_equal(s1.cpu().numpy(), w1) and np.array_equal(bits(c1.cpu().numpy()), bits(wc1))
    eng.close()


# ----------------------------------------------------------------------------- 2. the loop is the host loop
def host_loop(eng, x, cl, U, Tn, G, obs, reach, shift, table, t0=0, wrap=False, rates=None, trk=None, ci=None, lam=None):
    """the loop written with the public calls, one by one"""
    B = x.shape[0]
    x, U = x.clone(), U.clone()
    gather = eng.discs_from_obstacles if _lib.obstacle_width(eng.cfg) == 3 else eng.fields_from_obstacles
    if eng.m:
        lam = torch.zeros(B, eng.m, dtype=torch.float64, device=x.device) if lam is None else lam.clone()
    tx = torch.zeros(B, Tn, eng.nx, dtype=torch.float64, device=x.device)
    tu = torch.zeros(B, Tn, 2, dtype=torch.float64, device=x.device)
    tsel = torch.zeros(B, Tn, 2, dtype=torch.int32, device=x.device)
    tclear = torch.zeros(B, Tn, dtype=torch.float64, device=x.device)
    fails = torch.zeros(B, dtype=torch.int32, device=x.device)
    st = None
    for t in range(Tn):
        ti = t0 + t + 1
        if trk is not None:
            ci, _ = eng.track_select(x, trk, ci)
        X = eng.rollout(x, U)
        sel, _ = eng.obstacles_select(X, G, obs, ti, reach, wrap)
        assert gather(sel, G, obs, ti, wrap, out=table) is table
        U, lam, st = eng.solve(x, cl, U, lam=lam, cl_index=ci, inplace=True)
        if rates is not None:
            rates[:, 2:4] = U[:, :2]
        tu[:, t] = U[:, :2]
        x = eng.rollout(x, U[:, :2].contiguous())[:, 0].contiguous()
        if shift:
            U[:, :-2] = U[:, 2:].clone()
        tx[:, t], tsel[:, t] = x, sel
        fails += (st[:, 0] != 1).to(torch.int32)
        tclear[:, t] = eng.obstacles_select(x, G, obs, ti, INF, wrap)[1][:, 0]
    return mp.ObstacleLoopResult(x, U, lam, tx, tu, fails, st, tsel, tclear, table, ci)


def same(got, want):
    for name, a, b in zip(mp.ObstacleLoopResult._fields, got, want):
        assert (a is None and b is None) or torch.equal(a, b), name


LOOP_CASES = [(0, 20, 130, 5, 4, 5, True, False), (0, 20, 130, 5, 4, 5, False, True),
              (1, 12, 66, 3, 3, 3, True, False), (1, 12, 66, 3, 3, 3, False, False)]


@pytest.mark.parametrize("model,N,B,G,K,Tn,shift,tables", LOOP_CASES)
def test_the_loop_is_the_host_loop_bit_for_bit(dev, model, N, B, G, K, Tn, shift, tables):
    """model 0: a disc handle; model 1: a handle of CONSTR_LANE with fields.  tables: a parameter table and a rate table
    bound.  And two calls of T steps, the second with t0 = T, are one call of 2 T."""
    mode = mp.CONSTR_DISCS if model == 0 else mp.CONSTR_LANE
    eng = engine(dev, model, N, mode=mode, Sigma0=10.0, max_total_inner=1500)
    W = _lib.obstacle_width(eng.cfg)
    Lt = 2 * Tn + N - 3                                  # the last windows of the 2 T steps clamp at the end of the script
    X0, v_ref, obs_h = OC.loop_scene(model, B, G, K, Lt, W, seed=11 + model)
    obs = T(_lib.obstacle_tracks(eng.cfg, centres=obs_h[..., :2], radii=obs_h[..., 2]) if W == 3
            else _lib.obstacle_tracks(eng.cfg, sources=obs_h), dev)
    rates = first = None
    if tables:
        eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=v_ref), dev), arange32(B, dev))
        first = T(_lib.rate_rows(np.linspace(0.0, 0.2, B), 0.05), dev)
        rates = first.clone()
        eng.set_agent_rates(rates, arange32(B, dev))
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    reach = 0.6
    res = eng.closed_loop_obstacles(x0, cl, U0, 2 * Tn, G, obs, reach, shift=shift)      # makes and binds its table
    assert (eng.agent_discs_bound if W == 3 else eng.agent_fields_bound) and res.table.shape == (B, 2 * W * N)
    got = [None if t is None else t.clone() for t in res]
    if tables:
        assert torch.equal(rates[:, 2:], res.traj_u[:, -1]) and torch.equal(rates[:, :2], first[:, :2])
        rates.copy_(first)
    res.table.fill_(3.0)                                                                 # every word is rewritten
    want = host_loop(eng, x0, cl, U0, 2 * Tn, G, obs, reach, shift, res.table, rates=rates)
    same(got, want)
    tsel, tclear = got[7], got[8]
    print(f"model {model}: {0 if got[2] is None else int((got[2] < 0).sum())} multipliers below 0, {int((tsel >= 0).sum())} of "
          f"{tsel.numel()} slots in use, failures {int(got[5].sum())}, smallest realised clearance {float(tclear.min()):.4f}")
    assert bool((tsel >= 0).any()) and bool((tsel == -1).any())
    if model == 0:
        assert bool((got[2] < 0).any())
    else:   # a selected source within two of its length scales of a plan's first state (traj_clear is d^2 to the nearest)
        assert float(tclear.min()) < (2 * OC.FIELD_SIGMA) ** 2
    assert torch.equal(x0, T(X0, dev)) and not bool(U0.any())                            # the arguments are not written
    # two calls of T steps: the second continues the script at t0 = T, on the table handed in
    if tables:
        rates.copy_(first)
    a = eng.closed_loop_obstacles(x0, cl, U0, Tn, G, obs, reach, shift=shift, table=res.table)
    b = eng.closed_loop_obstacles(a.x, cl, a.U, Tn, G, obs, reach, t0=Tn, lam=a.lam, shift=shift, table=res.table)
    assert b.table is res.table
    for i in (0, 1, 2, 6, 9):
        assert (b[i] is None and got[i] is None) or torch.equal(b[i], got[i]), mp.ObstacleLoopResult._fields[i]
    for i in (3, 4, 7, 8):
        assert torch.equal(torch.cat([a[i], b[i]], 1), got[i]), mp.ObstacleLoopResult._fields[i]
    assert torch.equal(a.failures + b.failures, got[5])
    eng.close()


def test_the_loop_on_a_track_is_the_host_loop_with_track_select_in_front(dev):
    """lap driving among moving obstacles on a small stadium: one periodic obstacle circles the track ahead of the cars"""
    N, B, G, Tn = 20, 64, 4, 4
    eng = engine(dev, 0, N, Sigma0=10.0, max_total_inner=300)
    track = stadium_track(10, 3, 0.1)
    trk = eng.track_windows(T(track, dev), 4, 10, True)
    L = track.size // 2
    rng = np.random.default_rng(31)
    at = rng.integers(0, L, B)
    tx, ty = track[(at + 1) % L] - track[at], track[L + (at + 1) % L] - track[L + at]
    X0 = np.stack([track[at], track[L + at] + rng.uniform(-.05, .05, B), np.arctan2(ty, tx), rng.uniform(.6, 1.0, B)], 1)
    # one obstacle per scene: it circles the whole track, 8 points a sample, starting 4 points ahead of the scene's first car
    Lt = L // 8
    obs_h = np.zeros((B // G, 1, Lt, 3))
    for s in range(B // G):
        i = (at[s * G] + 4 + 8 * np.arange(Lt)) % L
        obs_h[s, 0, :, 0], obs_h[s, 0, :, 1], obs_h[s, 0, :, 2] = track[i], track[L + i] + 0.03, 0.12
    obs = T(_lib.obstacle_tracks(eng.cfg, centres=obs_h[..., :2], radii=obs_h[..., 2]), dev)
    x0 = T(X0, dev)
    U0 = T(np.tile([1., 0.], (B, N)), dev)
    ci0 = eng.track_locate(x0, trk)
    t0 = Lt - 2                                           # the windows wrap around the script's end
    res = eng.closed_loop_obstacles(x0, None, U0, Tn, G, obs, 0.8, t0=t0, wrap=True, cl_index=ci0, shift=True, track_obj=trk)
    got = [t.clone() for t in res]
    res.table.fill_(3.0)
    want = host_loop(eng, x0, trk.win, U0, Tn, G, obs, 0.8, True, res.table, t0=t0, wrap=True, trk=trk, ci=ci0)
    same(got, want)
    assert bool((got[7] >= 0).any()) and len(torch.unique(got[10])) > 20  # obstacles in reach; the cars are spread over the track
    assert torch.equal(ci0, eng.track_locate(x0, trk))                    # the argument is not written
    eng.close()


# ----------------------------------------------------------------------------- 3. degenerate cases
@pytest.mark.parametrize("model,N,mode", [(0, 20, mp.CONSTR_DISCS), (1, 12, mp.CONSTR_LANE)])
def test_all_samples_absent_is_closed_loop_on_a_zero_table(dev, model, N, mode):
    B, G, K, Tn = 70, 5, 3, 4
    eng = engine(dev, model, N, mode=mode, Sigma0=10.0, max_total_inner=3000)
    W = _lib.obstacle_width(eng.cfg)
    X0, _, obs_h = OC.loop_scene(model, B, G, K, 9, W, seed=3)
    obs_h[..., 2 if W == 3 else 4] = 0.0                      # everything else stays: junk behind the zero
    table = torch.zeros(B, 2 * W * N, dtype=torch.float64, device=dev)
    (eng.set_agent_discs if W == 3 else eng.set_agent_fields)(table, arange32(B, dev))
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    want = eng.closed_loop(x0, cl, U0, Tn, shift=True)
    res = eng.closed_loop_obstacles(x0, cl, U0, Tn, G, T(obs_h, dev), shift=True, table=table)
    for a, b in zip(res[:7], want):
        assert torch.equal(a, b)
    assert bool((res.traj_sel == -1).all()) and bool(torch.isposinf(res.traj_clear).all()) and not bool(table.any())
    eng.close()


def test_one_standing_disc_is_closed_loop_on_a_static_table(dev):
    """K = 1, Lt = 1, reach = +inf: the disc stands in slot 0 of every stage"""
    N, B, G, Tn = 20, 70, 5, 4
    eng = engine(dev, 0, N, Sigma0=10.0, max_total_inner=3000)
    X0, _, obs_h = OC.loop_scene(0, B, G, 1, 1, 3, seed=4)
    static = np.zeros((B, N, 2, 3))
    static[:, :, 0] = np.repeat(obs_h[:, 0, 0], G, 0)[:, None, :]
    table = T(static.reshape(B, -1), dev)
    eng.set_agent_discs(table, arange32(B, dev))
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    want = eng.closed_loop(x0, cl, U0, Tn, shift=True)
    assert bool((want[2] < 0).any())                           # the disc is in the way
    res = eng.closed_loop_obstacles(x0, cl, U0, Tn, G, T(obs_h, dev), INF, shift=True, table=table)
    for a, b in zip(res[:7], want):
        assert torch.equal(a, b)
    assert bool((res.traj_sel[:, :, 0] == 0).all()) and bool((res.traj_sel[:, :, 1] == -1).all())
    assert torch.equal(table, T(static.reshape(B, -1), dev))
    eng.close()


# ----------------------------------------------------------------------------- 4. the mirror loop
@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "obstacles_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    return ref


def script_engine(dev, ref, **kw):
    B = ref["X0"].shape[0]
    eng = engine(dev, 0, OC.SCRIPT_N, **kw)
    eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=ref["v_ref"]), dev), arange32(B, dev))
    args = (T(ref["X0"], dev), T(D.line_centerline(), dev), torch.zeros(B, 2 * OC.SCRIPT_N, dtype=torch.float64, device=dev))
    return eng, args, T(ref["obs"], dev)


def test_mirror_loop(dev):
    """8 steps of the 16 recorded scenes at discs_common's tight tolerances against the mirror loop on the CPU checker: the
    same selection step for step, the first controls within DU_METRIC, the states within STATE_BOUND"""
    ref = reference()
    Tn = 8
    eng, args, obs = script_engine(dev, ref, **TIGHT)
    res = eng.closed_loop_obstacles(*args, Tn, 1, obs, OC.SCRIPT_REACH, shift=True)
    eng.close()
    u, uref = res.traj_u.cpu().numpy(), ref["traj_u"][:, :Tn]
    du0 = np.abs(u[:, 0] - uref[:, 0]).max(1) / np.maximum(1.0, np.abs(uref[:, 0]).max(1))
    dx = np.abs(res.traj_x.cpu().numpy() - ref["traj_x"][:, :Tn])
    dc = np.abs(res.traj_clear.cpu().numpy() - ref["traj_clear"][:, :Tn])
    print(f"mirror loop: failures {int(res.failures.sum())}; du(step 0) {du0.max():.3e}; dx per step {dx.max((0, 2))}; "
          f"dx max {dx.max():.3e}; dclear max {dc.max():.3e}")
    assert int(res.failures.sum()) == 0
    assert np.array_equal(res.traj_sel.cpu().numpy(), ref["traj_sel"][:, :Tn])
    assert du0.max() <= DU_METRIC
    assert dx.max() <= STATE_BOUND


# ----------------------------------------------------------------------------- 5. end to end
def test_the_pass_end_to_end(dev):
    """16 scenes of one car and three scripted obstacles, 14 steps, the handle's default tolerances.  With every sample made
    absent the car drives through the slow obstacle: it passes within 0.05 of its centre.  With the loop it ends ahead of
    it, and its smallest realised clearance is no lower than the recorded mirror loop's minus CLEAR_MARGIN."""
    ref = reference()
    B, Tn = ref["X0"].shape[0], 14
    eng, args, obs = script_engine(dev, ref)
    gone = obs.clone()
    gone[..., 2] = 0.0
    alone = eng.closed_loop_obstacles(*args, Tn, 1, gone, OC.SCRIPT_REACH, shift=True)
    res = eng.closed_loop_obstacles(*args, Tn, 1, obs, OC.SCRIPT_REACH, shift=True, table=alone.table)
    eng.close()
    slow = ref["obs"][:, 0, 1:Tn + 1, :2]                       # where the slow obstacle is at times 1 .. T
    xa, tx, clear = alone.traj_x.cpu().numpy(), res.traj_x.cpu().numpy(), res.traj_clear.cpu().numpy()
    d_alone = np.hypot(xa[:, :, 0] - slow[:, :, 0], xa[:, :, 1] - slow[:, :, 1]).min(1)
    d_loop = np.hypot(tx[:, :, 0] - slow[:, :, 0], tx[:, :, 1] - slow[:, :, 1]).min(1)
    diff = ref["traj_clear"].min(1) - clear.min(1)
    print(f"pass: closest without avoidance {d_alone.max():.4f}, with {d_loop.min():.6f} (r = {OC.SCRIPT_RADIUS}); car y min "
          f"{tx[:, :, 1].min():.4f}; min clear loop {clear.min():.3e} mirror {ref['traj_clear'].min():.3e}; mirror - loop per car: "
          f"max {diff.max():.3e} min {diff.min():.3e}; failures {int(res.failures.sum())}")
    print("mirror - loop per car:", " ".join(f"{d:.2e}" for d in diff))
    assert bool((alone.traj_sel == -1).all()) and bool(torch.isposinf(alone.traj_clear).all())
    assert (d_alone < 0.05).all()
    assert (tx[:, -1, 0] > slow[:, -1, 0]).all()
    assert (clear.min(1) >= ref["traj_clear"].min(1) - CLEAR_MARGIN).all()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    """each MPC_E_ARG (-1) in the library's words, nothing launched: the outputs keep their sentinel"""
    N, B, G, K, Lt = 20, 12, 3, 2, 9
    X0, _, obs_h = OC.loop_scene(0, B, G, K, Lt, 3, seed=2)
    x0, cl, obs = T(X0, dev), T(D.line_centerline(), dev), T(obs_h, dev)
    fobs = torch.zeros(B // G, K, Lt, 8, dtype=torch.float64, device=dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    lam = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
    ftable = torch.zeros(B, 16 * N, dtype=torch.float64, device=dev)
    sel = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
    clear = torch.full((B, 2), 77.0, dtype=torch.float64, device=dev)
    out = torch.full((B, 16 * N), 77.0, dtype=torch.float64, device=dev)
    tsel = torch.full((B, 1, 2), 77, dtype=torch.int32, device=dev)
    big = 2 ** 31 - 1

    def loop(eng, B=B, Tn=1, G=G, K=K, Lt=Lt, t0=0, obs=obs, reach=INF, table=table, trk=None, ci=None):
        return eng.lib.mpc_closed_loop_obstacles(eng._h, B, Tn, 0, G, K, Lt, 0, t0, p(obs), float(reach), p(x0), p(cl), p(ci), p(U0),
                                                 p(lam), p(table), None, None, p(tsel), None, None, None, eng._stream(), trk)

    def select(eng, B=B, G=G, K=K, Lt=Lt, ti=0, Nst=1, X=x0, obs=obs, reach=INF, sel=sel):
        return eng.lib.mpc_obstacles_select(eng._h, B, G, K, Lt, 0, ti, Nst, p(X), p(obs), float(reach), p(sel), p(clear), eng._stream())

    def gather(name):
        def call(eng, B=B, G=G, K=K, Lt=Lt, ti=0, obs=obs, sel=sel, table=out):
            return getattr(eng.lib, name)(eng._h, B, G, K, Lt, 0, ti, p(obs), p(sel), p(table), eng._stream())
        return call
    discs_g, fields_g = gather("mpc_discs_from_obstacles"), gather("mpc_fields_from_obstacles")

    def refused(rc, who, words):
        msg = _lib.load().mpc_last_error().decode()
        assert rc == -1 and msg.startswith(who + ": ") and words in msg, (rc, msg)

    def untouched():
        torch.cuda.synchronize()
        assert bool((sel == 77).all()) and bool((clear == 77.0).all()) and bool((out == 77.0).all()) and bool((tsel == 77).all())
        assert not bool(table.any()) and not bool(ftable.any())
    # the kind of the handle: the disc gather off a disc handle, the field gather on one; selection and loop take any
    other = engine(dev, 0, N, mode=mp.CONSTR_LANE, max_total_inner=300)
    refused(discs_g(other), "mpc_discs_from_obstacles", "constr_mode is not MPC_CONSTR_DISCS")
    refused(loop(other, obs=fobs, table=ftable), "mpc_closed_loop_obstacles", "must be the field table that is bound (mpc_set_agent_fields)")
    with pytest.raises(mp.MpcError, match="mpc_discs_from_obstacles: .*MPC_CONSTR_DISCS"):
        other.discs_from_obstacles(sel, G, fobs)
    with pytest.raises(ValueError, match="obs"):
        other.obstacles_select(x0, G, obs)                              # W = 3 on a handle whose samples are sources
    other.close()
    eng = engine(dev, 0, N, max_total_inner=300)
    refused(fields_g(eng), "mpc_fields_from_obstacles", "there an obstacle is a disc (mpc_set_agent_discs)")
    with pytest.raises(mp.MpcError, match="mpc_fields_from_obstacles: .*MPC_CONSTR_DISCS"):
        eng.fields_from_obstacles(sel, G, obs)
    refused(loop(eng), "mpc_closed_loop_obstacles", "no disc table is bound (mpc_set_agent_discs)")
    # a bound table with P != B, another table than the bound one
    half = torch.zeros(B // 2, 6 * N, dtype=torch.float64, device=dev)
    eng.set_agent_discs(half, T(np.arange(B) // 2, dev, torch.int32))
    refused(loop(eng, table=half), "mpc_closed_loop_obstacles", "has 6 rows, the loop needs one per agent")
    eng.set_agent_discs(table, arange32(B, dev))
    refused(loop(eng, table=table.clone()), "mpc_closed_loop_obstacles", "must be the disc table that is bound")
    refused(loop(eng, table=None), "mpc_closed_loop_obstacles", "must be the disc table that is bound")
    # a rate table with P != B
    eng.set_agent_rates(T(_lib.rate_rows(0.1, 0.1), dev), torch.zeros(B, dtype=torch.int32, device=dev))
    refused(loop(eng), "mpc_closed_loop_obstacles", "the bound rate table has 1 rows")
    eng.clear_agent_rates()
    shared = ((dict(G=5), "B % G"), (dict(G=0), "scene size G"), (dict(G=65), "scene size G"), (dict(K=0), "obstacles K"),
              (dict(K=65), "obstacles K"), (dict(Lt=0), "Lt must be >= 1"), (dict(obs=None), "null obs"),
              (dict(B=6, G=3), "the bound disc table is for a batch of 12 agents, this call has 6"))
    for fn, who, tname in ((loop, "mpc_closed_loop_obstacles", "t0"), (select, "mpc_obstacles_select", "ti"),
                           (discs_g, "mpc_discs_from_obstacles", "ti")):
        for kw, words in shared + (({tname: -1}, tname + " must be >= 0"), ({tname: big}, "does not fit an int32")):
            refused(fn(eng, **kw), who, words)
        if fn is not discs_g:
            for r in (-0.5, float("nan")):
                refused(fn(eng, reach=r), who, "reach must be >= 0")
    refused(loop(eng, Tn=-1), "mpc_closed_loop_obstacles", "negative T")
    refused(loop(eng, t0=big - N, Tn=1), "mpc_closed_loop_obstacles", "does not fit an int32")
    refused(select(eng, Nst=0), "mpc_obstacles_select", "Nst must be >= 1")
    refused(select(eng, X=None), "mpc_obstacles_select", "null X or sel")
    refused(select(eng, sel=None), "mpc_obstacles_select", "null X or sel")
    refused(select(eng, ti=big, Nst=1), "mpc_obstacles_select", "does not fit an int32")
    refused(discs_g(eng, sel=None), "mpc_discs_from_obstacles", "null sel or table")
    refused(discs_g(eng, table=None), "mpc_discs_from_obstacles", "null sel or table")
    refused(discs_g(eng, ti=big - N + 1), "mpc_discs_from_obstacles", "does not fit an int32")
    # a track without the rows to start from, and a track that mpc_track_init did not fill
    trk = eng.track_windows(T(stadium_track(10, 3, 0.1), dev), 4, 10, True)
    refused(loop(eng, trk=C.byref(trk._c), ci=None), "mpc_closed_loop_obstacles", "null buffer")
    bad = _lib.MpcTrack.from_buffer_copy(trk._c)
    bad.R += 1
    refused(loop(eng, trk=C.byref(bad), ci=arange32(B, dev)), "mpc_closed_loop_obstacles", "the track's geometry")
    untouched()
    # the front end says the same before the library is asked
    for kw in (dict(G=5), dict(G=0), dict(G=65), dict(reach=-1.0), dict(reach=float("nan")), dict(t0=-1), dict(t0=big),
               dict(obs=obs[:3].contiguous()), dict(obs=obs.float()), dict(obs=obs.cpu()), dict(obs=obs[..., :2].contiguous())):
        with pytest.raises((ValueError, TypeError)):
            eng.closed_loop_obstacles(x0, cl, U0, 1, **{**dict(G=G, obs=obs, table=table), **kw})
    for kw in (dict(G=5), dict(G=0), dict(reach=-1.0), dict(ti=-1), dict(ti=big), dict(obs=obs[:3].contiguous())):
        with pytest.raises(ValueError):
            eng.obstacles_select(x0, **{**dict(G=G, obs=obs), **kw})
    with pytest.raises(ValueError):
        eng.closed_loop_obstacles(x0, cl, U0, -1, G, obs, table=table)
    with pytest.raises(ValueError):
        eng.discs_from_obstacles(sel, 5, obs)
    # the identity index: a bound table whose index is not arange(B)
    eng.set_agent_discs(table, arange32(B, dev).flip(0).contiguous())
    with pytest.raises(ValueError, match="arange"):
        eng.closed_loop_obstacles(x0, cl, U0, 1, G, obs, table=table)
    eng.set_agent_discs(table, arange32(B, dev))
    # while solve_async is in flight
    wait = eng.solve_async(x0, cl, U0)
    refused(loop(eng), "mpc_closed_loop_obstacles", "a solve of this handle is in flight")
    refused(select(eng), "mpc_obstacles_select", "a solve of this handle is in flight")
    refused(discs_g(eng), "mpc_discs_from_obstacles", "a solve of this handle is in flight")
    with pytest.raises(mp.MpcError):
        eng.obstacles_select(x0, G, obs)
    wait()
    untouched()
    good = torch.zeros(B, 2, dtype=torch.int32, device=dev)
    assert loop(eng) == 0 and select(eng) == 0 and discs_g(eng, sel=good) == 0     # ... and afterwards all are served
    torch.cuda.synchronize()
    eng.close()
