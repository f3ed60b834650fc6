"""GPU tests of the traffic selection and the traffic closed loop (mpc_opponents_from_plans, mpc_closed_loop_traffic;
BatchedMPC.opponents_from_plans / closed_loop_traffic).  The selection is compared bit for bit with the numpy restatement
of tests/traffic_common.py, the loop bit for bit with the host loop of the public calls it is made of, and -- within the
project's bars between two correct solvers -- with the mirror loop on the CPU checker recorded in
tests/golden/traffic_reference.npz (tests/golden/make_traffic_golden.py).  The measured figures behind the two bounds that
were measured (STATE_BOUND, CLEAR_MARGIN) are in profiles/r14_traffic_loop.txt."""
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

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402

DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)   # tests/test_gpu_agent_discs.py
# States of the loop against the recorded mirror loop, 8 steps at TIGHT: measured on an MI355X 3.47e-7, at step 1
# (profiles/r14_traffic_loop.txt); four times that (the solver-path differences between builds), and below the
# cap of 1e-4
STATE_BOUND = 1.4e-6
# min_t traj_clear (d^2 - r^2) of the loop at the handle's default tolerances against the recorded mirror loop's, per car:
# measured on an MI355X, the loop is at most 2.63e-8 lower (and at most 7.6e-8 higher, which the assertion does not bound);
# four times the former (profiles/r14_traffic_loop.txt)
CLEAR_MARGIN = 1.1e-7
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


# ----------------------------------------------------------------------------- 1. the selection
def check_selection(eng, dev, X, radius, G, reach, tot):
    B = X.shape[0]
    want_opp, want_clear, info = TC.select_opponents(X, G, radius, reach)
    for k in tot:
        tot[k] += info[k]
    Xt, rt = T(X, dev), T(radius, dev)
    opp, clear = eng.opponents_from_plans(Xt, G, rt, reach)
    opp, clear = opp.cpu().numpy(), clear.cpu().numpy()
    assert np.array_equal(opp, want_opp), (G, B, np.argwhere(opp != want_opp)[:5])
    assert np.array_equal(bits(clear), bits(want_clear)), (G, B)
    on = opp >= 0
    assert (opp[on] // G == np.broadcast_to(np.arange(B)[:, None] // G, opp.shape)[on]).all()   # no agent of another scene
    # clear = NULL is accepted and changes nothing
    opp2 = torch.full((B, 2), 7, dtype=torch.int32, device=dev)
    assert eng.lib.mpc_opponents_from_plans(eng._h, B, G, X.shape[1], p(Xt), p(rt), float(reach), p(opp2), None, eng._stream()) == 0
    assert np.array_equal(opp2.cpu().numpy(), want_opp)


@pytest.mark.parametrize("nx", [4, 6])
@pytest.mark.parametrize("Nst", TC.SELECTION_STAGES)
def test_selection_is_the_restatement_bit_for_bit(dev, nx, Nst):
    """Fails on a library without the entry point.  nx = 6 runs on a handle without constraints: the call reads nx alone."""
    eng = engine(dev, 0, 20) if nx == 4 else engine(dev, 1, 12, mode=mp.CONSTR_NONE)
    assert eng.nx == nx
    tot = dict(ties=0, short=0, nonfinite=0)
    for G, B in TC.SELECTION_SHAPES:
        X, radius = TC.selection_case(nx, Nst, G, B)
        check_selection(eng, dev, X, radius, G, TC.SELECTION_REACH, tot)
    print(f"nx {nx}, Nst {Nst}: {tot}")
    assert tot["ties"] >= 20 and tot["short"] >= 20 and tot["nonfinite"] >= 5, tot
    # reach = +inf (everybody is a candidate) and the states as they are now ([B, nx])
    X, radius = TC.selection_case(nx, Nst, 17, 255)
    check_selection(eng, dev, X, radius, 17, INF, dict(tot))
    x = np.ascontiguousarray(X[:, 0])
    o1, c1 = eng.opponents_from_plans(T(x, dev), 17, T(radius, dev), TC.SELECTION_REACH)
    w1, wc1, _ = TC.select_opponents(x, 17, radius, TC.SELECTION_REACH)
    assert np.array_equal(o1.cpu().numpy(), w1) and np.array_equal(bits(c1.cpu().numpy()), bits(wc1))
    eng.close()


@pytest.mark.parametrize("Nst", [33, 70])
def test_selection_with_more_stages_than_one_staging_pass_holds(dev, Nst):
    """The kernel stages 32 stages at a time: 33 and 70 take the path that stages again (a last chunk of 1 and of 6)"""
    eng = engine(dev, 0, 20)
    tot = dict(ties=0, short=0, nonfinite=0)
    for G, B in ((17, 255), (64, 128), (3, 258)):
        X, radius = TC.selection_case(4, Nst, G, B, seed=1)
        check_selection(eng, dev, X, radius, G, TC.SELECTION_REACH, tot)
    assert tot["ties"] >= 20 and tot["nonfinite"] >= 5, tot
    eng.close()


# ----------------------------------------------------------------------------- 2. the loop is the host loop
def clumps(model, B, G, seed):
    """B agents in scenes of G on discs_common.line_centerline(): every scene's cars in two or three clumps along the line,
    cars of a clump 0.25 .. 0.32 apart and a little to the side of each other, radii 0.2 .. 0.24 (nobody inside a disc at the
    start), the rear ones 0.2 m/s faster each: within the horizon a rear car's plan runs into the plan of the car ahead, so
    discs are active"""
    rng = np.random.default_rng(seed)
    cols = np.zeros((B, 6 if model else 4))
    v_ref = np.zeros(B)
    for s in range(0, B, G):
        nclump = int(rng.integers(2, 4))
        which = np.sort(rng.integers(0, nclump, G))
        for c in range(nclump):
            mine = s + np.flatnonzero(which == c)
            x = 1.2 + 1.5 * c + rng.uniform(0, 0.2)
            for i, b in enumerate(mine):
                x += rng.uniform(0.25, 0.32) * (i > 0)
                v_ref[b] = 1.0 - 0.2 * i + rng.uniform(-.05, .05)
                cols[b, :4] = (x, 0.5 + rng.uniform(-.04, .04), rng.uniform(-.05, .05), max(0.4, v_ref[b]))
    radius = rng.uniform(0.2, 0.24, B)
    radius[rng.integers(0, B, 3)] = 0.0
    return cols, np.maximum(v_ref, 0.4), radius


def host_loop(eng, x, cl, U, Tn, G, radius, reach, shift, table):
    """the loop written with the public calls, one by one"""
    B = x.shape[0]
    x, U = x.clone(), U.clone()
    lam = torch.zeros(B, eng.m, dtype=torch.float64, device=x.device)
    tx = torch.zeros(B, Tn, eng.nx, dtype=torch.float64, device=x.device)
    tu = torch.zeros(B, Tn, 2, dtype=torch.float64, device=x.device)
    topp = torch.zeros(B, Tn, 2, dtype=torch.int32, device=x.device)
    tclear = torch.zeros(B, Tn, dtype=torch.float64, device=x.device)
    fails = torch.zeros(B, dtype=torch.int32, device=x.device)
    st = None
    for t in range(Tn):
        X = eng.rollout(x, U)
        opp, _ = eng.opponents_from_plans(X, G, radius, reach)
        assert eng.discs_from_plans(X, opp, radius, out=table) is table
        U, lam, st = eng.solve(x, cl, U, lam=lam, inplace=True)
        tu[:, t] = U[:, :2]
        x = eng.rollout(x, U[:, :2].contiguous())[:, 0].contiguous()
        if shift:
            U[:, :-2] = U[:, 2:].clone()
        tx[:, t], topp[:, t] = x, opp
        fails += (st[:, 0] != 1).to(torch.int32)
        tclear[:, t] = eng.opponents_from_plans(x, G, radius)[1][:, 0]
    return x, U, lam, tx, tu, fails, st, topp, tclear, table


@pytest.mark.parametrize("model,N,B,G,Tn,shift,per_agent", [(0, 20, 130, 5, 5, True, False), (0, 20, 130, 5, 5, False, True),
                                                            (1, 12, 66, 3, 3, True, True), (1, 12, 66, 3, 3, False, False)])
def test_the_loop_is_the_host_loop_bit_for_bit(dev, model, N, B, G, Tn, shift, per_agent):
    X0, v_ref, radius = clumps(model, B, G, seed=11 + model)
    eng = engine(dev, model, N, Sigma0=10.0, max_total_inner=1500)
    if per_agent:
        eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=v_ref), dev), arange32(B, dev))
    x0, cl, rt = T(X0, dev), T(D.line_centerline(), dev), T(radius, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    reach = 0.6
    res = eng.closed_loop_traffic(x0, cl, U0, Tn, G, rt, reach, shift=shift)         # makes and binds its table
    assert eng.agent_discs_bound and res.table.shape == (B, 6 * N)
    got = [t.clone() for t in res]
    res.table.fill_(3.0)                                                             # every word is rewritten
    want = host_loop(eng, x0, cl, U0, Tn, G, rt, reach, shift, res.table)
    names = mp.TrafficLoopResult._fields
    for name, a, b in zip(names, got, want):
        assert torch.equal(a, b), name
    print(f"model {model}: {int((got[2] < 0).sum())} multipliers below 0, {int((got[7] >= 0).sum())} of {got[7].numel()} opponent slots in use, "
          f"failures {int(got[5].sum())}, smallest realised clearance {float(got[8].min()):.4f}")
    assert bool((got[2] < 0).any()) and bool((got[7] >= 0).any()) and bool((got[7] == -1).any())
    assert bool(torch.isfinite(got[8]).all())
    assert torch.equal(x0, T(X0, dev)) and not bool(U0.any())                        # the arguments are not written
    if model == 1:   # a table handed in: the bound one, rewritten in place (the shorter cases alone: a third run of the loop)
        again = eng.closed_loop_traffic(x0, cl, U0, Tn, G, rt, reach, shift=shift, table=res.table)
        assert again.table is res.table and torch.equal(again.traj_x, got[3]) and torch.equal(again.U, got[1])
    eng.close()


# ----------------------------------------------------------------------------- 3. G = 1
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_scenes_of_one_are_closed_loop(dev, model, N):
    B, Tn = 70, 4
    X0, _, radius = clumps(model, B, 5, seed=3)
    eng = engine(dev, model, N, Sigma0=10.0, max_total_inner=3000)
    table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
    eng.set_agent_discs(table, arange32(B, dev))
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    want = eng.closed_loop(x0, cl, U0, Tn, shift=True)
    res = eng.closed_loop_traffic(x0, cl, U0, Tn, 1, T(radius, dev), shift=True, table=table)
    for a, b in zip(res[:7], want):
        assert torch.equal(a, b)
    assert bool((res.traj_opp == -1).all()) and bool(torch.isposinf(res.traj_clear).all()) and not bool(table.any())
    eng.close()


# ----------------------------------------------------------------------------- 4. the mirror loop
@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "traffic_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    return ref


def overtake_engine(dev, ref, **kw):
    B = ref["X0"].shape[0]
    eng = engine(dev, 0, TC.OVERTAKE_N, **kw)
    eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=ref["v_ref"]), dev), arange32(B, dev))
    args = (T(ref["X0"], dev), T(D.line_centerline(), dev), torch.zeros(B, 2 * TC.OVERTAKE_N, dtype=torch.float64, device=dev))
    return eng, args, T(ref["radius"], dev)


def test_mirror_loop(dev):
    """8 steps of the 16 recorded overtake scenes at discs_common's tight tolerances against the mirror loop on the CPU
    checker: the same opponents step for step, the first controls within DU_METRIC, the states within STATE_BOUND"""
    ref = reference()
    Tn = 8
    eng, args, radius = overtake_engine(dev, ref, **TIGHT)
    res = eng.closed_loop_traffic(*args, Tn, 3, radius, TC.OVERTAKE_REACH, shift=True)
    eng.close()
    assert int(res.failures.sum()) == 0
    assert np.array_equal(res.traj_opp.cpu().numpy(), ref["traj_opp"][:, :Tn])
    u, uref = res.traj_u.cpu().numpy(), ref["traj_u"][:, :Tn]
    du0 = np.abs(u[:, 0] - uref[:, 0]).max(1) / np.maximum(1.0, np.abs(uref[:, 0]).max(1))
    dx = np.abs(res.traj_x.cpu().numpy() - ref["traj_x"][:, :Tn])
    dc = np.abs(res.traj_clear.cpu().numpy() - ref["traj_clear"][:, :Tn])
    print(f"mirror loop: du(step 0) {du0.max():.3e}; dx per step {dx.max((0, 2))}; dx max {dx.max():.3e}; dclear max {dc.max():.3e}")
    assert du0.max() <= DU_METRIC
    assert dx.max() <= STATE_BOUND


# ----------------------------------------------------------------------------- 5. the overtake
def test_the_overtake_end_to_end(dev):
    """16 scenes of three cars (B = 48), 14 steps, the handle's default tolerances.  Without avoidance (G = 1) the
    follower drives through the slow car: their lateral offset is 0.03, so where the follower passes, the centres are
    within 0.05.  With the loop it ends ahead without touching: every car's smallest realised clearance is no lower than
    the recorded mirror loop's minus CLEAR_MARGIN."""
    ref = reference()
    B, Tn = ref["X0"].shape[0], 14
    eng, args, radius = overtake_engine(dev, ref)
    alone = eng.closed_loop_traffic(*args, Tn, 1, radius, TC.OVERTAKE_REACH, shift=True)
    res = eng.closed_loop_traffic(*args, Tn, 3, radius, TC.OVERTAKE_REACH, shift=True, table=alone.table)
    eng.close()
    a, b = np.arange(0, B, 3), np.arange(1, B, 3)
    xa = alone.traj_x.cpu().numpy()
    d_alone = np.hypot(xa[a, :, 0] - xa[b, :, 0], xa[a, :, 1] - xa[b, :, 1]).min(1)
    tx, clear, opp = res.traj_x.cpu().numpy(), res.traj_clear.cpu().numpy(), res.traj_opp.cpu().numpy()
    d_loop = np.hypot(tx[a, :, 0] - tx[b, :, 0], tx[a, :, 1] - tx[b, :, 1]).min(1)
    diff = ref["traj_clear"].min(1) - clear.min(1)
    print(f"overtake: closest without avoidance {d_alone.max():.4f}, with {d_loop.min():.6f} (r = {TC.OVERTAKE_RADIUS}); "
          f"follower y min {tx[a, :, 1].min():.4f}; min clear loop {clear.min():.3e} mirror {ref['traj_clear'].min():.3e}; "
          f"mirror - loop per car: max {diff.max():.3e} min {diff.min():.3e}; failures {int(res.failures.sum())}")
    assert (d_alone < 0.05).all()
    assert (tx[a, -1, 0] > tx[b, -1, 0]).all()
    assert not (opp[a] == (a + 2)[:, None, None]).any() and not (opp[b] == (b + 1)[:, None, None]).any()   # the third car: never
    assert (clear.min(1) >= ref["traj_clear"].min(1) - CLEAR_MARGIN).all()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    """each MPC_E_ARG (-1) in the library's words, nothing launched"""
    N, B, G = 20, 12, 3
    X0, _, radius = clumps(0, B, G, seed=2)
    x0, cl, rt = T(X0, dev), T(D.line_centerline(), dev), T(radius, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    lam = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
    opp = torch.zeros(B, 2, dtype=torch.int32, device=dev)

    def loop(eng, B=B, Tn=1, G=G, radius=rt, reach=INF, table=table):
        return eng.lib.mpc_closed_loop_traffic(eng._h, B, Tn, 0, G, p(radius), float(reach), p(x0), p(cl), None, p(U0), p(lam), p(table),
                                               None, None, None, None, None, None, eng._stream())

    def select(eng, B=B, G=G, Nst=1, radius=rt, reach=INF):
        return eng.lib.mpc_opponents_from_plans(eng._h, B, G, Nst, p(x0), p(radius), float(reach), p(opp), None, eng._stream())

    def refused(rc, who, words):
        msg = _lib.load().mpc_last_error().decode()
        assert rc == -1 and msg.startswith(who + ": ") and words in msg, (rc, msg)
    # a handle of another constr_mode: the loop is refused, the selection is served
    for mode in (mp.CONSTR_NONE, mp.CONSTR_STATE_SQ, mp.CONSTR_LANE):
        other = engine(dev, 0, N, mode=mode)
        refused(loop(other), "mpc_closed_loop_traffic", "constr_mode is not MPC_CONSTR_DISCS")
        assert select(other) == 0
        with pytest.raises(mp.MpcError, match="mpc_closed_loop_traffic: .*MPC_CONSTR_DISCS"):
            other.closed_loop_traffic(x0, cl, U0, 1, G, rt, table=table)
        with pytest.raises(mp.MpcError, match="mpc_closed_loop_traffic: .*MPC_CONSTR_DISCS"):
            other.closed_loop_traffic(x0, cl, U0, 1, G, rt)                # no table made or bound for such a handle
        assert not other.agent_discs_bound
        other.close()
    eng = engine(dev, 0, N, max_total_inner=300)
    refused(loop(eng), "mpc_closed_loop_traffic", "no disc table is bound (mpc_set_agent_discs)")
    # a bound table with P != B
    half = torch.zeros(B // 2, 6 * N, dtype=torch.float64, device=dev)
    eng.set_agent_discs(half, T(np.arange(B) // 2, dev, torch.int32))
    refused(loop(eng, table=half), "mpc_closed_loop_traffic", "has 6 rows, the loop needs one per agent")
    eng.set_agent_discs(table, arange32(B, dev))
    refused(loop(eng, table=table.clone()), "mpc_closed_loop_traffic", "must be the disc table that is bound")
    refused(loop(eng, table=None), "mpc_closed_loop_traffic", "must be the disc table that is bound")
    for fn, who in ((loop, "mpc_closed_loop_traffic"), (select, "mpc_opponents_from_plans")):
        for kw, words in ((dict(G=5), "B % G"), (dict(G=0), "scene size G"), (dict(G=65), "scene size G"), (dict(radius=None), "null radius"),
                          (dict(reach=-0.5), "reach must be >= 0"), (dict(reach=float("nan")), "reach must be >= 0"),
                          (dict(B=6, G=3), "the bound disc table is for a batch of 12 agents, this call has 6")):
            refused(fn(eng, **kw), who, words)
    refused(loop(eng, Tn=-1), "mpc_closed_loop_traffic", "negative T")
    refused(select(eng, Nst=0), "mpc_opponents_from_plans", "Nst must be >= 1")
    # the front end says the same before the library is asked
    for kw in (dict(G=5), dict(G=0), dict(G=65), dict(reach=-1.0), dict(reach=float("nan"))):
        with pytest.raises(ValueError):
            eng.closed_loop_traffic(x0, cl, U0, 1, **{**dict(G=G, radius=rt, table=table), **kw})
        with pytest.raises(ValueError):
            eng.opponents_from_plans(x0, **{**dict(G=G, radius=rt), **kw})
    with pytest.raises(ValueError):
        eng.closed_loop_traffic(x0, cl, U0, -1, G, rt, table=table)
    for run in (lambda **kw: eng.closed_loop(x0, cl, U0, 1, **kw), lambda **kw: eng.closed_loop_traffic(x0, cl, U0, 1, G, rt, table=table, **kw)):
        with pytest.raises(ValueError, match="lam"):
            run(lam=lam[:, :-1].contiguous())                              # a lam of the wrong width: every loop, the plain one too
    # while solve_async is in flight
    wait = eng.solve_async(x0, cl, U0)
    refused(loop(eng), "mpc_closed_loop_traffic", "a solve of this handle is in flight")
    refused(select(eng), "mpc_opponents_from_plans", "a solve of this handle is in flight")
    with pytest.raises(mp.MpcError):
        eng.opponents_from_plans(x0, G, rt)
    wait()
    assert loop(eng) == 0 and select(eng) == 0                     # ... and afterwards both are served
    torch.cuda.synchronize()
    eng.close()
