"""GPU tests of the masked solve and the event-triggered closed loop (mpc_solve_active, mpc_trigger_eval,
mpc_closed_loop_event).  Agents are independent -- a sliced batch gives the sliced result bit for bit
(tests/test_gpu_parity.py, tests/test_gpu_agent_params.py) -- so the new paths are compared EXACTLY with existing entry
points: the masked solve with the solve of the whole batch, the loop at thr = 0 with mpc_closed_loop, at thr = inf with
mpc_rollout, in general with a host loop built from solve_active, trigger_eval and rollout; and with the CPU oracle's
mirror loop (tests/event_loop_common.py) on the configuration tests/test_event_loop_cpu.py checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import event_loop_common as E
from conftest import straight_centerline, circle_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(a, dev, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def same_bits(a, b):
    """bit equality of two float64 tensors (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


STATE_SQ = dict(constr_mode=1, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], Sigma0=10.0)


def hetero_table(cfg, model, P, seed):
    """P rows around the handle's values (row 0: the handle's own)"""
    rng = np.random.default_rng(seed)
    base = _lib.default_params(cfg)
    kw = dict(v_ref=base[24] * np.r_[1.0, rng.uniform(.7, 1.3, P - 1)],
              cost_w=base[25:31] * np.vstack([np.ones(6), rng.uniform(.7, 1.4, (P - 1, 6))]))
    if model == 0:
        kw.update(accel=base[22] * np.r_[1.0, rng.uniform(.75, 1.25, P - 1)],
                  friction=base[23] * np.r_[1.0, rng.uniform(.7, 1.3, P - 1)])
    else:
        veh = np.tile(base[:22], (P, 1))
        veh[1:, 7] *= rng.uniform(.9, 1.1, P - 1); veh[1:, 8] *= rng.uniform(.9, 1.1, P - 1)
        kw.update(veh=veh)
    return _lib.param_rows(cfg, P, **kw)


# ----------------------------------------------------------------------------- 1. masked solve
def masked_solve_case(dev, model, constr, table, B, inner, masks, two_centerlines=False):
    N = 10 if constr else (20 if model == 0 else 12)
    kw = dict(STATE_SQ) if constr else {}
    cfg = mp.default_config(model, N, max_total_inner=inner, **kw)
    eng = mp.BatchedMPC(cfg, dev)
    X0 = synthetic_states(model, B, seed=21)
    if constr:
        X0[:, 0] *= 3.9 / 5.0
        X0[:, 3] = np.minimum(X0[:, 3], 0.65)
    rng = np.random.default_rng(B + 7 * model + 3 * constr)
    cl, ci = T(straight_centerline(), dev), None
    if two_centerlines:
        cl = T(np.stack([straight_centerline(), circle_centerline()]), dev)
        ci = T(rng.integers(0, 2, B), dev, torch.int32)
    x0, U0 = T(X0, dev), T(np.tile([1., 0.], (B, N)), dev)
    keep = None
    if table:
        P = 5
        keep = (T(hetero_table(cfg, model, P, 3), dev), T(rng.integers(0, P, B), dev, torch.int32))
        eng.set_agent_params(*keep)
    Uf, lamf, stf = eng.solve(x0, cl, U0, cl_index=ci)
    for name, mask in masks(rng, B):
        mk = T(mask, dev, torch.bool)
        Uin, stin = U0.clone(), torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev)
        Uin[~mk] = float("nan")                       # rows of agents that are not solved: never read, never written
        lamin = None
        if eng.m:
            lamin = torch.zeros(B, eng.m, dtype=torch.float64, device=dev)
            lamin[~mk] = float("nan")
        U, lam, st, n = eng.solve_active(x0, cl, Uin, mk, lam=lamin, cl_index=ci, stats=stin)
        assert n == int(mask.sum()), name
        assert same_bits(U, torch.where(mk[:, None], Uf, Uin)), name
        assert same_bits(st, torch.where(mk[:, None], stf, stin)), name
        if eng.m:
            assert same_bits(lam, torch.where(mk[:, None], lamf, lamin)), name
        if n == 0:
            assert same_bits(U, Uin) and same_bits(st, stin)
        if n == B:
            assert same_bits(U, Uf) and same_bits(st, stf)
    del keep
    eng.close()


def small_masks(rng, B):
    return [("half", rng.random(B) < 0.5), ("tenth", rng.random(B) < 0.1), ("ones", np.ones(B, bool)),
            ("zeros", np.zeros(B, bool)), ("last", np.arange(B) == B - 1)]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("model,constr", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_masked_solve_equals_whole_batch_solve(dev, model, constr, table, B):
    """solve_active == solve of the whole batch followed by torch.where(mask, new, old), bit for bit on U, lambda and
    stats; all ones == mpc_solve_batch; all zeros changes nothing and reports 0; rows that are not solved keep their
    NaNs.  (The iteration budget is short: equality of bits does not need converged agents.)"""
    masked_solve_case(dev, model, constr, table, B, 300, small_masks, two_centerlines=(B == 65 and not table))


@pytest.mark.parametrize("model,constr,table", [(0, 0, False), (0, 0, True), (1, 0, False), (1, 0, True), (0, 1, False)])
def test_masked_solve_65536_agents(dev, model, constr, table):
    """A mask of about 10 % (6.5 thousand agents: beyond the batch that starts in the persistent kernel, one group on
    the round path that hands over to it), of a half (three groups) and of all agents (four groups) of 65 536."""
    def masks(rng, B):
        return [("tenth", rng.random(B) < 0.1), ("half", rng.random(B) < 0.5), ("ones", np.ones(B, bool)),
                ("zeros", np.zeros(B, bool))]
    masked_solve_case(dev, model, constr, table, 65536, 5000 if (model == 0 and not constr) else 300, masks)


# ----------------------------------------------------------------------------- 2. trigger
def np_trigger(x, xh, held, w, thr, max_hold):
    """event_loop_common.trigger, vectorised: the same IEEE operations in the same order"""
    e = x - xh
    e[:, 2] = e[:, 2] - E.TWO_PI * np.rint(e[:, 2] / E.TWO_PI)
    d2 = np.zeros(len(x))
    for i in range(x.shape[1]):
        d2 = d2 + w[i] * (e[:, i] * e[:, i])
    return d2, (held < 0) | (held >= max_hold) | ~(d2 < thr * thr)


@pytest.mark.parametrize("model", [0, 1])
def test_trigger_eval_matches_numpy(dev, model):
    B, max_hold, thr = 4096, 7, 0.05
    cfg = mp.default_config(model, 12)
    eng = mp.BatchedMPC(cfg, dev)
    nx = eng.nx
    rng = np.random.default_rng(5 + model)
    with np.errstate(invalid="ignore"):
        x = synthetic_states(model, B, seed=2)
        xh = x + rng.normal(0, thr / np.sqrt(nx), (B, nx))          # dev2 on both sides of thr^2
        w = rng.uniform(0.2, 3.0, nx)
        held = rng.integers(0, max_hold, B)
        held[:64] = -1                                                    # no plan yet
        held[64:128] = max_hold                                           # the hold limit
        x[128:256, 2] += E.TWO_PI * rng.integers(-3, 4, 128)              # whole turns of heading: no deviation
        x[256:272, rng.integers(0, nx, 16)] = np.nan                      # a non-finite dev2 fires
        x[272:280, 0] = np.inf
        d2, fire = np_trigger(x.copy(), xh, held, w, thr, max_hold)
        # the decisions are compared where they do not hang on the last bits: nudge what lies within 1e-9 of thr^2
        close = np.isfinite(d2) & (np.abs(d2 - thr * thr) <= 1e-9 * thr * thr)
        xh[close] = x[close]
        d2, fire = np_trigger(x.copy(), xh, held, w, thr, max_hold)
        assert not (np.isfinite(d2) & (np.abs(d2 - thr * thr) <= 1e-9 * thr * thr)).any()
        assert 0.1 < fire[280:].mean() < 0.9                              # the threshold cuts through the sample
    dd, df = eng.trigger_eval(T(x, dev), T(xh, dev), T(held, dev, torch.int32), w, thr, max_hold)
    dd, df = dd.cpu().numpy(), df.cpu().numpy()
    fin = np.isfinite(d2)
    assert np.array_equal(np.isfinite(dd), fin)
    ulps = np.abs(dd[fin] - d2[fin]) / np.spacing(np.abs(d2[fin]))
    print(f"model {model}: dev2 max {ulps.max():.1f} ulp from numpy")
    assert ulps.max() <= 4
    assert np.array_equal(df != 0, fire)
    assert df[:128].all() and df[256:280].all() and set(np.unique(df)) == {0, 1}
    # thr = 0 always fires; thr = inf leaves the hold limit (and the non-finite deviations)
    _, f0 = eng.trigger_eval(T(x, dev), T(xh, dev), T(held, dev, torch.int32), w, 0.0, max_hold)
    assert bool(f0.all())
    _, fi = eng.trigger_eval(T(x, dev), T(xh, dev), T(held, dev, torch.int32), w, float("inf"), max_hold)
    assert np.array_equal(fi.cpu().numpy() != 0, (held < 0) | (held >= max_hold) | ~fin)
    for bad in (dict(thr=-1.0, max_hold=3), dict(thr=0.1, max_hold=0), dict(thr=0.1, max_hold=13)):
        with pytest.raises(ValueError):
            eng.trigger_eval(T(x, dev), T(xh, dev), T(held, dev, torch.int32), w, **bad)
    wv = (C.c_double * nx)(*w)
    p = lambda t: C.c_void_p(t.data_ptr())
    a, b, c, d = T(x, dev), T(xh, dev), T(held, dev, torch.int32), torch.zeros(B, dtype=torch.int32, device=dev)
    assert eng.lib.mpc_trigger_eval(eng._h, B, p(a), p(b), p(c), wv, 0.1, 13, None, p(d), None) == -1   # max_hold > N
    assert eng.lib.mpc_trigger_eval(eng._h, B, p(a), p(b), p(c), wv, 0.1, 12, None, p(d), None) == 0    # dev2 may be NULL
    eng.close()


# ----------------------------------------------------------------------------- 3. thr = 0 is mpc_closed_loop
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_threshold_zero_is_the_closed_loop(dev, model, N, shift):
    B, Tn = 192, 7
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    x0, cl = T(synthetic_states(model, B, seed=8), dev), T(straight_centerline(), dev)
    U0 = T(np.tile([1., 0.], (B, N)), dev)
    xr, _, _, txr, tur, failr, _ = eng.closed_loop(x0, cl, U0, Tn, shift=shift)
    r = eng.closed_loop_event(x0, cl, U0, Tn, np.ones(eng.nx), 0.0, 3, shift=shift)
    assert same_bits(r.traj_x, txr) and same_bits(r.traj_u, tur) and same_bits(r.x, xr)
    assert torch.equal(r.failures, failr)
    assert bool((r.solved == 1).all()) and bool((r.solve_count == Tn).all()) and bool((r.held == 1).all())
    eng.close()


# ----------------------------------------------------------------------------- 4. thr = inf: the hold limit alone
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_infinite_threshold_replans_every_N_steps_and_rolls_the_plan_out(dev, model, N):
    B, Tn, P = 96, 2 * N + 5, 4
    cfg = mp.default_config(model, N, max_total_inner=1500)
    eng = mp.BatchedMPC(cfg, dev)
    rng = np.random.default_rng(11)
    tab = T(hetero_table(cfg, model, P, 4), dev)
    idx, pidx = T(rng.integers(0, P, B), dev, torch.int32), T(rng.integers(0, P, B), dev, torch.int32)
    x0, cl = T(synthetic_states(model, B, seed=9), dev), T(straight_centerline(), dev)
    U0 = T(np.tile([1., 0.], (B, N)), dev)
    eng.set_agent_params(tab, idx, pidx)
    r = eng.closed_loop_event(x0, cl, U0, Tn, np.ones(eng.nx), float("inf"), N, shift=True)
    want = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    want[:, ::N] = 1
    assert torch.equal(r.solved, want) and bool((r.solve_count == 3).all()) and bool((r.held == 5).all())
    eng.set_agent_params(tab, pidx)                    # mpc_rollout on the PLANT's rows
    for k in range(3):
        lo, hi = k * N, min(Tn, (k + 1) * N)
        start = x0 if k == 0 else r.traj_x[:, lo - 1].contiguous()
        plan = r.traj_u[:, lo:hi].reshape(B, 2 * (hi - lo)).contiguous()      # the stages applied ARE the plan's
        assert same_bits(r.traj_x[:, lo:hi], eng.rollout(start, plan)), k
    assert same_bits(r.U[:, :10], r.traj_u[:, 2 * N:].reshape(B, 10))             # U: the plan as last solved
    eng.close()


# ----------------------------------------------------------------------------- 5. the general case
def host_event_loop(eng, x, cl, U, Tn, w, thr, max_hold, shift, held=None, plant=None, dist=None, stats=None):
    """mpc_closed_loop_event from the host: trigger_eval, the shift in torch, solve_active, rollout(Nsim = 1).
    plant = (table, index, plant_index) when a table is bound (rebound around the plant's step)."""
    B, N, nx, dev = x.shape[0], eng.N, eng.nx, x.device
    x, U = x.clone(), U.clone()
    held = torch.full((B,), -1, dtype=torch.int32, device=dev) if held is None else held.clone()
    xhat = torch.zeros_like(x)
    stats = torch.zeros(B, 8, dtype=torch.float64, device=dev) if stats is None else stats.clone()
    solved = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    tx, tu = torch.zeros(B, Tn, nx, dtype=torch.float64, device=dev), torch.zeros(B, Tn, 2, dtype=torch.float64, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    ar = torch.arange(B, device=dev)
    stage = torch.arange(N, device=dev)
    for t in range(Tn):
        _, fire = eng.trigger_eval(x, xhat, held, w, thr, max_hold)
        fb = fire != 0
        if shift:
            src = torch.clamp(stage[None, :] + torch.clamp(held, min=0)[:, None].long(), max=N - 1)
            Us = torch.gather(U.view(B, N, 2), 1, src[:, :, None].expand(B, N, 2)).reshape(B, 2 * N)
            U = torch.where(fb[:, None], Us, U)
        U, _, stats, n = eng.solve_active(x, cl, U, fire, stats=stats)
        assert n == int(fb.sum())
        held = torch.where(fb, torch.zeros_like(held), held)
        xhat = torch.where(fb[:, None], x, xhat)
        u = U.view(B, N, 2)[ar, held.long()].contiguous()
        if plant is not None:
            eng.set_agent_params(plant[0], plant[2])
        xn = eng.rollout(x, u)[:, 0]
        if plant is not None:
            eng.set_agent_params(*plant)
        x = (xn + dist[:, t]) if dist is not None else xn
        x = x.contiguous()
        xhat = eng.rollout(xhat, u)[:, 0].contiguous()
        held = held + 1
        solved[:, t], tx[:, t], tu[:, t] = fb.to(torch.uint8), x, u
        count += fb.to(torch.int32)
    return dict(x=x, U=U, held=held, solved=solved, traj_x=tx, traj_u=tu, solve_count=count, stats=stats)


def general_case(dev, B, Tn, kind, split=None):
    N, model, thr, max_hold = 20, 0, 0.02, 10
    cfg = mp.default_config(model, N, max_total_inner=1500)
    eng = mp.BatchedMPC(cfg, dev)
    x0, cl = T(synthetic_states(model, B, seed=13), dev), T(straight_centerline(), dev)
    U0, w = T(np.tile([1., 0.], (B, N)), dev), np.array([1.0, 1.0, 0.5, 0.25])
    plant, dist = None, None
    if kind == "plant_index":
        tab = T(_lib.param_rows(cfg, 3, accel=[2.0, 2.0 * 0.97, 2.0 * 1.02], friction=[1.0, 1.1, 0.93]), dev)
        plant = (tab, torch.zeros(B, dtype=torch.int32, device=dev), T(1 + np.arange(B) % 2, dev, torch.int32))
        eng.set_agent_params(*plant)
    else:
        dist = T(np.random.default_rng(17).normal(0, 4e-3, (B, Tn, 4)) * [1, 1, 0.5, 2], dev)
    r = eng.closed_loop_event(x0, cl, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist)
    hl = host_event_loop(eng, x0, cl, U0, Tn, w, thr, max_hold, True, plant=plant, dist=dist)
    frac = float(r.solved.float().mean())
    print(f"B {B} {kind}: solve fraction {frac:.3f}")
    assert 0.05 < frac < 0.9                           # neither of the two limits the other tests cover
    assert torch.equal(r.solved, hl["solved"]) and torch.equal(r.held, hl["held"])
    assert torch.equal(r.solve_count, hl["solve_count"]) and torch.equal(r.solve_count, r.solved.sum(1).to(torch.int32))
    assert same_bits(r.traj_x, hl["traj_x"]) and same_bits(r.traj_u, hl["traj_u"]) and same_bits(r.x, hl["x"])
    assert same_bits(r.U, hl["U"]) and same_bits(r.stats, hl["stats"])
    if split:
        a = eng.closed_loop_event(x0, cl, U0, split, w, thr, max_hold, shift=True,
                                  disturbance=None if dist is None else dist[:, :split].contiguous())
        b = eng.closed_loop_event(a.x, cl, a.U, Tn - split, w, thr, max_hold, held=a.held, shift=True, stats=a.stats,
                                  disturbance=None if dist is None else dist[:, split:].contiguous())
        assert same_bits(torch.cat([a.traj_x, b.traj_x], 1), r.traj_x) and same_bits(torch.cat([a.traj_u, b.traj_u], 1), r.traj_u)
        assert torch.equal(torch.cat([a.solved, b.solved], 1), r.solved) and torch.equal(a.solve_count + b.solve_count, r.solve_count)
        assert torch.equal(a.failures + b.failures, r.failures) and torch.equal(b.held, r.held)
        assert same_bits(b.x, r.x) and same_bits(b.U, r.U) and same_bits(b.stats, r.stats)
    eng.close()


@pytest.mark.parametrize("kind", ["plant_index", "disturbance"])
def test_event_loop_equals_host_loop_4096_agents(dev, kind):
    """... and a call with T = 25 followed by one with T = 15 equals one call with T = 40"""
    general_case(dev, 4096, 40, kind, split=25)


def test_event_loop_equals_host_loop_65536_agents(dev):
    general_case(dev, 65536, 16, "plant_index")


# ----------------------------------------------------------------------------- 6. the oracle
# The bound on |traj_x(HIP) - traj_x(oracle)|: two orders above the larger of (a) that difference as measured on the
# MI355X (4.0e-10 at thr = 0.01, 6.8e-10 at thr = 0.03: profiles/r09_event_loop.txt) and (b) the difference of two
# oracle runs whose evaluations differ by two ulps, 1.3e-10.
HIP_VS_ORACLE_TRAJ_X = 6.8e-10
JITTERED_ORACLE_TRAJ_X = 1.3e-10
TRAJ_X_BOUND = 100.0 * max(HIP_VS_ORACLE_TRAJ_X, JITTERED_ORACLE_TRAJ_X)


@pytest.mark.parametrize("thr", E.THRESHOLDS)
def test_event_loop_matches_oracle_mirror(dev, O, thr):
    X0, cl, U0, w = E.case()
    cc = O.default_config(O.MODEL_KINEMATIC, E.N, **E.SOLVER)
    pc = O.default_config(O.MODEL_KINEMATIC, E.N, **E.SOLVER, **E.PLANT)
    ref = E.mirror_loop(O, cc, pc, X0, cl, U0, w, thr, E.MAX_HOLD, E.SHIFT, E.T)
    assert ref["margin"] > 1e-3, ref["margin"]        # no decision of the oracle hangs on what two solvers differ by
    assert ref["fails"].sum() == 0
    cfg = mp.default_config(mp.MODEL_KINEMATIC, E.N, **E.SOLVER)
    eng = mp.BatchedMPC(cfg, dev)
    tab = T(_lib.param_rows(cfg, 2, accel=[2.0, E.PLANT["accel"]], friction=[1.0, E.PLANT["friction"]]), dev)
    zero, one = torch.zeros(E.B, dtype=torch.int32, device=dev), torch.ones(E.B, dtype=torch.int32, device=dev)
    eng.set_agent_params(tab, zero, one)
    r = eng.closed_loop_event(T(X0, dev), T(cl, dev), T(U0, dev), E.T, w, thr, E.MAX_HOLD, shift=bool(E.SHIFT))
    tx, tu = r.traj_x.cpu().numpy(), r.traj_u.cpu().numpy()
    du = np.abs(tu - ref["traj_u"]).max((1, 2)) / np.maximum(1.0, np.abs(ref["traj_u"]).max((1, 2)))
    dx = np.abs(tx - ref["traj_x"]).max()
    print(f"thr {thr}: solve fraction {r.solved.float().mean():.4f}, max rel |traj_u - oracle| = {du.max():.3e}, "
          f"max |traj_x - oracle| = {dx:.3e} (bound {TRAJ_X_BOUND:.1e})")
    assert np.array_equal(r.solved.cpu().numpy() != 0, ref["solved"])
    assert np.array_equal(r.held.cpu().numpy(), ref["held"]) and int(r.failures.sum()) == 0
    assert du.max() <= 1e-5
    assert dx <= TRAJ_X_BOUND
    eng.close()
