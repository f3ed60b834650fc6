"""GPU tests of the input-rate cost (mpc_set_agent_rates / BatchedMPC.set_agent_rates): a table of per-agent move penalties
[w_d, w_delta, d_prev, delta_prev] in device memory and one row index per agent; stage k's cost gets
w_d (d_k - d_{k-1})^2 + w_delta (delta_k - delta_{k-1})^2 with u_{-1} the row's, and the closed loops carry u_{-1} forward
themselves.  The oracle does not know the term: the checker is the numpy restatement of tests/rate_common.py on the
oracle's calls; the reference solves are recorded in tests/golden/rates_reference.npz.  Shapes: N = 1 (u_{-1} alone),
N = 2, kinematic N = 20, Pacejka N = 12, kinematic N = 40 (two elements per lane), B = 130 (no multiple of 64), P = 3 rows
with a scattered index.  The tolerances are the project's HIP-vs-oracle bars and its bar between two
correct solvers (bench.DU_METRIC)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from agent_tables_common import T, box_rows_of, kwl, param_rows_of, table_of
from conftest import GOLDEN

import discs_common as D
import rate_common as R

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402

DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)     # of tests/test_gpu_agent_discs.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def arange32(B, dev):
    return torch.arange(B, dtype=torch.int32, device=dev)


def du_metric(U, Uref):
    return np.abs(U - Uref).max(1) / np.maximum(1.0, np.abs(Uref).max(1))


def rate_table(P, seed, zero_weights=False):
    """P rows: weights in [0, 1] x [0, 5] (row 0: w_d = 0, the drive is free), u_prev in the handle's box"""
    rng = np.random.default_rng(seed)
    wd, wl = rng.uniform(0.05, 1.0, P), rng.uniform(0.2, 5.0, P)
    wd[0] = 0.0
    if zero_weights:
        wd[:], wl[:] = 0.0, 0.0
    return _lib.rate_rows(wd, wl, np.stack([rng.uniform(-1.0, 1.0, P), rng.uniform(-0.32, 0.32, P)], 1))


def eval_case(model, N, B, seed=3):
    """B agents around the line y = 0.5 that starts at x = 0.9, inputs that move from stage to stage"""
    rng = np.random.default_rng(seed)
    cols = [rng.uniform(1.0, 4.0, B), 0.5 + rng.uniform(-.15, .15, B), rng.uniform(-.2, .2, B), rng.uniform(.4, 1.2, B)]
    if model == 1:
        cols += [rng.uniform(-.03, .03, B), rng.uniform(-.3, .3, B)]
    U = np.tile([0.6, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1.0, 0.3], N)
    return np.stack(cols, 1), D.line_centerline(), U


# ----------------------------------------------------------------------------- 1. evaluation
def every_route(dev, monkeypatch, make_engine, bind, args, B, cl):
    """psi, grad, yhat of the fused route; asserts that the wave evaluation, the two-kernel route (an engine of its own
    under MPC_UNFUSED_EVAL), per-agent centerline rows and cost-only requests give the same bits"""
    eq = lambda a, b: (a is None and b is None) or torch.equal(a, b)
    ci = T(np.arange(B) % 3, dev, torch.int32)
    cl3 = T(np.tile(cl, (3, 1)), dev)
    eng = make_engine()
    bind(eng)
    psi, grad, yhat = eng.eval_cost_grad(*args)
    for kw in (dict(wave=True), dict(cl_index=ci), dict(cl_index=ci, wave=True)):
        a = list(args)
        if "cl_index" in kw:
            a[1] = cl3
        p2, g2, y2 = eng.eval_cost_grad(*a, **kw)
        assert torch.equal(psi, p2) and torch.equal(grad, g2) and eq(yhat, y2), kw
    for wave in (False, True):
        p3, _, y3 = eng.eval_cost_grad(*args, want_grad=False, wave=wave)
        assert torch.equal(psi, p3) and eq(yhat, y3)
    eng.close()
    monkeypatch.setenv("MPC_UNFUSED_EVAL", "1")
    eng = make_engine()
    monkeypatch.delenv("MPC_UNFUSED_EVAL")
    bind(eng)
    for c in (None, ci):
        p4, g4, y4 = eng.eval_cost_grad(args[0], args[1] if c is None else cl3, *args[2:], cl_index=c)
        assert torch.equal(psi, p4) and torch.equal(grad, g4) and eq(yhat, y4)
    eng.close()
    return psi.cpu().numpy(), grad.cpu().numpy(), None if yhat is None else yhat.cpu().numpy()


@pytest.mark.parametrize("model,N", [(0, 1), (0, 2), (0, 20), (1, 12), (0, 40)])
def test_evaluation_matches_the_checker_and_every_route_agrees(dev, O, monkeypatch, model, N):
    """130 agents on 3 rows through a scattered index.  psi within 1e-12 relative and the gradient within 1e-9 of
    ||grad psi|| of the checker, agent by agent; the routes bit-equal.  Fails on a library without the entry point."""
    B, P = 130, 3
    X0, cl, U = eval_case(model, N, B)
    rows = rate_table(P, seed=5)
    idx = np.random.default_rng(6).integers(0, P, B)
    assert set(idx) == {0, 1, 2}
    args = (T(X0, dev), T(cl, dev), T(U, dev))
    psi, grad, _ = every_route(dev, monkeypatch, lambda: mp.BatchedMPC(mp.default_config(model, N), dev),
                               lambda e: e.set_agent_rates(T(rows, dev), T(idx, dev, torch.int32)), args, B, cl)
    ocfg = O.default_config(model, N)
    worst, share = [0.0, 0.0], 0.0
    for b in range(B):
        p, g = R.psi(O, ocfg, X0[b], cl, U[b], rows[idx[b]])
        worst[0] = max(worst[0], abs(psi[b] - p) / abs(p))
        worst[1] = max(worst[1], np.abs(grad[b] - g).max() / np.linalg.norm(g))
        share = max(share, R.rate_term(U[b], rows[idx[b]])[0] / p)
    print(f"model {model} N {N}: worst psi {worst[0]:.2e} grad {worst[1]:.2e}; the term is up to {share:.2f} of psi")
    assert share > 0.01                                    # the term does act
    assert worst[0] <= 1e-12 and worst[1] <= 1e-9


def test_evaluation_on_a_lane_handle(dev, O, monkeypatch):
    """CONSTR_LANE with the handle's own half-width (0.05: the band is active), multipliers of both signs"""
    model, N, B, P = 0, 20, 130, 3
    X0, cl, U = eval_case(model, N, B, seed=8)
    rng = np.random.default_rng(9)
    y, Sig = rng.uniform(-2.0, 2.0, (B, N)), 10 ** rng.uniform(0, 3, (B, N))
    rows = rate_table(P, seed=10)
    idx = rng.integers(0, P, B)
    kw = dict(constr_mode=mp.CONSTR_LANE, lane_halfwidth=0.05)
    args = (T(X0, dev), T(cl, dev), T(U, dev), T(y, dev), T(Sig, dev))
    psi, grad, yhat = every_route(dev, monkeypatch, lambda: mp.BatchedMPC(mp.default_config(model, N, **kw), dev),
                                  lambda e: e.set_agent_rates(T(rows, dev), T(idx, dev, torch.int32)), args, B, cl)
    ocfg = O.default_config(model, N, constr_mode=O.CONSTR_LANE, lane_halfwidth=0.05)
    worst = [0.0, 0.0]
    for b in range(B):
        p, g = R.psi(O, ocfg, X0[b], cl, U[b], rows[idx[b]], y[b], Sig[b])
        worst[0] = max(worst[0], abs(psi[b] - p) / abs(p))
        worst[1] = max(worst[1], np.abs(grad[b] - g).max() / np.linalg.norm(g))
    print(f"lane: worst psi {worst[0]:.2e} grad {worst[1]:.2e}; {int((yhat != 0).sum())} active of {yhat.size}")
    assert (yhat != 0).sum() >= B
    assert worst[0] <= 1e-12 and worst[1] <= 1e-9


def disc_eval_case(B, N, seed):
    """tests/test_gpu_agent_discs.py eval_case: discs from ones the plan runs through to r = 0"""
    X0, cl, U = eval_case(0, N, B, seed)
    rng = np.random.default_rng(seed + 100)
    discs = np.zeros((B, N, 2, 3))
    ahead = 0.05 * np.arange(1, N + 1)[None, :, None] * X0[:, 3][:, None, None]
    discs[..., 0] = X0[:, 0][:, None, None] + ahead + rng.uniform(-.15, .15, (B, N, 2))
    discs[..., 1] = X0[:, 1][:, None, None] + rng.uniform(-.15, .15, (B, N, 2))
    discs[..., 2] = rng.uniform(0.0, 0.25, (B, N, 2)) * (rng.uniform(size=(B, N, 2)) < 0.7)
    return X0, cl, U, discs, rng.uniform(-2.0, 0.5, (B, 2 * N)), 10 ** rng.uniform(0, 3, (B, 2 * N))


def test_evaluation_on_a_disc_handle(dev, O, monkeypatch):
    """CONSTR_DISCS with active discs: the DiscTab + RateTab forms"""
    model, N, B, P = 0, 20, 130, 3
    X0, cl, U, discs, y, Sig = disc_eval_case(B, N, seed=12)
    rows = rate_table(P, seed=13)
    idx = np.random.default_rng(14).integers(0, P, B)
    args = (T(X0, dev), T(cl, dev), T(U, dev), T(y, dev), T(Sig, dev))

    def bind(e):
        e.set_agent_discs(T(discs.reshape(B, -1), dev), arange32(B, dev))
        e.set_agent_rates(T(rows, dev), T(idx, dev, torch.int32))
    psi, grad, yhat = every_route(dev, monkeypatch, lambda: mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS), dev),
                                  bind, args, B, cl)
    cfgs = D.configs(O, model, N)
    worst, nact = [0.0, 0.0, 0.0], 0
    for b in range(B):
        p, yh, g, _ = R.psi_discs(O, cfgs, X0[b], cl, U[b], discs[b], y[b], Sig[b], rows[idx[b]])
        nact += int((yh < 0).sum())
        worst[0] = max(worst[0], abs(psi[b] - p) / abs(p))
        worst[1] = max(worst[1], np.abs(yhat[b] - yh).max() / max(1e-300, np.abs(yh).max()))
        worst[2] = max(worst[2], np.abs(grad[b] - g).max() / np.linalg.norm(g))
    print(f"discs: {nact} active of {B * 2 * N}; worst psi {worst[0]:.2e} yhat {worst[1]:.2e} grad {worst[2]:.2e}")
    assert nact >= B
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-9


# ----------------------------------------------------------------------------- 2. zero weights are no table
@pytest.mark.parametrize("model,N,B,mode", [(0, 20, 256, mp.CONSTR_NONE), (1, 12, 128, mp.CONSTR_NONE), (0, 20, 64, mp.CONSTR_DISCS)])
def test_zero_weights_are_no_table(dev, model, N, B, mode):
    """w = 0 with any finite u_prev: U, lambda and all eight statistics columns of solve are those of the solve without a
    table (the persistent kernel from the start; kinematic: the rounds too)"""
    X0, cl, U0 = eval_case(model, N, B, seed=20)
    kw = dict(max_total_inner=3000)
    if mode == mp.CONSTR_DISCS:
        kw.update(Sigma0=10.0)
        X0 = np.tile(D.X0_KIN, (B, 1))
        discs = np.stack([D.scene_standing(N, D.scene_shifts()[b % D.NSHIFT]) for b in range(B)])
    rows = rate_table(B, seed=21, zero_weights=True)
    assert not rows[:, :2].any() and np.abs(rows[:, 2:]).min() > 0
    x0, clt, Ut = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, **kw), dev)
    if mode == mp.CONSTR_DISCS:
        eng.set_agent_discs(T(discs.reshape(B, -1), dev), arange32(B, dev))
    for solo_max in ((None, 0) if model == 0 and mode == mp.CONSTR_NONE else (None,)):
        if solo_max is not None:
            eng.set_solo_max(solo_max)
        base = eng.solve(x0, clt, Ut)
        eng.set_agent_rates(T(rows, dev), T(np.random.default_rng(22).permutation(B), dev, torch.int32))
        got = eng.solve(x0, clt, Ut)
        eng.clear_agent_rates()
        assert bool((base[2][:, 0] == 1).sum() >= B // 2)
        assert torch.equal(base[0], got[0]) and torch.equal(base[2], got[2]), solo_max
        assert (base[1] is None and got[1] is None) or torch.equal(base[1], got[1])
    eng.close()


# ----------------------------------------------------------------------------- 3. the solve
@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "rates_reference.npz"))
    assert np.array_equal(ref["weights"], np.array(R.WEIGHTS))
    assert np.array_equal(ref["u_prev_kin"], R.scene_agents(0)[1]) and np.array_equal(ref["u_prev_moving"], R.disc_scene_agents()[2])
    return ref


@pytest.mark.parametrize("wi", [0, 1])
def test_solve_against_the_reference_solve(dev, wi):
    """The scene of the issue: kinematic N = 20, the car at (1.0, 0.62 +- small shifts) with v = 0.5 beside the line y = 0.5,
    16 agents, u_prev drawn in the box (agent 0: u_prev = 0, no shift), alm_eps = 1e-10, start U = 0 as the reference
    solve.  Controls within 1e-5 on bench.DU_METRIC.  With (0.5, 5.0) the first applied drive of agent 0 is below 0.6
    (the CPU figure is 0.488); with weights (0, 0) it is the bound 1.0."""
    N, B = 20, R.NAGENT
    X0, up = R.scene_agents(0)
    w = R.WEIGHTS[wi]
    eng = mp.BatchedMPC(mp.default_config(0, N, alm_eps=1e-10, max_total_inner=20000), dev)
    x0, cl, U0 = T(X0, dev), T(D.line_centerline(), dev), torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    eng.set_agent_rates(T(_lib.rate_rows(w[0], w[1], up), dev), arange32(B, dev))
    U, _, st = eng.solve(x0, cl, U0)
    eng.set_agent_rates(T(_lib.rate_rows(0.0, 0.0, up), dev), arange32(B, dev))
    Uf, _, stf = eng.solve(x0, cl, U0)
    eng.close()
    U, st = U.cpu().numpy(), st.cpu().numpy()
    assert (st[:, 0] == 1).all() and bool((stf[:, 0] == 1).all())
    du = du_metric(U, reference()[f"U_kin_{wi}"])
    steer = np.abs(np.diff(np.concatenate([up[:, None, 1], U[:, 1::2]], 1), axis=1)).max()
    print(f"weights {w}: dU max {du.max():.2e}; first drive of agent 0 {U[0, 0]:.4f} (free: {float(Uf[0, 0]):.4f}), "
          f"largest steering move {steer:.2e}; inner {st[:, 2].mean():.0f} (free: {float(stf[:, 2].mean()):.0f}), slowest {st[:, 2].max():.0f}")
    assert du.max() <= DU_METRIC
    assert float(Uf[0, 0]) == 1.0
    if wi == 1:
        assert U[0, 0] < 0.6


MEASURED_DU_DISCS = (2.25e-1, 1.85e-1)     # largest distance to the reference solve measured on an MI355X, per weight pair


@pytest.mark.parametrize("wi", [0, 1])
def test_solve_against_the_reference_solve_with_discs(dev, O, wi):
    """The moving-disc scene of discs_common with its 16 shifts, u_prev drawn in the box (the steering in its lower half:
    rate_common.disc_scene_agents says why), TIGHT of the disc tests, start U = 0 as the reference solve.
    The issue's bar -- controls within 1e-5 of the reference solve on bench.DU_METRIC -- is NOT met on this scene; as the
    issue provides for that case, the measured distance is reported and four times it asserted.  Measured on an MI355X:
      weights (0.1, 1.0): 14 of 16 agents within 4.7e-6; agent 5 ends with status 2 (its 20 000 inner iterations used up)
        8.0e-3 off; agent 8, Converged, 2.25e-1 off.  Inner iterations 12 101 on average, 12 .. 28 outer.
      weights (0.5, 5.0): 11 of 16 within 5.2e-6; agents 8 and 9 end with status 2, 3.5e-3 and 8.9e-4 off (agent 1 too,
        5.2e-6 off); agents 5 and 6, Converged, 1.79e-1 and 1.85e-1 off.  Inner iterations 16 026 on average, 17 .. 33 outer.
    Two causes, neither in the term's evaluation (within 1e-14 of the checker on this handle).  The budget: the scene needs
    11 813 of TIGHT's 20 000 inner iterations on average WITHOUT a rate table (profiles/r13_agent_discs.txt), so the
    stiffer problem takes a few agents over it.  The far-off Converged agents sit at other stationary points of the same
    problem: the reference solves there have a Lagrangian residual of 1e-11, and the library's points pass the solver's
    own stop test by the checker -- which is what is asserted for EVERY Converged agent, with bounds that come from the
    tolerances and not from a run: g >= -alm_delta, lambda <= 0 and lambda < 0 only where |g| <= alm_delta, the
    projected-gradient residual of f + term + lambda' g at most 10 alm_eps, and a Converged agent further than 1e-5 from
    the reference has another cost than the reference (by more than 1e-9: a distinct minimum, the rule of
    agent_tables_common.assert_tight; measured: 4.2e-3 and 2.6e-1 LOWER than the reference's, 5.6e-2 higher).
    Why 10 alm_eps and not the 2 of the disc tests: the stop test bounds the residual by alm_eps at the iterate x; what is
    returned is the prox point x + p with ||p|| <= gamma alm_eps, where the gradient has moved by at most L ||p|| --
    gamma L = 0.95 for the solver's local estimate of L, more where the constant along p exceeds that estimate, as it
    does under penalties of 1e6 .. 1e9 that switch on within ||p||.  An order of magnitude is allowed for that (measured:
    3.2e-8 and 4.1e-8 at the worst Converged agent, 5.3e-9 in the disc tests); the agents whose budget ran out are at
    1e-6 and more.  The figures are printed before anything is asserted."""
    model, N, _, _ = D.SCENES["moving"]
    B = R.NAGENT
    X0, discs, up = R.disc_scene_agents()
    w = R.WEIGHTS[wi]
    rows = _lib.rate_rows(w[0], w[1], up)
    cl = D.line_centerline()
    eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS, **TIGHT), dev)
    eng.set_agent_discs(T(discs.reshape(B, -1), dev), arange32(B, dev))
    eng.set_agent_rates(T(rows, dev), arange32(B, dev))
    U, lam, st = eng.solve(T(X0, dev), T(cl, dev), torch.zeros(B, 2 * N, dtype=torch.float64, device=dev))
    eng.close()
    U, lam, st = U.cpu().numpy(), lam.cpu().numpy(), st.cpu().numpy()
    cfgs = D.configs(O, model, N)
    Uref = reference()[f"U_moving_{wi}"]
    du = du_metric(U, Uref)
    conv = st[:, 0] == 1
    g = np.stack([D.disc_g(O.rollout(cfgs[0], X0[b], U[b]), discs[b])[0] for b in range(B)])
    res = np.array([R.lagrangian_residual(O, cfgs, X0[b], cl, U[b], discs[b], lam[b], rows[b]) for b in range(B)])
    cost = np.array([[R.psi(O, cfgs[0], X0[b], cl, u[b], rows[b], want_grad=False)[0] for b in range(B)] for u in (U, Uref)])
    print(f"weights {w}, discs: status {st[:, 0].astype(int).tolist()}; dU per agent {np.array2string(du, precision=2)}; "
          f"min g (Converged) {g[conv].min():.2e}; residual (Converged) {res[conv].max():.2e}, (budget used up) "
          f"{np.array2string(res[~conv], precision=1)}; cost - reference's "
          f"{np.array2string(cost[0] - cost[1], precision=2)}; outer {st[:, 1].min():.0f}..{st[:, 1].max():.0f}, "
          f"inner mean {st[:, 2].mean():.0f} max {st[:, 2].max():.0f}")
    assert np.isin(st[:, 0], (1, 2)).all() and conv.sum() >= B // 2 and (lam < 0).any()
    for b in np.flatnonzero(conv):
        assert g[b].min() >= -TIGHT["alm_delta"], (b, g[b].min())
        assert (lam[b] <= 0).all()
        act = lam[b] < 0
        assert not act.any() or np.abs(g[b][act]).max() <= TIGHT["alm_delta"], b
        assert res[b] <= 10 * TIGHT["alm_eps"], (b, res[b])
        assert du[b] <= DU_METRIC or abs(cost[0, b] - cost[1, b]) > 1e-9, (b, du[b], cost[:, b])
    assert du.max() <= 4 * MEASURED_DU_DISCS[wi]


# ----------------------------------------------------------------------------- 4. variants
def test_variants_change_no_bit(dev, O, monkeypatch):
    """Rates of different weights per agent beside a parameter table and a bounds table, 130 kinematic agents: the
    persistent kernel from the start (the default) against rounds only (MPC_SOLO_MAX=0); the same agents tiled to 4160,
    beyond the bound up to which a batch starts in the persistent kernel, in 1 and in 3 groups; a slice of the batch;
    solve_active on a mask"""
    model, N, B, P = 0, 20, 130, 4
    X0, cl, U0 = eval_case(model, N, B, seed=30)
    cfg = mp.default_config(model, N, max_total_inner=3000)
    prow, brow = param_rows_of(O, model, P, seed=31), box_rows_of(P, seed=32)
    ptab = table_of(cfg, prow)
    btab = table_of(cfg, brow, _lib.bound_rows, dict(u_lb=(0, 2), u_ub=(2, 2)))
    pidx, bidx = np.arange(B) % P, (np.arange(B) // 2) % P
    rtab = rate_table(B, seed=33)
    ridx = np.random.default_rng(34).permutation(B)
    for b in range(B):
        rtab[ridx[b], 2:] = np.clip(rtab[ridx[b], 2:], brow[bidx[b]]["u_lb"], brow[bidx[b]]["u_ub"])

    def run(sel, env=None, solo_max=None, groups=None, active=None):
        """the agents `sel` (indices into the 130) as a batch of their own"""
        if env:
            monkeypatch.setenv(*env)
        eng = mp.BatchedMPC(cfg, dev)
        if env:
            monkeypatch.delenv(env[0])
        n = len(sel)
        eng.set_agent_params(T(ptab, dev), T(pidx[sel], dev, torch.int32))
        eng.set_agent_bounds(T(btab, dev), T(bidx[sel], dev, torch.int32))
        eng.set_agent_rates(T(rtab, dev), T(ridx[sel], dev, torch.int32))
        if solo_max is not None:
            eng.set_solo_max(solo_max)
        if groups is not None:
            eng.set_groups(groups)
        a = (T(X0[sel], dev), T(cl, dev), T(U0[sel], dev))
        out = eng.solve(*a) if active is None else active(eng, a, n)
        info = eng.last_solve_info()
        eng.close()
        return out, info
    every = np.arange(B)
    (U, _, st), info = run(every)
    assert info["solo_agents"] == B and bool((st[:, 0] == 1).sum() >= B - 2)
    (U1, _, st1), info = run(every, env=("MPC_SOLO_MAX", "0"))
    assert info["rounds"] > 0 and info["solo_agents"] == 0
    assert torch.equal(U, U1) and torch.equal(st, st1)
    tiled = np.tile(every, 32)                                          # 4160 agents
    for groups in (1, 3):
        (U2, _, st2), info = run(tiled, groups=groups)
        assert info["rounds"] > 0
        assert torch.equal(U2.view(32, B, -1), U[None].expand(32, B, 2 * N)) and torch.equal(st2.view(32, B, 8), st[None].expand(32, B, 8)), groups
    sl = np.arange(17, 98)
    (U3, _, st3), _ = run(sl)
    assert torch.equal(U3, U[17:98]) and torch.equal(st3, st[17:98])

    def masked(eng, a, n):
        active = torch.zeros(n, dtype=torch.int32, device=dev)
        active[torch.arange(0, n, 3)] = 1
        fill = torch.full_like(a[2], 0.123)
        st_in = torch.full((n, 8), 7.0, dtype=torch.float64, device=dev)
        Ua, _, sa, cnt = eng.solve_active(a[0], a[1], torch.where(active[:, None] != 0, a[2], fill), active, stats=st_in)
        return Ua, sa, cnt, active != 0, fill, st_in
    (Ua, sa, cnt, on, fill, st_in), _ = run(every, active=masked)
    assert cnt == int(on.sum()) == 44
    assert torch.equal(Ua[on], U[on]) and torch.equal(sa[on], st[on])
    assert torch.equal(Ua[~on], fill[~on]) and torch.equal(sa[~on], st_in[~on])
    # the penalties do act: the same solve without the rate table moves the controls
    eng = mp.BatchedMPC(cfg, dev)
    eng.set_agent_params(T(ptab, dev), T(pidx, dev, torch.int32))
    eng.set_agent_bounds(T(btab, dev), T(bidx, dev, torch.int32))
    Un, _, _ = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    eng.close()
    assert float((Un - U).abs().max()) > 1e-3


# ----------------------------------------------------------------------------- 5. the loops carry u_{-1}
def loop_rates(B, seed, dev):
    return T(rate_table(B, seed), dev)


def host_closed_loop(eng, x, cl, U, Tn, shift, rtab):
    """mpc_closed_loop with the public calls: solve, the two-column write, rollout of one stage, the shift"""
    B = x.shape[0]
    x, U = x.clone(), U.clone()
    lam = torch.zeros(B, eng.m, dtype=torch.float64, device=x.device) if eng.m else None
    tx = torch.zeros(B, Tn, eng.nx, dtype=torch.float64, device=x.device)
    tu = torch.zeros(B, Tn, 2, dtype=torch.float64, device=x.device)
    fails = torch.zeros(B, dtype=torch.int32, device=x.device)
    st = None
    for t in range(Tn):
        U, lam, st = eng.solve(x, cl, U, lam=lam, inplace=True)
        rtab[:, 2:4] = U[:, :2]
        tu[:, t] = U[:, :2]
        x = eng.rollout(x, U[:, :2].contiguous())[:, 0].contiguous()
        if shift:
            U[:, :-2] = U[:, 2:].clone()
        tx[:, t] = x
        fails += (st[:, 0] != 1).to(torch.int32)
    return x, U, lam, tx, tu, fails, st


@pytest.mark.parametrize("model,N,B,shift", [(0, 20, 130, True), (0, 20, 130, False), (1, 12, 66, True), (1, 12, 66, False)])
def test_closed_loop_is_the_host_loop_bit_for_bit(dev, model, N, B, shift):
    Tn = 6
    X0, cl, _ = eval_case(model, N, B, seed=40 + model)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    x0, clt = T(X0, dev), T(cl, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    first = loop_rates(B, 41, dev)
    tab = first.clone()
    eng.set_agent_rates(tab, arange32(B, dev))
    got = eng.closed_loop(x0, clt, U0, Tn, shift=shift)
    assert torch.equal(tab[:, :2], first[:, :2])                                     # the weights are not written
    assert torch.equal(tab[:, 2:], got[4][:, -1])                                    # ... u_{-1} is the last applied input
    assert not torch.equal(tab[:, 2:], first[:, 2:])
    tab2 = first.clone()
    eng.set_agent_rates(tab2, arange32(B, dev))
    want = host_closed_loop(eng, x0, clt, U0, Tn, shift, tab2)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None and b is None) or torch.equal(a, b), i
    assert torch.equal(tab, tab2)
    # ... and it is not the loop that forgets what it applied
    tab3 = first.clone()
    eng.set_agent_rates(tab3, arange32(B, dev))
    x, U = x0.clone(), U0.clone()
    for t in range(2):
        U, _, _ = eng.solve(x, clt, U)
        x = eng.rollout(x, U[:, :2].contiguous())[:, 0].contiguous()
        if shift:
            U[:, :-2] = U[:, 2:].clone()
    assert not torch.equal(x, got[3][:, 1])
    eng.close()


def host_event_loop(eng, x, cl, U, Tn, w, thr, max_hold, shift, dist, rtab, trk=None, ci=None):
    """mpc_closed_loop_event (trk: mpc_closed_loop_track) with the public calls: trigger_eval, [track_select,] the shift
    in torch, solve_active, the two-column write of the stage about to be applied, rollout of one stage"""
    B, N, nx, dev = x.shape[0], eng.N, eng.nx, x.device
    x, U = x.clone(), U.clone()
    ci = None if ci is None else ci.clone()
    held = torch.full((B,), -1, dtype=torch.int32, device=dev)
    xhat = torch.zeros_like(x)
    stats = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    solved = torch.zeros(B, Tn, dtype=torch.uint8, device=dev)
    tx, tu = torch.zeros(B, Tn, nx, dtype=torch.float64, device=dev), torch.zeros(B, Tn, 2, dtype=torch.float64, device=dev)
    ar, stage = torch.arange(B, device=dev), torch.arange(N, device=dev)
    for t in range(Tn):
        _, fire = eng.trigger_eval(x, xhat, held, w, thr, max_hold)
        fb = fire != 0
        if trk is not None:
            ci, _ = eng.track_select(x, trk, ci, active=fire)
        if shift:
            src = torch.clamp(stage[None, :] + torch.clamp(held, min=0)[:, None].long(), max=N - 1)
            Us = torch.gather(U.view(B, N, 2), 1, src[:, :, None].expand(B, N, 2)).reshape(B, 2 * N)
            U = torch.where(fb[:, None], Us, U)
        U, _, stats, n = eng.solve_active(x, cl, U, fire, stats=stats, cl_index=ci)
        assert n == int(fb.sum())
        held = torch.where(fb, torch.zeros_like(held), held)
        xhat = torch.where(fb[:, None], x, xhat)
        u = U.view(B, N, 2)[ar, held.long()].contiguous()
        rtab[:, 2:4] = u
        x = (eng.rollout(x, u)[:, 0] + dist[:, t]).contiguous()
        xhat = eng.rollout(xhat, u)[:, 0].contiguous()
        held = held + 1
        solved[:, t], tx[:, t], tu[:, t] = fb.to(torch.uint8), x, u
    return dict(x=x, U=U, held=held, solved=solved, traj_x=tx, traj_u=tu, stats=stats)


@pytest.mark.parametrize("track", [False, True])
def test_event_and_track_loops_are_their_host_loops(dev, track):
    """thr > 0, max_hold = 3, a disturbance: agents hold for 1 .. 3 steps, so the column written is U[2 held ..] with held
    0, 1 and 2 (asserted).  track: closed_loop_track on a one-window track (L = S)."""
    model, N, B, Tn, thr, max_hold = 0, 20, 130, 7, 0.02, 3
    X0, cl, _ = eval_case(model, N, B, seed=50)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    x0, clt = T(X0, dev), T(cl, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    dist = T(np.random.default_rng(51).normal(0, 4e-3, (B, Tn, eng.nx)), dev)
    w = np.ones(eng.nx)
    first = loop_rates(B, 52, dev)
    tab = first.clone()
    eng.set_agent_rates(tab, arange32(B, dev))
    trk, zero = None, None
    if track:
        trk = eng.track_windows(clt, 4, 10, False)
        assert trk.R == 1
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        got = eng.closed_loop_track(x0, trk, U0, Tn, w, thr, max_hold, zero, shift=True, disturbance=dist)
    else:
        got = eng.closed_loop_event(x0, clt, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist)
    frac = float(got.solved.float().mean())
    assert 0.3 < frac < 0.95, frac
    assert torch.equal(tab[:, :2], first[:, :2]) and torch.equal(tab[:, 2:], got.traj_u[:, -1])
    sv, hold, seen = got.solved.cpu().numpy(), np.zeros(B, dtype=int), set()        # the stage every step applied
    for t in range(Tn):
        hold = np.where(sv[:, t] != 0, 0, hold + 1)
        seen |= set(hold.tolist())
    assert seen == {0, 1, 2} and np.array_equal(hold + 1, got.held.cpu().numpy())
    tab2 = first.clone()
    eng.set_agent_rates(tab2, arange32(B, dev))
    want = host_event_loop(eng, x0, trk.win if track else clt, U0, Tn, w, thr, max_hold, True, dist, tab2, trk, zero)
    for name, b in want.items():
        assert torch.equal(getattr(got, name), b), name
    assert torch.equal(tab, tab2)
    eng.close()


def test_traffic_loop_is_its_host_loop(dev):
    """scenes of 5 on a disc handle: the loop rewrites the disc table and the two columns of the rate table"""
    model, N, B, G, Tn, reach = 0, 20, 130, 5, 3, 0.6
    rng = np.random.default_rng(60)
    X0 = np.zeros((B, 4))
    for s in range(0, B, G):                     # five cars in a row 0.3 apart, the rear ones faster
        X0[s:s + G, 0] = 1.2 + 0.3 * np.arange(G) + rng.uniform(0, 0.02, G)
        X0[s:s + G, 1] = 0.5 + rng.uniform(-.04, .04, G)
        X0[s:s + G, 3] = 1.1 - 0.15 * np.arange(G)
    radius = T(rng.uniform(0.2, 0.24, B), dev)
    eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS, Sigma0=10.0, max_total_inner=1500), dev)
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    first = loop_rates(B, 61, dev)
    tab = first.clone()
    eng.set_agent_rates(tab, arange32(B, dev))
    res = eng.closed_loop_traffic(x0, cl, U0, Tn, G, radius, reach, shift=True)
    got = [t.clone() for t in res]
    assert torch.equal(tab[:, 2:], res.traj_u[:, -1]) and bool((res.lam < 0).any())
    tab2 = first.clone()
    eng.set_agent_rates(tab2, arange32(B, dev))
    x, U = x0.clone(), U0.clone()
    lam = torch.zeros(B, eng.m, dtype=torch.float64, device=dev)
    for t in range(Tn):
        X = eng.rollout(x, U)
        opp, _ = eng.opponents_from_plans(X, G, radius, reach)
        eng.discs_from_plans(X, opp, radius, out=res.table)
        U, lam, st = eng.solve(x, cl, U, lam=lam, inplace=True)
        tab2[:, 2:4] = U[:, :2]
        assert torch.equal(U[:, :2], got[4][:, t])
        x = eng.rollout(x, U[:, :2].contiguous())[:, 0].contiguous()
        U[:, :-2] = U[:, 2:].clone()
        assert torch.equal(x, got[3][:, t]) and torch.equal(opp, got[7][:, t])
    assert torch.equal(x, got[0]) and torch.equal(U, got[1]) and torch.equal(lam, got[2]) and torch.equal(st, got[6])
    assert torch.equal(tab, tab2)
    eng.close()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    """each MPC_E_ARG (-1) before any launch, in the library's words: P != B in a loop, a negative or NaN weight, a
    non-finite u_prev, a rate table beside a constraint table in either order, another batch size than the bound one,
    binding during an asynchronous solve"""
    model, N, B = 0, 20, 64
    X0, cl, U = eval_case(model, N, B, seed=70)
    x0, clt, Ut = T(X0, dev), T(cl, dev), T(U, dev)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=300), dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    index = arange32(B, dev)
    good = T(rate_table(B, 71), dev)
    # rows
    for col, v, words in ((0, -1e-3, "weights must not be negative"), (1, -1.0, "weights must not be negative"), (0, np.nan, "must be finite"),
                          (1, np.inf, "must be finite"), (2, np.inf, "must be finite"), (3, np.nan, "must be finite"), (2, -np.inf, "must be finite")):
        bad = good.clone()
        bad[5, col] = v
        assert eng.lib.mpc_set_agent_rates(eng._h, p(bad), B, p(index), B) == -1
        msg = eng.lib.mpc_last_error().decode()
        assert msg.startswith("mpc_set_agent_rates: row 5: ") and words in msg, msg
        with pytest.raises(mp.MpcError):
            eng.set_agent_rates(bad, index)
        assert not eng.agent_rates_bound
    with pytest.raises(ValueError):
        eng.set_agent_rates(good[:, :3].contiguous(), index)                 # the row width
    with pytest.raises(ValueError):
        eng.set_agent_rates(good, index + 1)                                 # index out of range
    # P != B, or an index that is not the identity, in a loop
    w, zi = np.ones(4), torch.zeros(B, dtype=torch.int32, device=dev)
    trk = eng.track_windows(clt, 1, 0, False)
    three = T(rate_table(3, 72), dev)
    i3 = T(np.arange(B) % 3, dev, torch.int32)
    loops = {"mpc_closed_loop": lambda: eng.closed_loop(x0, clt, Ut, 1),
             "mpc_closed_loop_event": lambda: eng.closed_loop_event(x0, clt, Ut, 1, w, 0.0, 3),
             "mpc_closed_loop_track": lambda: eng.closed_loop_track(x0, trk, Ut, 1, w, 0.0, 3, zi)}
    eng.set_agent_rates(three, i3)
    eng.solve(x0, clt, Ut)                                                   # (a solve takes any P)
    for fn in loops.values():
        with pytest.raises(ValueError, match="P == B"):
            fn()
    dummy = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.zeros(B, 8, dtype=torch.float64, device=dev)
    assert eng.lib.mpc_closed_loop(eng._h, B, 1, 0, p(x0.clone()), p(clt), None, p(Ut.clone()), None, None, None, p(dummy), p(st), None) == -1
    assert b"mpc_closed_loop: the bound rate table has 3 rows" in eng.lib.mpc_last_error() and b"P == B = 64" in eng.lib.mpc_last_error()
    held = torch.full((B,), -1, dtype=torch.int32, device=dev)
    wv = (C.c_double * 4)(1, 1, 1, 1)
    assert eng.lib.mpc_closed_loop_event(eng._h, B, 1, 0, wv, 0.0, 3, p(x0.clone()), p(clt), None, p(Ut.clone()), None, p(held), None, None,
                                         None, None, None, None, p(st), None) == -1
    assert b"mpc_closed_loop_event: the bound rate table has 3 rows" in eng.lib.mpc_last_error()
    eng.set_agent_rates(good, T(np.random.default_rng(73).permutation(B), dev, torch.int32))
    with pytest.raises(ValueError, match="arange"):
        eng.closed_loop(x0, clt, Ut, 1)
    # another batch size than the bound one
    eng.set_agent_rates(good, index)
    s = slice(0, 32)
    a = (x0[s].contiguous(), clt, Ut[s].contiguous())
    readers = {"mpc_eval_cost_grad": lambda: eng.eval_cost_grad(*a), "mpc_eval_cost_grad/wave": lambda: eng.eval_cost_grad(*a, wave=True),
               "mpc_solve_batch": lambda: eng.solve(*a), "mpc_solve_batch/async": lambda: eng.solve_async(*a)(),
               "mpc_solve_active": lambda: eng.solve_active(*a, torch.ones(32, dtype=torch.int32, device=dev))}
    for who, fn in readers.items():
        with pytest.raises(mp.MpcError) as err:
            fn()
        assert str(err.value) == (f"libmpc_hip error -1: {who.split('/')[0]}: the bound rate table is for a batch of 64 agents, "
                                  "this call has 32 (mpc_set_agent_rates)"), str(err.value)
    eng.rollout(a[0], a[2])                     # the calls that do not read the table serve any batch
    eng.stage_cost(a[0], a[2][:, :2].contiguous(), clt)
    for fn in loops.values():                   # ... and with P == B and the identity index the loops run
        fn()
    with pytest.raises(mp.MpcError, match="mpc_set_agent_bounds: the bound rate table is for a batch of 64 agents$"):
        eng.set_agent_bounds(T(_lib.bound_rows(eng.cfg, 2), dev), T(np.arange(32) % 2, dev, torch.int32))
    # binding during an asynchronous solve
    wait = eng.solve_async(x0, clt, Ut)
    rc = eng.lib.mpc_set_agent_rates(eng._h, p(good), B, p(index), B)
    msg = eng.lib.mpc_last_error()
    wait()
    assert rc == -1 and b"mpc_set_agent_rates: a solve of this handle is in flight" in msg
    eng.close()
    # beside a constraint table, in either order; the handle's own constraint data is fine
    for mode, kw in ((mp.CONSTR_STATE_SQ, {}), (mp.CONSTR_LANE, dict(lane_halfwidth=0.2))):
        ce = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, max_total_inner=300, **kw), dev)
        ctab, cidx = T(_lib.constraint_rows(ce.cfg, 2), dev), T(np.arange(B) % 2, dev, torch.int32)
        ce.set_agent_rates(good, index)
        with pytest.raises(mp.MpcError, match="mpc_set_agent_constraints: a rate table is bound .*cannot be bound together"):
            ce.set_agent_constraints(ctab, cidx)
        assert not ce.agent_constraints_bound
        ce.solve(x0, clt, Ut)                   # the handle's own constraint data beside the rates
        ce.clear_agent_rates()
        ce.set_agent_constraints(ctab, cidx)
        with pytest.raises(mp.MpcError, match="mpc_set_agent_rates: a constraint table is bound .*cannot be bound together"):
            ce.set_agent_rates(good, index)
        assert not ce.agent_rates_bound
        ce.solve(x0, clt, Ut)
        ce.close()
    torch.cuda.synchronize()
