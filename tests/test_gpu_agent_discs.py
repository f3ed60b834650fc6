"""GPU tests of the keep-out discs (constr_mode CONSTR_DISCS, mpc_set_agent_discs / BatchedMPC.set_agent_discs): a table
of per-agent, per-stage discs [N][NDISC][3] = (cx, cy, r) in device memory and one row index per agent, and the gather
mpc_discs_from_plans.  The oracle does not know discs: the checker is the numpy restatement of tests/discs_common.py,
built from the oracle's calls; the reference solves (an ALM loop around scipy's L-BFGS-B on that checker) are recorded in
tests/golden/discs_reference.npz.  Shapes: at most 256 agents, N = 20 kinematic and N = 12 Pacejka -- they cross a
workgroup boundary of every kernel form (256-thread fused blocks, 64-lane waves, N not dividing 64).  The tolerances are
the project's HIP-vs-oracle bars and its bar between two correct solvers (bench.DU_METRIC)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from agent_tables_common import T, kwl, param_rows_of, table_of
from conftest import GOLDEN

import discs_common as D

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402
from model_predictive_control_amd.tracks import stadium_track  # noqa: E402

DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)
MODELS = ((0, 20), (1, 12))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def engine(dev, model, N, **kw):
    return mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS, **kw), dev)


def arange32(B, dev):
    return torch.arange(B, dtype=torch.int32, device=dev)


def du_metric(U, Uref):
    return np.abs(U - Uref).max(1) / np.maximum(1.0, np.abs(Uref).max(1))


def eval_case(model, N, B, seed=3):
    """B agents with rows of their own around the centerline y = 0.5 that starts at x = 0.9 (positions away from 0), inputs
    near a gentle drive, discs from ones the plan runs through ("violated") over near misses to r = 0, multipliers of both
    signs and Sigma in [1, 1e3]"""
    rng = np.random.default_rng(seed)
    cols = [rng.uniform(1.0, 4.0, B), 0.5 + rng.uniform(-.15, .15, B), rng.uniform(-.2, .2, B), rng.uniform(.4, 1.2, B)]
    if model == 1:
        cols += [rng.uniform(-.03, .03, B), rng.uniform(-.3, .3, B)]
    X0 = np.stack(cols, 1)
    U = np.tile([0.6, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1.0, 0.3], N)
    discs = np.zeros((B, N, 2, 3))
    ahead = 0.05 * np.arange(1, N + 1)[None, :, None] * X0[:, 3][:, None, None]       # roughly where stage k ends
    discs[..., 0] = X0[:, 0][:, None, None] + ahead + rng.uniform(-.15, .15, (B, N, 2))
    discs[..., 1] = X0[:, 1][:, None, None] + rng.uniform(-.15, .15, (B, N, 2))
    discs[..., 2] = rng.uniform(0.0, 0.25, (B, N, 2)) * (rng.uniform(size=(B, N, 2)) < 0.7)  # 30 %: r = 0
    y = rng.uniform(-2.0, 0.5, (B, 2 * N))
    Sig = 10 ** rng.uniform(0, 3, (B, 2 * N))
    return X0, D.line_centerline(), U, discs, y, Sig


def check_eval(O, model, N, X0, cl, U, discs, y, Sig, psi, yhat, grad, overrides=None):
    """psi and yhat within 1e-12 relative, grad within 1e-9 ||grad psi||, agent by agent against the checker"""
    B = X0.shape[0]
    worst = [0.0, 0.0, 0.0]
    nact = 0
    for b in range(B):
        cfgs = D.configs(O, model, N, **(kwl(overrides[b]) if overrides else {}))
        p, yh, g, _ = D.psi_yhat(O, cfgs, X0[b], cl, U[b], discs[b], y[b], Sig[b])
        nact += int((yh < 0).sum())
        worst[0] = max(worst[0], abs(psi[b] - p) / abs(p))
        worst[1] = max(worst[1], np.abs(yhat[b] - yh).max() / max(1e-300, np.abs(yh).max()))
        worst[2] = max(worst[2], np.abs(grad[b] - g).max() / np.linalg.norm(g))
    print(f"model {model}: {nact} active discs of {B * 2 * N}; worst psi {worst[0]:.2e} yhat {worst[1]:.2e} grad {worst[2]:.2e}")
    assert nact >= B                                       # the discs do act
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-9


# ----------------------------------------------------------------------------- 1. evaluation
@pytest.mark.parametrize("model,N", MODELS)
def test_evaluation_matches_the_checker_and_every_form_agrees(dev, O, monkeypatch, model, N):
    """192 agents with distinct rows.  Fails on a library without the mode (mpc_create refuses constr_mode 3)."""
    B = 192
    X0, cl, U, discs, y, Sig = eval_case(model, N, B)
    perm = np.random.default_rng(9).permutation(B)         # agent b reads row perm[b]
    table = T(discs[np.argsort(perm)].reshape(B, -1), dev)
    assert np.array_equal(table.cpu().numpy()[perm].reshape(discs.shape), discs)
    index = T(perm, dev, torch.int32)
    args = (T(X0, dev), T(cl, dev), T(U, dev), T(y, dev), T(Sig, dev))
    eng = engine(dev, model, N)
    assert eng.m == 2 * N
    eng.set_agent_discs(table, index)
    psi, grad, yhat = eng.eval_cost_grad(*args)
    check_eval(O, model, N, X0, cl, U, discs, y, Sig, psi.cpu().numpy(), yhat.cpu().numpy(), grad.cpu().numpy())
    # the wave evaluation, the centerline through an index, and cost-only requests: the same bits
    for kw in (dict(wave=True), dict(cl_index=T(np.arange(B) % 3, dev, torch.int32))):
        a = list(args)
        if "cl_index" in kw:
            a[1] = T(np.tile(cl, (3, 1)), dev)
        p2, g2, y2 = eng.eval_cost_grad(*a, **kw)
        assert torch.equal(psi, p2) and torch.equal(grad, g2) and torch.equal(yhat, y2), kw
    p3, _, y3 = eng.eval_cost_grad(*args, want_grad=False)
    assert torch.equal(psi, p3) and torch.equal(yhat, y3)
    eng.close()
    # the two-kernel K1b + K1c path
    monkeypatch.setenv("MPC_UNFUSED_EVAL", "1")
    eng = engine(dev, model, N)
    eng.set_agent_discs(table, index)
    for ci in (None, T(np.arange(B) % 3, dev, torch.int32)):
        p4, g4, y4 = eng.eval_cost_grad(args[0], args[1] if ci is None else T(np.tile(cl, (3, 1)), dev), *args[2:], cl_index=ci)
        assert torch.equal(psi, p4) and torch.equal(grad, g4) and torch.equal(yhat, y4)
    eng.close()


# ----------------------------------------------------------------------------- 2. vacuous discs
@pytest.mark.parametrize("model,N", MODELS)
def test_vacuous_discs_are_the_vacuous_lane_band(dev, model, N):
    """Every r = 0 against CONSTR_LANE with a half-width of 1e6 (and against CONSTR_NONE): yhat == 0 and psi == f, bit for
    bit, in the evaluation.  m is 2N for the discs and N for the lane band, so no horizon makes the two problems the
    same size; the solves agree all the same: controls within 1e-5 on bench.DU_METRIC, and -- measured on an MI355X: dU = 0,
    statistics equal, both models, against the lane band and against no constraints -- bit for bit, which is asserted."""
    B = 128
    X0, cl, U, discs, _, _ = eval_case(model, N, B, seed=5)
    discs[..., 2] = 0.0
    x0, clt, Ut = T(X0, dev), T(cl, dev), T(U, dev)
    out = {}
    for name, mode, kw in (("discs", mp.CONSTR_DISCS, {}), ("lane", mp.CONSTR_LANE, dict(lane_halfwidth=1e6)), ("none", mp.CONSTR_NONE, {})):
        eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, **kw), dev)
        if name == "discs":
            eng.set_agent_discs(T(discs.reshape(B, -1), dev), arange32(B, dev))
        m = eng.m
        y = torch.zeros(B, m, dtype=torch.float64, device=dev) if m else None
        Sig = T(10 ** np.random.default_rng(1).uniform(0, 3, (B, max(m, 1))), dev) if m else None
        psi, grad, yhat = eng.eval_cost_grad(x0, clt, Ut, y, Sig)
        Us, lam, st = eng.solve(x0, clt, Ut)
        out[name] = (psi, grad, yhat, Us.cpu().numpy(), st.cpu().numpy(), lam)
        eng.close()
    for name in ("discs", "lane"):
        assert not bool(out[name][2].any()), name                               # yhat == 0
        assert torch.equal(out[name][0], out["none"][0]), name                  # psi == f
        assert torch.equal(out[name][1], out["none"][1]), name
        assert not bool(out[name][5].any()), name                               # no multiplier moves
    for a, b in (("discs", "lane"), ("discs", "none")):
        du = du_metric(out[a][3], out[b][3])
        print(f"model {model}: vacuous {a} vs {b}: dU max {du.max():.2e}, stats equal {np.array_equal(out[a][4], out[b][4])}")
        assert du.max() <= DU_METRIC
        # ... and in fact equal, controls and all eight statistics (status, outer, inner, n_evals among them): the
        # multipliers never move, so neither their number nor their kind reaches the iterates
        assert np.array_equal(out[a][3], out[b][3]) and np.array_equal(out[a][4], out[b][4])


# ----------------------------------------------------------------------------- 3. the solve
@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "discs_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    return ref


def scene_batch(name, B):
    """agent b: the scene with shift b % NSHIFT"""
    model, N, x0, scene = D.SCENES[name]
    shifts = D.scene_shifts()
    which = np.arange(B) % D.NSHIFT
    discs = np.stack([scene(N, shifts[p]) for p in which])
    return model, N, np.tile(x0, (B, 1)), D.line_centerline(), discs, which


def assert_solution(O, cfgs_of, X0, cl, discs, U, lam, st, eps, delta, boxes=None):
    """Converged; g >= -delta; lambda <= 0 and lambda < 0 => |g| <= delta; the projected-gradient residual of f + lambda' g
    at U <= 2 eps: the solver's own stop test plus evaluation differences"""
    assert np.all(st[:, 0] == 1), st[:, 0]
    worst_g, worst_r, nact = 0.0, 0.0, 0
    for b in range(X0.shape[0]):
        cfgs = cfgs_of(b)
        g = D.disc_g(O.rollout(cfgs[0], X0[b], U[b]), discs[b])[0]
        assert g.min() >= -delta, (b, g.min())
        assert (lam[b] <= 0).all()
        act = lam[b] < 0
        nact += int(act.sum())
        if act.any():
            assert np.abs(g[act]).max() <= delta, (b, np.abs(g[act]).max())
        box = boxes[b] if boxes is not None else {}
        r = D.lagrangian_residual(O, cfgs, X0[b], cl, U[b], discs[b], lam[b], **box)
        worst_g, worst_r = min(worst_g, g.min()), max(worst_r, r)
    print(f"min g {worst_g:.2e}, residual {worst_r:.2e}, active multipliers per agent {nact / X0.shape[0]:.1f}")
    assert worst_r <= 2 * eps
    return nact


@pytest.mark.parametrize("name", list(D.SCENES))
def test_solve_against_the_reference_solve(dev, O, name):
    """The three scenes, 64 agents each with the scene's discs shifted a little (16 distinct shifts).  Start U = 0, as the
    reference solve."""
    B = 64
    model, N, X0, cl, discs, which = scene_batch(name, B)
    ref = reference()
    eng = engine(dev, model, N, **TIGHT)
    eng.set_agent_discs(T(discs.reshape(B, -1), dev), arange32(B, dev))
    U, lam, st = eng.solve(T(X0, dev), T(cl, dev), torch.zeros(B, 2 * N, dtype=torch.float64, device=dev))
    U, lam, st = U.cpu().numpy(), lam.cpu().numpy(), st.cpu().numpy()
    eng.close()
    cfgs = D.configs(O, model, N)
    nact = assert_solution(O, lambda b: cfgs, X0, cl, discs, U, lam, st, TIGHT["alm_eps"], TIGHT["alm_delta"])
    assert nact >= B
    du = du_metric(U, ref["U_" + name][which])
    print(f"{name}: dU max {du.max():.2e}; outer {st[:, 1].min():.0f}..{st[:, 1].max():.0f}, inner {st[:, 2].mean():.0f}")
    assert du.max() <= DU_METRIC


# ----------------------------------------------------------------------------- 4. variants
@pytest.mark.parametrize("name", ["standing", "pacejka"])
def test_variants_change_no_bit(dev, monkeypatch, name):
    """persistent kernel from the start (64 agents: the default) vs rounds only, one sub-batch group vs two, speculation on
    and off: U, lambda and all eight statistics"""
    B = 64
    model, N, X0, cl, discs, _ = scene_batch(name, B)
    args = (T(X0, dev), T(cl, dev), torch.zeros(B, 2 * N, dtype=torch.float64, device=dev))
    table, index = T(discs.reshape(B, -1), dev), arange32(B, dev)

    def run(solo_max=None, groups=None, env=()):
        for k, v in env:
            monkeypatch.setenv(k, v)
        eng = engine(dev, model, N, Sigma0=10.0, alm_eps=1e-6, alm_delta=1e-6, max_total_inner=20000)
        for k, _ in env:
            monkeypatch.delenv(k)
        eng.set_agent_discs(table, index)
        if solo_max is not None:
            eng.set_solo_max(solo_max)
        if groups is not None:
            eng.set_groups(groups)
        out = eng.solve(*args)
        info = eng.last_solve_info()
        eng.close()
        return out, info
    base, info = run()
    assert info["solo_agents"] == B
    assert bool((base[2][:, 0] == 1).all()) and bool((base[1] < 0).any())
    for kw in (dict(solo_max=0, groups=1), dict(solo_max=0, groups=2), dict(solo_max=0, groups=1, env=(("MPC_NO_SPEC", "1"),))):
        got, info = run(**kw)
        if kw.get("solo_max") == 0:
            assert info["rounds"] > 0 and info["solo_agents"] == 0
        for a, b in zip(base, got):
            assert torch.equal(a, b), kw


# ----------------------------------------------------------------------------- 5. tables together, masked solve
def test_tables_together_and_masked_solve(dev, O):
    """Discs beside a parameter and a bounds table: every agent's checker runs on its own row of each.  solve_active on half
    of the agents is solve on those rows, bit for bit, and leaves the other rows' bytes alone."""
    B, model, N, P = 64, 0, 20, 4
    _, _, X0, cl, discs, _ = scene_batch("standing", B)
    cfg = mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS, **TIGHT)
    prow = param_rows_of(O, model, P, seed=31)
    rng = np.random.default_rng(32)             # boxes that leave room to steer round the disc (row 0: the handle's)
    brow = [dict(u_lb=[-1.0, -0.32], u_ub=[1.0, 0.32])]
    for _ in range(1, P):
        s_lo, s_hi = -rng.uniform(.2, .32), rng.uniform(.2, .32)
        brow.append(dict(u_lb=[-rng.uniform(.5, 1.0), s_lo], u_ub=[rng.uniform(.6, 1.0), s_hi]))
    pidx, bidx = np.arange(B) % P, (np.arange(B) // 2) % P
    eng = mp.BatchedMPC(cfg, dev)
    eng.set_agent_params(T(table_of(cfg, prow), dev), T(pidx, dev, torch.int32))
    eng.set_agent_bounds(T(table_of(cfg, brow, _lib.bound_rows, dict(u_lb=(0, 2), u_ub=(2, 2))), dev), T(bidx, dev, torch.int32))
    perm = np.random.default_rng(2).permutation(B)
    eng.set_agent_discs(T(discs[np.argsort(perm)].reshape(B, -1), dev), T(perm, dev, torch.int32))
    x0, clt = T(X0, dev), T(cl, dev)
    # evaluation on every agent's own vehicle and discs
    _, _, Ue, _, ye, Se = eval_case(model, N, B, seed=7)
    psi, grad, yhat = eng.eval_cost_grad(x0, clt, T(Ue, dev), T(ye, dev), T(Se, dev))
    check_eval(O, model, N, X0, cl, Ue, discs, ye, Se, psi.cpu().numpy(), yhat.cpu().numpy(), grad.cpu().numpy(),
               overrides=[prow[p] for p in pidx])
    # the solve: feasible stationary points of every agent's own problem
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    U, lam, st = eng.solve(x0, clt, U0)
    cfgs = [D.configs(O, model, N, **kwl(prow[p])) for p in range(P)]
    assert_solution(O, lambda b: cfgs[pidx[b]], X0, cl, discs, U.cpu().numpy(), lam.cpu().numpy(), st.cpu().numpy(),
                    TIGHT["alm_eps"], TIGHT["alm_delta"], boxes=[brow[p] for p in bidx])
    # masked
    active = torch.zeros(B, dtype=torch.int32, device=dev)
    active[torch.arange(0, B, 2)] = 1
    fill = torch.full_like(U0, 0.123)
    lam_in = torch.full((B, 2 * N), -0.5, dtype=torch.float64, device=dev)
    st_in = torch.full((B, 8), 7.0, dtype=torch.float64, device=dev)
    Ua, la, sa, n = eng.solve_active(x0, clt, torch.where(active[:, None] != 0, U0, fill), active,
                                     lam=torch.where(active[:, None] != 0, torch.zeros_like(lam_in), lam_in), stats=st_in)
    on = active != 0
    assert n == B // 2
    assert torch.equal(Ua[on], U[on]) and torch.equal(la[on], lam[on]) and torch.equal(sa[on], st[on])
    assert torch.equal(Ua[~on], fill[~on]) and torch.equal(la[~on], lam_in[~on]) and torch.equal(sa[~on], st_in[~on])
    eng.close()


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    """wrong mode, an unbound table, set_agent_constraints on a disc handle, another batch size than the bound one for
    every reader, non-finite values and a negative radius at bind time: MPC_E_ARG (-1), in the library's words"""
    N, B = 20, 64
    X0, cl, U, discs, y, Sig = eval_case(0, N, B)
    x0, clt, Ut, yt, St = (T(a, dev) for a in (X0, cl, U, y, Sig))
    table, index = T(discs.reshape(B, -1), dev), arange32(B, dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for mode in (mp.CONSTR_NONE, mp.CONSTR_STATE_SQ, mp.CONSTR_LANE):
        other = mp.BatchedMPC(mp.default_config(0, N, constr_mode=mode), dev)
        assert other.lib.mpc_set_agent_discs(other._h, p(table), B, p(index), B) == -1
        assert b"mpc_set_agent_discs: the handle's constr_mode is not MPC_CONSTR_DISCS" in other.lib.mpc_last_error()
        with pytest.raises(mp.MpcError):
            other.set_agent_discs(table, index)
        assert not other.agent_discs_bound
        other.close()
    eng = engine(dev, 0, N, max_total_inner=300)
    trk = eng.track_windows(clt, 1, 0, False)
    w, zi = np.ones(4), torch.zeros(B, dtype=torch.int32, device=dev)
    ones = torch.ones(B, dtype=torch.int32, device=dev)

    def readers(nb):
        s = slice(0, nb)
        a = (x0[s].contiguous(), clt, Ut[s].contiguous())
        return {"mpc_eval_cost_grad": lambda: eng.eval_cost_grad(*a, yt[s].contiguous(), St[s].contiguous()),
                "mpc_eval_cost_grad/wave": lambda: eng.eval_cost_grad(*a, yt[s].contiguous(), St[s].contiguous(), wave=True),
                "mpc_solve_batch": lambda: eng.solve(*a),
                "mpc_solve_batch/async": lambda: eng.solve_async(*a)(),
                "mpc_solve_active": lambda: eng.solve_active(*a, ones[s].contiguous()),
                "mpc_closed_loop": lambda: eng.closed_loop(*a, 1),
                "mpc_closed_loop_event": lambda: eng.closed_loop_event(*a, 1, w, 0.0, 3),
                "mpc_closed_loop_track": lambda: eng.closed_loop_track(a[0], trk, a[2], 1, w, 0.0, 3, zi[s].contiguous())}
    # nothing bound: every reader refuses and names the setter
    for who, fn in readers(B).items():
        with pytest.raises(mp.MpcError) as err:
            fn()
        msg = str(err.value)
        assert msg.startswith("libmpc_hip error -1: " + who.split("/")[0] + ":") and "(mpc_set_agent_discs)" in msg, msg
    # there is no constraint data to bind on a disc handle
    ctab = T(_lib.constraint_rows(eng.cfg, 2), dev)
    with pytest.raises(mp.MpcError, match="mpc_set_agent_constraints: .*MPC_CONSTR_DISCS"):
        eng.set_agent_constraints(ctab, T(np.arange(B) % 2, dev, torch.int32))
    assert not eng.agent_constraints_bound
    # bound for 64: 32 are refused by every reader
    eng.set_agent_discs(table, index)
    for who, fn in readers(32).items():
        with pytest.raises(mp.MpcError) as err:
            fn()
        assert str(err.value) == (f"libmpc_hip error -1: {who.split('/')[0]}: the bound disc table is for a batch of 64 agents, "
                                  "this call has 32 (mpc_set_agent_discs)"), str(err.value)
    for fn in readers(B).values():          # ... and 64 are served
        fn()
    # beside another table: for the same batch
    with pytest.raises(mp.MpcError, match="mpc_set_agent_bounds: the bound disc table is for a batch of 64 agents$"):
        eng.set_agent_bounds(T(_lib.bound_rows(eng.cfg, 2), dev), T(np.arange(32) % 2, dev, torch.int32))
    # bind-time checks of the rows; a refused bind leaves the bound table as it was
    for k, f, v, words in ((3, 2, -1e-3, "radius must not be negative"), (0, 0, np.nan, "must be finite"), (N - 1, 5, np.inf, "must be finite"),
                           (7, 4, -np.inf, "must be finite")):
        bad = discs.reshape(B, N, 6).copy()
        bad[5, k, f] = v
        with pytest.raises(mp.MpcError, match=f"mpc_set_agent_discs: row 5, stage {k}, disc {f // 3}: .*{words}"):
            eng.set_agent_discs(T(bad.reshape(B, -1), dev), index)
    with pytest.raises(ValueError):
        eng.set_agent_discs(table[:, :-1].contiguous(), index)              # the row width is the handle's 6 N
    with pytest.raises(ValueError):
        eng.set_agent_discs(table, index + 1)                               # index out of range
    assert eng.agent_discs_bound
    eng.solve(x0, clt, Ut)
    eng.clear_agent_discs()
    with pytest.raises(mp.MpcError, match="mpc_set_agent_discs"):
        eng.solve(x0, clt, Ut)
    torch.cuda.synchronize()
    eng.close()


# ----------------------------------------------------------------------------- 7. the gather
@pytest.mark.parametrize("model,N", MODELS)
def test_discs_from_plans_is_the_numpy_gather(dev, model, N):
    B = 200
    eng = engine(dev, model, N)
    rng = np.random.default_rng(4)
    X = rng.normal(size=(B, N, eng.nx))
    opp = rng.integers(-3, B + 3, (B, 2)).astype(np.int32)
    opp[0] = (-1, B - 1); opp[1] = (B, 0); opp[2] = (-2147483648, 2147483647)
    radius = rng.uniform(0.05, 0.2, B)
    want = np.zeros((B, N, 2, 3))
    for b in range(B):
        for j in range(2):
            o = int(opp[b, j])
            if 0 <= o < B:
                want[b, :, j, 0], want[b, :, j, 1], want[b, :, j, 2] = X[o, :, 0], X[o, :, 1], radius[o]
    assert ((opp < 0) | (opp >= B)).sum() >= 5
    got = eng.discs_from_plans(T(X, dev), T(opp, dev, torch.int32), T(radius, dev))
    assert got.shape == (B, 6 * N) and np.array_equal(got.cpu().numpy().view(np.int64), want.reshape(B, -1).view(np.int64))
    out = torch.full((B, 6 * N), 9.0, dtype=torch.float64, device=dev)
    assert eng.discs_from_plans(T(X, dev), T(opp, dev, torch.int32), T(radius, dev), out=out) is out
    assert torch.equal(out, got)
    eng.close()


def test_one_best_response_sweep_separates_two_cars(dev, O):
    """Two cars on the same line, the second 0.25 ahead, a little to the side and slower: each plans alone, then each avoids the other's plan
    (discs_from_plans, index = arange).  Afterwards no stage of either plan is inside the other's disc as it was planned
    against: g >= -alm_delta by the checker."""
    model, N, B, rad = 0, 20, 2, 0.07
    eps = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)
    eng = engine(dev, model, N, **eps)
    cl = D.line_centerline()
    X0 = np.array([[1.0, 0.5, 0.0, 1.1], [1.25, 0.56, 0.0, 0.4]])
    x0, clt = T(X0, dev), T(cl, dev)
    table = T(np.zeros((B, 6 * N)), dev)
    eng.set_agent_discs(table, arange32(B, dev))
    U, _, st = eng.solve(x0, clt, torch.zeros(B, 2 * N, dtype=torch.float64, device=dev))     # alone: r = 0 everywhere
    assert bool((st[:, 0] == 1).all())
    plans = eng.rollout(x0, U)
    opp = T(np.array([[1, -1], [0, -1]]), dev, torch.int32)
    radius = T(np.array([2 * rad, 2 * rad]), dev)             # two cars of radius `rad`: centres 2 rad apart
    eng.discs_from_plans(plans, opp, radius, out=table)       # in place: the bound table
    cfgs = D.configs(O, model, N)
    d = table.cpu().numpy().reshape(B, N, 2, 3)
    g0 = np.stack([D.disc_g(O.rollout(cfgs[0], X0[b], U[b].cpu().numpy()), d[b])[0] for b in range(B)])
    assert g0.min() < -1e-3                                   # the plans made alone do collide
    U2, lam2, st2 = eng.solve(x0, clt, U)
    assert bool((st2[:, 0] == 1).all()) and bool((lam2 < 0).any())
    g1 = np.stack([D.disc_g(O.rollout(cfgs[0], X0[b], U2[b].cpu().numpy()), d[b])[0] for b in range(B)])
    print(f"min g before {g0.min():.3e}, after {g1.min():.3e}")
    assert g1.min() >= -eps["alm_delta"]
    eng.close()


# ----------------------------------------------------------------------------- 8. lap driving past a standing disc
def test_track_loop_passes_a_standing_disc(dev, O):
    """A stadium track with one disc standing on the racing line of the lower straight; 16 agents start before it and drive
    past it.  Every re-plan reads the same table (stage k entry k: the obstacle stands).  No point of any trajectory is
    inside the disc beyond the slack a constraint violation of alm_delta in g = d^2 - r^2 allows in the distance
    (sqrt(r^2 - alm_delta) >= r - sqrt(alm_delta)), by the checker on the recorded trajectories."""
    model, N, B, Tn, delta = 0, 20, 16, 60, 1e-6
    eng = engine(dev, model, N, Sigma0=10.0, alm_eps=1e-6, alm_delta=delta, max_total_inner=20000)
    track = stadium_track(10, 3, 0.1)
    trk = eng.track_windows(T(track, dev), 4, 10, True)
    cx, cy, r = 1.6, 0.03, 0.12
    disc = np.zeros((N, 2, 3)); disc[:, 0] = (cx, cy, r)
    eng.set_agent_discs(T(disc.reshape(1, -1), dev), torch.zeros(B, dtype=torch.int32, device=dev))
    rng = np.random.default_rng(6)
    X0 = np.stack([rng.uniform(-0.5, 0.3, B), rng.uniform(-.05, .05, B), rng.uniform(-.1, .1, B), rng.uniform(.7, 1.0, B)], 1)
    x0 = T(X0, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    ci0 = eng.track_locate(x0, trk)
    res = eng.closed_loop_track(x0, trk, U0, Tn, np.ones(4), 0.0, 1, ci0, shift=True)
    tx = res.traj_x.cpu().numpy()
    assert int(res.failures.sum()) == 0
    assert (tx[:, -1, 0] > cx + r).all() and (X0[:, 0] < cx - r).all()               # everyone has passed it
    d2 = (tx[:, :, 0] - cx) ** 2 + (tx[:, :, 1] - cy) ** 2
    print(f"closest approach {np.sqrt(d2.min()):.6f} of r = {r}; unconstrained line would pass at {abs(cy):.3f}")
    assert np.sqrt(d2.min()) >= r - np.sqrt(delta)
    assert np.sqrt(d2.min(1)).max() <= r + 0.05                                      # ... and it was in the way
    eng.close()


@pytest.mark.parametrize("model,N", MODELS)
def test_one_window_track_is_the_event_loop_with_discs(dev, model, N):
    """An open track with L = S has one window: closed_loop_track is closed_loop_event on that row, bit for bit, in disc
    mode as without (tests/test_gpu_track_loop.py)"""
    B, Tn, thr, max_hold = 64, 5, 0.02, 3
    eng = engine(dev, model, N, Sigma0=10.0, max_total_inner=3000)
    _, _, x0n, cln, discs, _ = scene_batch("pacejka" if model else "standing", B)
    eng.set_agent_discs(T(discs.reshape(B, -1), dev), arange32(B, dev))
    cl = T(cln, dev)
    trk = eng.track_windows(cl, 4, 10, False)
    assert trk.R == 1
    x0 = T(x0n + np.random.default_rng(8).normal(0, 0.01, x0n.shape), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    dist = T(np.random.default_rng(5).normal(0, 4e-3, (B, Tn, eng.nx)), dev)
    w = np.ones(eng.nx)
    zero = torch.zeros(B, dtype=torch.int32, device=dev)
    r = eng.closed_loop_track(x0, trk, U0, Tn, w, thr, max_hold, zero, shift=True, disturbance=dist)
    e = eng.closed_loop_event(x0, trk.win, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist)
    assert bool((r.lam < 0).any())
    for a, b in ((r.traj_u, e.traj_u), (r.traj_x, e.traj_x), (r.x, e.x), (r.U, e.U), (r.lam, e.lam), (r.stats, e.stats),
                 (r.held, e.held), (r.solved, e.solved), (r.solve_count, e.solve_count), (r.failures, e.failures)):
        assert torch.equal(a, b)
    eng.close()
