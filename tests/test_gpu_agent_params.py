"""GPU tests of the per-agent parameter table (mpc_set_agent_params / BatchedMPC.set_agent_params): a table of rows of
vehicle and cost parameters in device memory and one row index per agent.  Every agent of a heterogeneous batch is
checked against the oracle run with that agent's own configuration; a table whose rows equal the handle's values must
give the bits of the solve without a table; the host's switch points must change no bit under a table either.
Tolerances are the ones tests/test_gpu_parity.py asserts for the same quantities on the shared path."""
import numpy as np
import pytest
import torch

from agent_tables_common import (T, assert_reference_tolerance, assert_tight, by_row, kwl, oracle_solve,
                                 param_rows_of as rows, problem, rel, table_of)
from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- the rows of the tests
def narrow_rows(O):
    """The rows of the state-constrained test: row 0 default, rows 1 .. 3 from default_rng(1)."""
    rng = np.random.default_rng(1)
    base = O.default_config(1, 10)
    out = [{}]
    for _ in range(3):
        veh = np.array(list(base.veh))
        veh[7] *= rng.uniform(.9, 1.1); veh[8] *= rng.uniform(.9, 1.1)
        out.append(dict(veh=veh, v_ref=rng.uniform(.85, 1.15), cost_w=np.array(list(base.cost_w)) * rng.uniform(.8, 1.25, 6)))
    return out


def bind(eng, dev, tab, idx, plant=None):
    t, i = T(tab, dev), T(idx, dev, torch.int32)
    eng.set_agent_params(t, i, None if plant is None else T(plant, dev, torch.int32))
    return t, i


def model_layer_checks(O, eng, dev, model, N, ocfg_of, idx, P, seed=5):
    """rhs, rollout, stage_cost and K1 of `eng` (table bound, or a handle with shared values) against the oracle run
    with every agent's own configuration: the tolerances of the shared path's tests."""
    B = len(idx)
    nx = eng.nx
    rng = np.random.default_rng(seed)
    X0 = synthetic_states(model, B, seed=B)
    cl = straight_centerline()
    u = np.stack([rng.uniform(-1, 1, B), rng.uniform(-.32, .32, B)], 1)
    U = np.tile([0.5, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N)
    dx = eng.rhs(T(X0, dev), T(u, dev)).cpu().numpy()
    X = eng.rollout(T(X0, dev), T(U, dev)).cpu().numpy()
    L = eng.stage_cost(T(X0, dev), T(u, dev), T(cl, dev)).cpu().numpy()
    psi, g, _ = eng.eval_cost_grad(T(X0, dev), T(cl, dev), T(U, dev))
    psiw, gw, _ = eng.eval_cost_grad(T(X0, dev), T(cl, dev), T(U, dev), wave=True)
    assert torch.equal(psi, psiw) and torch.equal(g, gw)                  # the wave-per-agent evaluation: same bits
    psi_c, g_c, _ = eng.eval_cost_grad(T(X0, dev), T(cl, dev), T(U, dev), want_grad=False)
    assert g_c is None and torch.equal(psi_c, psi)

    def one(p, sel):
        oc = ocfg_of(p)
        po, go = O.psi_batch(oc, X0[sel], cl, U[sel])
        return (np.stack([O.rhs(oc, X0[b], u[b]) for b in sel]), np.stack([O.rollout(oc, X0[b], U[b]) for b in sel]),
                np.array([O.stage_cost(oc, X0[b], u[b], cl) for b in sel]), po, go)
    dxo, Xo, Lo, po, go = by_row(idx, P, one)
    assert rel(dx, dxo) <= 1e-12 and np.allclose(dx, dxo, rtol=1e-10, atol=1e-13)
    assert rel(X, Xo) <= 1e-12
    assert np.allclose(L, Lo, rtol=1e-12)
    assert np.allclose(psi.cpu().numpy(), po, rtol=1e-12)
    assert rel(g.cpu().numpy(), go) <= 1e-9
    assert nx == X0.shape[1]


# ----------------------------------------------------------------------------- 6
@pytest.mark.parametrize("model,N,B", [(0, 20, 700), (0, 20, 6000), (0, 20, 20000), (1, 12, 700), (1, 12, 6000)])
def test_equal_rows_are_the_shared_path_bit_for_bit(dev, model, N, B):
    """A table whose rows all equal the handle's values: the per-agent kernels must give the bits of the kernels that
    run without a table (fixed roundings, the reciprocals of mass and inertia the correctly rounded quotients) -- in
    the persistent kernel (B = 700), through rounds and the hand-over (6 000), over several groups (20 000)."""
    cfg = mp.default_config(model, N)
    eng = mp.BatchedMPC(cfg, dev)
    X0, cl, U0 = problem(model, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    U1, _, s1 = eng.solve(X0, cl, U0)
    rng = np.random.default_rng(B)
    tab = _lib.param_rows(cfg, 3)
    keep = bind(eng, dev, tab, rng.integers(0, 3, B))
    assert eng.agent_params_bound
    U2, _, s2 = eng.solve(X0, cl, U0)
    assert torch.equal(U1, U2) and torch.equal(s1, s2)
    if B == 700:
        u = T(np.stack([rng.uniform(-1, 1, B), rng.uniform(-.32, .32, B)], 1), dev)
        Ue = T(np.tile([0.5, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N), dev)
        bound = [eng.rhs(X0, u), eng.rollout(X0, Ue), eng.stage_cost(X0, u, cl), *eng.eval_cost_grad(X0, cl, Ue)[:2],
                 *eng.eval_cost_grad(X0, cl, Ue, wave=True)[:2]]
        eng.clear_agent_params()
        assert not eng.agent_params_bound
        plain = [eng.rhs(X0, u), eng.rollout(X0, Ue), eng.stage_cost(X0, u, cl), *eng.eval_cost_grad(X0, cl, Ue)[:2],
                 *eng.eval_cost_grad(X0, cl, Ue, wave=True)[:2]]
        for a, b in zip(bound, plain):
            assert torch.equal(a, b)
    else:
        eng.clear_agent_params()
    U3, _, s3 = eng.solve(X0, cl, U0)                                      # unbound: the handle is what it was
    assert torch.equal(U1, U3) and torch.equal(s1, s3)
    del keep


# ----------------------------------------------------------------------------- 7
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12), (0, 40), (1, 20)])
def test_model_layer_matches_oracle_row_by_row(dev, O, model, N):
    P, B = 8, 300
    rws = rows(O, model, P, 1)
    cfg = mp.default_config(model, N)
    eng = mp.BatchedMPC(cfg, dev)
    idx = np.arange(B) % P
    keep = bind(eng, dev, table_of(cfg, rws), idx)
    model_layer_checks(O, eng, dev, model, N, lambda p: O.default_config(model, N, **kwl(rws[p])), idx, P)
    del keep


@pytest.mark.parametrize("constr,model", [(1, 1), (1, 0), (2, 1), (2, 0)])
def test_augmented_lagrangian_terms_match_oracle_row_by_row(dev, O, constr, model):
    """As test_augmented_lagrangian_terms_match_oracle, every agent with its own row."""
    N, B, P = 10, 96, 8
    common = dict(constr_mode=constr, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], lane_halfwidth=0.05)
    rws = rows(O, model, P, 1)
    cfg = mp.default_config(model, N, **common)
    eng = mp.BatchedMPC(cfg, dev)
    m = eng.m
    idx = np.arange(B) % P
    keep = bind(eng, dev, table_of(cfg, rws), idx)
    X0 = synthetic_states(model, B, seed=3)
    rng = np.random.default_rng(9)
    U = np.tile([0.7, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N)
    y = rng.uniform(-2, 2, (B, m)); Sig = rng.uniform(1, 1e4, (B, m))
    cl = straight_centerline()
    psi, g, yh = eng.eval_cost_grad(T(X0, dev), T(cl, dev), T(U, dev), T(y, dev), T(Sig, dev))

    def one(p, sel):
        oc = O.default_config(model, N, **common, **kwl(rws[p]))
        assert O.m(oc) == m and m > 0
        po, go = O.psi_batch(oc, X0[sel], cl, U[sel], y[sel], Sig[sel])
        return po, go, np.stack([O.constraints(oc, X0[b], cl, U[b]) for b in sel])
    po, go, gU = by_row(idx, P, one)
    assert np.allclose(psi.cpu().numpy(), po, rtol=1e-12)
    assert rel(g.cpu().numpy(), go) <= 1e-9
    zeta = gU + y / Sig
    lbd = -0.05 if constr == 2 else -np.inf
    ubd = 0.05 if constr == 2 else 0.0
    ref = Sig * (zeta - np.clip(zeta, lbd, ubd))
    assert np.allclose(yh.cpu().numpy(), ref, rtol=1e-10, atol=1e-9)
    del keep


# ----------------------------------------------------------------------------- 8
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_handle_with_non_default_shared_values_matches_oracle(dev, O, model, N):
    """No table: rows 1 .. 7 each passed through mpc_config.  The model code is written for general values; this is
    the first test that runs it away from the reference's defaults on the shared path."""
    rws = rows(O, model, 8, 1)
    B = 64
    for p in range(1, 8):
        eng = mp.BatchedMPC(mp.default_config(model, N, **kwl(rws[p])), dev)
        ocfg = O.default_config(model, N, **kwl(rws[p]))
        model_layer_checks(O, eng, dev, model, N, lambda _p: ocfg, np.zeros(B, dtype=int), 1, seed=p)
        eng.close()
    Bs = 96
    X0, cl, U0 = problem(model, N, Bs)
    for p in (2, 5):
        kw = dict(alm_eps=1e-10, max_total_inner=4000)
        eng = mp.BatchedMPC(mp.default_config(model, N, **kw, **kwl(rws[p])), dev)
        U, _, st = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
        Uo, _, sto = O.solve_batch(O.default_config(model, N, **kw, **kwl(rws[p])), X0, cl, U0)
        assert_tight(U.cpu().numpy(), st.cpu().numpy(), Uo, sto)
        eng.close()


# ----------------------------------------------------------------------------- 9
SOLVE_CASES = [(0, 20, 192), (1, 12, 128)]


@pytest.mark.parametrize("model,N,B", SOLVE_CASES)
def test_solve_matches_oracle_row_by_row(dev, O, model, N, B):
    P = 8
    rws = rows(O, model, P, 1)
    idx = np.arange(B) % P
    X0, cl, U0 = problem(model, N, B)
    for kw, check in ((dict(alm_eps=1e-10, max_total_inner=4000), assert_tight),
                      (dict(max_total_inner=2000), assert_reference_tolerance)):
        cfg = mp.default_config(model, N, **kw)
        eng = mp.BatchedMPC(cfg, dev)
        keep = bind(eng, dev, table_of(cfg, rws), idx)
        U, _, st = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
        Uo, sto, _ = oracle_solve(O, model, N, [rws[p] for p in idx], X0, cl, U0, **kw)
        check(U.cpu().numpy(), st.cpu().numpy(), Uo, sto)
        del keep
        eng.close()


# ----------------------------------------------------------------------------- 10
@pytest.mark.parametrize("model,N,B", [(0, 20, 4096), (1, 12, 1536)])
def test_the_table_is_per_agent(dev, O, model, N, B):
    """Permuting the agents with their indices permutes the results; a slice of the batch with its slice of the index
    gives the slice of the results; one row per agent (P = B) equals P = 8 when the B rows are copies of the 8."""
    P = 8
    rws = rows(O, model, P, 1)
    cfg = mp.default_config(model, N)
    tab = table_of(cfg, rws)
    rng = np.random.default_rng(7)
    idx = rng.integers(0, P, B)
    X0, cl, U0 = problem(model, N, B)
    eng = mp.BatchedMPC(cfg, dev)
    clt = T(cl, dev)

    def run(X, U_, table, index):
        keep = bind(eng, dev, table, index)
        U, _, st = eng.solve(T(X, dev), clt, T(U_, dev))
        del keep
        return U, st
    U, st = run(X0, U0, tab, idx)
    assert len(torch.unique(U[:64 * P:P, :2], dim=0)) > 1                 # (the rows do differ)
    perm = rng.permutation(B)
    Up, stp = run(X0[perm], U0[perm], tab, idx[perm])
    pt = torch.as_tensor(perm, device=dev)
    assert torch.equal(Up, U[pt]) and torch.equal(stp, st[pt])
    lo, hi = B // 4 + 3, B // 4 + 3 + B // 3
    Us, sts = run(X0[lo:hi], U0[lo:hi], tab, idx[lo:hi])
    assert torch.equal(Us, U[lo:hi]) and torch.equal(sts, st[lo:hi])
    Ub, stb = run(X0, U0, tab[idx], np.arange(B))                          # P = B
    assert torch.equal(Ub, U) and torch.equal(stb, st)


# ----------------------------------------------------------------------------- 11
@pytest.mark.parametrize("model,N,B", SOLVE_CASES)
def test_host_switches_change_nothing_under_a_table(dev, O, monkeypatch, model, N, B):
    """The solves of test_solve_matches_oracle_row_by_row (alm_eps = 1e-10) through every path the host can choose:
    the persistent kernel from the start (default at this size), rounds only, no memo, no lookahead, and each
    per-agent K1 kernel -- kinematic: wave per request / two lanes / one thread per request, fused and unfused
    K1b + K1c; Pacejka: four lanes / one thread per request."""
    P = 8
    rws = rows(O, model, P, 1)
    idx = np.arange(B) % P
    X0, cl, U0 = problem(model, N, B)
    cfg = mp.default_config(model, N, alm_eps=1e-10, max_total_inner=4000)
    tab = table_of(cfg, rws)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)

    def run(env=(), solo0=False, memo=True):
        for k, v in env:
            monkeypatch.setenv(k, v)
        eng = mp.BatchedMPC(cfg, dev)          # (the switches are read when the handle is created)
        for k, _ in env:
            monkeypatch.delenv(k)
        if solo0:
            eng.set_solo_max(0)
        eng.set_memo(memo)
        keep = bind(eng, dev, tab, idx)
        U, _, st = eng.solve(X0, cl, U0)
        info = eng.last_solve_info()
        del keep
        eng.close()
        return U, st, info
    U, st, info = run()
    assert info["solo_agents"] == B
    variants = [dict(solo0=True), dict(memo=False), dict(solo0=True, memo=False),
                dict(env=(("MPC_SOLO_MAX", "0"), ("MPC_NO_QUAD", "1"), ("MPC_WIDE_MAX", "-1"))),
                dict(env=(("MPC_SOLO_MAX", "0"), ("MPC_UNFUSED_EVAL", "1")))]
    if model == 0:
        variants += [dict(env=(("MPC_SOLO_MAX", "0"), ("MPC_WIDE_MAX", "-1"))),
                     dict(env=(("MPC_SOLO_MAX", "0"), ("MPC_WIDE_MAX", "-1"), ("MPC_UNFUSED_EVAL", "1"))),
                     dict(env=(("MPC_SOLO_MAX", "24"),))]
    else:
        variants += [dict(env=(("MPC_NO_LOOKAHEAD", "1"),)), dict(env=(("MPC_SOLO_MAX", "16"), ("MPC_PAC_QUAD_MAX", "100")))]
    for v in variants:
        Uv, stv, iv = run(**v)
        assert torch.equal(U, Uv) and torch.equal(st, stv), v
        if v.get("solo0") or ("MPC_SOLO_MAX", "0") in v.get("env", ()):
            assert iv["solo_agents"] == 0 and iv["rounds"] > 0


def test_groups_change_nothing_under_a_table(dev, O):
    model, N, B, P = 0, 20, 20000, 8
    cfg = mp.default_config(model, N)
    tab = table_of(cfg, rows(O, model, P, 1))
    idx = np.random.default_rng(3).integers(0, P, B)
    X0, cl, U0 = problem(model, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx)
    eng.set_groups(1)
    U1, _, s1 = eng.solve(X0, cl, U0)
    eng.set_groups(3)
    U3, _, s3 = eng.solve(X0, cl, U0)
    assert eng.last_solve_info()["groups"] == 3
    assert torch.equal(U1, U3) and torch.equal(s1, s3)
    del keep


# ----------------------------------------------------------------------------- 12
def test_in_place_row_refresh_is_seen(dev, O):
    """The library reads the caller's table at every call: a row rewritten in place is used by the next solve
    without binding again."""
    model, N, B, P = 0, 20, 192, 8
    rws = rows(O, model, P, 1)
    cfg = mp.default_config(model, N)
    tab = table_of(cfg, rws)
    idx = np.arange(B) % P
    X0, cl, U0 = problem(model, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    t, i = bind(eng, dev, tab, idx)
    U1, _, _ = eng.solve(X0, cl, U0)
    tab2 = tab.copy()
    tab2[3] = table_of(cfg, rows(O, model, P, 2))[5]
    t.data[3].copy_(T(tab2[3], dev))
    U2, _, s2 = eng.solve(X0, cl, U0)
    fresh = mp.BatchedMPC(cfg, dev)
    keep = bind(fresh, dev, tab2, idx)
    U3, _, s3 = fresh.solve(X0, cl, U0)
    assert torch.equal(U2, U3) and torch.equal(s2, s3)
    changed = torch.as_tensor(idx == 3, device=dev)
    assert not torch.equal(U1[changed], U2[changed]) and torch.equal(U1[~changed], U2[~changed])
    del keep, i


# ----------------------------------------------------------------------------- 13
def test_state_constraints_row_by_row(dev, O):
    """The assertions of test_solve_with_state_constraints_matches_oracle, every agent on its own (narrow) row."""
    N, B, P = 10, 48, 4
    common = dict(constr_mode=1, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], Sigma0=10.0,
                  alm_eps=1e-8, max_total_inner=6000)
    rws = narrow_rows(O)
    cfg = mp.default_config(1, N, **common)
    X0 = synthetic_states(1, B, seed=4)
    X0[:, 0] *= 3.9 / 5.0
    X0[:, 3] = np.minimum(X0[:, 3], 0.65)
    cl, U0 = straight_centerline(), np.tile([1., 0.], (B, N))
    idx = np.arange(B) % P
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, table_of(cfg, rws), idx)
    U, lam, st = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    U, lam, st = U.cpu().numpy(), lam.cpu().numpy(), st.cpu().numpy()
    Uo, sto, lamo = oracle_solve(O, 1, N, [rws[p] for p in idx], X0, cl, U0, **common)
    assert (sto[:, 0] == 1).all() and (st[:, 0] == 1).mean() >= 0.97
    conv = (st[:, 0] == 1) & (sto[:, 0] == 1)
    d = np.abs(U - Uo).max(1)
    match = conv & (d <= 1e-5)
    assert match.sum() >= 0.9 * conv.sum()
    assert np.allclose(lam[match], lamo[match], rtol=1e-3, atol=1e-5)
    assert lam.min() >= 0.0 and lam[conv].max() > 1e-3
    gU = np.stack([O.constraints(O.default_config(1, N, **common, **kwl(rws[idx[b]])), X0[b], cl, U[b]) for b in range(B)])
    assert gU[conv].max() <= 2e-4
    assert np.all(st[conv, 1] == sto[conv, 1])
    del keep


# ----------------------------------------------------------------------------- 14
def test_closed_loop_with_a_different_plant(dev, O):
    """mpc_closed_loop under a table: the controller solves with row index[b], the plant advances with row
    plant_index[b] -- against the same loop driven from the host (the pattern of
    test_device_closed_loop_matches_host_loop)."""
    N, B, Tn, P = 12, 32, 10, 4
    cfg = mp.default_config(1, N, max_total_inner=1500)
    tab = table_of(cfg, rows(O, 1, P, 1))
    rng = np.random.default_rng(2)
    idx, pidx = rng.integers(0, P, B), rng.integers(0, P, B)
    assert (idx != pidx).any()
    X0 = T(synthetic_states(1, B, seed=13), dev)
    cl = T(straight_centerline(), dev)
    U0 = T(np.tile([1., 0.], (B, N)), dev)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx, pidx)
    xT, U, _, tx, tu, fails, _ = eng.closed_loop(X0, cl, U0, Tn)
    ctl, plant = mp.BatchedMPC(cfg, dev), mp.BatchedMPC(cfg, dev)
    k1, k2 = bind(ctl, dev, tab, idx), bind(plant, dev, tab, pidx)
    x, Uw = X0, U0
    for t in range(Tn):
        Uw, _, st = ctl.solve(x, cl, Uw)
        u0 = Uw[:, :2].contiguous()
        x = plant.rollout(x, u0)[:, 0, :].contiguous()
        assert torch.equal(tx[:, t], x) and torch.equal(tu[:, t], u0)
    assert torch.equal(xT, x) and torch.equal(U, Uw)
    # plant_index = None is plant_index = index
    keep = bind(eng, dev, tab, idx, idx)
    a = eng.closed_loop(X0, cl, U0, 3)
    keep = bind(eng, dev, tab, idx)
    b = eng.closed_loop(X0, cl, U0, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert not torch.equal(a[3], tx[:, :3])                               # (and the other plant does differ)
    del keep, k1, k2


# ----------------------------------------------------------------------------- 15
def test_controller_honours_rewritten_vehicle_parameters(dev):
    """MPCController.__call__ after the caller changed the mass in problem.param (main.py:119) returns what a
    controller constructed with the new param returns; unchanged parameters take the path without a table."""
    from model_predictive_control_amd import main as mpc_main
    from model_predictive_control_amd.car_dynamics import KinematicBicyclePacejka
    model = KinematicBicyclePacejka(); model.dynamics()
    cl = mpc_main.get_centerline(100).ravel(order="F")
    y0 = np.array([0.2, 0.1, 0.05, 0.7, 0.0, 0.1])

    def controller(mass_factor):
        prob = mpc_main.create_casadi_problem(model, 12, 100, 1.0, 1.0, 0.32)
        prob.param[6 + 200 + 7] *= mass_factor
        c = mpc_main.MPCController(model, prob, 12); c.verbose = False
        return c, prob
    c1, prob1 = controller(1.0)
    bound = []
    orig = c1.solver.solve
    c1.solver.solve = lambda *a, **k: (bound.append(c1.solver.agent_params_bound), orig(*a, **k))[1]
    Ua = c1(y0, cl).copy()
    assert bound == [False] and not c1.solver.agent_params_bound         # unchanged: today's path
    prob1.param[6 + 200 + 7] *= 1.15
    c1.U = np.tile([1, 0], 12)
    Ub = c1(y0, cl).copy()
    assert bound == [False, True] and not c1.solver.agent_params_bound
    c2, _ = controller(1.15)
    Uc = c2(y0, cl)
    assert np.array_equal(Ub, Uc) and np.array_equal(c1.last_stats, c2.last_stats)
    assert not np.array_equal(Ua, Ub)
    # the batched entry points take a table for one call
    Y = np.stack([y0, y0, y0])
    tab = _lib.param_rows(c2.cfg, 2)
    tab[1, 7] /= 1.15
    Ut, _ = c2.solve(Y, cl, params=tab, param_index=[0, 1, 0])
    assert not c2.solver.agent_params_bound
    assert np.array_equal(Ut[0].cpu().numpy(), Uc) and torch.equal(Ut[0], Ut[2]) and np.array_equal(Ut[1].cpu().numpy(), Ua)
    assert torch.equal(c2.step(Y, cl, params=tab, param_index=[0, 1, 0]), Ut[:, :2])


# ----------------------------------------------------------------------------- 16
def test_refusals(dev):
    """None of these reaches a kernel."""
    N, B = 12, 64
    cfg = mp.default_config(1, N)
    eng = mp.BatchedMPC(cfg, dev)
    tab = _lib.param_rows(cfg, 4)
    idx = np.arange(B) % 4
    X0, cl, U0 = problem(1, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    keep = bind(eng, dev, tab, idx)
    u = T(np.zeros((B - 1, 2)), dev)
    for call in (lambda: eng.solve(X0[:B - 1].contiguous(), cl, U0[:B - 1].contiguous()),
                 lambda: eng.rhs(X0[:B - 1].contiguous(), u), lambda: eng.rollout(X0[:B - 1].contiguous(), u),
                 lambda: eng.stage_cost(X0[:B - 1].contiguous(), u, cl),
                 lambda: eng.eval_cost_grad(X0[:B - 1].contiguous(), cl, U0[:B - 1].contiguous()),
                 lambda: eng.eval_cost_grad(X0[:B - 1].contiguous(), cl, U0[:B - 1].contiguous(), wave=True),
                 lambda: eng.closed_loop(X0[:B - 1].contiguous(), cl, U0[:B - 1].contiguous(), 2)):
        with pytest.raises(mp.MpcError, match="bound parameter table"):
            call()
    eng.solve(X0, cl, U0)                                                  # the bound size is served
    # binding while an asynchronous solve is in flight
    wait = eng.solve_async(X0, cl, U0)
    with pytest.raises(mp.MpcError):
        bind(eng, dev, tab, idx)
    rc = eng.lib.mpc_set_agent_params(eng._h, None, 0, None, None, 0)      # the library refuses as well
    assert rc == -1 and b"in flight" in eng.lib.mpc_last_error()
    wait()
    # rows the model cannot run
    for col, val, models in ((5, np.nan, (0, 1)), (30, np.inf, (0, 1)), (1, -0.06, (0, 1)), (7, 0.0, (1,)), (8, -1.0, (1,))):
        for model in models:
            c = mp.default_config(model, N)
            e = mp.BatchedMPC(c, dev)
            bad = _lib.param_rows(c, 4)
            bad[2, col] = val
            with pytest.raises(mp.MpcError, match="row 2"):
                bind(e, dev, bad, idx)
            assert not e.agent_params_bound
            e.close()
    # the kinematic model does not read mass or inertia: not refused there
    c = mp.default_config(0, N)
    e = mp.BatchedMPC(c, dev)
    ok = _lib.param_rows(c, 4)
    ok[2, 7] = 0.0
    k2 = bind(e, dev, ok, idx)
    e.close()
    # index ranges, shapes and dtypes are the front end's to refuse
    t = T(tab, dev)
    for bad_idx in (np.where(np.arange(B) == 5, 4, idx), np.where(np.arange(B) == 9, -1, idx)):
        with pytest.raises(ValueError, match="out of range"):
            eng.set_agent_params(t, T(bad_idx, dev, torch.int32))
        with pytest.raises(ValueError, match="out of range"):
            eng.set_agent_params(t, T(idx, dev, torch.int32), T(bad_idx, dev, torch.int32))
    with pytest.raises(TypeError):
        eng.set_agent_params(t, T(idx, dev, torch.int64))
    with pytest.raises(TypeError):
        eng.set_agent_params(t.float(), T(idx, dev, torch.int32))
    with pytest.raises(ValueError):
        eng.set_agent_params(t[:, :30].contiguous(), T(idx, dev, torch.int32))
    with pytest.raises(ValueError):
        eng.set_agent_params(t.cpu(), T(idx, dev, torch.int32))
    with pytest.raises(ValueError):
        eng.set_agent_params(T(np.tile(tab, (1, 2)), dev)[:, ::2], T(idx, dev, torch.int32))   # not contiguous
    del keep, k2


# ----------------------------------------------------------------------------- 17
def test_full_size_heterogeneous_batch(dev, O):
    model, N, B, P = 0, 20, 65536, 4096
    kw = dict(alm_eps=1e-10, max_total_inner=4000)
    rws = rows(O, model, P, 1)
    cfg = mp.default_config(model, N, **kw)
    tab = table_of(cfg, rws)
    rng = np.random.default_rng(17)
    idx = rng.integers(0, P, B)
    X0, cl, U0 = problem(model, N, B)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx)
    Xt, ct, Ut = T(X0, dev), T(cl, dev), T(U0, dev)
    U, _, st = eng.solve(Xt, ct, Ut)
    U2, _, st2 = eng.solve(Xt, ct, Ut)
    assert torch.equal(U, U2) and torch.equal(st, st2)                    # deterministic
    lb, ub = T(list(cfg.u_lb), dev).repeat(N), T(list(cfg.u_ub), dev).repeat(N)
    assert bool(((U >= lb) & (U <= ub)).all())
    psi0, _, _ = eng.eval_cost_grad(Xt, ct, Ut, want_grad=False)
    conv = st[:, 0] == 1
    assert conv.float().mean() >= 0.97
    assert bool((st[conv, 6] <= psi0[conv] + 1e-12).all())                # not above the warm start's cost
    sample = np.sort(rng.choice(B, 512, replace=False))
    Uo, sto = np.empty((512, 2 * N)), np.empty((512, 8))
    for j, b in enumerate(sample):
        Uo[j], _, sto[j] = O.solve(O.default_config(model, N, **kw, **kwl(rws[idx[b]])), X0[b], cl, U0[b])
    s = torch.as_tensor(sample, device=dev)
    assert_tight(U[s].cpu().numpy(), st[s].cpu().numpy(), Uo, sto)
    del keep
