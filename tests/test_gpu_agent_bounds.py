"""GPU tests of the per-agent bounds table (mpc_set_agent_bounds / BatchedMPC.set_agent_bounds): a table of input boxes
[u_lb[0], u_lb[1], u_ub[0], u_ub[1]] in device memory and one row index per agent, beside the parameter table.  Every
agent of a batch with different boxes is checked against the oracle run with that agent's own u_lb / u_ub; a table
whose rows equal the handle's box must give the bits of the solve without a table; the host's switch points must
change no bit under a table either.  Tolerances are the ones tests/test_gpu_parity.py and
tests/test_gpu_agent_params.py assert for the same quantities (the helpers are those of tests/agent_tables_common.py)."""
import numpy as np
import pytest
import torch

from agent_tables_common import (T, assert_reference_tolerance, assert_tight, box_rows_of as bound_rows, kwl,
                                 oracle_solve, param_rows_of as rows, problem, table_of)
from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- the rows of the tests
def btable(rws):
    """[P, 4] host table of the rows."""
    return np.array([list(r["u_lb"]) + list(r["u_ub"]) for r in rws], dtype=np.float64)


def bind(eng, dev, tab, idx):
    t, i = T(tab, dev), T(idx, dev, torch.int32)
    eng.set_agent_bounds(t, i)
    return t, i


def bind_params(eng, dev, tab, idx):
    t, i = T(tab, dev), T(idx, dev, torch.int32)
    eng.set_agent_params(t, i)
    return t, i


def assert_inside(U, tab, idx, N):
    """Every control inside its agent's own box, exactly."""
    t = np.asarray(tab)[np.asarray(idx)]
    lb, ub = np.tile(t[:, 0:2], (1, N)), np.tile(t[:, 2:4], (1, N))
    U = U.cpu().numpy() if isinstance(U, torch.Tensor) else U
    assert np.all(U >= lb) and np.all(U <= ub)


# ----------------------------------------------------------------------------- 1
SOLVE_CASES = [(0, 20, 192), (1, 12, 128), (0, 40, 64)]


@pytest.mark.parametrize("model,N,B", SOLVE_CASES)
def test_solve_matches_oracle_agent_by_agent(dev, O, model, N, B):
    P = 8
    rws = bound_rows(P, 7)
    tab = btable(rws)
    idx = np.arange(B) % P
    X0, cl, U0 = problem(model, N, B)
    # the warm start [1, 0] lies outside the box of 7 rows in 8: the first prox step must bring it in
    assert sum(not (r["u_lb"][0] <= 1.0 <= r["u_ub"][0]) for r in rws) == 7
    for kw, check in ((dict(alm_eps=1e-10, max_total_inner=4000), assert_tight),
                      (dict(max_total_inner=2000), assert_reference_tolerance)):
        cfg = mp.default_config(model, N, **kw)
        eng = mp.BatchedMPC(cfg, dev)
        keep = bind(eng, dev, tab, idx)
        assert eng.agent_bounds_bound
        U, _, st = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
        Uo, sto, _ = oracle_solve(O, model, N, [rws[p] for p in idx], X0, cl, U0, **kw)
        check(U.cpu().numpy(), st.cpu().numpy(), Uo, sto)
        assert_inside(U, tab, idx, N)
        # (a bound is active at the solution for most agents: the active-set code is what is being tested)
        t = tab[idx]
        Un = U.cpu().numpy()
        active = ((Un == np.tile(t[:, 0:2], (1, N))) | (Un == np.tile(t[:, 2:4], (1, N)))).any(1)
        assert active.mean() >= 0.5
        del keep
        eng.close()


# ----------------------------------------------------------------------------- 2
@pytest.mark.parametrize("model,N,B", [(0, 20, 700), (0, 20, 6000), (0, 20, 20000), (1, 12, 700), (1, 12, 6000)])
def test_equal_rows_are_the_shared_path_bit_for_bit(dev, model, N, B):
    """A table whose rows all equal the handle's box: the per-agent-box kernels must give the bits of the kernels that
    run without a table -- in the persistent kernel (B = 700), through rounds and the hand-over (6 000), over several
    groups (20 000); with one row and with 64 rows under random indices; with and without a parameter table."""
    cfg = mp.default_config(model, N)
    eng = mp.BatchedMPC(cfg, dev)
    X0, cl, U0 = problem(model, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    lam0 = None
    U1, lam1, s1 = eng.solve(X0, cl, U0, lam0)
    rng = np.random.default_rng(B)
    assert np.array_equal(_lib.bound_rows(cfg, 1)[0], [-1.0, -0.32, 1.0, 0.32])
    for P, idx in ((1, np.zeros(B, dtype=int)), (64, rng.integers(0, 64, B))):
        keep = bind(eng, dev, _lib.bound_rows(cfg, P), idx)
        U2, lam2, s2 = eng.solve(X0, cl, U0, lam0)
        assert torch.equal(U1, U2) and torch.equal(s1, s2), P
        assert lam1 is None and lam2 is None                               # (no constraints: no multipliers)
        del keep
    # ... and with a parameter table of equal rows bound beside it (either order of binding)
    kp = bind_params(eng, dev, _lib.param_rows(cfg, 3), rng.integers(0, 3, B))
    keep = bind(eng, dev, _lib.bound_rows(cfg, 64), rng.integers(0, 64, B))
    assert eng.agent_params_bound and eng.agent_bounds_bound
    U3, _, s3 = eng.solve(X0, cl, U0)
    assert torch.equal(U1, U3) and torch.equal(s1, s3)
    eng.clear_agent_params()
    U4, _, s4 = eng.solve(X0, cl, U0)                                      # the bounds table alone again
    assert torch.equal(U1, U4) and torch.equal(s1, s4)
    eng.clear_agent_bounds()
    assert not eng.agent_bounds_bound
    U5, _, s5 = eng.solve(X0, cl, U0)                                      # unbound: the handle is what it was
    assert torch.equal(U1, U5) and torch.equal(s1, s5)
    del keep, kp


# ----------------------------------------------------------------------------- 3
@pytest.mark.parametrize("model,N,B", [(0, 20, 4096), (1, 12, 1536)])
def test_the_table_is_per_agent(dev, model, N, B):
    """Permuting the agents with their indices permutes the results; a slice of the batch with its slice of the index
    gives the slice of the results; one row per agent (P = B) equals P = 8 when the B rows are copies of the 8."""
    P = 8
    tab = btable(bound_rows(P, 7))
    cfg = mp.default_config(model, N)
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
    assert_inside(U, tab, idx, N)
    eng.clear_agent_bounds()
    Uplain, _, _ = eng.solve(T(X0, dev), clt, T(U0, dev))
    other = torch.as_tensor(idx != 0, device=dev)
    assert not torch.equal(U[other], Uplain[other])                        # the rows do change the result
    same = torch.as_tensor(idx == 0, device=dev)
    assert torch.equal(U[same], Uplain[same])                              # ... and row 0 is the handle's box
    perm = rng.permutation(B)
    Up, stp = run(X0[perm], U0[perm], tab, idx[perm])
    pt = torch.as_tensor(perm, device=dev)
    assert torch.equal(Up, U[pt]) and torch.equal(stp, st[pt])
    lo, hi = B // 4 + 3, B // 4 + 3 + B // 3
    Us, sts = run(X0[lo:hi], U0[lo:hi], tab, idx[lo:hi])
    assert torch.equal(Us, U[lo:hi]) and torch.equal(sts, st[lo:hi])
    Ub, stb = run(X0, U0, tab[idx], np.arange(B))                          # P = B
    assert torch.equal(Ub, U) and torch.equal(stb, st)


# ----------------------------------------------------------------------------- 4
@pytest.mark.parametrize("model,N,B", SOLVE_CASES)
def test_host_switches_change_nothing_under_a_bounds_table(dev, monkeypatch, model, N, B):
    """The solves of test_solve_matches_oracle_agent_by_agent (alm_eps = 1e-10) through every path the host can choose:
    the persistent kernel from the start (default at this size), rounds only, no memo, no lookahead, each K1 kernel,
    the hand-over at a small count, and every instantiation of the step kernel -- chain blocks, history from global
    memory, a short LDS copy, 4 and 64 agents per workgroup."""
    P = 8
    tab = btable(bound_rows(P, 7))
    idx = np.arange(B) % P
    X0, cl, U0 = problem(model, N, B)
    cfg = mp.default_config(model, N, alm_eps=1e-10, max_total_inner=4000)
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
    r0 = ("MPC_SOLO_MAX", "0")
    variants = [dict(solo0=True), dict(memo=False), dict(solo0=True, memo=False),
                dict(env=(r0, ("MPC_NO_QUAD", "1"), ("MPC_WIDE_MAX", "-1"))),
                dict(env=(r0, ("MPC_UNFUSED_EVAL", "1"))),
                dict(env=(r0, ("MPC_CHAIN_MIN", "0"))),
                dict(env=(r0, ("MPC_STEP_REGS", "1"))), dict(env=(r0, ("MPC_LDS_PAIRS", "3"))),
                dict(env=(r0, ("MPC_APB", "4"))), dict(env=(r0, ("MPC_APB", "64"))),
                dict(env=(r0, ("MPC_APB", "64"), ("MPC_CHAIN_MIN", "0"), ("MPC_LDS_PAIRS", "3"))),
                dict(env=(("MPC_STEP_REGS", "1"),))]
    if model == 0:
        variants += [dict(env=(r0, ("MPC_WIDE_MAX", "-1"))),
                     dict(env=(r0, ("MPC_WIDE_MAX", "-1"), ("MPC_UNFUSED_EVAL", "1"))),
                     dict(env=(("MPC_SOLO_MAX", "24"),))]
    else:
        variants += [dict(env=(("MPC_NO_LOOKAHEAD", "1"),)), dict(env=(("MPC_SOLO_MAX", "16"), ("MPC_PAC_QUAD_MAX", "100")))]
    for v in variants:
        Uv, stv, iv = run(**v)
        assert torch.equal(U, Uv) and torch.equal(st, stv), v
        if v.get("solo0") or r0 in v.get("env", ()):
            assert iv["solo_agents"] == 0 and iv["rounds"] > 0


def test_groups_change_nothing_under_a_bounds_table(dev):
    model, N, B, P = 0, 20, 20000, 8
    cfg = mp.default_config(model, N)
    tab = btable(bound_rows(P, 7))
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
    assert_inside(U1, tab, idx, N)
    del keep


# ----------------------------------------------------------------------------- 5
def test_state_constraints_agent_by_agent(dev, O, monkeypatch):
    """The assertions of test_state_constraints_row_by_row, every agent on its own box and no parameter table."""
    N, B, P = 10, 48, 4
    common = dict(constr_mode=1, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], Sigma0=10.0,
                  alm_eps=1e-8, max_total_inner=6000)
    rws = bound_rows(P, 11)
    tab = btable(rws)
    cfg = mp.default_config(1, N, **common)
    X0 = synthetic_states(1, B, seed=4)
    X0[:, 0] *= 3.9 / 5.0
    X0[:, 3] = np.minimum(X0[:, 3], 0.65)
    cl, U0 = straight_centerline(), np.tile([1., 0.], (B, N))
    idx = np.arange(B) % P
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx)
    Ut, lamt, stt = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    U, lam, st = Ut.cpu().numpy(), lamt.cpu().numpy(), stt.cpu().numpy()
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
    assert_inside(U, tab, idx, N)
    del keep
    eng.close()
    # the constrained (HASM) step kernels' box forms: rounds only, with the history in LDS and from global memory
    for env in ((), (("MPC_STEP_REGS", "1"),)):
        for k, v in env:
            monkeypatch.setenv(k, v)
        e2 = mp.BatchedMPC(cfg, dev)
        for k, _ in env:
            monkeypatch.delenv(k)
        e2.set_solo_max(0)
        keep = bind(e2, dev, tab, idx)
        U2, lam2, st2 = e2.solve(T(X0, dev), T(cl, dev), T(U0, dev))
        assert e2.last_solve_info()["solo_agents"] == 0
        assert torch.equal(U2, Ut) and torch.equal(lam2, lamt) and torch.equal(st2, stt), env
        del keep
        e2.close()


# ----------------------------------------------------------------------------- 6
@pytest.mark.parametrize("model,N,B", [(0, 20, 192), (1, 12, 128)])
def test_both_tables_at_once(dev, O, model, N, B):
    kw = dict(alm_eps=1e-10, max_total_inner=4000)
    prw, brw = rows(O, model, 8, 1), bound_rows(8, 7)
    pidx, bidx = np.arange(B) % 8, (np.arange(B) // 8) % 8
    assert (pidx != bidx).any()
    cfg = mp.default_config(model, N, **kw)
    X0, cl, U0 = problem(model, N, B)
    eng = mp.BatchedMPC(cfg, dev)
    kp = bind_params(eng, dev, table_of(cfg, prw), pidx)
    kb = bind(eng, dev, btable(brw), bidx)
    U, _, st = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    Uo, sto, _ = oracle_solve(O, model, N, [dict(prw[pidx[b]], **brw[bidx[b]]) for b in range(B)], X0, cl, U0, **kw)
    assert_tight(U.cpu().numpy(), st.cpu().numpy(), Uo, sto)
    assert_inside(U, btable(brw), bidx, N)
    eng.set_solo_max(0)                                                    # the same through the rounds
    U2, _, st2 = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    assert torch.equal(U, U2) and torch.equal(st, st2)
    del kp, kb


# ----------------------------------------------------------------------------- 7
def test_in_place_row_refresh_is_seen(dev):
    """The library reads the caller's table at every call: a row rewritten in place is used by the next solve
    without binding again."""
    model, N, B, P = 0, 20, 192, 8
    cfg = mp.default_config(model, N)
    tab = btable(bound_rows(P, 7))
    idx = np.arange(B) % P
    X0, cl, U0 = problem(model, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    t, i = bind(eng, dev, tab, idx)
    U1, _, _ = eng.solve(X0, cl, U0)
    tab2 = tab.copy()
    tab2[3] = btable(bound_rows(P, 8))[5]
    assert not np.array_equal(tab2[3], tab[3])
    t.data[3].copy_(T(tab2[3], dev))
    U2, _, s2 = eng.solve(X0, cl, U0)
    fresh = mp.BatchedMPC(cfg, dev)
    keep = bind(fresh, dev, tab2, idx)
    U3, _, s3 = fresh.solve(X0, cl, U0)
    assert torch.equal(U2, U3) and torch.equal(s2, s3)
    changed = torch.as_tensor(idx == 3, device=dev)
    assert not torch.equal(U1[changed], U2[changed]) and torch.equal(U1[~changed], U2[~changed])
    del keep, i


# ----------------------------------------------------------------------------- 8
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_masked_solve_and_loops_under_a_bounds_table(dev, model, N):
    B, P, Tn = 96, 8, 6
    cfg = mp.default_config(model, N, max_total_inner=2000)
    tab = btable(bound_rows(P, 7))
    rng = np.random.default_rng(5)
    idx = rng.integers(0, P, B)
    X0, cl, U0 = problem(model, N, B, seed=13)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx)
    # solve_active = the whole solve + where; the rows of inactive agents are not written
    U, _, st = eng.solve(X0, cl, U0)
    mask = T(rng.random(B) < 0.4, dev, torch.bool)
    assert 0 < int(mask.sum()) < B
    Uin = torch.where(mask[:, None], U0, torch.full_like(U0, float("nan")))
    stin = torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev)
    Ua, _, sta, n = eng.solve_active(X0, cl, Uin, mask, stats=stin)
    assert n == int(mask.sum())
    assert torch.equal(Ua[mask], U[mask]) and torch.equal(sta[mask], st[mask])
    assert bool(torch.isnan(Ua[~mask]).all()) and bool(torch.isnan(sta[~mask]).all())
    # closed_loop = the host loop of solve and rollout
    xT, Uc, _, tx, tu, fails, _ = eng.closed_loop(X0, cl, U0, Tn)
    host = mp.BatchedMPC(cfg, dev)
    k2 = bind(host, dev, tab, idx)
    x, Uw = X0, U0
    for t in range(Tn):
        Uw, _, _ = host.solve(x, cl, Uw)
        u0 = Uw[:, :2].contiguous()
        x = host.rollout(x, u0)[:, 0, :].contiguous()
        assert torch.equal(tx[:, t], x) and torch.equal(tu[:, t], u0)
    assert torch.equal(xT, x) and torch.equal(Uc, Uw)
    # closed_loop_event with thr = 0 re-plans every agent at every step: closed_loop, bit for bit
    r = eng.closed_loop_event(X0, cl, U0, Tn, np.ones(eng.nx), 0.0, 3)
    assert bool((r.solved == 1).all())
    assert torch.equal(r.traj_x, tx) and torch.equal(r.traj_u, tu) and torch.equal(r.x, xT) and torch.equal(r.U, Uc)
    # an event-triggered loop that does hold plans: every applied control inside its agent's box
    r2 = eng.closed_loop_event(X0, cl, U0, Tn, np.ones(eng.nx), 0.05, 3, shift=True)
    assert 0 < int(r2.solved.sum()) < B * Tn
    t4 = tab[idx]
    for tu_ in (tu, r2.traj_u):
        tun = tu_.cpu().numpy()
        assert np.all(tun >= t4[:, None, 0:2]) and np.all(tun <= t4[:, None, 2:4])
    del keep, k2


# ----------------------------------------------------------------------------- 9
def test_prox_step_per_agent(dev):
    """K2 under a table of different boxes: p = clamp(-gamma grad, lb_b - x, ub_b - x) with comparison-selects is exact
    arithmetic -> bit-exact (sums as test_prox_step_matches_definition)."""
    N, B, P = 20, 257, 8
    eng = mp.BatchedMPC(mp.default_config(0, N), dev)
    tab = btable(bound_rows(P, 7))
    rng = np.random.default_rng(4)
    idx = rng.integers(0, P, B)
    keep = bind(eng, dev, tab, idx)
    x = rng.uniform(-1.2, 1.2, (B, 2 * N)) * np.tile([1, .32], N)
    g = rng.standard_normal((B, 2 * N)); gam = rng.uniform(1e-3, 2.0, B)
    g[3, 5] = np.nan                                                       # a NaN gradient stays a NaN step
    xh, p, out = eng.prox_step(T(x, dev), T(g, dev), T(gam, dev))
    t4 = tab[idx]
    lo, hi = np.tile(t4[:, 0:2], (1, N)) - x, np.tile(t4[:, 2:4], (1, N)) - x
    pr = -gam[:, None] * g
    pr = np.where(pr < lo, lo, pr)
    pr = np.where(hi < pr, hi, pr)
    assert np.isnan(pr[3, 5]) and np.isnan(p.cpu().numpy()[3, 5])
    assert np.array_equal(p.cpu().numpy(), pr, equal_nan=True)
    assert np.array_equal(xh.cpu().numpy(), x + pr, equal_nan=True)
    ok = np.arange(B) != 3
    assert np.allclose(out.cpu().numpy()[ok, 0], (pr * pr).sum(1)[ok], rtol=1e-13)
    assert np.allclose(out.cpu().numpy()[ok, 1], (g * pr).sum(1)[ok], rtol=1e-12, atol=1e-12)
    assert (pr[ok] != np.minimum(np.maximum(-gam[:, None] * g, np.tile([-1, -.32], N) - x), np.tile([1, .32], N) - x)[ok]).any()
    del keep


# ----------------------------------------------------------------------------- 10
def test_refusals(dev):
    """None of these reaches a kernel, and the handle stays usable."""
    N, B, E_ARG = 12, 64, -1
    cfg = mp.default_config(1, N)
    eng = mp.BatchedMPC(cfg, dev)
    tab = btable(bound_rows(4, 7))
    idx = np.arange(B) % 4
    X0, cl, U0 = problem(1, N, B)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    Uplain, _, splain = eng.solve(X0, cl, U0)
    t, i = T(tab, dev), T(idx, dev, torch.int32)
    ptr = lambda z: None if z is None else z.data_ptr()
    raw = lambda table, P, index, Bn: eng.lib.mpc_set_agent_bounds(eng._h, ptr(table), P, ptr(index), Bn)
    # lb > ub in a row, a NaN row
    for col, val in ((0, 2.0), (3, -0.4), (1, np.nan), (2, np.nan)):
        bad = tab.copy(); bad[2, col] = val
        assert raw(T(bad, dev), 4, i, B) == E_ARG and b"row 2" in eng.lib.mpc_last_error()
        with pytest.raises(mp.MpcError, match="row 2"):
            bind(eng, dev, bad, idx)
        assert not eng.agent_bounds_bound
    # infinities pass (the rule of mpc_create)
    inf = tab.copy(); inf[1] = [-np.inf, -np.inf, np.inf, np.inf]
    assert raw(T(inf, dev), 4, i, B) == 0
    assert raw(None, 0, None, 0) == 0
    # P <= 0, a NULL index, B <= 0
    assert raw(t, 0, i, B) == E_ARG and raw(t, -1, i, B) == E_ARG
    assert raw(t, 4, None, B) == E_ARG and b"mpc_set_agent_bounds" in eng.lib.mpc_last_error()
    assert raw(t, 4, i, 0) == E_ARG
    # another batch size at solve time, in every call that reads the box
    keep = bind(eng, dev, tab, idx)
    Xs, Us = X0[:B - 1].contiguous(), U0[:B - 1].contiguous()
    gam = torch.ones(B - 1, dtype=torch.float64, device=dev)
    act = torch.ones(B - 1, dtype=torch.int32, device=dev)
    for call in (lambda: eng.solve(Xs, cl, Us), lambda: eng.prox_step(Us, Us, gam), lambda: eng.solve_active(Xs, cl, Us, act),
                 lambda: eng.closed_loop(Xs, cl, Us, 2),
                 lambda: eng.closed_loop_event(Xs, cl, Us, 2, np.ones(eng.nx), 0.0, 3)):
        with pytest.raises(mp.MpcError, match="bound bounds table"):
            call()
    eng.rollout(Xs, Us[:, :2].contiguous())                                # (the model layer does not read the box)
    Ub, _, sb = eng.solve(X0, cl, U0)                                      # the bound size is served
    # a second table for another B than the bound one's, either way round
    ptab = T(_lib.param_rows(cfg, 2), dev)
    with pytest.raises(mp.MpcError, match="bounds table"):
        eng.set_agent_params(ptab, torch.zeros(B - 1, dtype=torch.int32, device=dev))
    assert not eng.agent_params_bound
    eng.clear_agent_bounds()
    eng.set_agent_params(ptab, torch.zeros(B - 1, dtype=torch.int32, device=dev))
    with pytest.raises(mp.MpcError, match="parameter table"):
        bind(eng, dev, tab, idx)
    assert not eng.agent_bounds_bound
    eng.clear_agent_params()
    # binding during an asynchronous solve
    wait = eng.solve_async(X0, cl, U0)
    with pytest.raises(mp.MpcError):
        bind(eng, dev, tab, idx)
    assert raw(t, 4, i, B) == E_ARG and b"in flight" in eng.lib.mpc_last_error()
    assert raw(None, 0, None, 0) == E_ARG
    Ua, _, sa = wait()
    # unbinding restores the shared results; the handle is usable
    assert torch.equal(Ua, Uplain) and torch.equal(sa, splain)
    assert not torch.equal(Ub, Uplain)
    # index ranges, shapes and dtypes are the front end's to refuse
    for bad_idx in (np.where(np.arange(B) == 5, 4, idx), np.where(np.arange(B) == 9, -1, idx)):
        with pytest.raises(ValueError, match="out of range"):
            eng.set_agent_bounds(t, T(bad_idx, dev, torch.int32))
    with pytest.raises(TypeError):
        eng.set_agent_bounds(t, T(idx, dev, torch.int64))
    with pytest.raises(TypeError):
        eng.set_agent_bounds(t.float(), i)
    with pytest.raises(ValueError):
        eng.set_agent_bounds(t[:, :3].contiguous(), i)
    with pytest.raises(ValueError):
        eng.set_agent_bounds(t.cpu(), i)
    assert not eng.agent_bounds_bound
    del keep


def test_controller_takes_bounds_for_one_call(dev):
    from model_predictive_control_amd import main as mpc_main
    from model_predictive_control_amd.car_dynamics import KinematicBicyclePacejka
    model = KinematicBicyclePacejka(); model.dynamics()
    cl = mpc_main.get_centerline(100).ravel(order="F")
    prob = mpc_main.create_casadi_problem(model, 12, 100, 1.0, 1.0, 0.32)
    c = mpc_main.MPCController(model, prob, 12); c.verbose = False
    y0 = np.array([0.2, 0.1, 0.05, 0.7, 0.0, 0.1])
    Y = np.stack([y0, y0, y0])
    tab = _lib.bound_rows(c.cfg, 2)
    tab[1] = [-0.5, -0.1, 0.6, 0.12]
    U0, _ = c.solve(Y, cl)
    Ut, _ = c.solve(Y, cl, bounds=tab)                                     # b % P
    assert not c.solver.agent_bounds_bound
    assert torch.equal(Ut[0], U0[0]) and torch.equal(Ut[2], U0[2]) and not torch.equal(Ut[1], U0[1])
    assert_inside(Ut, tab, [0, 1, 0], 12)
    Ui, _ = c.solve(Y, cl, bounds=tab, bound_index=[1, 0, 1])
    assert torch.equal(Ui[1], U0[1]) and torch.equal(Ui[0], Ut[1]) and torch.equal(Ui[2], Ut[1])
    assert torch.equal(c.step(Y, cl, bounds=tab, bound_index=[1, 0, 1]), Ui[:, :2])
    with pytest.raises(ValueError):
        c.solve(Y, cl, bound_index=[0, 0, 0])


# ----------------------------------------------------------------------------- 11
def test_full_size_batch_of_different_boxes(dev, O):
    model, N, B, P = 0, 20, 65536, 4096
    kw = dict(max_total_inner=2000)
    rws = bound_rows(P, 7)
    tab = btable(rws)
    cfg = mp.default_config(model, N, **kw)
    rng = np.random.default_rng(17)
    idx = rng.integers(0, P, B)
    X0, cl, U0 = problem(model, N, B)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx)
    Xt, ct, Ut = T(X0, dev), T(cl, dev), T(U0, dev)
    U, _, st = eng.solve(Xt, ct, Ut)
    U2, _, st2 = eng.solve(Xt, ct, Ut)
    assert torch.equal(U, U2) and torch.equal(st, st2)                    # deterministic
    assert bool((st[:, 0] == 1).all())
    assert_inside(U, tab, idx, N)
    sample = np.arange(0, B, 64)
    Uo, sto, _ = oracle_solve(O, model, N, [rws[idx[b]] for b in sample], X0[sample], cl, U0[sample], **kw)
    s = torch.as_tensor(sample, device=dev)
    assert_reference_tolerance(U[s].cpu().numpy(), st[s].cpu().numpy(), Uo, sto)
    del keep
