"""GPU tests of the per-agent constraint table (mpc_set_agent_constraints / BatchedMPC.set_agent_constraints): a table of
constraint data [g_off[6], D_lb[6], D_ub[6], lane_halfwidth] in device memory and one row index per agent, beside the
parameter and bounds tables.  Every agent of a batch with different speed limits, minimum speeds or lane widths is
checked against the oracle run with that agent's own values; a table whose rows equal the handle's values must give the
bits of the call without a table; the host's switch points must change no bit under a table either.  The helpers are
those of tests/agent_tables_common.py; the tolerances are the ones those
files and tests/test_gpu_parity.py assert for the same quantities.

The rows and inputs (recipes A, B, C, C') are fixed draws: their order is part of the test.  They were checked with the
oracle alone and against the oracle under eval_jitter(2, 5) (every psi value and gradient component moved by a whole
number of ulps in [-2, 2]: another correct implementation), which stays at 97.9 % of the agents within 1e-5 or above in
all four; the 90 % asserted below is a cap, not a measurement."""
import functools

import numpy as np
import pytest
import torch

from agent_tables_common import T, box_rows_of, by_row, kwl, oracle_solve, param_rows_of, rel, table_of
from conftest import straight_centerline, synthetic_states

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402

ctable = functools.partial(table_of, make=_lib.constraint_rows, fields=_lib.CONSTR_FIELDS)   # [P, 19] host table of the rows
BASE_OFF = np.array([20, 1, 1, 0.5, 1, 0.1])
SQ_COMMON = dict(constr_mode=1, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], Sigma0=10.0, alm_eps=1e-8,
                 max_total_inner=6000)
LANE_COMMON = dict(constr_mode=2, lane_halfwidth=0.05, Sigma0=10.0, alm_eps=1e-8, max_total_inner=6000,
                   cost_w=[0.5, 0, 0, 0.01, 0.1, 0.01])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- the rows of the tests
def rows_A(P=4):
    """Speed limits.  Row p as the override of the oracle's configuration AND the content of table row p (row 0: the
    handle's values); P = 8 continues the draws."""
    rng = np.random.default_rng(11)
    out = [{}]
    for p in range(1, P):
        off = BASE_OFF * rng.uniform(.8, 1.2, 6)
        ub = np.zeros(6); ub[3] = rng.uniform(-.05, .05)
        lb = np.full(6, -np.inf)
        if p % 3 == 0:
            lb[3] = -0.4
        hw = rng.uniform(.03, .12)                         # (drawn, unused in this mode)
        out.append(dict(g_off=off, D_lb=lb, D_ub=ub, lane_halfwidth=hw))
    return out


def rows_B():
    """Minimum speeds: the finite lower side of component 3 is active, except in row 2."""
    rng = np.random.default_rng(17)
    out = []
    for p in range(4):
        off = BASE_OFF * (1.0 if p == 0 else rng.uniform(.8, 1.2, 6))
        vmin = 0.515 if p == 0 else rng.uniform(.45, .58)
        lb = np.full(6, -np.inf); lb[3] = vmin * vmin - off[3]
        ub = np.zeros(6); ub[3] = 0.81 - off[3]
        out.append(dict(g_off=off, D_lb=lb, D_ub=ub))
    out[2]["D_lb"][3] = -np.inf
    return out


def rows_lane(hws=(0.05, 0.03, 0.04, 0.07)):
    return [dict(lane_halfwidth=float(h)) for h in hws]


def states_A(B):
    X0 = synthetic_states(1, B, seed=4)
    X0[:, 0] *= 3.9 / 5.0
    X0[:, 3] = np.minimum(X0[:, 3], 0.6)
    return X0


def states_B(B):
    X0 = synthetic_states(1, B, seed=4)
    X0[:, 0] *= 3.9 / 5.0
    X0[:, 3] = 0.62 + 0.2 * (X0[:, 3] - 0.3) / 1.2
    return X0


def states_lane(model, B):
    rng = np.random.default_rng(3)
    cols = [rng.uniform(0, 5, B), rng.uniform(-.01, .01, B), rng.uniform(-.3, .3, B), rng.uniform(.6, 1.0, B)]
    if model == 1:
        cols += [rng.uniform(-.02, .02, B), rng.uniform(-.1, .1, B)]
    return np.stack(cols, 1)


def recipe(name, B=None):
    """(model, N, common, rows, idx, X0, cl, U0) of recipe A, B, C or C' (`Cp`)."""
    if name == "A":
        model, N, B, common, rws = 1, 10, B or 48, dict(SQ_COMMON), rows_A()
        X0 = states_A(B)
    elif name == "B":
        model, N, B, common, rws = 1, 10, B or 48, dict(SQ_COMMON, v_ref=0.4, max_total_inner=12000), rows_B()
        X0 = states_B(B)
    elif name == "C":
        model, N, B, common, rws = 0, 12, B or 64, dict(LANE_COMMON), rows_lane()
        X0 = states_lane(0, B)
    else:
        model, N, B, common, rws = 1, 12, B or 64, dict(LANE_COMMON, cost_w=[0.5, 0, 0, 0.02, 0.1, 0.01]), rows_lane()
        X0 = states_lane(1, B)
    return model, N, common, rws, np.arange(B) % 4, X0, straight_centerline(), np.tile([1., 0.], (B, N))


@functools.lru_cache(maxsize=None)
def _oracle_of(name):
    from oracle import oracle as O
    O.build()
    model, N, common, rws, idx, X0, cl, U0 = recipe(name)
    res = oracle_solve(O, model, N, [rws[p] for p in idx], X0, cl, U0, **common)
    for a in res:
        a.setflags(write=False)
    return res


def own_bounds(model, N, common, row):
    """[m] lower and upper bounds of an agent whose row is `row`."""
    nx = 6 if model else 4
    if common["constr_mode"] == 2:
        hw = row.get("lane_halfwidth", common["lane_halfwidth"])
        return np.full(N, -hw), np.full(N, hw)
    lb = np.asarray(row.get("D_lb", common["D_lb"]), dtype=float)[:nx]
    ub = np.asarray(row.get("D_ub", common["D_ub"]), dtype=float)[:nx]
    return np.tile(lb, N), np.tile(ub, N)


def assert_within_own_bounds(O, model, N, common, overrides, X0, cl, U, conv):
    """Every converged agent's own constraint values within its own bounds + 2e-4."""
    for b in np.nonzero(conv)[0]:
        g = O.constraints(O.default_config(model, N, **{**common, **kwl(overrides[b])}), X0[b], cl, U[b])
        lb, ub = own_bounds(model, N, common, overrides[b])
        assert np.all(g <= ub + 2e-4) and np.all(g >= lb - 2e-4), b


def bind(eng, dev, tab, idx):
    t, i = T(tab, dev), T(idx, dev, torch.int32)
    eng.set_agent_constraints(t, i)
    return t, i


def solve_with_table(dev, name, B=None, env=(), monkeypatch=None, prepare=None, **over):
    """The recipe's batch through a fresh engine with its table bound: (U, lam, stats, info)."""
    model, N, common, rws, idx, X0, cl, U0 = recipe(name, B)
    cfg = mp.default_config(model, N, **{**common, **over})
    for k, v in env:
        monkeypatch.setenv(k, v)
    eng = mp.BatchedMPC(cfg, dev)                  # (the switches are read when the handle is created)
    for k, _ in env:
        monkeypatch.delenv(k)
    if prepare:
        prepare(eng)
    keep = bind(eng, dev, ctable(cfg, rws), idx)
    U, lam, st = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    info = eng.last_solve_info()
    del keep
    eng.close()
    return U, lam, st, info


# ----------------------------------------------------------------------------- 1
@pytest.mark.parametrize("constr,model", [(1, 1), (1, 0), (2, 1), (2, 0)])
def test_k1_agent_by_agent(dev, O, constr, model):
    """As test_augmented_lagrangian_terms_match_oracle_row_by_row, every agent with its own constraint row."""
    N, B, P = 10, 96, 8
    common = dict(constr_mode=constr, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], lane_halfwidth=0.05)
    rws = rows_A(P) if constr == 1 else rows_lane(np.linspace(.02, .09, P))
    cfg = mp.default_config(model, N, **common)
    eng = mp.BatchedMPC(cfg, dev)
    m = eng.m
    idx = np.arange(B) % P
    keep = bind(eng, dev, ctable(cfg, rws), idx)
    assert eng.agent_constraints_bound
    X0 = synthetic_states(model, B, seed=3)
    rng = np.random.default_rng(9)
    U = np.tile([0.7, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N)
    y = rng.uniform(-2, 2, (B, m)); Sig = rng.uniform(1, 1e4, (B, m))
    cl = straight_centerline()
    args = (T(X0, dev), T(cl, dev), T(U, dev), T(y, dev), T(Sig, dev))
    psi, g, yh = eng.eval_cost_grad(*args)
    psiw, gw, yhw = eng.eval_cost_grad(*args, wave=True)
    assert torch.equal(psi, psiw) and torch.equal(g, gw) and torch.equal(yh, yhw)   # the wave evaluation: same bits

    def one(p, sel):
        oc = O.default_config(model, N, **{**common, **kwl(rws[p])})
        assert O.m(oc) == m and m > 0
        po, go = O.psi_batch(oc, X0[sel], cl, U[sel], y[sel], Sig[sel])
        lb, ub = own_bounds(model, N, common, rws[p])
        return (po, go, np.stack([O.constraints(oc, X0[b], cl, U[b]) for b in sel]), np.tile(lb, (len(sel), 1)),
                np.tile(ub, (len(sel), 1)))
    po, go, gU, lbd, ubd = by_row(idx, P, one)
    assert np.allclose(psi.cpu().numpy(), po, rtol=1e-12)
    assert rel(g.cpu().numpy(), go) <= 1e-9
    zeta = gU + y / Sig
    ref = Sig * (zeta - np.clip(zeta, lbd, ubd))
    assert np.allclose(yh.cpu().numpy(), ref, rtol=1e-10, atol=1e-9)
    # (the rows do differ from the handle's: without the table the values are others)
    eng.clear_agent_constraints()
    psi0, _, yh0 = eng.eval_cost_grad(*args)
    other = torch.as_tensor(idx != 0 if constr == 1 else np.abs(np.linspace(.02, .09, P)[idx] - .05) > 1e-9, device=dev)
    assert not torch.equal(psi0[other], psi[other]) and not torch.equal(yh0[other], yh[other])
    del keep


# ----------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["A", "B", "C", "Cp"])
def test_solves_match_oracle_agent_by_agent(dev, O, name):
    model, N, common, rws, idx, X0, cl, U0 = recipe(name)
    B = len(idx)
    Uo, sto, lamo = _oracle_of(name)
    Ut, lamt, stt, _ = solve_with_table(dev, name)
    U, lam, st = Ut.cpu().numpy(), lamt.cpu().numpy(), stt.cpu().numpy()
    assert (sto[:, 0] == 1).all()
    assert (st[:, 0] == 1).mean() >= (0.97 if name in ("A", "B") else 0.95)
    conv = (st[:, 0] == 1) & (sto[:, 0] == 1)
    d = np.abs(U - Uo).max(1)
    match = conv & (d <= 1e-5)
    print(name, "converged", (st[:, 0] == 1).mean(), "within 1e-5", match.sum(), "of", conv.sum(), "worst", d[conv].max())
    assert match.sum() >= 0.9 * conv.sum()
    assert_within_own_bounds(O, model, N, common, [rws[p] for p in idx], X0, cl, U, st[:, 0] == 1)
    if name != "Cp":
        assert np.allclose(lam[match], lamo[match], rtol=1e-3, atol=1e-5)
    if name == "A":
        assert np.all(st[conv, 1] == sto[conv, 1])
        assert lam.min() >= 0.0
        assert np.all(np.abs(lamo).max(1) > 1e-3)                         # (the recipe: every agent has an active limit)
    if name == "B":
        # the finite lower side is active (negative multipliers) -- but not in row 2, whose lower side is infinite:
        # the per-agent isinf of detail::project_y
        assert lam[conv].min() < -1e-3
        assert np.all(lam[idx == 2][:, 3::6] >= 0.0)
    if name == "C":
        assert ((np.abs(lam) > 1e-3).any(1) & (st[:, 0] == 1)).sum() >= 16


# ----------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name,B", [("A", 96), ("A", 1536), ("C", 96), ("C", 5000)])
def test_equal_rows_are_the_shared_path_bit_for_bit(dev, name, B):
    """A table of copies of the handle's own row under a random index: the constraint forms must give the bits of the
    kernels that run without a table -- in the persistent kernel (B = 96) and, above the whole-batch persistent bound,
    through rounds and the hand-over."""
    model, N, common, _, _, X0, cl, U0 = recipe(name, B)
    cfg = mp.default_config(model, N, **{**common, "alm_eps": 1e-6, "max_total_inner": 1500})
    eng = mp.BatchedMPC(cfg, dev)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    U1, lam1, s1 = eng.solve(X0, cl, U0)
    rng = np.random.default_rng(B)
    Ue = T(np.tile([0.7, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N), dev)
    y, Sig = T(rng.uniform(-2, 2, (B, eng.m)), dev), T(rng.uniform(1, 1e4, (B, eng.m)), dev)
    plain = [*eng.eval_cost_grad(X0, cl, Ue, y, Sig), *eng.eval_cost_grad(X0, cl, Ue, y, Sig, wave=True)]
    if B > 1000:
        assert eng.last_solve_info()["rounds"] > 0
    tab = _lib.constraint_rows(cfg, 3)
    assert np.array_equal(tab[1], _lib.default_constraints(cfg))
    keep = bind(eng, dev, tab, rng.integers(0, 3, B))
    U2, lam2, s2 = eng.solve(X0, cl, U0)
    assert torch.equal(U1, U2) and torch.equal(lam1, lam2) and torch.equal(s1, s2)
    bound = [*eng.eval_cost_grad(X0, cl, Ue, y, Sig), *eng.eval_cost_grad(X0, cl, Ue, y, Sig, wave=True)]
    for a, b in zip(bound, plain):
        assert torch.equal(a, b)
    eng.clear_agent_constraints()
    assert not eng.agent_constraints_bound
    U3, lam3, s3 = eng.solve(X0, cl, U0)                                   # unbound: the handle is what it was
    assert torch.equal(U1, U3) and torch.equal(lam1, lam3) and torch.equal(s1, s3)
    del keep


# ----------------------------------------------------------------------------- 4
def test_the_table_is_per_agent(dev):
    """Permuting the agents with their indices permutes the results; changing one row changes only its agents."""
    model, N, common, rws, idx, X0, cl, U0 = recipe("A")
    B = len(idx)
    cfg = mp.default_config(model, N, **common)
    tab = ctable(cfg, rws)
    eng = mp.BatchedMPC(cfg, dev)
    clt = T(cl, dev)

    def run(X, U_, table, index):
        keep = bind(eng, dev, table, index)
        U, lam, st = eng.solve(T(X, dev), clt, T(U_, dev))
        del keep
        return U, lam, st
    U, lam, st = run(X0, U0, tab, idx)
    perm = np.random.default_rng(7).permutation(B)
    Up, lamp, stp = run(X0[perm], U0[perm], tab, idx[perm])
    pt = torch.as_tensor(perm, device=dev)
    assert torch.equal(Up, U[pt]) and torch.equal(lamp, lam[pt]) and torch.equal(stp, st[pt])
    tab2 = tab.copy()
    tab2[1, 12 + 3] -= 0.03                                                # a lower speed limit for row 1
    U2, lam2, st2 = run(X0, U0, tab2, idx)
    changed = torch.as_tensor(idx == 1, device=dev)
    assert torch.equal(U2[~changed], U[~changed]) and torch.equal(lam2[~changed], lam[~changed]) and torch.equal(st2[~changed], st[~changed])
    assert not torch.equal(U2[changed], U[changed])


# ----------------------------------------------------------------------------- 5
R0 = ("MPC_SOLO_MAX", "0")
SWITCH_VARIANTS = {
    "rounds_no_memo": dict(prepare=lambda e: (e.set_solo_max(0), e.set_memo(False))),
    "no_quad_no_wide": dict(env=(R0, ("MPC_NO_QUAD", "1"), ("MPC_WIDE_MAX", "-1"))),
    "unfused_eval": dict(env=(R0, ("MPC_UNFUSED_EVAL", "1"))),
    "chain_min_0": dict(env=(R0, ("MPC_CHAIN_MIN", "0"))),
    "step_regs": dict(env=(R0, ("MPC_STEP_REGS", "1"))),
    "lds_pairs_3": dict(env=(R0, ("MPC_LDS_PAIRS", "3"))),
    "apb_4": dict(env=(R0, ("MPC_APB", "4"))),
    "apb_64": dict(env=(R0, ("MPC_APB", "64"))),
    "small_solo_max": dict(env=(("MPC_SOLO_MAX", "16"),)),
}


@functools.lru_cache(maxsize=None)
def _default_path(name):
    """The recipe's batch through the default path (the persistent kernel from the start), computed once."""
    return solve_with_table(torch.device("cuda:0"), name)


@pytest.mark.parametrize("variant", list(SWITCH_VARIANTS))
@pytest.mark.parametrize("name", ["A", "C"])
def test_host_switches_change_nothing_under_a_constraint_table(dev, monkeypatch, name, variant):
    """The variants of test_host_switches_change_nothing_under_a_bounds_table: rounds only and no memo, each K1 kernel,
    chain blocks, history from global memory, a short LDS copy, 4 and 64 agents per workgroup, a small hand-over count."""
    U, lam, st, info = _default_path(name)
    assert info["solo_agents"] == len(st)
    v = SWITCH_VARIANTS[variant]
    Uv, lamv, stv, iv = solve_with_table(dev, name, monkeypatch=monkeypatch, **v)
    assert torch.equal(U, Uv) and torch.equal(lam, lamv) and torch.equal(st, stv)
    if "prepare" in v or R0 in v.get("env", ()):
        assert iv["solo_agents"] == 0 and iv["rounds"] > 0


# ----------------------------------------------------------------------------- 6
def test_groups_change_nothing_under_a_constraint_table(dev):
    model, N, common, rws, idx, X0, cl, U0 = recipe("C", 2048)
    cfg = mp.default_config(model, N, **{**common, "alm_eps": 1e-6})
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, ctable(cfg, rws), idx)
    eng.set_solo_max(0)                # (a batch this small is the persistent kernel's from the start, which has no groups:
    eng.set_groups(1)                  # the rounds are what is split, and sliced indices are what is being tested)
    U1, lam1, s1 = eng.solve(X0, cl, U0)
    assert eng.last_solve_info()["groups"] == 1 and eng.last_solve_info()["rounds"] > 0
    eng.set_groups(2)
    U2, lam2, s2 = eng.solve(X0, cl, U0)
    assert eng.last_solve_info()["groups"] == 2 and eng.last_solve_info()["solo_agents"] == 0
    assert torch.equal(U1, U2) and torch.equal(lam1, lam2) and torch.equal(s1, s2)
    del keep


# ----------------------------------------------------------------------------- 7
def test_three_tables_at_once(dev, O):
    model, N, common, crw, cidx, X0, cl, U0 = recipe("A")
    B = len(cidx)
    prw, brw = param_rows_of(O, 1, 4, 1), box_rows_of(4, 11)
    # three indices that differ for every agent (chosen with the oracle alone: under (b // 4, b // 2) three agents of the
    # oracle's run out of the 6 000 inner iterations of the recipe, under these all 48 converge)
    pidx, bidx = (np.arange(B) + 1) % 4, (np.arange(B) + 2) % 4
    assert (pidx != bidx).all() and (pidx != cidx).all() and (bidx != cidx).all()
    cfg = mp.default_config(model, N, **common)
    ptab = table_of(cfg, prw)
    btab = np.array([list(r["u_lb"]) + list(r["u_ub"]) for r in brw])
    eng = mp.BatchedMPC(cfg, dev)
    kp = (T(ptab, dev), T(pidx, dev, torch.int32)); eng.set_agent_params(*kp)
    kb = (T(btab, dev), T(bidx, dev, torch.int32)); eng.set_agent_bounds(*kb)
    kc = bind(eng, dev, ctable(cfg, crw), cidx)
    assert eng.agent_params_bound and eng.agent_bounds_bound and eng.agent_constraints_bound
    Ut, lamt, stt = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    eng.set_solo_max(0)                                                    # the same through the rounds
    U2, lam2, st2 = eng.solve(T(X0, dev), T(cl, dev), T(U0, dev))
    assert eng.last_solve_info()["solo_agents"] == 0
    assert torch.equal(Ut, U2) and torch.equal(lamt, lam2) and torch.equal(stt, st2)
    merged = [dict(prw[pidx[b]], **brw[bidx[b]], **crw[cidx[b]]) for b in range(B)]
    Uo, sto, lamo = oracle_solve(O, model, N, merged, X0, cl, U0, **common)
    U, lam, st = Ut.cpu().numpy(), lamt.cpu().numpy(), stt.cpu().numpy()
    assert (sto[:, 0] == 1).all() and (st[:, 0] == 1).mean() >= 0.97
    conv = (st[:, 0] == 1) & (sto[:, 0] == 1)
    match = conv & (np.abs(U - Uo).max(1) <= 1e-5)
    print("three tables: within 1e-5", match.sum(), "of", conv.sum())
    assert match.sum() >= 0.9 * conv.sum()
    assert np.allclose(lam[match], lamo[match], rtol=1e-3, atol=1e-5)
    assert_within_own_bounds(O, model, N, common, merged, X0, cl, U, st[:, 0] == 1)
    t4 = btab[bidx]
    assert np.all(U >= np.tile(t4[:, 0:2], (1, N))) and np.all(U <= np.tile(t4[:, 2:4], (1, N)))
    del kp, kb, kc


# ----------------------------------------------------------------------------- 8
def test_in_place_row_refresh_is_seen(dev):
    """The library reads the caller's table at every call: a row rewritten in place is used by the next solve
    without binding again."""
    model, N, common, rws, idx, X0, cl, U0 = recipe("C")
    cfg = mp.default_config(model, N, **common)
    tab = ctable(cfg, rws)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    t, i = bind(eng, dev, tab, idx)
    U1, lam1, _ = eng.solve(X0, cl, U0)
    tab2 = tab.copy()
    tab2[1, 18] = 0.02
    t.data[1].copy_(T(tab2[1], dev))
    U2, lam2, s2 = eng.solve(X0, cl, U0)
    fresh = mp.BatchedMPC(cfg, dev)
    keep = bind(fresh, dev, tab2, idx)
    U3, lam3, s3 = fresh.solve(X0, cl, U0)
    assert torch.equal(U2, U3) and torch.equal(lam2, lam3) and torch.equal(s2, s3)
    changed = torch.as_tensor(idx == 1, device=dev)
    assert not torch.equal(U1[changed], U2[changed]) and torch.equal(U1[~changed], U2[~changed])
    del keep, i


# ----------------------------------------------------------------------------- 9
@pytest.mark.parametrize("name", ["A", "C"])
def test_masked_solve_under_a_constraint_table(dev, name):
    """solve_active on a mask = solve on the gathered subset with the gathered index; no other byte is written."""
    model, N, common, rws, idx, X0, cl, U0 = recipe(name)
    B = len(idx)
    cfg = mp.default_config(model, N, **common)
    tab = ctable(cfg, rws)
    mask_np = np.random.default_rng(5).random(B) < 0.4
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, tab, idx)
    mask = T(mask_np, dev, torch.bool)
    assert 0 < int(mask.sum()) < B
    sub = mp.BatchedMPC(cfg, dev)
    ks = bind(sub, dev, tab, idx[mask_np])
    Us, lams, sts = sub.solve(X0[mask].contiguous(), cl, U0[mask].contiguous())
    nan = float("nan")
    Uin = torch.where(mask[:, None], U0, torch.full_like(U0, nan))
    lamin = torch.where(mask[:, None], torch.zeros(B, eng.m, dtype=torch.float64, device=dev),
                        torch.full((B, eng.m), nan, dtype=torch.float64, device=dev))
    stin = torch.full((B, 8), nan, dtype=torch.float64, device=dev)
    Ua, lama, sta, n = eng.solve_active(X0, cl, Uin, mask, lam=lamin, stats=stin)
    assert n == int(mask.sum())
    assert torch.equal(Ua[mask], Us) and torch.equal(lama[mask], lams) and torch.equal(sta[mask], sts)
    assert bool(torch.isnan(Ua[~mask]).all()) and bool(torch.isnan(lama[~mask]).all()) and bool(torch.isnan(sta[~mask]).all())
    del keep, ks


LOOP_T = 3


@functools.lru_cache(maxsize=None)
def _closed_loop_of(name):
    """closed_loop(T = 3) of the recipe's batch under its table, computed once: (x_T, U, lam, traj_x, traj_u)."""
    dev = torch.device("cuda:0")
    model, N, common, rws, idx, X0, cl, U0 = recipe(name)
    cfg = mp.default_config(model, N, **common)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, ctable(cfg, rws), idx)
    xT, Uc, lamc, tx, tu, _, _ = eng.closed_loop(T(X0, dev), T(cl, dev), T(U0, dev), LOOP_T)
    del keep
    eng.close()
    return xT, Uc, lamc, tx, tu


@pytest.mark.parametrize("name", ["A", "C"])
def test_closed_loop_is_the_host_loop_under_a_constraint_table(dev, name):
    model, N, common, rws, idx, X0, cl, U0 = recipe(name)
    cfg = mp.default_config(model, N, **common)
    xT, Uc, lamc, tx, tu = _closed_loop_of(name)
    host = mp.BatchedMPC(cfg, dev)
    keep = bind(host, dev, ctable(cfg, rws), idx)
    x, cl, Uw, lamw = T(X0, dev), T(cl, dev), T(U0, dev), None
    for t in range(LOOP_T):
        Uw, lamw, _ = host.solve(x, cl, Uw, lamw)
        u0 = Uw[:, :2].contiguous()
        x = host.rollout(x, u0)[:, 0, :].contiguous()
        assert torch.equal(tx[:, t], x) and torch.equal(tu[:, t], u0)
    assert torch.equal(xT, x) and torch.equal(Uc, Uw) and torch.equal(lamc, lamw)
    del keep


@pytest.mark.parametrize("name", ["A", "C"])
def test_event_loop_at_threshold_zero_is_closed_loop_under_a_constraint_table(dev, name):
    """closed_loop_event with thr = 0 re-plans every agent at every step: closed_loop, bit for bit."""
    model, N, common, rws, idx, X0, cl, U0 = recipe(name)
    cfg = mp.default_config(model, N, **common)
    xT, Uc, lamc, tx, tu = _closed_loop_of(name)
    eng = mp.BatchedMPC(cfg, dev)
    keep = bind(eng, dev, ctable(cfg, rws), idx)
    r = eng.closed_loop_event(T(X0, dev), T(cl, dev), T(U0, dev), LOOP_T, np.ones(eng.nx), 0.0, 3)
    assert bool((r.solved == 1).all())
    assert torch.equal(r.traj_x, tx) and torch.equal(r.traj_u, tu) and torch.equal(r.x, xT) and torch.equal(r.U, Uc)
    assert torch.equal(r.lam, lamc)
    del keep


# ----------------------------------------------------------------------------- 10
def test_refusals(dev):
    """None of these reaches a kernel, and the handle stays usable."""
    E_ARG = -1
    model, N, common, rws, idx, X0, cl, U0 = recipe("A")
    B = len(idx)
    cfg = mp.default_config(model, N, **{**common, "alm_eps": 1e-6, "max_total_inner": 1500})
    eng = mp.BatchedMPC(cfg, dev)
    tab = ctable(cfg, rws)
    X0, cl, U0 = T(X0, dev), T(cl, dev), T(U0, dev)
    Uplain, lplain, splain = eng.solve(X0, cl, U0)
    t, i = T(tab, dev), T(idx, dev, torch.int32)
    ptr = lambda z: None if z is None else z.data_ptr()
    raw = lambda e, table, P, index, Bn: e.lib.mpc_set_agent_constraints(e._h, ptr(table), P, ptr(index), Bn)
    # a handle without general constraints has nothing to bind to (unbinding is still a no-op)
    none = mp.BatchedMPC(mp.default_config(model, N), dev)
    assert raw(none, t, 4, i, B) == E_ARG and b"MPC_CONSTR_NONE" in none.lib.mpc_last_error()
    with pytest.raises(mp.MpcError):
        none.set_agent_constraints(t, i)
    assert not none.agent_constraints_bound and raw(none, None, 0, None, 0) == 0
    none.solve(X0, cl, U0)
    none.close()
    # D_lb > D_ub in a row, a NaN bound, a g_off that is not finite
    for col, val in ((6 + 3, 0.5), (6 + 4, 1e-3), (6 + 2, np.nan), (12 + 5, np.nan), (0, np.nan), (4, np.inf)):
        bad = tab.copy(); bad[2, col] = val
        assert raw(eng, T(bad, dev), 4, i, B) == E_ARG and b"row 2" in eng.lib.mpc_last_error(), (col, val)
        with pytest.raises(mp.MpcError, match="row 2"):
            bind(eng, dev, bad, idx)
        assert not eng.agent_constraints_bound
    # infinities pass as bounds; the lane halfwidth is not read in this mode
    ok = tab.copy(); ok[1, 6:18] = [-np.inf] * 6 + [np.inf] * 6; ok[3, 18] = np.nan
    assert raw(eng, T(ok, dev), 4, i, B) == 0
    assert raw(eng, None, 0, None, 0) == 0
    # a lane halfwidth that is not positive and finite, in lane mode (where the three vectors are not read)
    lcfg = mp.default_config(0, 12, **LANE_COMMON)
    lane = mp.BatchedMPC(lcfg, dev)
    for val in (0.0, -0.05, np.nan, np.inf):
        bad = ctable(lcfg, rows_lane()); bad[2, 18] = val
        assert raw(lane, T(bad, dev), 4, i, B) == E_ARG and b"row 2" in lane.lib.mpc_last_error(), val
    good = ctable(lcfg, rows_lane()); good[0, 0:18] = np.nan
    assert raw(lane, T(good, dev), 4, i, B) == 0
    lane.close()
    # P <= 0, a NULL index, B <= 0
    assert raw(eng, t, 0, i, B) == E_ARG and raw(eng, t, -1, i, B) == E_ARG
    assert raw(eng, t, 4, None, B) == E_ARG and b"mpc_set_agent_constraints" in eng.lib.mpc_last_error()
    assert raw(eng, t, 4, i, 0) == E_ARG
    # another batch size, in every call that reads constraint data
    keep = bind(eng, dev, tab, idx)
    Xs, Us = X0[:B - 1].contiguous(), U0[:B - 1].contiguous()
    ys = torch.ones(B - 1, eng.m, dtype=torch.float64, device=dev)
    act = torch.ones(B - 1, dtype=torch.int32, device=dev)
    for call in (lambda: eng.solve(Xs, cl, Us), lambda: eng.eval_cost_grad(Xs, cl, Us, ys, ys),
                 lambda: eng.eval_cost_grad(Xs, cl, Us, ys, ys, wave=True), lambda: eng.solve_active(Xs, cl, Us, act),
                 lambda: eng.closed_loop(Xs, cl, Us, 2),
                 lambda: eng.closed_loop_event(Xs, cl, Us, 2, np.ones(eng.nx), 0.0, 3)):
        with pytest.raises(mp.MpcError, match="bound constraint table"):
            call()
    eng.rollout(Xs, Us[:, :2].contiguous())                                # (the model layer reads no constraint data)
    Ub, _, sb = eng.solve(X0, cl, U0)                                      # the bound size is served
    # a second table for another B than the bound one's, either way round
    ptab = T(_lib.param_rows(cfg, 2), dev)
    with pytest.raises(mp.MpcError, match="constraint table"):
        eng.set_agent_params(ptab, torch.zeros(B - 1, dtype=torch.int32, device=dev))
    with pytest.raises(mp.MpcError, match="constraint table"):
        eng.set_agent_bounds(T(_lib.bound_rows(cfg, 2), dev), torch.zeros(B - 1, dtype=torch.int32, device=dev))
    assert not eng.agent_params_bound and not eng.agent_bounds_bound
    eng.clear_agent_constraints()
    eng.set_agent_params(ptab, torch.zeros(B - 1, dtype=torch.int32, device=dev))
    with pytest.raises(mp.MpcError, match="parameter table"):
        bind(eng, dev, tab, idx)
    assert not eng.agent_constraints_bound
    eng.clear_agent_params()
    # binding during an asynchronous solve
    wait = eng.solve_async(X0, cl, U0)
    with pytest.raises(mp.MpcError):
        bind(eng, dev, tab, idx)
    assert raw(eng, t, 4, i, B) == E_ARG and b"in flight" in eng.lib.mpc_last_error()
    assert raw(eng, None, 0, None, 0) == E_ARG
    Ua, la, sa = wait()
    # unbinding restores the shared results; the handle is usable
    assert torch.equal(Ua, Uplain) and torch.equal(la, lplain) and torch.equal(sa, splain)
    assert not torch.equal(Ub, Uplain)
    # index ranges, shapes, dtypes and devices are the front end's to refuse
    for bad_idx in (np.where(np.arange(B) == 5, 4, idx), np.where(np.arange(B) == 9, -1, idx)):
        with pytest.raises(ValueError, match="out of range"):
            eng.set_agent_constraints(t, T(bad_idx, dev, torch.int32))
    with pytest.raises(TypeError):
        eng.set_agent_constraints(t, T(idx, dev, torch.int64))
    with pytest.raises(TypeError):
        eng.set_agent_constraints(t.float(), i)
    with pytest.raises(ValueError):
        eng.set_agent_constraints(t[:, :18].contiguous(), i)
    with pytest.raises(ValueError):
        eng.set_agent_constraints(t.cpu(), i)
    assert not eng.agent_constraints_bound
    del keep


# ----------------------------------------------------------------------------- 11
def test_controller_takes_constraints_for_one_call(dev):
    from model_predictive_control_amd import main as mpc_main
    from model_predictive_control_amd.car_dynamics import KinematicBicyclePacejka
    model = KinematicBicyclePacejka(); model.dynamics()
    cl = mpc_main.get_centerline(100).ravel(order="F")
    prob = mpc_main.create_casadi_problem(model, 12, 100, 1.0, 1.0, 0.32)
    prob.D.upperbound = np.zeros(6 * 12)                                   # main.py:43-52 with D = (-inf, 0]: a constrained problem
    prob.max_total_inner = 400                                             # (bits are compared here, not minima: bounded work)
    c = mpc_main.MPCController(model, prob, 12); c.verbose = False
    assert c.cfg.constr_mode == _lib.CONSTR_STATE_SQ
    y0 = np.array([0.2, 0.1, 0.05, 0.7, 0.0, 0.1])
    Y = np.stack([y0, y0, y0])
    tab = _lib.constraint_rows(c.cfg, 2)
    tab[1, 12 + 3] = 0.75 * 0.75 - tab[1, 3]                               # row 1: vx <= 0.75
    dev_ = c.device
    # bind + solve + clear by hand
    eng = c.solver
    X = torch.as_tensor(Y, dtype=torch.float64, device=dev_).contiguous()
    clt = torch.as_tensor(cl, dtype=torch.float64, device=dev_).contiguous()
    U0 = torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev_).repeat(3, 12)
    keep = (T(tab, dev_), T([0, 1, 0], dev_, torch.int32))
    eng.set_agent_constraints(*keep)
    Uh, _, sth = eng.solve(X, clt, U0)
    eng.clear_agent_constraints()
    Up, _ = c.solve(Y, cl)
    Ut, stt = c.solve(Y, cl, constraints=tab)                              # b % P
    assert not c.solver.agent_constraints_bound
    assert torch.equal(Ut, Uh) and torch.equal(stt, sth)
    assert torch.equal(Ut[0], Up[0]) and torch.equal(Ut[2], Up[2]) and not torch.equal(Ut[1], Up[1])
    Ui, _ = c.solve(Y, cl, constraints=tab, constraint_index=[1, 0, 1])
    assert torch.equal(Ui[1], Up[1]) and torch.equal(Ui[0], Ut[1]) and torch.equal(Ui[2], Ut[1])
    assert torch.equal(c.step(Y, cl, constraints=tab, constraint_index=[1, 0, 1]), Ui[:, :2])
    with pytest.raises(ValueError):
        c.solve(Y, cl, constraint_index=[0, 0, 0])
    # ... and after an exception inside the call the handle is unbound too
    with pytest.raises(ValueError):
        c.solve(Y, cl, constraints=tab, constraint_index=[0, 2, 0])
    assert not c.solver.agent_constraints_bound
    with pytest.raises(Exception):
        c.solve(Y[:, :5], cl, constraints=tab)
    assert not c.solver.agent_constraints_bound
    del keep
