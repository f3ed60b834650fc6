"""GPU tests of the risk-field cost (mpc_set_agent_fields / BatchedMPC.set_agent_fields): a table of per-agent, per-stage
soft obstacle potentials [N][NFIELD][cx, cy, c, s, A, kx, ky, alpha] in device memory and one row index per agent; stage
k's cost gets A exp(-E) of its sources at the state at the end of the stage.  The oracle does not know the term: the
checker is the numpy restatement of tests/field_common.py on the oracle's calls; the reference solves are recorded in
tests/golden/fields_reference.npz.  Shapes: N = 1, N = 2, kinematic N = 20,
Pacejka N = 12, kinematic N = 40 (two stages per lane of the wave evaluation), B = 130 (no multiple of 64), P = 3 rows with
a scattered index.  The tolerances are the project's HIP-vs-oracle bars.  Every test here fails on a
library without the entry point."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from agent_tables_common import T, box_rows_of, param_rows_of, table_of
from conftest import GOLDEN

import discs_common as D
import field_common as F
from test_gpu_agent_rates import (arange32, eval_case, every_route, host_closed_loop, host_event_loop,  # noqa: F401  (helpers)
                                  rate_table)

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


LINE_Y = 1.5     # the evaluation cases run along y = 1.5: over 40 stages a car drifts up to 0.5 sideways, and the checker's
                 # VJP machine divides by the positions


def field_eval_case(model, N, B, seed=3):
    """eval_case of the rate tests, moved from the line y = 0.5 to y = LINE_Y"""
    X0, _, U = eval_case(model, N, B, seed)
    X0[:, 1] += LINE_Y - 0.5
    return X0, D.line_centerline(y=LINE_Y), U


def field_table(P, N, seed, zero=False, line_y=0.5):
    """[P, 16 N]: field_common.random_rows around the line y = line_y; zero: every A = 0 and the other seven words as drawn"""
    tab = F.random_rows(np.random.default_rng(seed), P, N, y_range=(line_y - 0.15, line_y + 0.15))
    if zero:
        tab[..., 4] = 0.0
    return tab.reshape(P, -1)


# ----------------------------------------------------------------------------- 1. evaluation
def check_eval(O, model, N, B, X0, cl, U, rows, idx, psi, grad, okw=None, y=None, Sig=None, rates=None, ridx=None):
    """agent by agent against the checker: (worst psi, worst grad), the largest share of the term in psi"""
    ocfg = O.default_config(model, N, **(okw or {}))
    cfgs = F.machine(O, model, N)
    worst, share = [0.0, 0.0], 0.0
    for b in range(B):
        yb, sb = (None, None) if y is None else (y[b], Sig[b])
        rr = None if rates is None else rates[ridx[b]]
        p, g = F.psi(O, ocfg, cfgs, X0[b], cl, U[b], rows[idx[b]], yb, sb, rr)
        worst[0] = max(worst[0], abs(psi[b] - p) / abs(p))
        worst[1] = max(worst[1], np.abs(grad[b] - g).max() / np.linalg.norm(g))
        share = max(share, F.field_term(O, cfgs, X0[b], cl, U[b], rows[idx[b]], False)[0] / p)
    return worst, share


@pytest.mark.parametrize("model,N", [(0, 1), (0, 2), (0, 20), (1, 12), (0, 40)])
def test_evaluation_matches_the_checker_and_every_route_agrees(dev, O, monkeypatch, model, N):
    """130 agents on 3 rows through a scattered index, both slots live, rotated frames, alpha != 0, some A = 0.  psi within
    1e-12 relative and the gradient within 1e-9 of ||grad psi|| of the checker, agent by agent; the fused route, the
    two-kernel route, the wave evaluation, an indexed centerline and cost-only requests bit-equal."""
    B, P = 130, 3
    X0, cl, U = field_eval_case(model, N, B)
    rows = field_table(P, N, seed=5, line_y=LINE_Y)
    assert (rows.reshape(P, N, 2, 8)[..., 4] == 0).any() or N < 3
    idx = np.random.default_rng(6).integers(0, P, B)
    assert set(idx) == {0, 1, 2}
    args = (T(X0, dev), T(cl, dev), T(U, dev))
    psi, grad, _ = every_route(dev, monkeypatch, lambda: mp.BatchedMPC(mp.default_config(model, N), dev),
                               lambda e: e.set_agent_fields(T(rows, dev), T(idx, dev, torch.int32)), args, B, cl)
    worst, share = check_eval(O, model, N, B, X0, cl, U, rows, idx, psi, grad)
    print(f"model {model} N {N}: worst psi {worst[0]:.2e} grad {worst[1]:.2e}; the term is up to {share:.2f} of psi")
    assert share > 0.01                                    # the term does act
    assert worst[0] <= 1e-12 and worst[1] <= 1e-9


@pytest.mark.parametrize("mode", ["lane", "state_sq", "rates"])
def test_evaluation_on_constrained_handles_and_beside_a_rate_table(dev, O, monkeypatch, mode):
    """kinematic N = 20: CONSTR_LANE with the handle's own half-width (0.05: the band is active) and CONSTR_STATE_SQ, random
    y and Sigma; yhat -- which does not see a cost term -- within 1e-12 of the oracle's and bit-equal to the one of the same
    call without the table; and beside a rate table (RateTab the caller's, not the handle's zeros)"""
    model, N, B, P = 0, 20, 130, 3
    X0, cl, U = field_eval_case(model, N, B, seed=8)
    rng = np.random.default_rng(9)
    sq = dict(g_off=[0.0] * 6, D_lb=[0.0] * 6, D_ub=[4.0, 2.2, 0.01, 0.5, 1.0, 1.0])    # x^2 <= 4, y^2 <= 2.2, ...: active for many
    kw = dict(lane=dict(constr_mode=mp.CONSTR_LANE, lane_halfwidth=0.05), state_sq=dict(constr_mode=mp.CONSTR_STATE_SQ, **sq), rates={})[mode]
    m = dict(lane=N, state_sq=4 * N, rates=0)[mode]
    y, Sig = (rng.uniform(-2.0, 2.0, (B, m)), 10 ** rng.uniform(0, 3, (B, m))) if m else (None, None)
    rows = field_table(P, N, seed=10, line_y=LINE_Y)
    idx = rng.integers(0, P, B)
    rates, ridx = (rate_table(P, seed=11), rng.integers(0, P, B)) if mode == "rates" else (None, None)
    args = (T(X0, dev), T(cl, dev), T(U, dev)) + ((T(y, dev), T(Sig, dev)) if m else ())

    def bind(e):
        e.set_agent_fields(T(rows, dev), T(idx, dev, torch.int32))
        if rates is not None:
            e.set_agent_rates(T(rates, dev), T(ridx, dev, torch.int32))
    psi, grad, yhat = every_route(dev, monkeypatch, lambda: mp.BatchedMPC(mp.default_config(model, N, **kw), dev), bind, args, B, cl)
    okw = dict(lane=dict(constr_mode=O.CONSTR_LANE, lane_halfwidth=0.05), state_sq=dict(constr_mode=O.CONSTR_STATE_SQ, **sq), rates={})[mode]
    worst, share = check_eval(O, model, N, B, X0, cl, U, rows, idx, psi, grad, okw, y, Sig, rates, ridx)
    print(f"{mode}: worst psi {worst[0]:.2e} grad {worst[1]:.2e}; the term is up to {share:.2f} of psi")
    assert share > 0.01
    assert worst[0] <= 1e-12 and worst[1] <= 1e-9
    if m:
        # yhat against the oracle's own (a cost term has no multiplier: the field must not show in it), 1e-12 relative as the
        # disc tests hold theirs; and bit-equal to the same call without the table
        ocfg, cfgs = O.default_config(model, N, **okw), F.machine(O, model, N)
        wy = max(np.abs(yhat[b] - F.psi_yhat_lane(O, ocfg, cfgs, X0[b], cl, U[b], rows[idx[b]], y[b], Sig[b], False)[2]).max() /
                 np.abs(yhat[b]).max() for b in range(B))
        print(f"{mode}: worst yhat {wy:.2e}")
        assert wy <= 1e-12
        eng = mp.BatchedMPC(mp.default_config(model, N, **kw), dev)
        _, _, yh0 = eng.eval_cost_grad(*args)
        eng.close()
        assert np.array_equal(yhat, yh0.cpu().numpy()) and (yhat != 0).sum() >= B


# ----------------------------------------------------------------------------- 2. the device exp
def test_device_exp(dev):
    """op 5 of the math probe, the out-of-line exp field_term calls, over [-700, 20]: at most 2 ulp from numpy on normal
    results (the bar test_device_math holds the other functions to)"""
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-700.0, 20.0, 200000), np.linspace(-700.0, 20.0, 4001), [0.0, -0.0, 1.0, -1.0, 20.0, -700.0],
                        rng.uniform(-1.0, 1.0, 20000)])
    eng = mp.BatchedMPC(mp.default_config(0, 20), dev)
    got = eng.math_probe(5, T(a, dev)).cpu().numpy()
    eng.close()
    want = np.exp(a)
    assert (want >= np.finfo(np.float64).tiny).all()
    ulp = np.abs(got.view(np.int64) - want.view(np.int64))
    print(f"exp: worst {ulp.max()} ulp over {a.size} arguments")
    assert ulp.max() <= 2 and got[a == 0.0].tolist() == [1.0, 1.0]


# ----------------------------------------------------------------------------- 3. a zero table is no table
@pytest.mark.parametrize("model,N,B,mode", [(0, 20, 256, mp.CONSTR_NONE), (1, 12, 128, mp.CONSTR_NONE), (0, 20, 64, mp.CONSTR_LANE)])
def test_a_zero_table_is_no_table(dev, model, N, B, mode):
    """A = 0 in every source, the other seven words as drawn: U, lambda and all eight statistics columns of solve are those
    of the solve without a field table (the persistent kernel from the start; kinematic NONE: the rounds too) -- and with
    a rate table bound, those of the rate table alone"""
    X0, cl, U0 = eval_case(model, N, B, seed=20)
    kw = dict(max_total_inner=3000)
    if mode == mp.CONSTR_LANE:
        kw.update(lane_halfwidth=0.1)
    rows = field_table(B, N, seed=21, zero=True)
    assert not rows.reshape(B, N, 2, 8)[..., 4].any() and np.abs(rows.reshape(B, N, 2, 8)[..., [0, 1, 5, 6, 7]]).min() > 0
    x0, clt, Ut = T(X0, dev), T(cl, dev), T(U0, dev)
    ftab, fidx = T(rows, dev), T(np.random.default_rng(22).permutation(B), dev, torch.int32)
    eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, **kw), dev)
    for with_rates in (False, True):
        if with_rates:
            eng.set_agent_rates(T(rate_table(B, seed=23), dev), arange32(B, dev))
        for solo_max in ((None, 0) if model == 0 and mode == mp.CONSTR_NONE else (None,)):
            if solo_max is not None:
                eng.set_solo_max(solo_max)
            base = eng.solve(x0, clt, Ut)
            eng.set_agent_fields(ftab, fidx)
            got = eng.solve(x0, clt, Ut)
            eng.clear_agent_fields()
            assert mode == mp.CONSTR_LANE or bool((base[2][:, 0] == 1).sum() >= B // 2)
            assert torch.equal(base[0], got[0]) and torch.equal(base[2], got[2]), (with_rates, solo_max)
            assert (base[1] is None and got[1] is None) or torch.equal(base[1], got[1])
            if mode == mp.CONSTR_LANE:
                assert bool((base[1] != 0).any())
    eng.close()


# ----------------------------------------------------------------------------- 4. solves against the recorded reference
DU_METRIC = 1e-5      # bench.DU_METRIC: the project's bound on controls between two correct solvers
TIGHT = dict(Sigma0=10.0, alm_eps=1e-8, alm_delta=1e-8, max_total_inner=20000)     # of tests/test_gpu_agent_discs.py


def du_metric(U, Uref):
    return np.abs(U - Uref).max(1) / np.maximum(1.0, np.abs(Uref).max(1))


@functools.lru_cache(maxsize=None)
def reference():
    ref = np.load(os.path.join(GOLDEN, "fields_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts()) and float(ref["lane_hw"]) == F.LANE_HW
    assert np.array_equal(ref["source"], [F.SOURCE["A"], *F.SOURCE["sigma"]])
    return ref


def scene_batch(name, B, dev, lane=False):
    model, N, x0, _ = D.SCENES[name]
    rows = np.stack([F.scene_row(name, D.scene_shifts()[b], lane)[3] for b in range(B)])
    return model, N, T(np.tile(x0, (B, 1)), dev), rows, T(D.line_centerline(), dev), torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("name", ["standing", "moving", "pacejka"])
def test_solve_against_the_reference_solve(dev, name):
    """The scenes of field_common.scene_row over the 16 shifts of discs_common.scene_shifts(), unconstrained handles,
    alm_eps = 1e-10, start U = 0: every one of the 16 agents within 1e-5 of the recorded reference solve on
    bench.DU_METRIC (the reference alone is within 1e-14 of itself from three starts: recorded, asserted here too), none left
    out.  The field acts: the plan leaves the centerline by more than 0.05, and the solve without the table does not.  The
    kinematic sources sit 0.10 - 0.11 beside the line: on the path the problem has two local minima (field_common.SOURCE_Y)."""
    B = D.NSHIFT
    model, N, x0, rows, cl, U0 = scene_batch(name, B, dev)
    eng = mp.BatchedMPC(mp.default_config(model, N, alm_eps=1e-10, max_total_inner=20000), dev)
    Uf, _, _ = eng.solve(x0, cl, U0)
    eng.set_agent_fields(T(rows.reshape(B, -1), dev), arange32(B, dev))
    U, _, st = eng.solve(x0, cl, U0)
    dev_f = float((eng.rollout(x0, Uf)[:, :, 1] - 0.5).abs().max())
    dev_y = float((eng.rollout(x0, U)[:, :, 1] - 0.5).abs().max())
    eng.close()
    ref = reference()
    du = du_metric(U.cpu().numpy(), ref[f"U_none_{name}"])
    st = st.cpu().numpy()
    print(f"{name}: dU per agent {np.array2string(du, precision=2)}; status {st[:, 0].astype(int).tolist()}; inner mean {st[:, 2].mean():.0f} "
          f"max {st[:, 2].max():.0f}; sideways {dev_y:.3f} (without the table {dev_f:.3f}); reference spread {ref[f'spread_none_{name}'].max():.1e}")
    assert ref[f"spread_none_{name}"].max() <= 1e-8
    assert (st[:, 0] == 1).all()
    assert du.max() <= DU_METRIC
    assert dev_y > 0.05 and dev_f < 1e-3


@pytest.mark.parametrize("name", ["standing", "pacejka"])
def test_solve_on_a_lane_handle_against_the_reference_solve(dev, O, name):
    """The road scenario: lane_halfwidth = 0.10 and a source in one solve, TIGHT of the disc tests, 4 shifts.  The bar per
    scene is max(1e-5, 4 x the spread between the three starts of the reference, recorded in the golden file), capped at
    1e-4 (the factor the traffic test puts over its measured figure, for solver-path differences between builds); it holds
    for every agent, whatever its status.  And the solver's own conditions by the checker, in the way
    test_gpu_agent_rates.py asserts them for its disc scene -- for every Converged agent, bounds from the tolerances: the
    band violated by at most alm_delta, the projected-gradient residual of f + field + lambda' g at most 10 alm_eps (the
    order of magnitude allowed there between the iterate the stop test saw and the prox point returned).
    Measured on an MI355X: `standing` (the source at y = 0.555, 6 - 7 active multipliers) within 5.3e-6 of the reference
    (bar 1.4e-5; the reference's own starts spread by 3.5e-6), all Converged in 2 797 .. 5 592 inner iterations, violation at
    most 1.4e-9, residual at most 5.3e-9; `pacejka` within 1.7e-7, all Converged, residual at most 2.1e-8."""
    B = F.LANE_SHIFTS
    model, N, x0, rows, cl, U0 = scene_batch(name, B, dev, lane=True)
    eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_LANE, lane_halfwidth=F.LANE_HW, **TIGHT), dev)
    eng.set_agent_fields(T(rows.reshape(B, -1), dev), arange32(B, dev))
    U, lam, st = eng.solve(x0, cl, U0)
    eng.close()
    U, lam, st = U.cpu().numpy(), lam.cpu().numpy(), st.cpu().numpy()
    ref = reference()
    spread = float(ref[f"spread_lane_{name}"].max())
    bar = min(1e-4, max(DU_METRIC, 4.0 * spread))
    du = du_metric(U, ref[f"U_lane_{name}"])
    ocfg = O.default_config(model, N, constr_mode=O.CONSTR_LANE, lane_halfwidth=F.LANE_HW)
    cfgs = F.machine(O, model, N)
    x0n, cln = x0.cpu().numpy(), cl.cpu().numpy()
    cond = np.array([F.lane_conditions(O, ocfg, cfgs, x0n[b], cln, U[b], rows[b], lam[b], F.LANE_HW) for b in range(B)])
    print(f"lane {name}: dU per agent {np.array2string(du, precision=2)} against a bar of {bar:.1e} (reference spread {spread:.1e}); status "
          f"{st[:, 0].astype(int).tolist()}; active multipliers {[int((l != 0).sum()) for l in lam]} (reference "
          f"{[int((l != 0).sum()) for l in ref[f'lam_lane_{name}']]}); violation per agent {np.array2string(cond[:, 0], precision=1)}, "
          f"Lagrangian residual per agent {np.array2string(cond[:, 1], precision=1)}; outer {st[:, 1].astype(int).tolist()}, "
          f"inner {st[:, 2].astype(int).tolist()}")
    conv = st[:, 0] == 1
    assert conv.all() and (lam != 0).any()             # (measured: all four Converged, at most 5 592 of the 20 000 inner iterations)
    for b in np.flatnonzero(conv):             # as test_gpu_agent_rates.py does for its disc scene: every Converged agent
        assert cond[b, 0] <= TIGHT["alm_delta"], (b, cond[b, 0])
        assert cond[b, 1] <= 10 * TIGHT["alm_eps"], (b, cond[b, 1])
    assert du.max() <= bar                     # every agent, whatever its status


# ----------------------------------------------------------------------------- 5. variants
def test_variants_change_no_bit(dev, O, monkeypatch):
    """Fields of different sources per agent beside a parameter table and a bounds table, 130 kinematic agents: the
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
    ftab = field_table(B, N, seed=33)
    fidx = np.random.default_rng(34).permutation(B)

    def run(sel, env=None, solo_max=None, groups=None, active=None, fields=True):
        """the agents `sel` (indices into the 130) as a batch of their own"""
        if env:
            monkeypatch.setenv(*env)
        eng = mp.BatchedMPC(cfg, dev)
        if env:
            monkeypatch.delenv(env[0])
        n = len(sel)
        eng.set_agent_params(T(ptab, dev), T(pidx[sel], dev, torch.int32))
        eng.set_agent_bounds(T(btab, dev), T(bidx[sel], dev, torch.int32))
        if fields:
            eng.set_agent_fields(T(ftab, dev), T(fidx[sel], dev, torch.int32))
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
    # the fields do act: the same solve without the field table moves the controls
    (Un, _, _), _ = run(every, fields=False)
    assert float((Un - U).abs().max()) > 1e-3


# ----------------------------------------------------------------------------- 6. the loops read the table as bound
@pytest.mark.parametrize("with_rates", [False, True])
@pytest.mark.parametrize("model,N,B,shift", [(0, 20, 130, True), (0, 20, 130, False), (1, 12, 66, True), (1, 12, 66, False)])
def test_closed_loop_is_the_host_loop_bit_for_bit(dev, model, N, B, shift, with_rates):
    """a static field table (obstacles standing on the track), T = 6; with_rates: a rate table of P == B beside it, whose
    two columns both loops write"""
    Tn = 6
    X0, cl, _ = eval_case(model, N, B, seed=40 + model)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    x0, clt = T(X0, dev), T(cl, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    ftab = T(field_table(B, N, seed=41), dev)
    keep = ftab.clone()
    eng.set_agent_fields(ftab, T(np.random.default_rng(42).permutation(B), dev, torch.int32))
    first = T(rate_table(B, 43), dev)
    tab = first.clone()
    if with_rates:
        eng.set_agent_rates(tab, arange32(B, dev))
    got = eng.closed_loop(x0, clt, U0, Tn, shift=shift)
    tab2 = first.clone()
    if with_rates:
        eng.set_agent_rates(tab2, arange32(B, dev))
    want = host_closed_loop(eng, x0, clt, U0, Tn, shift, tab2)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None and b is None) or torch.equal(a, b), i
    assert torch.equal(ftab, keep)                                                   # the loop does not write the field table
    if with_rates:
        assert torch.equal(tab, tab2) and not torch.equal(tab, first)
    # ... and the fields act in the loop: without the table the states differ
    eng.clear_agent_fields()
    if with_rates:
        eng.set_agent_rates(first.clone(), arange32(B, dev))
    free = eng.closed_loop(x0, clt, U0, Tn, shift=shift)
    assert not torch.equal(free[3], got[3])
    eng.close()


@pytest.mark.parametrize("with_rates", [False, True])
def test_event_loop_is_its_host_loop(dev, with_rates):
    """thr = 0.02, max_hold = 3, a disturbance: agents hold for 1 .. 3 steps (asserted), a static field table"""
    model, N, B, Tn, thr, max_hold = 0, 20, 130, 6, 0.02, 3
    X0, cl, _ = eval_case(model, N, B, seed=50)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    x0, clt = T(X0, dev), T(cl, dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    dist = T(np.random.default_rng(51).normal(0, 4e-3, (B, Tn, eng.nx)), dev)
    w = np.ones(eng.nx)
    eng.set_agent_fields(T(field_table(B, N, seed=52), dev), T(np.random.default_rng(53).permutation(B), dev, torch.int32))
    first = T(rate_table(B, 54), dev)
    tab = first.clone()
    if with_rates:
        eng.set_agent_rates(tab, arange32(B, dev))
    got = eng.closed_loop_event(x0, clt, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist)
    frac = float(got.solved.float().mean())
    assert 0.3 < frac < 0.95, frac
    tab2 = first.clone()
    if with_rates:
        eng.set_agent_rates(tab2, arange32(B, dev))
    want = host_event_loop(eng, x0, clt, U0, Tn, w, thr, max_hold, True, dist, tab2)
    for name, b in want.items():
        assert torch.equal(getattr(got, name), b), name
    if with_rates:
        assert torch.equal(tab, tab2)
    eng.clear_agent_fields()
    if with_rates:
        eng.set_agent_rates(first.clone(), arange32(B, dev))
    free = eng.closed_loop_event(x0, clt, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist)
    assert not torch.equal(free.traj_x, got.traj_x)
    eng.close()


# ----------------------------------------------------------------------------- 7. the gather and the traffic loop
@pytest.mark.parametrize("model,N", [(0, 20), (1, 12)])
def test_fields_from_plans_against_numpy(dev, model, N):
    """B = 70 (no multiple of 64; 70 N 2 threads: more than one block, the last one partial): the copied words and alpha
    bit-equal to numpy, (c, s) within 2 ulp at 1; an opponent out of range (>= B, and far beyond), an unused slot (-1), an
    agent that is its own opponent"""
    B = 70
    rng = np.random.default_rng(60 + model)
    X0, _, U = eval_case(model, N, B, seed=61)
    eng = mp.BatchedMPC(mp.default_config(model, N), dev)
    X = eng.rollout(T(X0, dev), T(U, dev))
    Xn = X.cpu().numpy()
    opp = rng.integers(0, B, (B, 2)).astype(np.int32)
    opp[3] = (-1, 5); opp[4] = (B, -7); opp[5] = (1 << 30, 6); opp[6] = (6, 6); opp[B - 1] = (0, -1)
    shape = np.stack([rng.uniform(0.1, 0.5, B), rng.uniform(1.0, 20.0, B), rng.uniform(10.0, 100.0, B), rng.uniform(-0.5, 0.5, B)], 1)
    out = torch.full((B, _lib.field_row(N)), 7.0, dtype=torch.float64, device=dev)
    got = eng.fields_from_plans(X, T(opp, dev, torch.int32), T(shape, dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    new = eng.fields_from_plans(X, T(opp, dev, torch.int32), T(shape, dev))
    assert torch.equal(new, got)
    # what the gather made binds: it passes the row rule
    eng.set_agent_fields(got, arange32(B, dev))
    eng.close()
    got = got.cpu().numpy().reshape(B, N, 2, 8)
    want = F.gather(Xn, opp, shape)
    cols = [0, 1, 4, 5, 6, 7]
    assert np.array_equal(got[..., cols], want[..., cols])
    err = np.abs(got[..., 2:4] - want[..., 2:4]).max()
    print(f"model {model}: (c, s) within {err / np.finfo(np.float64).eps:.2f} ulp at 1")
    assert err <= 2 * np.finfo(np.float64).eps
    for b, j in ((3, 0), (4, 0), (4, 1), (5, 0), (B - 1, 1)):
        assert not got[b, :, j].any()
    assert got[3, :, 1].any() and np.abs(got[..., 7]).max() > 0 and not got[6, :, :, 7].any()


def traffic_scene(B, G, seed):
    """scenes of G cars in a row 0.3 apart on the line y = 0.5, the rear ones faster: (X0, radius, shape)"""
    rng = np.random.default_rng(seed)
    X0 = np.zeros((B, 4))
    for s in range(0, B, G):
        X0[s:s + G, 0] = 1.2 + 0.3 * np.arange(G) + rng.uniform(0, 0.02, G)
        X0[s:s + G, 1] = 0.5 + rng.uniform(-.04, .04, G)
        X0[s:s + G, 3] = 1.1 - 0.15 * np.arange(G)
    radius = rng.uniform(0.2, 0.24, B)
    shape = np.stack([rng.uniform(0.2, 0.4, B), 1.0 / (2.0 * rng.uniform(0.15, 0.25, B) ** 2), 1.0 / (2.0 * rng.uniform(0.05, 0.08, B) ** 2),
                      rng.uniform(0.1, 0.3, B)], 1)
    return X0, radius, shape


@pytest.mark.parametrize("with_rates", [False, True])
def test_traffic_field_loop_is_its_host_loop(dev, with_rates):
    """a LANE handle (the road scenario: a lane band and soft obstacles in one solve), scenes of 5, T = 6: the loop equals
    the host loop of rollout, opponents_from_plans, fields_from_plans, solve and the plant step bit for bit, traj_opp and
    traj_clear included"""
    model, N, B, G, Tn, reach = 0, 20, 130, 5, 6, 0.6
    X0, radius, shape = traffic_scene(B, G, seed=70)
    radius, shape = T(radius, dev), T(shape, dev)
    eng = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_LANE, lane_halfwidth=0.1, max_total_inner=1500), dev)
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    first = T(rate_table(B, 71), dev)
    tab = first.clone()
    if with_rates:
        eng.set_agent_rates(tab, arange32(B, dev))
    res = eng.closed_loop_traffic_field(x0, cl, U0, Tn, G, radius, shape, reach, shift=True)
    got = [None if t is None else t.clone() for t in res]
    assert eng.agent_fields_bound and res.table.shape == (B, _lib.field_row(N))
    assert bool((res.traj_opp >= 0).any()) and bool((res.lam != 0).any()) and bool((res.table.view(B, N, 2, 8)[..., 4] > 0).any())
    tab2 = first.clone()
    if with_rates:
        eng.set_agent_rates(tab2, arange32(B, dev))
    x, U = x0.clone(), U0.clone()
    lam = torch.zeros(B, eng.m, dtype=torch.float64, device=dev)
    for t in range(Tn):
        X = eng.rollout(x, U)
        opp, _ = eng.opponents_from_plans(X, G, radius, reach)
        eng.fields_from_plans(X, opp, shape, out=res.table)
        U, lam, st = eng.solve(x, cl, U, lam=lam, inplace=True)
        tab2[:, 2:4] = U[:, :2]
        assert torch.equal(U[:, :2], got[4][:, t])
        x = eng.rollout(x, U[:, :2].contiguous())[:, 0].contiguous()
        U[:, :-2] = U[:, 2:].clone()
        _, clear = eng.opponents_from_plans(x, G, radius)
        assert torch.equal(x, got[3][:, t]) and torch.equal(opp, got[7][:, t]) and torch.equal(clear[:, 0], got[8][:, t]), t
    assert torch.equal(x, got[0]) and torch.equal(U, got[1]) and torch.equal(lam, got[2]) and torch.equal(st, got[6])
    assert torch.equal(res.table, got[9])
    if with_rates:
        assert torch.equal(tab, tab2)
    eng.close()


def test_traffic_field_loop_on_an_unconstrained_handle(dev):
    """CONSTR_NONE (lambda NULL), Pacejka, scenes of 3: runs, returns lam None, and the fields keep the cars further apart
    than the same loop with A = 0"""
    model, N, B, G, Tn = 1, 12, 66, 3, 4
    X0k, radius, shape = traffic_scene(B, G, seed=72)
    X0 = np.concatenate([X0k, np.zeros((B, 2))], 1)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=1500), dev)
    x0, cl = T(X0, dev), T(D.line_centerline(), dev)
    U0 = torch.zeros(B, 2 * N, dtype=torch.float64, device=dev)
    res = eng.closed_loop_traffic_field(x0, cl, U0, Tn, G, T(radius, dev), T(shape, dev))
    assert res.lam is None and bool(torch.isfinite(res.traj_x).all()) and bool((res.traj_opp >= 0).all())
    shape0 = shape.copy(); shape0[:, 0] = 0.0
    free = eng.closed_loop_traffic_field(x0, cl, U0, Tn, G, T(radius, dev), T(shape0, dev), table=res.table)
    assert not torch.equal(free.traj_x, res.traj_x)
    eng.close()


# States of the loop against the recorded mirror loop, 14 steps at alm_eps = 1e-10: measured on an MI355X 1.83e-10, at step 10
# (profiles/r17_risk_field.txt); four times that (the solver-path differences between builds), below the cap of 1e-4
STATE_BOUND = 7.4e-10


def test_traffic_field_loop_against_the_mirror_loop(dev):
    """The recorded mirror loop on the CPU checker (field_common.mirror_loop; tests/golden/fields_reference.npz): two shifted
    scenes of three cars on an unconstrained handle at alm_eps = 1e-10, the rear one passing the slow one at step 12 of 14.
    The same opponents step for step; the first controls of step 0 within bench.DU_METRIC; the states within STATE_BOUND."""
    ref = reference()
    N, Tn, B = F.TRAFFIC_N, F.TRAFFIC_T, ref["traffic_X0"].shape[0]
    assert np.array_equal(ref["traffic_X0"], F.traffic_scenes()[0]) and ref["traffic_traj_x"].shape == (B, Tn, 4)
    eng = mp.BatchedMPC(mp.default_config(0, N, alm_eps=1e-10, max_total_inner=20000), dev)
    eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=ref["traffic_v_ref"]), dev), arange32(B, dev))
    x0, cl = T(ref["traffic_X0"], dev), T(D.line_centerline(), dev)
    res = eng.closed_loop_traffic_field(x0, cl, torch.zeros(B, 2 * N, dtype=torch.float64, device=dev), Tn, 3, T(ref["traffic_radius"], dev),
                                        T(ref["traffic_shape"], dev), F.TRAFFIC_REACH, shift=True)
    eng.close()
    tx, tu = res.traj_x.cpu().numpy(), res.traj_u.cpu().numpy()
    dx = np.abs(tx - ref["traffic_traj_x"])
    du0 = du_metric(tu[:, 0], ref["traffic_traj_u"][:, 0])
    dc = np.abs(res.traj_clear.cpu().numpy() - ref["traffic_traj_clear"])
    passed = [int(np.argmax(tx[3 * s, :, 0] > tx[3 * s + 1, :, 0])) for s in range(B // 3)]
    print(f"mirror loop: du(step 0) {du0.max():.3e}; dx per step {np.array2string(dx.max((0, 2)), precision=2)}; dx max {dx.max():.3e}; "
          f"dclear max {dc.max():.3e}; failures {res.failures.cpu().numpy().tolist()}; past the slow car at steps {passed}")
    assert np.array_equal(res.traj_opp.cpu().numpy(), ref["traffic_traj_opp"])
    assert int(res.failures.sum()) == 0 and all(p > 0 for p in passed)
    assert du0.max() <= DU_METRIC
    assert dx.max() <= STATE_BOUND


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals(dev):
    """each MPC_E_ARG (-1) before any launch, in the library's words: a DISCS handle; a constraint table bound first, and
    bound second; a bad row (A < 0, a NaN, alpha != 0 with kx = 0); a wrong B; a table that is not the bound one, or
    P != B, in the traffic loop; a solve in flight"""
    model, N, B = 0, 20, 64
    X0, cl, U = eval_case(model, N, B, seed=80)
    x0, clt, Ut = T(X0, dev), T(cl, dev), T(U, dev)
    eng = mp.BatchedMPC(mp.default_config(model, N, max_total_inner=300), dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    index = arange32(B, dev)
    good = T(field_table(B, N, 81), dev)
    # rows: source (stage 7, slot 1) of row 5
    at = (7 * 2 + 1) * 8
    for col, v, words in ((4, -1e-3, "A, kx and ky must not be negative"), (5, -1.0, "must not be negative"), (6, -1e-300, "must not be negative"),
                          (0, np.nan, "must be finite"), (7, np.inf, "must be finite"), (4, np.nan, "must be finite"), (3, -np.inf, "must be finite"),
                          (5, 0.0, "a skew (alpha != 0) needs kx > 0")):
        bad = good.clone()
        bad[5, at + col] = v
        if col == 5 and v == 0.0:
            bad[5, at + 7] = 0.25
        assert eng.lib.mpc_set_agent_fields(eng._h, p(bad), B, p(index), B) == -1
        msg = eng.lib.mpc_last_error().decode()
        assert msg.startswith("mpc_set_agent_fields: row 5, stage 7, source 1: ") and words in msg, msg
        with pytest.raises(mp.MpcError):
            eng.set_agent_fields(bad, index)
        assert not eng.agent_fields_bound
    ok = good.clone()
    ok[5, at + 5], ok[5, at + 7] = 0.0, 0.0                                  # kx = 0 without a skew is a valid source
    eng.set_agent_fields(ok, index)
    eng.clear_agent_fields()
    with pytest.raises(ValueError):
        eng.set_agent_fields(good[:, :-1].contiguous(), index)               # the row width
    with pytest.raises(ValueError):
        eng.set_agent_fields(good, index + 1)                                # index out of range
    # another batch size than the bound one
    eng.set_agent_fields(good, index)
    s = slice(0, 32)
    a = (x0[s].contiguous(), clt, Ut[s].contiguous())
    w = np.ones(4)
    readers = {"mpc_eval_cost_grad": lambda: eng.eval_cost_grad(*a), "mpc_eval_cost_grad/wave": lambda: eng.eval_cost_grad(*a, wave=True),
               "mpc_solve_batch": lambda: eng.solve(*a), "mpc_solve_batch/async": lambda: eng.solve_async(*a)(),
               "mpc_solve_active": lambda: eng.solve_active(*a, torch.ones(32, dtype=torch.int32, device=dev)),
               "mpc_closed_loop": lambda: eng.closed_loop(*a, 1),
               "mpc_closed_loop_event": lambda: eng.closed_loop_event(*a, 1, w, 0.0, 3)}
    for who, fn in readers.items():
        with pytest.raises(mp.MpcError) as err:
            fn()
        assert str(err.value) == (f"libmpc_hip error -1: {who.split('/')[0]}: the bound field table is for a batch of 64 agents, "
                                  "this call has 32 (mpc_set_agent_fields)"), str(err.value)
    eng.rollout(a[0], a[2])                     # the calls that do not read the table serve any batch
    eng.stage_cost(a[0], a[2][:, :2].contiguous(), clt)
    with pytest.raises(mp.MpcError, match="mpc_set_agent_bounds: the bound field table is for a batch of 64 agents$"):
        eng.set_agent_bounds(T(_lib.bound_rows(eng.cfg, 2), dev), T(np.arange(32) % 2, dev, torch.int32))
    # the traffic loop: the table that is bound, with P == B
    radius, shape = torch.full((B,), 0.2, dtype=torch.float64, device=dev), T(np.tile([0.3, 10.0, 50.0, 0.2], (B, 1)), dev)
    other = good.clone()
    with pytest.raises(mp.MpcError, match="mpc_closed_loop_traffic_field: table must be the field table that is bound"):
        eng.closed_loop_traffic_field(x0, clt, Ut, 1, 4, radius, shape, table=other)
    eng.set_agent_fields(T(field_table(3, N, 82), dev), T(np.arange(B) % 3, dev, torch.int32))
    three = eng._keep["fields"][0]
    dummy, st = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, 8, dtype=torch.float64, device=dev)
    rc = eng.lib.mpc_closed_loop_traffic_field(eng._h, B, 1, 0, 4, p(radius), p(shape), 1.0, p(x0.clone()), p(clt), None, p(Ut.clone()), None,
                                               p(three), None, None, None, None, p(dummy), p(st), None)
    assert rc == -1 and b"mpc_closed_loop_traffic_field: the bound field table has 3 rows" in eng.lib.mpc_last_error()
    eng.clear_agent_fields()
    rc = eng.lib.mpc_closed_loop_traffic_field(eng._h, B, 1, 0, 4, p(radius), p(shape), 1.0, p(x0.clone()), p(clt), None, p(Ut.clone()), None,
                                               p(good), None, None, None, None, p(dummy), p(st), None)
    assert rc == -1 and b"table must be the field table that is bound" in eng.lib.mpc_last_error()
    rc = eng.lib.mpc_closed_loop_traffic_field(eng._h, B, 1, 0, 4, p(radius), None, 1.0, p(x0.clone()), p(clt), None, p(Ut.clone()), None,
                                               p(good), None, None, None, None, p(dummy), p(st), None)
    assert rc == -1 and b"null shape" in eng.lib.mpc_last_error()
    # binding during an asynchronous solve
    wait = eng.solve_async(x0, clt, Ut)
    rc = eng.lib.mpc_set_agent_fields(eng._h, p(good), B, p(index), B)
    msg = eng.lib.mpc_last_error()
    wait()
    assert rc == -1 and b"mpc_set_agent_fields: a solve of this handle is in flight" in msg
    eng.close()
    # a DISCS handle: there an obstacle is a disc
    de = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mp.CONSTR_DISCS, max_total_inner=300), dev)
    with pytest.raises(mp.MpcError, match="mpc_set_agent_fields: the handle's constraints are keep-out discs"):
        de.set_agent_fields(good, index)
    assert not de.agent_fields_bound
    with pytest.raises(ValueError, match="CONSTR_DISCS"):
        de.closed_loop_traffic_field(x0, clt, Ut, 1, 4, radius, shape)
    assert not de.agent_fields_bound
    rc = de.lib.mpc_closed_loop_traffic_field(de._h, B, 1, 0, 4, p(radius), p(shape), 1.0, p(x0.clone()), p(clt), None, p(Ut.clone()), None,
                                              p(good), None, None, None, None, p(dummy), p(st), None)
    assert rc == -1 and b"the handle's constr_mode is MPC_CONSTR_DISCS" in de.lib.mpc_last_error()
    de.close()
    # beside a constraint table, in either order; the handle's own constraint data is fine
    for mode, kw in ((mp.CONSTR_STATE_SQ, {}), (mp.CONSTR_LANE, dict(lane_halfwidth=0.2))):
        ce = mp.BatchedMPC(mp.default_config(model, N, constr_mode=mode, max_total_inner=300, **kw), dev)
        ctab, cidx = T(_lib.constraint_rows(ce.cfg, 2), dev), T(np.arange(B) % 2, dev, torch.int32)
        ce.set_agent_fields(good, index)
        with pytest.raises(mp.MpcError, match="mpc_set_agent_constraints: a field table is bound .*cannot be bound together"):
            ce.set_agent_constraints(ctab, cidx)
        assert not ce.agent_constraints_bound
        ce.solve(x0, clt, Ut)                   # the handle's own constraint data beside the fields
        ce.clear_agent_fields()
        ce.set_agent_constraints(ctab, cidx)
        with pytest.raises(mp.MpcError, match="mpc_set_agent_fields: a constraint table is bound .*cannot be bound together"):
            ce.set_agent_fields(good, index)
        assert not ce.agent_fields_bound
        ce.solve(x0, clt, Ut)
        ce.close()
    torch.cuda.synchronize()
