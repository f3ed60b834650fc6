"""GPU tests at `nfe` other than 4 and with `clip_inputs` set: every evaluation route, the solves and the closed loop
against the CPU oracle (oracle/mpc_oracle.c) built with the same configuration.

`nfe == 4` is a dispatch key, not only a loop count.  Any other value sends every kinematic request to the
thread-per-request rollout (mpc_launch.hpp: the wide and the two-lane rollouts need nfe == 4), every stage through
stage_forward_steps and the generic stage_tangents (mpc_device.hpp), makes step_trig the kinematic model's only trig
route, and puts the kinematic model on the lane-serial rollout of the persistent kernel -- the two-half LDS layout with
the speculative gradient on lanes 32 .. 63 for N <= 32 (solo_dual), the single layout on lane 0 beyond.  `clip_inputs`
puts the masks of the clipped components into every vjp / jvp and into the two-lane kernel's exchange.

Tolerances are the ones tests/test_gpu_parity.py asserts for the same quantities at nfe = 4: model layer 1e-12, psi
1e-12 relative, gradient 1e-9 of its largest component, controls 1e-5 relative with a median of 1e-7, psi of a solve
1e-10.  Lines that start with "r21" are the measured figures (pytest -s); profiles/r21_integrator_steps.txt keeps them."""
import ctypes as C

import numpy as np
import pytest
import torch

from agent_tables_common import by_row
from conftest import straight_centerline, synthetic_states
from test_gpu_parity import T, both, rel

pytestmark = pytest.mark.gpu

import model_predictive_control_amd as mp  # noqa: E402
from model_predictive_control_amd import _lib  # noqa: E402

NARROW = (0.2, 0.6)          # veh[9] (steering limit), veh[10] (drive limit) of the clipped cases: inside the inputs' range
# Drives drawn from [-1, 1] and clipped at 0.6 brake as often as they accelerate: from the generator's 0.3 .. 1.5 m/s a
# Pacejka car crosses vx = 0 inside ten stages, where the model is singular and RK4 on it unstable (below 0.25 m/s:
# test_rollout_matches_reference_derived_vectors) -- there the ORACLE's gradient moves by 4e-9 of its largest component
# when x0 moves by one ulp, four times the bar.  0.8 m/s more keep every trajectory of these tests above 0.6 m/s, where
# the same perturbation moves psi by 3e-15 and the gradient by 1e-15 (measured with the oracle alone).
PAC_CLIP_VX = 0.8
ROUTES = (("default", {}), ("unfused", {"MPC_UNFUSED_EVAL": "1"}), ("no_quad", {"MPC_NO_QUAD": "1"}))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=1.25), torch.nan_to_num(b, nan=1.25))


def narrow_veh(model, steer=NARROW[0], drive=NARROW[1]):
    veh = list(mp.default_config(model, 4).veh)
    veh[9], veh[10] = steer, drive
    return veh


def clipped_inputs(B, N, seed, steer=NARROW[0], drive=NARROW[1]):
    """Drives uniform in [-1, 1], steering in [-0.32, 0.32], a few entries exactly on +-limit (not clipped: the comparison
    is strict).  steer / drive: scalars or [B]."""
    rng = np.random.default_rng(seed)
    U = np.stack([rng.uniform(-1, 1, (B, N)), rng.uniform(-.32, .32, (B, N))], 2)
    steer, drive = np.broadcast_to(steer, (B,)), np.broadcast_to(drive, (B,))
    k = np.arange(B) % N
    for a in range(0, B, 5):
        U[a, k[a], 0] = drive[a] * (1 if a % 2 else -1)
    for a in range(2, B, 7):
        U[a, k[a], 1] = steer[a] * (-1 if a % 2 else 1)
    return U.reshape(B, 2 * N)


def clip_masks(U, steer, drive):
    """[B, N, 2] True where the component is clipped."""
    B = U.shape[0]
    u = U.reshape(B, -1, 2)
    lim = np.stack([np.broadcast_to(drive, (B,)), np.broadcast_to(steer, (B,))], 1)[:, None, :]
    return np.abs(u) > lim


def ordinary_inputs(B, N, seed):
    """The input recipe of test_cost_and_gradient_match_oracle."""
    rng = np.random.default_rng(seed)
    return np.tile([0.5, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N)


def every_route(monkeypatch, dev, cfg, X0, cl, U, y=None, Sig=None, bind=None, routes=ROUTES):
    """eval_cost_grad under the default switches, with K1b and K1c as two launches, with the thread-per-request rollout
    (a fresh engine per switch) and through the wave-per-agent evaluation; the cost-only request beside the first.
    Returns [(name, psi, grad, yhat)] and the cost-only psi.  bind(eng): binds the per-agent tables of the case."""
    outs, first = [], None
    for name, env in routes:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = mp.BatchedMPC(cfg, dev)
        for k in env:
            monkeypatch.delenv(k)
        if bind:
            bind(eng)
        outs.append((name, *eng.eval_cost_grad(X0, cl, U, y, Sig)))
        first = first or eng
    outs.append(("wave", *first.eval_cost_grad(X0, cl, U, y, Sig, wave=True)))
    psi_only, none, _ = first.eval_cost_grad(X0, cl, U, y, Sig, want_grad=False)
    assert none is None
    return outs, psi_only, first


def assert_routes_agree(outs, psi_only):
    name0, p0, g0, y0 = outs[0]
    for name, p, g, yh in outs[1:]:
        assert same(p, p0) and same(g, g0), (name, name0)
        assert (yh is None and y0 is None) or same(yh, y0), (name, name0)
    assert same(psi_only, p0)


def report(tag, pn, gn, po, go, extra=""):
    """Prints and returns (largest relative psi deviation, gradient deviation over its largest component)."""
    dp = float(np.max(np.abs(pn - po) / np.abs(po)))
    dg = float(rel(gn, go))
    print("r21 %s psi %.2e (bar 1e-12) grad %.2e (bar 1e-9)%s" % (tag, dp, dg, extra))
    return dp, dg


def assert_oracle(tag, outs, po, go, extra=""):
    pn, gn = outs[0][1].cpu().numpy(), outs[0][2].cpu().numpy()
    report(tag, pn, gn, po, go, extra)
    assert np.isfinite(po).all() and np.isfinite(go).all()
    assert np.allclose(pn, po, rtol=1e-12)
    assert rel(gn, go) <= 1e-9


# ----------------------------------------------------------------------------- (a) rollout and plant step
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("nfe", [1, 2, 3, 5, 8, 16])
@pytest.mark.parametrize("model", [0, 1])
def test_rollout_matches_oracle(dev, O, model, nfe, clip):
    """eng.rollout (stage_forward_steps for every stage) against O.rollout: two waves plus two lanes, 1e-12; no NaN or
    infinity on either side.  The clipped cases take the inputs and the narrowed limits of the clipped-input tests."""
    B, N = 130, 7
    kw = dict(nfe=nfe, clip_inputs=clip)
    if clip:
        kw["veh"] = narrow_veh(model)
    cfg, ocfg = both(O, model, N, **kw)
    X0 = synthetic_states(model, B, seed=40 + nfe)
    U = clipped_inputs(B, N, seed=nfe) if clip else ordinary_inputs(B, N, seed=nfe)
    if clip and model == 1:
        X0[:, 3] += PAC_CLIP_VX
    eng = mp.BatchedMPC(cfg, dev)
    X = eng.rollout(T(X0, dev), T(U, dev)).cpu().numpy()
    Xo = np.stack([O.rollout(ocfg, X0[a], U[a]) for a in range(B)])
    worst = np.max(np.abs(X - Xo) / (1.0 + np.abs(Xo)))          # the quantity allclose bounds by 1e-12 below
    print("r21 rollout model %d nfe %d clip %d: %.2e (bar 1e-12), min vx %.2f" % (model, nfe, clip, worst, Xo[:, :, 3].min()))
    assert np.isfinite(Xo).all() and (model == 0 or Xo[:, :, 3].min() > 0.25)
    assert np.array_equal(np.isnan(X), np.isnan(Xo)) and np.array_equal(np.isinf(X), np.isinf(Xo))
    assert np.allclose(X, Xo, rtol=1e-12, atol=1e-12)
    # the plant step of the closed loop is the same stage: Nsim = 1
    x1 = eng.rollout(T(X0, dev), T(U[:, :2], dev)).cpu().numpy()[:, 0]
    xo = np.stack([O.fd(ocfg, X0[a], U[a, :2]) for a in range(B)])
    assert np.allclose(x1, xo, rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------- (b) cost and gradient on every route
KIN_CASES = [(0, N, nfe) for N in (1, 7, 32, 33, 64) for nfe in (1, 3, 8)] + [(0, 7, 16)]
PAC_CASES = [(1, N, nfe) for N in (1, 12, 33) for nfe in (2, 8)]


@pytest.mark.parametrize("model,N,nfe", KIN_CASES + PAC_CASES)
def test_cost_and_gradient_on_every_route(dev, O, monkeypatch, model, N, nfe):
    """Default switches, K1b / K1c as two launches, MPC_NO_QUAD and the wave-per-agent evaluation: the same bits, the
    cost-only request the same psi bits, and the oracle's psi and gradient within 1e-12 / 1e-9.  N = 32 / 33 is where the
    persistent kernel's evaluation changes from the two-half layout to the single one; N = 64 is MPC_MAX_N."""
    B = 67 if N == 64 else 130
    cfg, ocfg = both(O, model, N, nfe=nfe)
    X0 = synthetic_states(model, B, seed=B)
    U = ordinary_inputs(B, N, seed=N)
    cl = straight_centerline()
    outs, psi_only, _ = every_route(monkeypatch, dev, cfg, T(X0, dev), T(cl, dev), T(U, dev))
    assert_routes_agree(outs, psi_only)
    po, go = O.psi_batch(ocfg, X0, cl, U)
    assert_oracle("every_route model %d N %d nfe %d:" % (model, N, nfe), outs, po, go)


# ----------------------------------------------------------------------------- (c) stages outside step_trig's range
@pytest.mark.parametrize("nfe", [1, 2, 3])
def test_stages_outside_the_trig_range_at_other_step_counts(dev, O, monkeypatch, nfe):
    """The recipe of test_stages_outside_the_fast_range_are_the_same_in_every_rollout where step_trig is the only trig
    route: speeds up to 6, 8 % of the stages with the wheels near 90 degrees, a few steering entries of 2e5.  Lanes of one
    wave take different routes here (rotations where the step's heading increments are small, the plain RK4 angles where
    they are not): thread-per-request, unfused and wave evaluations give the same bits, and the oracle's psi and gradient
    within 1e-12 / 1e-9 wherever its cost is finite.  step_trig's test, restated for the first RK4 step of stage 0, fails
    for between 3 % and 50 % of the requests."""
    B, N = 330, 9
    rng = np.random.default_rng(41)
    x0 = synthetic_states(0, B, seed=29)
    x0[:, 3] = rng.uniform(0.3, 6.0, B)
    U = np.tile([0.6, 0.0], (B, N)) + rng.uniform(-.4, .4, (B, 2 * N)) * np.tile([1, .6], N)
    wild = rng.random((B, N)) < 0.08
    wild[::7] = False
    wild[3::50] = True
    U[:, 1::2] = np.where(wild, np.sign(rng.standard_normal((B, N))) * rng.uniform(1.3, 1.85, (B, N)), U[:, 1::2])
    U[5::90, 1] = 2.0e5
    cl = straight_centerline()
    cfg, ocfg = both(O, 0, N, nfe=nfe)
    outs, psi_only, _ = every_route(monkeypatch, dev, cfg, T(x0, dev), T(cl, dev), T(U, dev))
    assert_routes_agree(outs, psi_only)
    # step_trig (mpc_device.hpp), first RK4 step of stage 0
    lf, lr, h = cfg.veh[1], cfg.veh[2], cfg.Ts / cfg.nfe
    beta = np.arctan2(lf * np.tan(U[:, 1]), lf + lr)
    sb_lr, ad = np.sin(beta) / lr, cfg.accel * U[:, 0]
    v1 = x0[:, 3]
    v2 = v1 + 0.5 * h * (ad - cfg.friction * v1)
    v3 = v1 + 0.5 * h * (ad - cfg.friction * v2)
    d2, d3, d4 = 0.5 * h * v1 * sb_lr, 0.5 * h * v2 * sb_lr, h * v3 * sb_lr
    ok = (np.abs(d2) <= 0.75) & (np.abs(d3) <= 0.75) & (np.abs(d4) <= 0.75) & (np.abs(x0[:, 2] + beta) < 1.0e5)
    out0 = float((~ok).mean())
    assert 0.03 <= out0 <= 0.5, out0
    mixed = np.array([0 < (~ok)[i:i + 64].sum() < len(ok[i:i + 64]) for i in range(0, B, 64)])
    assert mixed.sum() >= 3                                       # waves of the thread-per-request rollout that take both routes
    po, go = O.psi_batch(ocfg, x0, cl, U)
    fin = np.isfinite(po)
    pn, gn = outs[0][1].cpu().numpy(), outs[0][2].cpu().numpy()
    report("trig_range nfe %d:" % nfe, pn[fin], gn[fin], po[fin], go[fin], " out of range %.1f %%, oracle finite %d / %d" % (100 * out0, fin.sum(), B))
    assert fin.mean() > 0.95
    assert np.array_equal(np.isnan(pn), np.isnan(po))
    assert np.allclose(pn[fin], po[fin], rtol=1e-12, atol=0)
    assert np.abs(gn[fin] - go[fin]).max() <= 1e-9 * np.abs(go[fin]).max()


# ----------------------------------------------------------------------------- (d) clipped inputs
def clipped_problem(model, B, N, steer=NARROW[0], drive=NARROW[1]):
    X0 = synthetic_states(model, B, seed=61)
    if model == 1:
        X0[:, 3] += PAC_CLIP_VX
    U = clipped_inputs(B, N, seed=7, steer=steer, drive=drive)
    U2 = clipped_inputs(B, N, seed=8, steer=steer, drive=drive)
    return X0, U, U2


@pytest.mark.parametrize("nfe", [4, 2])
@pytest.mark.parametrize("model", [0, 1])
def test_clipped_inputs_on_every_route(dev, O, monkeypatch, model, nfe):
    """clip_inputs = 1 with limits narrower than the inputs (veh[9] = 0.2, veh[10] = 0.6): between 20 % and 60 % of the
    inputs are clipped, every agent has a clipped and an unclipped stage, and a few inputs lie exactly on a limit.  At
    nfe = 4 the two-lane / four-lane rollout, the thread-per-request one, the unfused launches, the wave-per-agent
    evaluation and (kinematic model) the two-points-in-one-trip evaluation; at nfe = 2 the routes of the other step
    counts.  The same bits from all of them, the oracle's psi and gradient within 1e-12 / 1e-9."""
    B, N = 130, 10
    cfg, ocfg = both(O, model, N, nfe=nfe, clip_inputs=1, veh=narrow_veh(model))
    X0, U, U2 = clipped_problem(model, B, N)
    mk = clip_masks(U, *NARROW)
    share = float(mk.mean())
    st_clipped = mk.any(2)
    assert 0.2 <= share <= 0.6, share
    assert st_clipped.any(1).all() and (~st_clipped).any(1).all()
    on_limit = (np.abs(U.reshape(B, N, 2)) == np.array([NARROW[1], NARROW[0]])).sum()
    assert on_limit >= 20 and not mk[np.abs(U.reshape(B, N, 2)) == np.array([NARROW[1], NARROW[0]])].any()
    cl = straight_centerline()
    X0t, clt, Ut, U2t = T(X0, dev), T(cl, dev), T(U, dev), T(U2, dev)
    outs, psi_only, eng = every_route(monkeypatch, dev, cfg, X0t, clt, Ut)
    assert_routes_agree(outs, psi_only)
    if model == 1:
        assert min(O.rollout(ocfg, X0[a], U[a])[:, 3].min() for a in range(B)) > 0.25      # see PAC_CLIP_VX
    po, go = O.psi_batch(ocfg, X0, cl, U)
    assert_oracle("clipped model %d nfe %d:" % (model, nfe), outs, po, go, " clipped share %.1f %%" % (100 * share))
    if model == 0 and nfe == 4:
        outs2, _, _ = every_route(monkeypatch, dev, cfg, X0t, clt, U2t, routes=ROUTES[:1])
        psi, grad, grad2, _ = eng.eval_cost_grad_pair(X0t, clt, Ut, U2t)
        assert same(psi, outs[0][1]) and same(grad, outs[0][2]) and same(grad2, outs2[0][2])
        po2, go2 = O.psi_batch(ocfg, X0, cl, U2)
        assert rel(grad2.cpu().numpy(), go2) <= 1e-9


@pytest.mark.parametrize("nfe", [4, 2])
@pytest.mark.parametrize("model", [0, 1])
def test_clip_limits_come_from_the_agents_parameter_row(dev, O, monkeypatch, model, nfe):
    """include/mpc_hip.h: with a parameter table bound the clip limits are those of the agent's row.  Two rows whose
    veh[9] / veh[10] differ (0.2 / 0.6 and 0.3 / 0.9), agents alternating between them, against the oracle run per agent
    with that row's values; the routes of test_clipped_inputs_on_every_route, the same bits, 1e-12 / 1e-9."""
    B, N = 130, 10
    rows = ((0.2, 0.6), (0.3, 0.9))
    idx = (np.arange(B) % 2).astype(np.int32)
    steer, drive = np.array([rows[i][0] for i in idx]), np.array([rows[i][1] for i in idx])
    cfg = mp.default_config(model, N, nfe=nfe, clip_inputs=1)
    tab = _lib.param_rows(cfg, 2, veh=np.stack([narrow_veh(model, *r) for r in rows]))
    assert tab[0, 9] == 0.2 and tab[1, 10] == 0.9
    X0, U, U2 = clipped_problem(model, B, N, steer, drive)
    mk = clip_masks(U, steer, drive)
    assert mk[idx == 0].mean() > 2 * mk[idx == 1].mean() > 0.05      # the rows do clip differently
    cl = straight_centerline()
    X0t, clt, Ut, U2t = T(X0, dev), T(cl, dev), T(U, dev), T(U2, dev)
    tabt, idxt = T(tab, dev), T(idx, dev, torch.int32)
    bind = lambda e: e.set_agent_params(tabt, idxt)
    outs, psi_only, eng = every_route(monkeypatch, dev, cfg, X0t, clt, Ut, bind=bind)
    assert_routes_agree(outs, psi_only)

    def oracle_of(Uany):
        return by_row(idx, 2, lambda p, sel: O.psi_batch(O.default_config(model, N, nfe=nfe, clip_inputs=1, veh=narrow_veh(model, *rows[p])),
                                                          X0[sel], cl, Uany[sel]))
    po, go = oracle_of(U)
    assert_oracle("clip_rows model %d nfe %d:" % (model, nfe), outs, po, go)
    # the rows matter: the handle's own limits (the defaults, wider than both rows) give another cost
    plain = mp.BatchedMPC(cfg, dev).eval_cost_grad(X0t, clt, Ut)[0]
    touched = torch.tensor(mk.any((1, 2)), device=dev)
    assert touched.float().mean() > 0.8 and (~torch.isclose(plain, outs[0][1], rtol=1e-9))[touched].float().mean() > 0.9
    if model == 0 and nfe == 4:
        outs2, _, _ = every_route(monkeypatch, dev, cfg, X0t, clt, U2t, bind=bind, routes=ROUTES[:1])
        psi, grad, grad2, _ = eng.eval_cost_grad_pair(X0t, clt, Ut, U2t)
        assert same(psi, outs[0][1]) and same(grad, outs[0][2]) and same(grad2, outs2[0][2])
        assert rel(grad2.cpu().numpy(), oracle_of(U2)[1]) <= 1e-9


# ----------------------------------------------------------------------------- (e) ALM terms
@pytest.mark.parametrize("constr,model", [(1, 1), (1, 0), (2, 1), (2, 0)])
def test_augmented_lagrangian_terms_at_two_steps(dev, O, constr, model):
    """test_augmented_lagrangian_terms_match_oracle at nfe = 2, through eval_cost_grad and the wave-per-agent evaluation:
    the same bits; psi, gradient and yhat = Sigma (zeta - Pi_D zeta) at that test's tolerances."""
    N, B = 10, 96
    kw = dict(constr_mode=constr, D_lb=[-np.inf] * 6, D_ub=[0.0] * 6, g_off=[20, 1, 1, 0.5, 1, 0.1], lane_halfwidth=0.05, nfe=2)
    cfg, ocfg = both(O, model, N, **kw)
    eng = mp.BatchedMPC(cfg, dev)
    m = eng.m
    assert m == O.m(ocfg) and m > 0
    X0 = synthetic_states(model, B, seed=3)
    rng = np.random.default_rng(9)
    U = np.tile([0.7, 0.0], (B, N)) + rng.uniform(-.3, .3, (B, 2 * N)) * np.tile([1, .3], N)
    y = rng.uniform(-2, 2, (B, m)); Sig = rng.uniform(1, 1e4, (B, m))
    cl = straight_centerline()
    args = (T(X0, dev), T(cl, dev), T(U, dev), T(y, dev), T(Sig, dev))
    psi, g, yh = eng.eval_cost_grad(*args)
    psiw, gw, yhw = eng.eval_cost_grad(*args, wave=True)
    assert same(psi, psiw) and same(g, gw) and same(yh, yhw)
    po, go = O.psi_batch(ocfg, X0, cl, U, y, Sig)
    report("alm constr %d model %d nfe 2:" % (constr, model), psi.cpu().numpy(), g.cpu().numpy(), po, go)
    assert np.allclose(psi.cpu().numpy(), po, rtol=1e-12)
    assert rel(g.cpu().numpy(), go) <= 1e-9
    gU = np.stack([O.constraints(ocfg, X0[b], cl, U[b]) for b in range(B)])
    zeta = gU + y / Sig
    lbd = -0.05 if constr == 2 else -np.inf
    ubd = 0.05 if constr == 2 else 0.0
    ref = Sig * (zeta - np.clip(zeta, lbd, ubd))
    assert np.allclose(yh.cpu().numpy(), ref, rtol=1e-10, atol=1e-9)


# ----------------------------------------------------------------------------- (f) solves
@pytest.mark.parametrize("model,N,B,kw", [
    (0, 10, 96, dict(nfe=1)), (0, 10, 96, dict(nfe=8)), (0, 36, 40, dict(nfe=3)), (1, 8, 70, dict(nfe=2)), (1, 20, 40, dict(nfe=3)),
    (0, 10, 96, dict(nfe=2, clip_inputs=1)), (1, 8, 70, dict(nfe=4, clip_inputs=1))])
def test_solves_match_oracle_on_every_path(dev, O, model, N, B, kw):
    """Rounds only, the persistent kernel from the start and a switch in mid-solve (test_persistent_kernel_is_bit_identical)
    give the same controls and statistics bit for bit; against the oracle with both converged to 1e-10: every agent
    Converged on both sides, the same number of outer iterations, controls within 1e-5 relative (median 1e-7), psi 1e-10.
    The kinematic model runs the lane-serial rollout of the persistent kernel here: two halves with a speculative gradient
    for N <= 32, lane 0 alone at N = 36."""
    cfg, ocfg = both(O, model, N, alm_eps=1e-10, max_total_inner=4000, **kw)
    X0 = synthetic_states(model, B, seed=21)
    cl = straight_centerline()
    U0 = np.tile([1., 0.], (B, N))
    X0t, clt, U0t = T(X0, dev), T(cl, dev), T(U0, dev)
    out = []
    for solo_max in (0, 100000, (5 * B) // 8):   # rounds only / persistent kernel from the start / switch in mid-solve
        eng = mp.BatchedMPC(cfg, dev)
        eng.set_poll_timeout(30.0)               # a solve that stops making progress is an error, not a long wait
        eng.set_solo_max(solo_max)
        U, lam, st = eng.solve(X0t, clt, U0t)
        out.append((U, st, eng.last_solve_info()))
    (Ur, sr, ir), (Us, ss, is_), (Um, sm, im) = out
    assert ir["solo_agents"] == 0 and ir["rounds"] > 0
    assert is_["solo_agents"] == B and is_["rounds"] == 0
    assert 0 < im["solo_agents"] < B and im["rounds"] > 0, im
    for U, st in ((Us, ss), (Um, sm)):
        assert torch.equal(U, Ur) and torch.equal(st, sr)
    U, st = Ur.cpu().numpy(), sr.cpu().numpy()
    Uo, _, sto = O.solve_batch(ocfg, X0, cl, U0)
    d = np.abs(U - Uo).max(1) / np.maximum(1.0, np.abs(Uo).max(1))
    dpsi = np.abs(st[:, 6] - sto[:, 6]) / np.abs(sto[:, 6])
    print("r21 solve model %d N %d B %d %s: controls max %.2e (bar 1e-5) median %.2e (bar 1e-7) psi %.2e (bar 1e-10) "
          "switch at %d of %d agents" % (model, N, B, kw, d.max(), np.median(np.abs(U - Uo).max(1)), dpsi.max(), im["solo_agents"], B))
    assert (st[:, 0] == 1).all() and (sto[:, 0] == 1).all()
    assert np.array_equal(st[:, 1], sto[:, 1])
    assert (d <= 1e-5).all()
    assert np.median(np.abs(U - Uo).max(1)) <= 1e-7
    assert np.allclose(st[:, 6], sto[:, 6], rtol=1e-10, atol=0)


# ----------------------------------------------------------------------------- (g) closed loop
@pytest.mark.parametrize("model", [0, 1])
def test_closed_loop_at_two_steps(dev, O, model):
    """test_device_closed_loop_matches_host_loop at nfe = 2: mpc_closed_loop against solve + rollout(Nsim = 1) driven from
    the host, bit for bit; the first plant state within 1e-12 of the oracle's plant."""
    N, B, Tn = 8, 64, 3
    cfg, ocfg = both(O, model, N, max_total_inner=1500, nfe=2)
    eng = mp.BatchedMPC(cfg, dev)
    eng.set_poll_timeout(30.0)
    X0 = synthetic_states(model, B, seed=13)
    cl = straight_centerline()
    U0 = np.tile([1., 0.], (B, N))
    xT, U, _, tx, tu, fails, _ = eng.closed_loop(T(X0, dev), T(cl, dev), T(U0, dev), Tn)
    x = T(X0, dev); Uw = T(U0, dev)
    for t in range(Tn):
        Uw, _, st = eng.solve(x, T(cl, dev), Uw)
        u0 = Uw[:, :2].contiguous()
        x = eng.rollout(x, u0)[:, 0, :].contiguous()
        assert torch.equal(tx[:, t], x) and torch.equal(tu[:, t], u0)
    assert torch.equal(xT, x) and int(fails.sum()) == 0
    xo = np.stack([O.fd(ocfg, X0[b], tu[b, 0].cpu().numpy()) for b in range(B)])
    assert np.allclose(tx[:, 0].cpu().numpy(), xo, rtol=1e-12, atol=1e-13)


# ----------------------------------------------------------------------------- (h) refusal
def test_two_points_in_one_trip_is_refused_at_two_steps(dev):
    """mpc_eval_cost_grad_wave2 is the half-wave form of the WIDE rollout (nfe = 4): a kinematic handle with nfe = 2 refuses
    it with the argument error and leaves the output buffers as they were."""
    N, B = 12, 16
    eng = mp.BatchedMPC(mp.default_config(0, N, nfe=2), dev)
    X0 = T(synthetic_states(0, B, seed=2), dev)
    cl = T(straight_centerline(), dev)
    U = T(ordinary_inputs(B, N, seed=1), dev); U2 = T(ordinary_inputs(B, N, seed=2), dev)
    with pytest.raises(_lib.MpcError, match="nfe = 4"):
        eng.eval_cost_grad_pair(X0, cl, U, U2)
    psi = torch.full((B,), 7.5, dtype=torch.float64, device=dev)
    grad = torch.full((B, 2 * N), -3.25, dtype=torch.float64, device=dev)
    grad2 = torch.full((B, 2 * N), 11.0, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = eng.lib.mpc_eval_cost_grad_wave2(eng._h, B, p(X0), p(cl), None, p(U), p(U2), None, None, p(psi), p(grad), p(grad2), None, stream)
    torch.cuda.synchronize(dev)
    assert rc == -1                                                    # MPC_E_ARG
    assert (psi == 7.5).all() and (grad == -3.25).all() and (grad2 == 11.0).all()
    # the one-point evaluations of the same handle are served
    assert torch.isfinite(eng.eval_cost_grad(X0, cl, U, wave=True)[0]).all()
