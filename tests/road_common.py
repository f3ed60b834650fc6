"""The checker of the road cost (mpc_set_agent_roads): a numpy restatement on top of the frozen oracle, which does not know
the term.  Shared by tests/test_agent_roads_cpu.py and tests/test_gpu_agent_roads.py.

  row      [N][NROAD], one stage [off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v]
  e        [N] the signed lateral offset of the state at the end of every stage: O.constraints on a CONSTR_LANE
           configuration of the same model, N and overrides (positive to the right of the direction of travel; on
           discs_common.line_centerline(), e = -(y - 0.5))
  term     sum over the stages, in stage order, of  w_off (e - off)^2 + w_lo min(e - lo, 0)^2 + w_hi max(e - hi, 0)^2
           + w_v (sp - v_tgt)^2;  a part whose weight is 0 adds nothing.  sp: x[3], Pacejka sqrt(x[3]^2 + x[4]^2)
  de       [N] d term / d e_k = 2 w_off (e - off) + 2 w_lo min(e - lo, 0) + 2 w_hi max(e - hi, 0)
  grad     exactly, without finite differences.
           lateral: on the lane configuration with Sigma = 1 the oracle's yhat = zeta - clip(zeta, -hw, hw), zeta = e + y;
           y = de + hw sign(de) - e where de != 0 and y = -e elsewhere makes yhat = de, and O.psi's gradient minus grad f
           is J_e' de (the trick of field_common.lane_conditions).
           speed: the STATE_SQ "VJP machine" of discs_common.configs with t[k, 3] = 2 w_v ev / (2 v) (kinematic) or
           t[k, 3] = t[k, 4] = 2 w_v ev / (2 sp) (Pacejka).  Speeds must stay away from 0.
  beside other tables: rate_common's, field_common's and discs_common's terms on top.
  solve    m = 0: rate_common's inner solve; discs: the ALM loop of discs_common.reference_solve around the extended psi.
Configuration overrides (`common`) go into all three configurations of the machine alike."""
import numpy as np

import discs_common as D
import field_common as F
import rate_common as R

NROAD = 8
MACHINE_HW = 0.25          # the half-width of the lane configuration that serves as the VJP machine (any positive value)


def machine(O, model, N, **common):
    """(the unconstrained configuration, the STATE_SQ one, the LANE one)"""
    c0, c1 = D.configs(O, model, N, **common)
    return c0, c1, O.default_config(model, N, constr_mode=O.CONSTR_LANE, lane_halfwidth=MACHINE_HW, **common)


def speed(X):
    return X[:, 3] if X.shape[1] == 4 else np.sqrt(X[:, 3] * X[:, 3] + X[:, 4] * X[:, 4])


def road_values(e, X, row):
    """(term, de [N], dv [N] = 2 w_v ev) of the offsets e [N] and the end-of-stage states X [N, nx]; the term summed in
    stage order, part by part, as the kernels add it"""
    r = np.asarray(row, dtype=np.float64).reshape(X.shape[0], NROAD)
    sp = speed(X)
    term = 0.0
    de, dv = np.zeros(X.shape[0]), np.zeros(X.shape[0])
    for k in range(X.shape[0]):
        off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v = r[k]
        if w_off != 0.0:
            t = e[k] - off
            term += w_off * t * t
            de[k] += 2.0 * w_off * t
        if w_lo != 0.0 and e[k] - lo < 0.0:
            q = e[k] - lo
            term += w_lo * q * q
            de[k] += 2.0 * w_lo * q
        if w_hi != 0.0 and e[k] - hi > 0.0:
            p = e[k] - hi
            term += w_hi * p * p
            de[k] += 2.0 * w_hi * p
        if w_v != 0.0:
            ev = sp[k] - v_tgt
            term += w_v * ev * ev
            dv[k] = 2.0 * w_v * ev
    return float(term), de, dv


def road_term(O, mach, x0, cl, U, row, want_grad=True):
    """(term, its gradient [2N] with respect to U, or None)"""
    c0, c1, cL = mach
    N = c0.N
    X = O.rollout(c0, x0, U)
    e = O.constraints(cL, x0, cl, U)
    term, de, dv = road_values(e, X, row)
    if not want_grad:
        return term, None
    _, g0 = O.psi(c0, x0, cl, U)
    y = np.where(de != 0.0, de + MACHINE_HW * np.sign(de) - e, -e)
    _, gl = O.psi(cL, x0, cl, U, y, np.ones(N))
    nx = X.shape[1]
    t = np.zeros((N, nx))
    sp = speed(X)
    t[:, 3] = dv / (2.0 * sp)
    if nx == 6:
        t[:, 4] = dv / (2.0 * sp)
    g_sq = O.constraints(c1, x0, cl, U)
    _, gs = O.psi(c1, x0, cl, U, t.reshape(-1) - g_sq, np.ones(N * nx))
    return term, (gl - g0) + (gs - g0)


def psi(O, cfg, mach, x0, cl, U, row, y=None, Sigma=None, rate_row=None, field_row=None, want_grad=True):
    """(psi, grad or None) on the handle's oracle configuration `cfg` (NONE, STATE_SQ or LANE), mach = machine(...)"""
    p, g = O.psi(cfg, x0, cl, U, y, Sigma, want_grad=want_grad)
    parts = [road_term(O, mach, x0, cl, U, row, want_grad)]
    if field_row is not None:
        parts.append(F.field_term(O, mach[:2], x0, cl, U, field_row, want_grad))
    if rate_row is not None:
        parts.append(R.rate_term(U, rate_row, want_grad))
    for t, tg in parts:
        p = p + t
        if want_grad:
            g = g + tg
    return p, (g if want_grad else None)


def psi_discs(O, mach, x0, cl, U, discs, y, Sigma, row, rate_row=None, want_grad=True):
    """(psi, yhat, grad or None, g) on a disc handle: discs_common.psi_yhat plus the term (and rate_common's)"""
    p, yh, g, gv = D.psi_yhat(O, mach[:2], x0, cl, U, discs, y, Sigma, want_grad)
    parts = [road_term(O, mach, x0, cl, U, row, want_grad)]
    if rate_row is not None:
        parts.append(R.rate_term(U, rate_row, want_grad))
    for t, tg in parts:
        p = p + t
        if want_grad:
            g = g + tg
    return p, yh, (g if want_grad else None), gv


def psi_fd_grad(fun, U, h=1e-6):
    """central differences of fun(U) -> psi"""
    U = np.asarray(U, dtype=np.float64)
    out = np.empty(U.size)
    for i in range(U.size):
        e = np.zeros(U.size); e[i] = h
        out[i] = (fun(U + e) - fun(U - e)) / (2 * h)
    return out


def _box(N, u_lb, u_ub):
    return [(u_lb[i % 2], u_ub[i % 2]) for i in range(2 * N)], np.tile(u_lb, N), np.tile(u_ub, N)


def reference_solve(O, cfg, mach, x0, cl, row, U0=None, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """U of the unconstrained problem (m = 0) with the road cost of `row`; row None: without it"""
    N = cfg.N
    bounds, lb_, ub_ = _box(N, u_lb, u_ub)
    U = np.zeros(2 * N) if U0 is None else np.asarray(U0, dtype=np.float64).copy()
    if row is None:
        return R._inner(lambda u: O.psi(cfg, x0, cl, u), U, lb_, ub_, bounds)
    return R._inner(lambda u: psi(O, cfg, mach, x0, cl, u, row), U, lb_, ub_, bounds)


def reference_solve_discs(O, mach, x0, cl, discs, row, U0=None, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32), Sigma0=10.0, tol=1e-8,
                          max_outer=12):
    """(U, lambda, outer iterations): the ALM loop of discs_common.reference_solve around the extended psi"""
    N = mach[0].N
    bounds, lb_, ub_ = _box(N, u_lb, u_ub)
    U = np.zeros(2 * N) if U0 is None else np.asarray(U0, dtype=np.float64).copy()
    y = np.zeros(D.NDISC * N)
    Sigma = np.full(D.NDISC * N, float(Sigma0))
    for outer in range(1, max_outer + 1):
        def fun(u):
            p, _, gr, _ = psi_discs(O, mach, x0, cl, u, discs, y, Sigma, row)
            return p, gr
        U = R._inner(fun, U, lb_, ub_, bounds)
        _, yhat, _, _ = psi_discs(O, mach, x0, cl, U, discs, y, Sigma, row, None, False)
        e = (yhat - y) / Sigma
        y = yhat
        if np.abs(e).max() < tol:
            return U, y, outer
        Sigma = Sigma * 10.0
    raise AssertionError("the reference solve did not reach ||e|| < %g in %d outer iterations" % (tol, max_outer))


def projected_gradient(O, cfg, mach, x0, cl, U, row, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """|| U - proj_C(U - grad (f + road)(U)) ||_inf on an unconstrained configuration"""
    _, g = psi(O, cfg, mach, x0, cl, U, row)
    _, lb, ub = _box(cfg.N, u_lb, u_ub)
    return np.abs(U - np.clip(U - g, lb, ub)).max()


def disc_conditions(O, mach, x0, cl, U, discs, lam, row, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """(disc violation max(-g, 0), projected-gradient residual of f + road + lam' g) of a solve on a disc handle:
    discs_common.lagrangian_residual's machine, fed the multipliers, with the road term's gradient added"""
    c0, c1 = mach[:2]
    N = c0.N
    X = O.rollout(c0, x0, U)
    g, dx, dy = D.disc_g(X, discs)
    lm = np.asarray(lam, dtype=np.float64).reshape(N, D.NDISC)
    nx = X.shape[1]
    t = np.zeros((N, nx))
    t[:, 0] = np.sum(lm * 2.0 * dx, 1) / (2.0 * X[:, 0])
    t[:, 1] = np.sum(lm * 2.0 * dy, 1) / (2.0 * X[:, 1])
    g_sq = O.constraints(c1, x0, cl, U)
    _, grad = O.psi(c1, x0, cl, U, t.reshape(-1) - g_sq, np.ones(N * nx))
    grad = grad + road_term(O, mach, x0, cl, U, row)[1]
    _, lb, ub = _box(N, u_lb, u_ub)
    return np.maximum(-g, 0.0).max(), np.abs(U - np.clip(U - grad, lb, ub)).max()


# ----------------------------------------------------------------------------- rows
def rows(N, offset=0.0, w_offset=0.0, lo=0.0, w_lo=0.0, hi=0.0, w_hi=0.0, v_target=0.0, w_speed=0.0):
    """one row [N, NROAD]; every argument a scalar or an [N]"""
    r = np.zeros((N, NROAD))
    for i, v in enumerate((offset, w_offset, lo, w_lo, hi, w_hi, v_target, w_speed)):
        r[:, i] = v
    return r


def random_rows(rng, P, N, off_zero=0.2):
    """P rows [P, N, NROAD] for the evaluation tests: every part live on most stages (the edges 0.04 .. 0.10 apart around
    the line, so that cars spread +-0.3 about it are beyond one of them), about a fifth of the weights switched off (0, the
    word beside it left as drawn: it must not be read)"""
    tab = np.zeros((P, N, NROAD))
    tab[..., 0] = rng.uniform(-0.15, 0.15, (P, N))
    tab[..., 2] = rng.uniform(-0.08, -0.01, (P, N))
    tab[..., 4] = rng.uniform(0.01, 0.08, (P, N))
    tab[..., 6] = rng.uniform(0.3, 1.2, (P, N))
    for i, (a, b) in zip((1, 3, 5, 7), ((1.0, 8.0), (5.0, 60.0), (5.0, 60.0), (0.5, 4.0))):
        tab[..., i] = rng.uniform(a, b, (P, N)) * (rng.uniform(0, 1, (P, N)) > off_zero)
    return tab


def zero_weight_rows(rng, P, N):
    """P rows whose weights are all 0 and whose other words are drawn at random: no table at all"""
    tab = np.zeros((P, N, NROAD))
    for i in (0, 2, 4, 6):
        tab[..., i] = rng.uniform(-1.0, 1.0, (P, N))
    return tab


def script_window(script, index, ti, N, wrap=False):
    """mpc_roads_from_script in numpy: [B, N, NROAD] from script [Ps, Lt, NROAD] and index [B]"""
    script = np.asarray(script)
    Lt = script.shape[1]
    k = ti + np.arange(N)
    s = k % Lt if wrap else np.minimum(k, Lt - 1)
    return script[np.asarray(index)][:, s]


# ----------------------------------------------------------------------------- the scenes of the solve tests
# The Pacejka scene starts 0.12 beside the line as rate_common.X0_PAC does, but at 0.8 m/s, not at its 0.5: from 0.5 the third
# start of shift 15 (a draw of the whole input box that brakes hard for most of the horizon) takes the car down to 0.036 m/s,
# where the tyre model's slip angles atan(vy / vx) are singular, and the reference's L-BFGS-B stalls there with a projected
# gradient of 0.64 -- not a minimum of anything (spread between the starts 2.0; the other 47 solves agreed to 1e-15).  From
# 0.8 m/s no start of any shift gets below 0.79 and all 48 agree to 6e-15.
X0_PAC = np.array([1.0, 0.62, 0.0, 0.8, 0.0, 0.0])
# name -> (model, N, x0, handle); every scene on discs_common.line_centerline() (the line y = 0.5) from x0
SCENES = {"change": (0, 20, D.X0_KIN, "none"), "edges": (0, 20, R.X0_KIN, "none"), "brake": (0, 20, D.X0_KIN, "none"),
          "pacejka": (1, 12, X0_PAC, "none"), "disc_road": (0, 20, D.X0_KIN, "discs")}
NONE_SCENES = ("change", "edges", "brake", "pacejka")
DISC_SHIFTS = 4
CHANGE_AT, CHANGE_OFF, CHANGE_W = 6, -0.10, 5.0
EDGE_HALF, EDGE_W = 0.05, 50.0
BRAKE_V, BRAKE_W = (0.8, 0.3), 2.0
DISC_EDGE_HALF, DISC_EDGE_W = 0.06, 20.0


def scene_row(name, shift=(0.0, 0.0)):
    """(model, N, x0, row [N, NROAD], discs [N, NDISC, 3] or None) of the scenes
    change     the lateral target leaves the line at stage 6: off = 0, then -0.10 + shift_y (0.10 to the left), w_off = 5
    edges      the car starts 0.12 beside the line, the road is +-0.05 (+ shift_y) wide, w_lo = w_hi = 50
    brake      the speed target falls from 0.8 to 0.3 (+ shift_x) along the horizon, w_v = 2
    pacejka    the `edges` row on the Pacejka model, N = 12, from 0.8 m/s (X0_PAC above says why)
    disc_road  discs_common.scene_standing(N, shift) on a disc handle and road edges at +-0.06, w_lo = w_hi = 20"""
    model, N, x0, _ = SCENES[name]
    discs = None
    if name == "change":
        off = np.where(np.arange(N) < CHANGE_AT, 0.0, CHANGE_OFF + shift[1])
        row = rows(N, offset=off, w_offset=CHANGE_W)
    elif name in ("edges", "pacejka"):
        row = rows(N, lo=-EDGE_HALF + shift[1], w_lo=EDGE_W, hi=EDGE_HALF + shift[1], w_hi=EDGE_W)
    elif name == "brake":
        row = rows(N, v_target=np.linspace(BRAKE_V[0], BRAKE_V[1], N) + shift[0], w_speed=BRAKE_W)
    else:
        row = rows(N, lo=-DISC_EDGE_HALF, w_lo=DISC_EDGE_W, hi=DISC_EDGE_HALF, w_hi=DISC_EDGE_W)
        discs = D.scene_standing(N, shift)
    return model, N, x0, row, discs


starts = F.starts


# ----------------------------------------------------------------------------- the lane change commanded in time
# One script row: the lateral target is the line until sample SCRIPT_AT, then 0.10 to the left (the `change` scene's offset
# and weight), SCRIPT_LT samples; a host loop of SCRIPT_T steps from discs_common.X0_KIN on the line.
SCRIPT_AT, SCRIPT_LT, SCRIPT_T = 8, 30, 6


def lane_change_script():
    """[1, SCRIPT_LT, NROAD]"""
    s = np.zeros((1, SCRIPT_LT, NROAD))
    s[0, :, 1] = CHANGE_W
    s[0, SCRIPT_AT:, 0] = CHANGE_OFF
    return s


def mirror_script_loop(O, x0=None, Tn=SCRIPT_T, N=20):
    """The host loop of roads_from_script, solve and rollout on the CPU checker (kinematic model, unconstrained, U0 = 0):
    the numpy window of the script at time t, reference_solve from the shifted plan of the step before, the plant step
    x <- x_1 of the solved plan, the shift with the last input repeated.  Returns (traj_x [Tn, nx], the last plan's states
    [N, nx])."""
    x = np.asarray(D.X0_KIN if x0 is None else x0, dtype=np.float64).copy()
    mach = machine(O, 0, N)
    cl = D.line_centerline()
    script = lane_change_script()
    U = np.zeros(2 * N)
    tx = np.zeros((Tn, x.size))
    for t in range(Tn):
        row = script_window(script, [0], t, N)[0]
        U = reference_solve(O, mach[0], mach, x, cl, row, U0=U)
        plan = O.rollout(mach[0], x, U)
        x = plan[0].copy()
        tx[t] = x
        if t < Tn - 1:
            U = np.concatenate([U[2:], U[-2:]])
    return tx, plan
