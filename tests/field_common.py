"""The checker of the risk-field cost (mpc_set_agent_fields): a numpy restatement on top of the frozen oracle, which does
not know the term.  Shared by tests/test_agent_fields_cpu.py and tests/test_gpu_agent_fields.py.

  row      [N][NFIELD][NFSRC], one source [cx, cy, c, s, A, kx, ky, alpha]
  term     sum_k sum_j V,  at (x, y) of the state at the end of stage k (O.rollout):
           dx = x - cx, dy = y - cy, a = c dx + s dy, l = c dy - s dx, E = kx a^2 + ky l^2 + alpha a, V = A exp(-E);
           a source with A == 0 adds nothing
  w_k      dV/d(x, y) = (c ga - s gl, s ga + c gl),  ga = -V (2 kx a + alpha),  gl = -V (2 ky l)
  psi      O.psi (any constr_mode of the oracle's, with y and Sigma) plus the term
  grad     exactly, without finite differences, through the STATE_SQ "VJP machine" of discs_common (its t_{k,0} =
           w_{k,x} / (2 x_k), t_{k,1} = w_{k,y} / (2 y_k) with w_k of the field in the disc term's place):
           grad = grad_handle + (grad_c1 - grad_c0), grad_c1 the machine's gradient (grad f + J' w) and grad_c0 = grad f
           of the unconstrained configuration.  Positions must stay away from 0.
  beside a rate table: rate_common's term on top.
  solve    m = 0: rate_common's inner solve (L-BFGS-B restarted, then discs_common.newton_polish); LANE: the ALM loop of
           discs_common.reference_solve around the extended psi, with the oracle's own yhat.
Configuration overrides (`common`) go into the handle's configuration and the two of the VJP machine alike."""
import numpy as np

import discs_common as D
import rate_common as R

NFIELD, NFSRC = 2, 8


def field_values(X, row):
    """(V [N, NFIELD], w [N, 2] = dV/d(x, y) summed over the sources) at the end-of-stage states X [N, nx]"""
    s = np.asarray(row, dtype=np.float64).reshape(X.shape[0], NFIELD, NFSRC)
    dx = X[:, None, 0] - s[:, :, 0]
    dy = X[:, None, 1] - s[:, :, 1]
    c, sn, A, kx, ky, al = (s[:, :, i] for i in range(2, 8))
    a = c * dx + sn * dy
    l = c * dy - sn * dx
    E = kx * a * a + ky * l * l + al * a
    V = np.where(A == 0.0, 0.0, A * np.exp(-E))
    ga = -(V * (2.0 * kx * a + al))
    gl = -(V * (2.0 * ky * l))
    w = np.stack([np.sum(c * ga - sn * gl, 1), np.sum(sn * ga + c * gl, 1)], 1)
    return V, w


def machine(O, model, N, **common):
    """(the unconstrained configuration, the STATE_SQ one): discs_common.configs"""
    return D.configs(O, model, N, **common)


def field_term(O, cfgs, x0, cl, U, row, want_grad=True):
    """(term, its gradient [2N] with respect to U, or None)"""
    c0, c1 = cfgs
    N = c0.N
    X = O.rollout(c0, x0, U)
    V, w = field_values(X, row)
    term = 0.0
    for k in range(N):                       # stage order, source 0 before source 1, as the kernels add them
        for j in range(NFIELD):
            term += float(V[k, j])
    if not want_grad:
        return term, None
    nx = X.shape[1]
    t = np.zeros((N, nx))
    t[:, 0] = w[:, 0] / (2.0 * X[:, 0])
    t[:, 1] = w[:, 1] / (2.0 * X[:, 1])
    g_sq = O.constraints(c1, x0, cl, U)
    _, g1 = O.psi(c1, x0, cl, U, t.reshape(-1) - g_sq, np.ones(N * nx))
    _, g0 = O.psi(c0, x0, cl, U)
    return term, g1 - g0


def psi(O, cfg, cfgs, x0, cl, U, row, y=None, Sigma=None, rate_row=None, want_grad=True):
    """(psi, grad or None) on the handle's oracle configuration `cfg` (NONE, STATE_SQ or LANE), cfgs = machine(...)"""
    p, g = O.psi(cfg, x0, cl, U, y, Sigma, want_grad=want_grad)
    t, tg = field_term(O, cfgs, x0, cl, U, row, want_grad)
    p = p + t
    if want_grad:
        g = g + tg
    if rate_row is not None:
        rt, rg = R.rate_term(U, rate_row, want_grad)
        p = p + rt
        if want_grad:
            g = g + rg
    return p, (g if want_grad else None)


def psi_fd_grad(O, cfg, cfgs, x0, cl, U, row, y=None, Sigma=None, rate_row=None, h=1e-6):
    """central differences of the numpy psi"""
    U = np.asarray(U, dtype=np.float64)
    out = np.empty(U.size)
    for i in range(U.size):
        e = np.zeros(U.size); e[i] = h
        out[i] = (psi(O, cfg, cfgs, x0, cl, U + e, row, y, Sigma, rate_row, False)[0] -
                  psi(O, cfg, cfgs, x0, cl, U - e, row, y, Sigma, rate_row, False)[0]) / (2 * h)
    return out


def reference_solve(O, cfg, cfgs, x0, cl, row, U0=None, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """U of the unconstrained problem (m = 0) with the risk field of `row`"""
    N = cfg.N
    bounds = [(u_lb[i % 2], u_ub[i % 2]) for i in range(2 * N)]
    lb_, ub_ = np.tile(u_lb, N), np.tile(u_ub, N)
    U = np.zeros(2 * N) if U0 is None else np.asarray(U0, dtype=np.float64).copy()
    return R._inner(lambda u: psi(O, cfg, cfgs, x0, cl, u, row), U, lb_, ub_, bounds)


def psi_yhat_lane(O, cfg, cfgs, x0, cl, U, row, y, Sigma, want_grad=True):
    """(psi, grad or None, yhat [m]) on a constrained oracle configuration: the oracle's own yhat (a cost term has no
    multiplier), from the optional output of its psi"""
    import ctypes as C
    p, g = psi(O, cfg, cfgs, x0, cl, U, row, y, Sigma, None, want_grad)
    yhat = np.empty(O.m(cfg))
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a = [f64(v) for v in (x0, cl, U, y, Sigma)]
    O.lib().orc_psi(C.byref(cfg), *(ptr(v) for v in a), None, ptr(yhat))
    return p, g, yhat


def reference_solve_lane(O, cfg, cfgs, x0, cl, row, U0=None, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32), Sigma0=10.0, tol=1e-8, max_outer=12):
    """(U, lambda, outer iterations): the ALM loop of discs_common.reference_solve (Sigma0 = 10, x 10 per outer iteration,
    y <- yhat, until ||e||_inf < tol) around the extended psi of a constrained configuration (CONSTR_LANE)"""
    N, m = cfg.N, O.m(cfg)
    bounds = [(u_lb[i % 2], u_ub[i % 2]) for i in range(2 * N)]
    lb_, ub_ = np.tile(u_lb, N), np.tile(u_ub, N)
    U = np.zeros(2 * N) if U0 is None else np.asarray(U0, dtype=np.float64).copy()
    y, Sigma = np.zeros(m), np.full(m, float(Sigma0))
    for outer in range(1, max_outer + 1):
        U = R._inner(lambda u: psi(O, cfg, cfgs, x0, cl, u, row, y, Sigma), U, lb_, ub_, bounds)
        yhat = psi_yhat_lane(O, cfg, cfgs, x0, cl, U, row, y, Sigma, False)[2]
        e = (yhat - y) / Sigma
        y = yhat
        if np.abs(e).max() < tol:
            return U, y, outer
        Sigma = Sigma * 10.0
    raise AssertionError("the reference solve did not reach ||e|| < %g in %d outer iterations" % (tol, max_outer))


def lane_conditions(O, cfg, cfgs, x0, cl, U, row, lam, hw, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """(constraint violation, Lagrangian projected-gradient residual) of a LANE solve: g = O.constraints within [-hw, hw],
    and || U - proj_C(U - grad (f + field + lam' g)(U)) ||_inf.  The oracle's psi gradient is grad f + J' yhat; at Sigma = 1,
    y is chosen so that its yhat equals lam (y = lam + hw sign(lam) - g where lam != 0, y = -g elsewhere), which is asserted."""
    N = cfg.N
    g = O.constraints(cfg, x0, cl, U)
    lam = np.asarray(lam, dtype=np.float64)
    y = np.where(lam != 0.0, lam + hw * np.sign(lam) - g, -g)
    _, grad, yhat = psi_yhat_lane(O, cfg, cfgs, x0, cl, U, row, y, np.ones(g.size))
    assert np.abs(yhat - lam).max() <= 1e-12 * max(1.0, np.abs(lam).max())
    lb, ub = np.tile(u_lb, N), np.tile(u_ub, N)
    viol = np.maximum(np.abs(g) - hw, 0.0).max()
    return viol, np.abs(U - np.clip(U - grad, lb, ub)).max()


# ----------------------------------------------------------------------------- the scenes of the solve tests
SOURCE = dict(A=0.3, sigma=(0.15, 0.06))
# The height of the source's centre; the line is y = 0.5.  On unconstrained handles the kinematic sources sit 0.11 and 0.10
# beside the line: ON the path (0.53, 0.52) the problem has two local minima, one on either side of the source, and a start
# drawn in the whole input box took the reference round the far side for 3 of the 16 `standing` and 4 of the 16 `moving`
# agents (spread 0.64); from 0.07 further out every start of every shift reaches the same point.  The Pacejka scene
# (N = 12, a shorter horizon) has one minimum at 0.53.  In the LANE scenes (half-width 0.10) the kinematic source sits at 0.555: at 0.61 it pushes
# the car 0.066 aside, which the band never sees; at 0.53 a whole-box start again passes on the far side (1 of 4 shifts); at
# 0.555 the band is active (6 - 7 multipliers) and the three starts agree to 3.5e-6; from 0.565 on the band is idle.
SOURCE_Y = dict(standing=0.61, moving=0.60, pacejka=0.53)
SOURCE_Y_LANE = dict(standing=0.555, pacejka=0.53)
LANE_HW = 0.10
LANE_SHIFTS = 4


def scene_row(name, shift=(0.0, 0.0), lane=False):
    """(model, N, x0, row [N, NFIELD, NFSRC]) of the scenes `standing`, `moving`, `pacejka`: the discs of discs_common's
    scenes of those names turned into sources -- standing at x = 1.55, moving along the moving disc's path with alpha = 1,
    Pacejka at x = 1.35, at the heights SOURCE_Y (lane: SOURCE_Y_LANE) -- A = 0.3, sigma = (0.15, 0.06), the second slot A = 0"""
    model, N, x0, _ = D.SCENES[name]
    cy = (SOURCE_Y_LANE if lane else SOURCE_Y)[name]
    if name == "standing":
        row = source_rows(N, (1.55 + shift[0], cy + shift[1]), 0.0, SOURCE["A"], SOURCE["sigma"])
    elif name == "moving":
        k = np.arange(N)
        ce = np.stack([1.25 + 0.02 * (k + 1) + shift[0], np.full(N, cy + shift[1])], 1)
        row = source_rows(N, ce, 0.0, SOURCE["A"], SOURCE["sigma"], 1.0)
    else:
        row = source_rows(N, (1.35 + shift[0], cy + shift[1]), 0.0, SOURCE["A"], SOURCE["sigma"])
    return model, N, x0, row


def starts(N, b):
    """the three starts every reference solve is run from: U = 0, tile(1, 0), a random point of the whole input box"""
    rng = np.random.default_rng(1000 + b)
    return [np.zeros(2 * N), np.tile([1.0, 0.0], N), np.stack([rng.uniform(-1, 1, N), rng.uniform(-.32, .32, N)], 1).reshape(-1)]


def source_rows(N, centre, heading, A, sigma, alpha=0.0, second=None):
    """one row [N, NFIELD, NFSRC] with a source in slot 0 -- centre [2] (standing) or [N, 2] (moving) -- and slot 1 empty
    (A = 0) unless `second` = (centre, heading, A, sigma, alpha) fills it"""
    row = np.zeros((N, NFIELD, NFSRC))
    for j, src in enumerate(((centre, heading, A, sigma, alpha), second)):
        if src is None:
            continue
        ce, hd, Aj, sg, al = src
        row[:, j, 0:2] = np.asarray(ce, dtype=np.float64)
        row[:, j, 2], row[:, j, 3], row[:, j, 4] = np.cos(hd), np.sin(hd), Aj
        row[:, j, 5], row[:, j, 6], row[:, j, 7] = 1.0 / (2.0 * sg[0] ** 2), 1.0 / (2.0 * sg[1] ** 2), al
    return row


def random_rows(rng, P, N, x_range=(1.0, 5.0), y_range=(0.35, 0.65)):
    """P rows [P, N, NFIELD, NFSRC] for the evaluation tests: both slots live on most stages, rotated frames, alpha != 0,
    and about a fifth of the sources switched off (A = 0, the other seven words left as drawn: they must not be read).
    Wide enough along the frame (sigma_x 0.3 .. 0.8) that agents spread over x_range feel them; E >= -alpha^2 / (4 kx)
    >= -0.32."""
    tab = np.zeros((P, N, NFIELD, NFSRC))
    th = rng.uniform(-0.6, 0.6, (P, N, NFIELD))
    tab[..., 0] = rng.uniform(*x_range, (P, N, NFIELD))
    tab[..., 1] = rng.uniform(*y_range, (P, N, NFIELD))
    tab[..., 2], tab[..., 3] = np.cos(th), np.sin(th)
    tab[..., 4] = rng.uniform(0.05, 0.5, (P, N, NFIELD)) * (rng.uniform(0, 1, (P, N, NFIELD)) > 0.2)
    tab[..., 5] = 1.0 / (2.0 * rng.uniform(0.3, 0.8, (P, N, NFIELD)) ** 2)
    tab[..., 6] = 1.0 / (2.0 * rng.uniform(0.08, 0.25, (P, N, NFIELD)) ** 2)
    tab[..., 7] = rng.uniform(-1.0, 1.0, (P, N, NFIELD))
    return tab


def gather(X, opp, shape):
    """the rule of mpc_fields_from_plans in numpy: table [B, N, NFIELD, NFSRC] from X [B, N, nx], opp [B, NFIELD],
    shape [B, 4] = [A, kx, ky, gain]; (c, s) by numpy's cos and sin"""
    B, N = X.shape[0], X.shape[1]
    tab = np.zeros((B, N, NFIELD, NFSRC))
    for b in range(B):
        for j in range(NFIELD):
            o = int(opp[b, j])
            if o < 0 or o >= B:
                continue
            tab[b, :, j, 0] = X[o, :, 0]
            tab[b, :, j, 1] = X[o, :, 1]
            tab[b, :, j, 2] = np.cos(X[o, :, 2])
            tab[b, :, j, 3] = np.sin(X[o, :, 2])
            tab[b, :, j, 4:7] = shape[o, 0:3]
            tab[b, :, j, 7] = shape[o, 3] * (X[b, :, 3] - X[o, :, 3])
    return tab


# ----------------------------------------------------------------------------- the traffic scene and the mirror loop
TRAFFIC_N = 20
TRAFFIC_X0 = np.array([[1.0, 0.5, 0.0, 1.0], [1.35, 0.58, 0.0, 0.4], [3.5, 0.5, 0.0, 0.5]])   # the slow car beside the line
TRAFFIC_VREF = np.array([1.0, 0.4, 0.5])
TRAFFIC_RADIUS = 0.14
TRAFFIC_REACH = 0.5
TRAFFIC_SHAPE = np.array([SOURCE["A"], 1.0 / (2.0 * SOURCE["sigma"][0] ** 2), 1.0 / (2.0 * SOURCE["sigma"][1] ** 2), 0.2])
TRAFFIC_T = 14
TRAFFIC_SCENES = 2


def traffic_scenes(nscenes=TRAFFIC_SCENES):
    """(X0 [3 nscenes, 4], v_ref, radius, shape [3 nscenes, 4]): three cars on the line y = 0.5 -- the rear one at v_ref = 1
    closes on a slow one 0.35 ahead and 0.08 beside the line, a third is far ahead --, scene s moved as a whole by
    discs_common.scene_shifts()[s]"""
    sh = D.scene_shifts()
    X0 = np.concatenate([TRAFFIC_X0 + np.array([sh[s][0], sh[s][1], 0.0, 0.0]) for s in range(nscenes)])
    B = 3 * nscenes
    return X0, np.tile(TRAFFIC_VREF, nscenes), np.full(B, TRAFFIC_RADIUS), np.tile(TRAFFIC_SHAPE, (B, 1))


def mirror_loop(O, N, X0, v_ref, radius, shape, reach, G, T, cl, shift=True, log=None):
    """The steps of mpc_closed_loop_traffic_field on the CPU checker (kinematic model, unconstrained handle, U0 = 0): the
    oracle's rollout, the selection restated in traffic_common, the numpy gather, reference_solve from the plan the step
    before left (the warm start the library has too), the plant step x <- x_1 of the solved plan, the shift, the realised
    clearance.  Returns traj_x [B, T, nx], traj_u [B, T, 2], traj_opp [B, T, NFIELD], traj_clear [B, T], margin [T] (the
    selection margin of every step)."""
    import traffic_common as TC
    X0 = np.asarray(X0, dtype=np.float64)
    B, nx = X0.shape
    cfg = [O.default_config(0, N, constr_mode=O.CONSTR_NONE, v_ref=float(v_ref[b])) for b in range(B)]
    cfgs = [machine(O, 0, N, v_ref=float(v_ref[b])) for b in range(B)]
    x, U = X0.copy(), np.zeros((B, 2 * N))
    out = dict(traj_x=np.zeros((B, T, nx)), traj_u=np.zeros((B, T, 2)), traj_opp=np.zeros((B, T, NFIELD), dtype=np.int32),
               traj_clear=np.zeros((B, T)), margin=np.zeros(T))
    for t in range(T):
        X = np.stack([O.rollout(cfg[b], x[b], U[b]) for b in range(B)])
        opp, _, info = TC.select_opponents(X, G, radius, reach)
        tab = gather(X, opp, shape)
        for b in range(B):
            U[b] = reference_solve(O, cfg[b], cfgs[b], x[b], cl, tab[b], U0=U[b])
        out["traj_u"][:, t] = U[:, :2]
        x = np.stack([O.rollout(cfg[b], x[b], U[b])[0] for b in range(B)])
        if shift:
            U[:, :-2] = U[:, 2:].copy()
        out["traj_x"][:, t], out["traj_opp"][:, t], out["margin"][t] = x, opp, info["margin"]
        out["traj_clear"][:, t] = TC.select_opponents(x, G, radius)[1][:, 0]
        if log:
            log(f"step {t}: margin {info['margin']:.3e}, min clear {out['traj_clear'][:, t].min():.6f}, x {np.round(x[:3, 0], 3).tolist()}, "
                f"y {np.round(x[:3, 1], 3).tolist()}, opp {opp.reshape(-1).tolist()}")
    return out
