"""The checker of the keep-out discs (constr_mode CONSTR_DISCS): a numpy restatement built from the frozen oracle's calls,
which does not know discs.  Shared by tests/test_agent_discs_cpu.py and tests/test_gpu_agent_discs.py.

  f        O.psi with CONSTR_NONE; the states x_1 .. x_N from O.rollout
  g        g[2k + j] = (dx dx + dy dy) - r r,  dx = x_{k+1} - cx, dy = y_{k+1} - cy, disc j of stage k; D = [0, +inf)
  zeta     g + y / Sigma;  yhat = Sigma min(zeta, 0);  psi = f + 1/2 sum Sigma min(zeta, 0)^2
  grad     exactly, without finite differences: the oracle's STATE_SQ mode is a VJP machine.  With g_off = 0,
           D_lb = D_ub = 0 and Sigma = 1 its yhat is g_sq + y, so y = t - g_sq (g_sq from O.constraints) makes O.psi return
           grad f + sum_k J_k' (2 x_{k,i} t_{k,i})_i; t_{k,0} = w_{k,x} / (2 x_k), t_{k,1} = w_{k,y} / (2 y_k) with
           w_k = sum_j yhat_{k,j} 2 (dx, dy) gives the disc gradient.  Positions must stay away from 0.
  solve    an ALM loop (Sigma0 = 10, x 10 per outer iteration, y <- yhat, until ||e||_inf < 1e-8) around scipy's L-BFGS-B
           with the box, gtol 1e-10, the exact gradient, start U = 0; every inner solve finished by projected Newton steps
           (newton_polish), because L-BFGS-B alone stalls above its gtol once the penalty is large.
Configuration overrides (`common`: Ts, veh, cost_w, ...) go into both oracle configurations."""
import numpy as np

NDISC = 2


def configs(O, model, N, **common):
    """(the unconstrained configuration, the STATE_SQ one that serves as the VJP machine)"""
    c0 = O.default_config(model, N, constr_mode=O.CONSTR_NONE, **common)
    c1 = O.default_config(model, N, constr_mode=O.CONSTR_STATE_SQ, g_off=[0.0] * 6, D_lb=[0.0] * 6, D_ub=[0.0] * 6, **common)
    return c0, c1


def disc_g(X, discs):
    """g [2N] of the end-of-stage states X [N, nx] and the row discs [N, NDISC, 3]; (dx, dy) [N, NDISC] with it"""
    discs = np.asarray(discs, dtype=np.float64).reshape(X.shape[0], NDISC, 3)
    dx = X[:, None, 0] - discs[:, :, 0]
    dy = X[:, None, 1] - discs[:, :, 1]
    r = discs[:, :, 2]
    return ((dx * dx + dy * dy) - r * r).reshape(-1), dx, dy


def psi_yhat(O, cfgs, x0, cl, U, discs, y, Sigma, want_grad=True):
    """(psi, yhat [2N], grad [2N] or None, g [2N]) of one agent"""
    c0, c1 = cfgs
    N = c0.N
    X = O.rollout(c0, x0, U)
    g, dx, dy = disc_g(X, discs)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Sigma = np.asarray(Sigma, dtype=np.float64).reshape(-1)
    zeta = g + y / Sigma
    d = np.minimum(zeta, 0.0)
    yhat = Sigma * d
    f, _ = O.psi(c0, x0, cl, U, want_grad=False)
    psi = f + 0.5 * np.sum(Sigma * d * d)
    if not want_grad:
        return psi, yhat, None, g
    yh = yhat.reshape(N, NDISC)
    wx = np.sum(yh * 2.0 * dx, 1)
    wy = np.sum(yh * 2.0 * dy, 1)
    nx = X.shape[1]
    t = np.zeros((N, nx))
    t[:, 0] = wx / (2.0 * X[:, 0])
    t[:, 1] = wy / (2.0 * X[:, 1])
    g_sq = O.constraints(c1, x0, cl, U)
    _, grad = O.psi(c1, x0, cl, U, t.reshape(-1) - g_sq, np.ones(N * nx))
    # O.psi added 1/2 |t|^2 to f: only its gradient is used
    return psi, yhat, grad, g


def psi_fd_grad(O, cfgs, x0, cl, U, discs, y, Sigma, h=1e-6):
    """central differences of the numpy psi"""
    U = np.asarray(U, dtype=np.float64)
    out = np.empty(U.size)
    for i in range(U.size):
        e = np.zeros(U.size); e[i] = h
        out[i] = (psi_yhat(O, cfgs, x0, cl, U + e, discs, y, Sigma, False)[0] -
                  psi_yhat(O, cfgs, x0, cl, U - e, discs, y, Sigma, False)[0]) / (2 * h)
    return out


def newton_polish(grad, U, lb, ub, gtol, max_steps=12, h=1e-6):
    """Projected Newton steps from U towards a point whose projected gradient || U - clip(U - grad(U)) ||_inf is below gtol:
    the Hessian by central differences of the exact gradient, on the variables that are not held at a bound by the
    gradient's sign (psi is C1 with a piecewise smooth gradient: a semismooth Newton step, taken only while it lowers the
    projected gradient).  Returns the best point met."""
    def pgn(u, g):
        return np.abs(u - np.clip(u - g, lb, ub)).max()
    g = grad(U)
    best = pgn(U, g)
    for _ in range(max_steps):
        if best <= gtol:
            break
        free = ~(((U <= lb) & (g > 0)) | ((U >= ub) & (g < 0)))
        idx = np.flatnonzero(free)
        H = np.empty((idx.size, idx.size))
        for c, i in enumerate(idx):
            e = np.zeros(U.size); e[i] = h
            H[:, c] = (grad(U + e)[idx] - grad(U - e)[idx]) / (2 * h)
        step = np.zeros(U.size)
        step[idx] = np.linalg.solve(0.5 * (H + H.T), -g[idx])
        t, better = 1.0, False
        while t >= 1.0 / 64:
            Un = np.clip(U + t * step, lb, ub)
            gn = grad(Un)
            if pgn(Un, gn) < best:
                U, g, best, better = Un, gn, pgn(Un, gn), True
                break
            t /= 2
        if not better:
            break
    return U


def reference_solve(O, cfgs, x0, cl, discs, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32), Sigma0=10.0, tol=1e-8, max_outer=12):
    """(U, lambda, outer iterations) of the ALM loop around L-BFGS-B"""
    from scipy.optimize import minimize
    N = cfgs[0].N
    bounds = [(u_lb[i % 2], u_ub[i % 2]) for i in range(2 * N)]
    lb_, ub_ = np.tile(u_lb, N), np.tile(u_ub, N)
    U = np.zeros(2 * N)
    y = np.zeros(NDISC * N)
    Sigma = np.full(NDISC * N, float(Sigma0))
    for outer in range(1, max_outer + 1):
        def fun(u):
            p, _, gr, _ = psi_yhat(O, cfgs, x0, cl, u, discs, y, Sigma)
            return p, gr
        # L-BFGS-B gives up on its line search before gtol where the penalty makes psi stiff (it stalls at a projected
        # gradient of 1e-7 .. 1e-6, which leaves the controls 1e-5 off): it is started again from where it stopped (a fresh
        # memory) while that helps, and the point is then finished by projected Newton steps on the exact gradient
        for _ in range(20):
            res = minimize(fun, U, jac=True, method="L-BFGS-B", bounds=bounds,
                           options=dict(gtol=1e-10, ftol=0.0, maxiter=2000, maxfun=20000, maxcor=20, maxls=40))
            moved = np.abs(res.x - U).max()
            U = res.x
            pg = np.abs(U - np.clip(U - res.jac, lb_, ub_)).max()
            if pg <= 1e-10 or moved == 0.0:
                break
        U = newton_polish(lambda u: fun(u)[1], U, lb_, ub_, 1e-10)
        _, yhat, _, _ = psi_yhat(O, cfgs, x0, cl, U, discs, y, Sigma, False)
        e = (yhat - y) / Sigma
        y = yhat
        if np.abs(e).max() < tol:
            return U, y, outer
        Sigma = Sigma * 10.0
    raise AssertionError("the reference solve did not reach ||e|| < %g in %d outer iterations" % (tol, max_outer))


def lagrangian_residual(O, cfgs, x0, cl, U, discs, lam, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """|| U - proj_C(U - grad (f + lam' g)(U)) ||_inf, the projected-gradient residual of the Lagrangian at U: the VJP
    machine of psi_yhat, fed the multipliers where psi_yhat feeds it yhat."""
    c0, c1 = cfgs
    N = c0.N
    X = O.rollout(c0, x0, U)
    _, dx, dy = disc_g(X, discs)
    lm = np.asarray(lam, dtype=np.float64).reshape(N, NDISC)
    nx = X.shape[1]
    t = np.zeros((N, nx))
    t[:, 0] = np.sum(lm * 2.0 * dx, 1) / (2.0 * X[:, 0])
    t[:, 1] = np.sum(lm * 2.0 * dy, 1) / (2.0 * X[:, 1])
    g_sq = O.constraints(c1, x0, cl, U)
    _, grad = O.psi(c1, x0, cl, U, t.reshape(-1) - g_sq, np.ones(N * nx))
    lb = np.tile(u_lb, N); ub = np.tile(u_ub, N)
    return np.abs(U - np.clip(U - grad, lb, ub)).max()


# ----------------------------------------------------------------------------- the scenes of the solve tests
def line_centerline(y=0.5, S=100, x_start=0.9):
    """a straight centerline at height y (flat: x's then y's) that starts at x_start: positions stay away from 0"""
    return np.concatenate([x_start + 0.1 * np.arange(S), np.full(S, float(y))])


X0_KIN = np.array([1.0, 0.5, 0.0, 0.8])
X0_PAC = np.array([1.0, 0.5, 0.0, 0.8, 0.0, 0.0])


def scene_standing(N=20, shift=(0.0, 0.0)):
    """a standing disc (1.55, 0.53, 0.12) on every stage, the second slot empty"""
    d = np.zeros((N, NDISC, 3))
    d[:, 0] = (1.55 + shift[0], 0.53 + shift[1], 0.12)
    return d


def scene_moving(N=20, shift=(0.0, 0.0)):
    """a disc moving ahead at 0.4 m/s plus a standing one"""
    d = np.zeros((N, NDISC, 3))
    k = np.arange(N)
    d[:, 0, 0] = 1.25 + 0.02 * (k + 1) + shift[0]
    d[:, 0, 1] = 0.52 + shift[1]
    d[:, 0, 2] = 0.1
    d[:, 1] = (1.7 + shift[0], 0.38 + shift[1], 0.08)
    return d


def scene_pacejka(N=12, shift=(0.0, 0.0)):
    d = np.zeros((N, NDISC, 3))
    d[:, 0] = (1.35 + shift[0], 0.53 + shift[1], 0.1)
    return d


# name -> (model, N, x0, scene); every scene on line_centerline() from x0
SCENES = {"standing": (0, 20, X0_KIN, scene_standing), "moving": (0, 20, X0_KIN, scene_moving),
          "pacejka": (1, 12, X0_PAC, scene_pacejka)}
NSHIFT = 16


def scene_shifts():
    """the NSHIFT small shifts (dx, dy) of a scene's discs that the agents of the solve test cycle through (shift 0: none):
    small enough that every agent passes on the side the unshifted scene picks"""
    rng = np.random.default_rng(23)
    s = np.stack([rng.uniform(-0.02, 0.02, NSHIFT), rng.uniform(-0.005, 0.005, NSHIFT)], 1)
    s[0] = 0.0
    return s
