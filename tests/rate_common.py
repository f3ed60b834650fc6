"""The checker of the input-rate cost (mpc_set_agent_rates): a numpy restatement on top of the frozen oracle, which does
not know the term.  Shared by tests/test_agent_rates_cpu.py and tests/test_gpu_agent_rates.py.

  row      [w_d, w_delta, d_prev, delta_prev]; u_{-1} = (d_prev, delta_prev)
  term     sum_k  w_d e_k[0]^2 + w_delta e_k[1]^2,   e_k = u_k - u_{k-1}
  grad     d term / d u_k = 2 w o e_k - 2 w o e_{k+1}   (the second part absent at k = N - 1)
  psi      O.psi (any constr_mode of the oracle's, with y and Sigma) -- or discs_common.psi_yhat on a disc handle -- plus
           the term; the gradient likewise.  The term is on the decision variables as they are: no clipping.
  solve    m = 0: scipy's L-BFGS-B with the box, restarted while it moves, finished by discs_common.newton_polish;
           discs: the ALM loop of discs_common.reference_solve around the extended psi.
"""
import numpy as np

import discs_common as D

NRATE = 4


def rate_term(U, row, want_grad=True):
    """(term, its gradient [2N] or None) of the controls U [2N] and the table row [4]"""
    u = np.asarray(U, dtype=np.float64).reshape(-1, 2)
    row = np.asarray(row, dtype=np.float64)
    w, prev = row[:2], row[2:]
    e = u - np.vstack([prev[None, :], u[:-1]])
    term = float(np.sum(w[None, :] * e * e))
    if not want_grad:
        return term, None
    g = 2.0 * w[None, :] * e
    g[:-1] -= 2.0 * w[None, :] * e[1:]
    return term, g.reshape(-1)


def psi(O, cfg, x0, cl, U, row, y=None, Sigma=None, want_grad=True):
    """(psi, grad or None) on an oracle configuration of any of its constraint modes"""
    p, g = O.psi(cfg, x0, cl, U, y, Sigma, want_grad=want_grad)
    t, tg = rate_term(U, row, want_grad)
    return p + t, (g + tg if want_grad else None)


def psi_discs(O, cfgs, x0, cl, U, discs, y, Sigma, row, want_grad=True):
    """(psi, yhat, grad or None, g) on a disc handle: discs_common.psi_yhat plus the term"""
    p, yh, g, gv = D.psi_yhat(O, cfgs, x0, cl, U, discs, y, Sigma, want_grad)
    t, tg = rate_term(U, row, want_grad)
    return p + t, yh, (g + tg if want_grad else None), gv


def psi_fd_grad(O, cfg, x0, cl, U, row, y=None, Sigma=None, h=1e-6):
    """central differences of the numpy psi"""
    U = np.asarray(U, dtype=np.float64)
    out = np.empty(U.size)
    for i in range(U.size):
        e = np.zeros(U.size); e[i] = h
        out[i] = (psi(O, cfg, x0, cl, U + e, row, y, Sigma, False)[0] - psi(O, cfg, x0, cl, U - e, row, y, Sigma, False)[0]) / (2 * h)
    return out


def _inner(fun, U, lb_, ub_, bounds):
    """L-BFGS-B from U, started again from where it stopped while that moves the point, then projected Newton steps"""
    from scipy.optimize import minimize
    for _ in range(20):
        res = minimize(fun, U, jac=True, method="L-BFGS-B", bounds=bounds,
                       options=dict(gtol=1e-10, ftol=0.0, maxiter=2000, maxfun=20000, maxcor=20, maxls=40))
        moved = np.abs(res.x - U).max()
        U = res.x
        pg = np.abs(U - np.clip(U - res.jac, lb_, ub_)).max()
        if pg <= 1e-10 or moved == 0.0:
            break
    return D.newton_polish(lambda u: fun(u)[1], U, lb_, ub_, 1e-10)


def reference_solve(O, cfg, x0, cl, row, U0=None, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """U of the unconstrained problem (m = 0) with the move penalty of `row`"""
    N = cfg.N
    bounds = [(u_lb[i % 2], u_ub[i % 2]) for i in range(2 * N)]
    lb_, ub_ = np.tile(u_lb, N), np.tile(u_ub, N)
    U = np.zeros(2 * N) if U0 is None else np.asarray(U0, dtype=np.float64).copy()
    return _inner(lambda u: psi(O, cfg, x0, cl, u, row), U, lb_, ub_, bounds)


def reference_solve_discs(O, cfgs, x0, cl, discs, row, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32), Sigma0=10.0, tol=1e-8, max_outer=12):
    """(U, lambda, outer iterations): the ALM loop of discs_common.reference_solve around the extended psi"""
    N = cfgs[0].N
    bounds = [(u_lb[i % 2], u_ub[i % 2]) for i in range(2 * N)]
    lb_, ub_ = np.tile(u_lb, N), np.tile(u_ub, N)
    U = np.zeros(2 * N)
    y = np.zeros(D.NDISC * N)
    Sigma = np.full(D.NDISC * N, float(Sigma0))
    for outer in range(1, max_outer + 1):
        def fun(u):
            p, _, gr, _ = psi_discs(O, cfgs, x0, cl, u, discs, y, Sigma, row)
            return p, gr
        U = _inner(fun, U, lb_, ub_, bounds)
        _, yhat, _, _ = psi_discs(O, cfgs, x0, cl, U, discs, y, Sigma, row, False)
        e = (yhat - y) / Sigma
        y = yhat
        if np.abs(e).max() < tol:
            return U, y, outer
        Sigma = Sigma * 10.0
    raise AssertionError("the reference solve did not reach ||e|| < %g in %d outer iterations" % (tol, max_outer))


# ----------------------------------------------------------------------------- the scene of the solve tests
X0_KIN = np.array([1.0, 0.62, 0.0, 0.5])
X0_PAC = np.array([1.0, 0.62, 0.0, 0.5, 0.0, 0.0])
WEIGHTS = ((0.1, 1.0), (0.5, 5.0))
NAGENT = 16


def scene_agents(model):
    """(X0 [16, nx], u_prev [16, 2]): the car 0.12 beside the line y = 0.5 of discs_common.line_centerline, agent 0 exactly
    there with u_prev = 0, the others shifted a little sideways with u_prev drawn in the box"""
    rng = np.random.default_rng(41)
    X0 = np.tile(X0_PAC if model else X0_KIN, (NAGENT, 1))
    X0[1:, 1] += rng.uniform(-0.02, 0.02, NAGENT - 1)
    up = np.stack([rng.uniform(-1.0, 1.0, NAGENT), rng.uniform(-0.32, 0.32, NAGENT)], 1)
    up[0] = 0.0
    return X0, up


def disc_scene_agents():
    """(X0 [16, 4], discs [16, N, NDISC, 3], u_prev [16, 2]): the moving-disc scene of discs_common with its NSHIFT small
    shifts, agent 0 unshifted with u_prev = 0, the others with u_prev drawn in the box -- the drive in all of it, the
    steering in its lower half [-0.32, 0].  Why the half: the scene has more than one way round its two discs (between
    them, below both, above both), and the steering last applied decides which one a plan takes -- drawn in the whole
    box, the REFERENCE solves of the 16 agents took two (weights (0.1, 1.0)) and three ((0.5, 5.0)) different routes, the
    ones with delta_prev >= 0.08 leaving agent 0's.  Two correct solvers are only comparable to 1e-5 where the route is
    not in question (discs_common.scene_shifts keeps its shifts small for the same reason): with delta_prev <= 0 every
    reference solve passes between the discs as agent 0's does (route(), asserted where the reference is used)."""
    model, N, x0, scene = D.SCENES["moving"]
    shifts = D.scene_shifts()
    rng = np.random.default_rng(42)
    up = np.stack([rng.uniform(-1.0, 1.0, NAGENT), rng.uniform(-0.32, 0.0, NAGENT)], 1)
    up[0] = 0.0
    return np.tile(x0, (NAGENT, 1)), np.stack([scene(N, shifts[p]) for p in range(NAGENT)]), up


def route(O, cfg0, x0, U, discs):
    """on which side the plan U passes each disc: the sign of y - cy at the stage of the closest approach, per disc"""
    X = O.rollout(cfg0, x0, U)
    discs = np.asarray(discs).reshape(X.shape[0], D.NDISC, 3)
    out = []
    for j in range(D.NDISC):
        d2 = (X[:, 0] - discs[:, j, 0]) ** 2 + (X[:, 1] - discs[:, j, 1]) ** 2
        k = int(d2.argmin())
        out.append(int(np.sign(X[k, 1] - discs[k, j, 1])))
    return tuple(out)


def lagrangian_residual(O, cfgs, x0, cl, U, discs, lam, row, u_lb=(-1.0, -0.32), u_ub=(1.0, 0.32)):
    """|| U - proj_C(U - grad (f + term + lam' g)(U)) ||_inf: discs_common.lagrangian_residual with the move penalty's
    gradient added -- the VJP machine fed the multipliers, plus rate_term"""
    c0, c1 = cfgs
    N = c0.N
    X = O.rollout(c0, x0, U)
    _, dx, dy = D.disc_g(X, discs)
    lm = np.asarray(lam, dtype=np.float64).reshape(N, D.NDISC)
    nx = X.shape[1]
    t = np.zeros((N, nx))
    t[:, 0] = np.sum(lm * 2.0 * dx, 1) / (2.0 * X[:, 0])
    t[:, 1] = np.sum(lm * 2.0 * dy, 1) / (2.0 * X[:, 1])
    g_sq = O.constraints(c1, x0, cl, U)
    _, grad = O.psi(c1, x0, cl, U, t.reshape(-1) - g_sq, np.ones(N * nx))
    grad = grad + rate_term(U, row)[1]
    lb = np.tile(u_lb, N); ub = np.tile(u_ub, N)
    return np.abs(U - np.clip(U - grad, lb, ub)).max()
