"""The event-triggered closed loop restated in numpy on the CPU oracle (shared by tests/test_event_loop_cpu.py and
tests/test_gpu_event_loop.py): the trigger of include/mpc_hip.h (mpc_trigger_eval) and the five steps of
mpc_closed_loop_event, one agent at a time, with the oracle's solve and the oracle's f_d."""
import numpy as np

from conftest import straight_centerline, synthetic_states

TWO_PI = 2.0 * np.pi

# the configuration both suites check: kinematic model, N = 20, 16 agents on the straight centerline, solves converged
# to eps = 1e-10; the plant accelerates 3 % less and has 10 % more friction than the controller's model
N, B, T, MAX_HOLD, SHIFT = 20, 16, 40, 10, 1
SOLVER = dict(alm_eps=1e-10, max_total_inner=4000)
PLANT = dict(accel=2.0 * 0.97, friction=1.0 * 1.1)
THRESHOLDS = (0.01, 0.03)


def case():
    """(X0 [B, 4], centerline, U0 [B, 2N], w [4])"""
    return synthetic_states(0, B, seed=1), straight_centerline(), np.tile([1.0, 0.0], (B, N)), np.ones(4)


def trigger(x, xhat, held, w, thr, max_hold):
    """(dev2, fire) of one agent, every operation an IEEE double operation in the header's order"""
    e = x - xhat
    e[2] = e[2] - TWO_PI * np.rint(e[2] / TWO_PI)
    d2 = 0.0
    for i in range(len(x)):
        d2 = d2 + w[i] * (e[i] * e[i])
    return d2, bool(held < 0 or held >= max_hold or not d2 < thr * thr)


def shift_plan(U, held):
    """`held` applications of the one-stage shift: the last stage is repeated into the tail"""
    n = U.shape[0] // 2
    S = U.reshape(n, 2)
    return S[np.minimum(np.arange(n) + held, n - 1)].ravel()


def mirror_loop(O, ccfg, pcfg, X0, cl, U0, w, thr, max_hold, shift, T, disturbance=None):
    """Returns a dict: solved [B, T] bool, traj_x [B, T, nx], traj_u [B, T, 2], held [B], fails [B], U [B, 2N] and
    margin = min over all decisions taken on dev2 of |dev2 - thr^2| / thr^2 (how close a decision came to flipping)."""
    nB, nx = X0.shape
    x, xhat, U = X0.copy(), np.zeros_like(X0), U0.copy()
    held = np.full(nB, -1)
    solved = np.zeros((nB, T), bool)
    tx, tu = np.zeros((nB, T, nx)), np.zeros((nB, T, 2))
    fails = np.zeros(nB, int)
    margin = np.inf
    for t in range(T):
        fire = np.zeros(nB, bool)
        for b in range(nB):
            d2, fire[b] = trigger(x[b], xhat[b], held[b], w, thr, max_hold)
            if 0 <= held[b] < max_hold and np.isfinite(thr) and thr > 0:
                margin = min(margin, abs(d2 - thr * thr) / (thr * thr))
            if fire[b] and shift and held[b] > 0:
                U[b] = shift_plan(U[b], held[b])
        idx = np.flatnonzero(fire)
        if idx.size:
            Us, _, st = O.solve_batch(ccfg, x[idx], cl, U[idx])
            U[idx] = Us
            fails[idx] += st[:, 0] != 1
            held[idx] = 0
            xhat[idx] = x[idx]
        solved[:, t] = fire
        for b in range(nB):
            u = U[b, 2 * held[b]:2 * held[b] + 2].copy()
            x[b] = O.fd(pcfg, x[b], u)
            if disturbance is not None:
                x[b] = x[b] + disturbance[b, t]
            xhat[b] = O.fd(ccfg, xhat[b], u)
            held[b] += 1
            tx[b, t], tu[b, t] = x[b], u
    return dict(solved=solved, traj_x=tx, traj_u=tu, held=held, fails=fails, U=U, x=x, margin=margin)
