"""Lap driving restated in numpy on the CPU oracle (shared by tests/test_track_loop_cpu.py and
tests/test_gpu_track_loop.py), on top of event_loop_common: the windows of a track, the select rule and the first
placement of include/mpc_hip.h (mpc_track_windows, mpc_track_select, mpc_track_locate) and the loop of
mpc_closed_loop_track, one agent at a time, with the oracle's nearest point, the oracle's solve and the oracle's f_d."""
import collections

import numpy as np

import event_loop_common as E

Geom = collections.namedtuple("Geom", "K L S stride lead closed R")


def geom(K, L, S, stride, lead, closed):
    """the header's counts: closed R = ceil(L / w), open R = (L - S) / w + 1"""
    assert K >= 1 and L >= S and stride >= 1 and 0 <= lead <= S - 2
    R = -(-L // stride) if closed else (L - S) // stride + 1
    return Geom(K, L, S, stride, lead, bool(closed), R)


def windows(track, g):
    """win [K * R, 2S] from track [K, 2L]: window r of track k holds points r*w + i, i < S (mod L when closed)"""
    track = np.asarray(track, dtype=np.float64).reshape(g.K, 2 * g.L)
    p = np.arange(g.R)[:, None] * g.stride + np.arange(g.S)[None, :]
    if g.closed:
        p = p % g.L
    assert p.max() < g.L
    win = np.concatenate([track[:, p], track[:, g.L + p]], axis=2)        # [K, R, 2S]
    return np.ascontiguousarray(win.reshape(g.K * g.R, 2 * g.S))


def new_window(g, along):
    """the rule, on Python integers (// floors towards minus infinity, % is non-negative)"""
    p = int(along) - g.lead
    if g.closed:
        return (p % g.L) // g.stride
    return min(max(p // g.stride, 0), g.R - 1)


def select(O, cfg, x, win, rows, g, active=None, gaps=None):
    """(rows', pos) of mpc_track_select: the oracle's nearest index on each agent's current row, then the rule.
    pos = -1 and the row kept for agents that are masked out or whose pose is not finite.  gaps (a list): receives the
    relative gap between the two smallest squared distances of every selection made."""
    rows = np.array(rows, dtype=np.int64)
    pos = np.full(len(rows), -1, dtype=np.int64)
    for b in range(len(rows)):
        if (active is not None and not active[b]) or not np.isfinite(x[b, :2]).all():
            continue
        k, r = divmod(int(rows[b]), g.R)
        i = O.nearest(cfg, x[b, :2], win[rows[b]])
        if gaps is not None:
            d = np.sort((win[rows[b], :g.S - 1] - x[b, 0]) ** 2 + (win[rows[b], g.S:2 * g.S - 1] - x[b, 1]) ** 2)
            gaps.append((d[1] - d[0]) / d[1] if d[1] > 0 else 0.0)
        along = r * g.stride + i
        rows[b] = k * g.R + new_window(g, along)
        pos[b] = along % g.L if g.closed else along
    return rows, pos


def locate(O, cfgL, x, track, g, track_index=None):
    """mpc_track_locate: the oracle's nearest with S = L on the agent's whole track row, then the rule (cfgL: an oracle
    configuration whose S is L)"""
    assert cfgL.S == g.L
    track = np.asarray(track, dtype=np.float64).reshape(g.K, 2 * g.L)
    rows = np.zeros(len(x), dtype=np.int64)
    for b in range(len(x)):
        k = 0 if track_index is None else int(track_index[b])
        rows[b] = k * g.R + new_window(g, O.nearest(cfgL, x[b, :2], track[k]))
    return rows


def mirror_loop(O, ccfg, pcfg, X0, win, g, rows0, U0, w, thr, max_hold, shift, T, disturbance=None):
    """event_loop_common.mirror_loop with the select step between the trigger and the solve.  Returns its dict plus
    rows [B], traj_row [B, T], row_changes, seam_crossings (selections that moved an agent from the last windows of a
    closed track to the first) and gap = the smallest relative gap between the two nearest squared distances at any selection."""
    nB, nx = X0.shape
    x, xhat, U = X0.copy(), np.zeros_like(X0), U0.copy()
    rows = np.array(rows0, dtype=np.int64)
    held = np.full(nB, -1)
    solved = np.zeros((nB, T), bool)
    tx, tu = np.zeros((nB, T, nx)), np.zeros((nB, T, 2))
    trow = np.zeros((nB, T), dtype=np.int64)
    fails = np.zeros(nB, int)
    margin, gaps, changes, seams = np.inf, [], 0, 0
    for t in range(T):
        fire = np.zeros(nB, bool)
        for b in range(nB):
            d2, fire[b] = E.trigger(x[b], xhat[b], held[b], w, thr, max_hold)
            if 0 <= held[b] < max_hold and np.isfinite(thr) and thr > 0:
                margin = min(margin, abs(d2 - thr * thr) / (thr * thr))
            if fire[b] and shift and held[b] > 0:
                U[b] = E.shift_plan(U[b], held[b])
        new_rows, pos = select(O, ccfg, x, win, rows, g, active=fire, gaps=gaps)
        changes += int((new_rows != rows).sum())
        if g.closed:
            seams += int((new_rows % g.R < rows % g.R - g.R // 2).sum())
        rows = new_rows
        trow[:, t] = rows
        idx = np.flatnonzero(fire)
        if idx.size:
            Us, _, st = O.solve_batch(ccfg, x[idx], win, U[idx], cl_index=rows[idx])
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
    return dict(solved=solved, traj_x=tx, traj_u=tu, held=held, fails=fails, U=U, x=x, margin=margin, rows=rows,
                traj_row=trow, row_changes=changes, seam_crossings=seams, gap=min(gaps) if gaps else np.inf)


# ----------------------------------------------------------------------------- the seam case (both suites)
SEAM = dict(straight=10, radius=3, ds=0.1, L=388, stride=4, lead=10, R=97, B=16, T=40, max_hold=10, shift=1)
SEAM_MODELS = ((0, 20), (1, 12))           # (model, N): kinematic N = 20, Pacejka N = 12
SEAM_THRESHOLDS = (0.0, 0.02)


def seam_case(model, N):
    """(X0 [16, nx], track [2L], U0, w, Geom) of the oracle mirror across the seam: default_rng(1) draws x ~ U(-3, -0.2),
    y, phi ~ U(-.3, .3), v ~ U(.3, 1.5) and on the Pacejka model vy ~ U(-.05, .05), omega ~ U(-.5, .5), in that order"""
    from model_predictive_control_amd.tracks import stadium_track
    track = stadium_track(SEAM["straight"], SEAM["radius"], SEAM["ds"])
    assert track.shape == (2 * SEAM["L"],)
    B = SEAM["B"]
    rng = np.random.default_rng(1)
    cols = [rng.uniform(-3, -0.2, B), rng.uniform(-.3, .3, B), rng.uniform(-.3, .3, B), rng.uniform(.3, 1.5, B)]
    if model == 1:
        cols += [rng.uniform(-.05, .05, B), rng.uniform(-.5, .5, B)]
    X0 = np.stack(cols, 1)
    g = geom(1, SEAM["L"], 100, SEAM["stride"], SEAM["lead"], True)
    assert g.R == SEAM["R"]
    return X0, track, np.tile([1.0, 0.0], (B, N)), np.ones(X0.shape[1]), g


def seam_mirror(O, model, N, thr, jitter=None):
    """the oracle's run of the seam case (under eval_jitter(*jitter) when given)"""
    X0, track, U0, w, g = seam_case(model, N)
    cc = O.default_config(model, N, **E.SOLVER)
    win = windows(track, g)
    rows0 = locate(O, O.default_config(model, N, S=g.L), X0, track, g)

    def run():
        return mirror_loop(O, cc, cc, X0, win, g, rows0, U0, w, thr, SEAM["max_hold"], SEAM["shift"], SEAM["T"])
    if jitter is None:
        return run()
    with O.eval_jitter(*jitter):
        return run()
