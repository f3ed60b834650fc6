"""The checker of the traffic selection and the traffic closed loop (mpc_opponents_from_plans, mpc_closed_loop_traffic):
the rule of include/mpc_hip.h restated in numpy with plain loops -- np.float64 scalars, the kernel's operation order, so
that the bits agree --, the generator of the selection cases, and the loop's six steps on the CPU checker of the discs
(tests/discs_common.py: the oracle's rollout, reference_solve).  Shared by tests/test_traffic_cpu.py,
tests/test_gpu_traffic_loop.py and tests/golden/make_traffic_golden.py."""
import numpy as np

import discs_common as D

NDISC = D.NDISC
SCENE_MAX = 64


# ----------------------------------------------------------------------------- the rule
def pair_clearance(X, b, o, r_o):
    """c(b, o) = min_k (dx dx + dy dy) - r_o r_o over the stages of X [B, Nst, nx], every operation rounded on its own;
    None when a g_k is not finite"""
    c = np.float64(np.inf)
    r2 = np.float64(r_o) * np.float64(r_o)
    for k in range(X.shape[1]):
        dx = X[b, k, 0] - X[o, k, 0]
        dy = X[b, k, 1] - X[o, k, 1]
        g = (dx * dx + dy * dy) - r2
        if not np.isfinite(g):
            return None
        if g < c:
            c = g
    return c


def candidates(X, G, radius, reach, b):
    """the candidates of agent b sorted in the order (c, o): [(c, o)], o global; and the number of pairs of b that a
    non-finite stage took out"""
    r2 = np.float64(reach) * np.float64(reach)
    s0 = (b // G) * G
    out, nonfinite = [], 0
    for o in range(s0, s0 + G):
        if o == b:
            continue
        c = pair_clearance(X, b, o, radius[o])
        if c is None:
            nonfinite += 1
        elif c < r2:
            out.append((float(c), o))
    out.sort()
    return out, nonfinite


def select_opponents(X, G, radius, reach=np.inf):
    """(opp [B, NDISC] int32, clear [B, NDISC], info) of X [B, Nst, nx] (or [B, nx]: one stage).  info counts what the
    selection had to decide: `ties` slots whose c equals the next candidate's (the index decided), `short` agents with
    fewer than NDISC candidates, `nonfinite` excluded pairs; `margin` is the smallest gap between the last selected c and
    the first rejected one, or from the nearer of the two to reach^2 (inf where nothing could flip)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[:, None, :]
    radius = np.asarray(radius, dtype=np.float64)
    B = X.shape[0]
    assert 1 <= G <= SCENE_MAX and B % G == 0 and X.shape[1] >= 1 and reach >= 0
    opp = np.full((B, NDISC), -1, dtype=np.int32)
    clear = np.full((B, NDISC), np.inf)
    info = dict(ties=0, short=0, nonfinite=0, margin=np.inf)
    r2 = float(np.float64(reach) * np.float64(reach))
    with np.errstate(all="ignore"):
        for b in range(B):
            cand, nf = candidates(X, G, radius, reach, b)
            info["nonfinite"] += nf
            info["short"] += len(cand) < NDISC
            for j, (c, o) in enumerate(cand[:NDISC]):
                opp[b, j], clear[b, j] = o, c
                info["ties"] += j + 1 < len(cand) and cand[j + 1][0] == c
            # what a small change of the states could flip: the order of the selected ones does not count, the boundary
            # between selected and rejected and the boundary at reach^2 do
            if len(cand) > NDISC:
                info["margin"] = min(info["margin"], cand[NDISC][0] - cand[NDISC - 1][0])
            if np.isfinite(r2):
                s0 = (b // G) * G
                for o in range(s0, s0 + G):
                    c = None if o == b else pair_clearance(X, b, o, radius[o])
                    if c is not None and (c >= r2 or len(cand) <= NDISC or (float(c), o) <= cand[NDISC - 1]):
                        info["margin"] = min(info["margin"], abs(float(c) - r2))
    return opp, clear, info


def gather_discs(X, opp, radius):
    """mpc_discs_from_plans in numpy: [B, N, NDISC, 3]"""
    B, N = X.shape[0], X.shape[1]
    d = np.zeros((B, N, NDISC, 3))
    for b in range(B):
        for j in range(NDISC):
            o = int(opp[b, j])
            if 0 <= o < B:
                d[b, :, j, 0], d[b, :, j, 1], d[b, :, j, 2] = X[o, :, 0], X[o, :, 1], radius[o]
    return d


# ----------------------------------------------------------------------------- the selection cases
SELECTION_SHAPES = ((1, 70), (2, 130), (3, 258), (17, 255), (64, 320))   # (G, B): scenes straddle waves and workgroups
SELECTION_STAGES = (1, 12, 20)
SELECTION_REACH = 2.5


def selection_case(nx, Nst, G, B, seed=0):
    """(X [B, Nst, nx], radius [B]): 60 % of the agents move on the integer grid with integer velocities (exact
    arithmetic: equal clearances abound), the others anywhere; in every scene of three or more, agent 1 is a copy of agent
    0 half of the time (exact ties along the whole plan); radii from {0, 0.3, 0.5, 1}; a few NaN and infinite positions"""
    rng = np.random.default_rng(1000 * seed + 100 * nx + 7 * Nst + G)
    X = rng.normal(size=(B, Nst, nx))
    p0 = rng.integers(0, 6, (B, 2)).astype(np.float64)
    v = np.array([(0, 0), (1, 0), (0, 1), (1, 1)], dtype=np.float64)[rng.integers(0, 4, B)]
    free = rng.uniform(size=B) < 0.4
    p0[free] = rng.uniform(0, 6, (int(free.sum()), 2))
    v[free] = rng.uniform(-0.3, 0.3, (int(free.sum()), 2))
    X[:, :, :2] = p0[:, None, :] + np.arange(Nst)[None, :, None] * v[:, None, :]
    radius = np.array([0.0, 0.3, 0.5, 1.0])[rng.integers(0, 4, B)]
    if G >= 3:
        for s in range(0, B, G):
            if rng.uniform() < 0.5:
                X[s + 1], radius[s + 1] = X[s], radius[s]
    for i in range(max(3, B // 40)):
        X[rng.integers(0, B), rng.integers(0, Nst), rng.integers(0, 2)] = (np.nan, np.inf, -np.inf)[i % 3]
    return X, radius


# ----------------------------------------------------------------------------- the overtake scene and the mirror loop
OVERTAKE_N = 20
OVERTAKE_X0 = np.array([[1.0, 0.5, 0.0, 1.0], [1.35, 0.53, 0.0, 0.4], [3.5, 0.5, 0.0, 0.5]])
OVERTAKE_VREF = np.array([1.0, 0.4, 0.5])
OVERTAKE_RADIUS = 0.14
OVERTAKE_REACH = 0.5
MARGIN_MIN = 1e-3        # the recording asserts this selection margin at every step: a 1e-5 state difference flips no list


def overtake_scenes(nscenes):
    """(X0 [3 nscenes, 4], v_ref [3 nscenes], radius [3 nscenes]): scene s is the overtake scene moved as a whole by
    discs_common.scene_shifts()[s % NSHIFT] (scene 0: not moved)"""
    sh = D.scene_shifts()
    X0 = np.concatenate([OVERTAKE_X0 + np.array([sh[s % D.NSHIFT][0], sh[s % D.NSHIFT][1], 0.0, 0.0]) for s in range(nscenes)])
    return X0, np.tile(OVERTAKE_VREF, nscenes), np.full(3 * nscenes, OVERTAKE_RADIUS)


def mirror_loop(O, model, N, X0, v_ref, radius, reach, G, T, cl, shift=True, log=None):
    """Steps 1 to 6 of mpc_closed_loop_traffic on the CPU checker, U0 = 0: the oracle's rollout, the restated selection,
    the numpy gather, discs_common.reference_solve (which starts every solve at U = 0, y = 0: the solution of a step does
    not depend on the warm start where the problem has one local solution, and the recorded scene has), the plant step
    x <- x_1 of the solved plan, the realised clearance.  Returns a dict of traj_x [B, T, nx], traj_u [B, T, 2],
    traj_opp [B, T, NDISC], traj_clear [B, T], margin [T] (the selection margin of every step)."""
    X0 = np.asarray(X0, dtype=np.float64)
    B, nx = X0.shape
    cfgs = [D.configs(O, model, N, v_ref=float(v_ref[b])) for b in range(B)]
    x, U = X0.copy(), np.zeros((B, 2 * N))
    out = dict(traj_x=np.zeros((B, T, nx)), traj_u=np.zeros((B, T, 2)), traj_opp=np.zeros((B, T, NDISC), dtype=np.int32),
               traj_clear=np.zeros((B, T)), margin=np.zeros(T))
    for t in range(T):
        X = np.stack([O.rollout(cfgs[b][0], x[b], U[b]) for b in range(B)])
        opp, _, info = select_opponents(X, G, radius, reach)
        discs = gather_discs(X, opp, radius)
        for b in range(B):
            U[b] = D.reference_solve(O, cfgs[b], x[b], cl, discs[b])[0]
        out["traj_u"][:, t] = U[:, :2]
        x = np.stack([O.rollout(cfgs[b][0], x[b], U[b])[0] for b in range(B)])
        if shift:
            U[:, :-2] = U[:, 2:].copy()
        out["traj_x"][:, t], out["traj_opp"][:, t], out["margin"][t] = x, opp, info["margin"]
        out["traj_clear"][:, t] = select_opponents(x, G, radius)[1][:, 0]
        if log:
            log(f"step {t}: margin {info['margin']:.3e}, min clear {out['traj_clear'][:, t].min():.6f}, opp {opp.reshape(-1).tolist()}")
    return out
