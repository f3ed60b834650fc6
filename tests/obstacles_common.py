"""The checker of the scripted obstacles (mpc_obstacles_select, mpc_discs_from_obstacles / mpc_fields_from_obstacles,
mpc_closed_loop_obstacles): the rule of include/mpc_hip.h restated in numpy with plain loops over agents, obstacles and
stages -- np.float64 scalars, the kernel's operation order, so that the bits agree --, the generator of the selection
cases, the scenes of the loop tests, and the loop's steps on the CPU checker of the discs (tests/discs_common.py: the
oracle's rollout, reference_solve).  Shared by tests/test_obstacles_cpu.py, tests/test_gpu_obstacles.py and
tests/golden/make_obstacles_golden.py."""
import numpy as np

import discs_common as D
import traffic_common as TC

NDISC = D.NDISC
SCENE_MAX = 64
NFSRC = 8


# ----------------------------------------------------------------------------- the rule
def sample_index(i, Lt, wrap):
    """the sample of time i >= 0 of a track of Lt samples, in integers"""
    i, Lt = int(i), int(Lt)
    assert i >= 0 and Lt >= 1
    return i % Lt if wrap else min(i, Lt - 1)


def absent(sample):
    """r == 0 of a disc (cx, cy, r), A == 0 of a source (cx, cy, c, s, A, kx, ky, alpha)"""
    return sample[2 if len(sample) == 3 else 4] == 0.0


def pair_clearance(X, b, track, ti, wrap):
    """(c, present, gone): c(b, o) = min_k (dx dx + dy dy) - r2 over the stages of X [B, Nst, nx] whose sample of track
    [Lt, W] is present, every operation rounded on its own (r2 = r r for discs, 0 for fields); c is None when a g_k is not
    finite and +inf when no sample is present; `present` and `gone` count the window's samples"""
    W = track.shape[1]
    c = np.float64(np.inf)
    present = gone = 0
    bad = False
    for k in range(X.shape[1]):
        s = track[sample_index(ti + k, track.shape[0], wrap)]
        if absent(s):
            gone += 1
            continue
        present += 1
        r2 = s[2] * s[2] if W == 3 else np.float64(0.0)
        dx = X[b, k, 0] - s[0]
        dy = X[b, k, 1] - s[1]
        g = (dx * dx + dy * dy) - r2
        if not np.isfinite(g):
            bad = True
        elif g < c:
            c = g
    return (None if bad else c), present, gone


def select_obstacles(X, G, obs, ti=0, reach=np.inf, wrap=False):
    """(sel [B, NDISC] int32, clear [B, NDISC], info) of X [B, Nst, nx] (or [B, nx]: one stage) and obs [B / G, K, Lt, W].
    sel holds indices within the scene.  info counts what the selection had to decide: `ties` slots whose c equals the next
    candidate's (the index decided), `short` agents with fewer than NDISC candidates, `nonfinite` excluded pairs, `absent`
    absent samples inside the window of a selected obstacle, `empty` pairs whose window holds no present sample; `margin`
    is the smallest gap between two selected c's (the order of the slots), between the last selected c and the first rejected
    one, or from a c that counts to reach^2."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[:, None, :]
    obs = np.asarray(obs, dtype=np.float64)
    B, K = X.shape[0], obs.shape[1]
    assert 1 <= G <= SCENE_MAX and 1 <= K <= SCENE_MAX and B % G == 0 and obs.shape[0] == B // G and reach >= 0
    sel = np.full((B, NDISC), -1, dtype=np.int32)
    clear = np.full((B, NDISC), np.inf)
    info = dict(ties=0, short=0, nonfinite=0, absent=0, empty=0, margin=np.inf)
    r2 = np.float64(reach) * np.float64(reach)
    with np.errstate(all="ignore"):
        for b in range(B):
            cand, gone, rest = [], {}, []
            for o in range(K):
                c, present, gone[o] = pair_clearance(X, b, obs[b // G, o], ti, wrap)
                if c is None:
                    info["nonfinite"] += 1
                elif present == 0:
                    info["empty"] += 1
                elif c < r2:
                    cand.append((float(c), o))
                else:
                    rest.append(float(c))
            cand.sort()
            info["short"] += len(cand) < NDISC
            for j, (c, o) in enumerate(cand[:NDISC]):
                sel[b, j], clear[b, j] = o, c
                info["ties"] += j + 1 < len(cand) and cand[j + 1][0] == c
                info["absent"] += gone[o]
            if len(cand) > NDISC:
                info["margin"] = min(info["margin"], cand[NDISC][0] - cand[NDISC - 1][0])
            for j in range(1, min(len(cand), NDISC)):               # the order of the slots: sel is compared slot for slot
                info["margin"] = min(info["margin"], cand[j][0] - cand[j - 1][0])
            if np.isfinite(r2):
                for c in rest + [c for c, _ in (cand if len(cand) <= NDISC else cand[:NDISC])]:
                    info["margin"] = min(info["margin"], abs(c - float(r2)))
    return sel, clear, info


def gather_rows(sel, G, obs, ti, N, wrap=False):
    """mpc_discs_from_obstacles / mpc_fields_from_obstacles in numpy: [B, N, NDISC, W]"""
    obs = np.asarray(obs, dtype=np.float64)
    B, K, Lt, W = sel.shape[0], obs.shape[1], obs.shape[2], obs.shape[3]
    out = np.zeros((B, N, NDISC, W))
    for b in range(B):
        for j in range(NDISC):
            o = int(sel[b, j])
            if not 0 <= o < K:
                continue
            for k in range(N):
                s = obs[b // G, o, sample_index(ti + k, Lt, wrap)]
                if not absent(s):
                    out[b, k, j] = s
    return out


# ----------------------------------------------------------------------------- the selection cases
# (G, K, B): K no power of two, K > G and K < G, the last workgroup partly filled
SELECTION_SHAPES = ((1, 1, 70), (5, 3, 130), (17, 64, 255), (64, 17, 128), (3, 33, 258))
# the kernel stages 16 stages at a time: 17 leaves a last chunk of 1, 37 a ragged one of 5 (20: 16 + 4)
SELECTION_STAGES = (1, 12, 20, 17, 37)
SELECTION_REACH = 2.5


def selection_window(Nst, which):
    """(Lt, ti, wrap) of selection case `which`: a track of one sample behind whose end the window lies; a window that
    clamps across Lt - 1; one that wraps; one wholly behind the end; one inside a periodic track"""
    return ((1, 3, False), (Nst // 2 + 2, 1, False), (7, 5, True), (9, 30, False), (Nst + 6, 3, True))[which % 5]


def selection_case(nx, W, Nst, G, K, B, which, seed=0):
    """(X [B, Nst, nx], obs [B / G, K, Lt, W], ti, wrap).  60 % of the agents and of the obstacles move on the integer grid
    with integer velocities (exact arithmetic: equal clearances abound), the others anywhere; where K >= 2, obstacle 1 of a
    scene is a copy of obstacle 0 half of the time (exact ties along the whole window); radii from {0.3, 0.5, 1}; 15 % of
    the samples are absent, with junk (a NaN among it) behind the zero; every sixth obstacle is absent throughout; a few
    NaN and infinite positions among the agents' stages and the present samples"""
    Lt, ti, wrap = selection_window(Nst, which)
    rng = np.random.default_rng(100000 * seed + 1000 * W + 100 * nx + 7 * Nst + 3 * G + K)
    X = rng.normal(size=(B, Nst, nx))

    def paths(n, length):
        p0 = rng.integers(0, 6, (n, 2)).astype(np.float64)
        v = np.array([(0, 0), (1, 0), (0, 1), (1, 1)], dtype=np.float64)[rng.integers(0, 4, n)]
        free = rng.uniform(size=n) < 0.4
        p0[free] = rng.uniform(0, 6, (int(free.sum()), 2))
        v[free] = rng.uniform(-0.3, 0.3, (int(free.sum()), 2))
        return p0, v, p0[:, None, :] + np.arange(length)[None, :, None] * v[:, None, :]
    X[:, :, :2] = paths(B, Nst)[2]
    S = B // G
    obs = rng.normal(size=(S, K, Lt, W))
    # an obstacle's sample i is where it is at time i: agents' stage k meets sample ti + k
    p0, v, _ = paths(S * K, 1)
    idx = np.arange(Lt)
    obs[..., :2] = (p0[:, None, :] + idx[None, :, None] * v[:, None, :]).reshape(S, K, Lt, 2)
    if W == 3:
        obs[..., 2] = np.array([0.3, 0.5, 1.0])[rng.integers(0, 3, (S, K, Lt))]
        key = 2
    else:
        obs[..., 4] = np.array([0.3, 1.0])[rng.integers(0, 2, (S, K, Lt))]
        obs[..., 5:7] = np.abs(obs[..., 5:7])
        key = 4
    if K >= 2:
        for s in range(S):
            if rng.uniform() < 0.5:
                obs[s, 1] = obs[s, 0]
    for i in range(max(3, S * K // 40)):
        obs[rng.integers(0, S), rng.integers(0, K), rng.integers(0, Lt), rng.integers(0, 2)] = (np.nan, np.inf, -np.inf)[i % 3]
    gone = rng.uniform(size=(S, K, Lt)) < 0.15
    gone[(np.arange(S * K) % 6 == 5).reshape(S, K)] = True
    junk = obs[gone]
    junk[:, key] = 0.0
    junk[::3, 0] = np.nan
    obs[gone] = junk
    for i in range(max(3, B // 40)):
        X[rng.integers(0, B), rng.integers(0, Nst), rng.integers(0, 2)] = (np.nan, np.inf, -np.inf)[i % 3]
    return X, obs, ti, wrap


# ----------------------------------------------------------------------------- the scenes of the host-loop test
def loop_scene(model, B, G, K, Lt, W, seed, Ts=0.05):
    """(X0 [B, nx], v_ref [B], obs [B / G, K, Lt, W]) on discs_common.line_centerline(): the agents of a scene stand
    0.5 .. 0.9 apart along the line; obstacle o < K - 1 starts 0.3 .. 0.4 ahead of agent o % G a little beside the line
    and drives at 0.3 m/s (the agent's plan runs into it within the horizon); obstacle 1 is absent for its first 4 samples;
    obstacle K - 1 stands far away (never a candidate at a finite reach).  Discs: r 0.10 .. 0.14.  Sources: the frame of
    the line, A = 0.3, sigma_x = sigma_y = FIELD_SIGMA, a small skew."""
    rng = np.random.default_rng(seed)
    nx = 6 if model else 4
    X0 = np.zeros((B, nx))
    v_ref = rng.uniform(0.8, 1.0, B)
    obs = np.zeros((B // G, K, Lt, W))
    i = np.arange(Lt)
    for s in range(B // G):
        x = 1.2 + rng.uniform(0, 0.2)
        for a in range(G):
            b = s * G + a
            x += rng.uniform(0.5, 0.9) * (a > 0)
            X0[b, :4] = (x, 0.5 + rng.uniform(-.03, .03), rng.uniform(-.05, .05), v_ref[b])
        for o in range(K):
            if o == K - 1 and K > 1:
                cx, cy = np.full(Lt, 3.0), np.full(Lt, 5.0)
            else:
                cx = X0[s * G + o % G, 0] + rng.uniform(0.3, 0.4) + 0.3 * Ts * i
                cy = np.full(Lt, 0.5 + rng.uniform(-.04, .04))
            obs[s, o, :, 0], obs[s, o, :, 1] = cx, cy
            if W == 3:
                obs[s, o, :, 2] = rng.uniform(0.10, 0.14)
            else:
                obs[s, o, :, 2:] = (1.0, 0.0, 0.3, 0.5 / FIELD_SIGMA ** 2, 0.5 / FIELD_SIGMA ** 2, 0.1)
        if K > 2:
            obs[s, 1, :4] = 0.0
    return X0, v_ref, obs


FIELD_SIGMA = 0.15


# ----------------------------------------------------------------------------- the recorded scene and the mirror loop
SCRIPT_N = TC.OVERTAKE_N
SCRIPT_X0 = TC.OVERTAKE_X0[0]                 # one kinematic car on discs_common.line_centerline(), v_ref = 1
SCRIPT_VREF = 1.0
SCRIPT_LT = 40
SCRIPT_REACH = 0.5
SCRIPT_RADIUS = 0.14
SCRIPT_APPEARS = 6
MARGIN_MIN = TC.MARGIN_MIN    # the recording asserts this selection margin at every step: a 1e-5 state difference flips no list


def script_tracks(Ts=0.05):
    """obs [3, SCRIPT_LT, 3] of one scene: a slower obstacle ahead, 0.03 beside the line, r = 0.14, at 0.4 m/s (where the
    slow car of the traffic test starts); one crossing the line ahead of the car, from above to below, before the car gets there (the second nearest at the
    first step, then it is gone below and the third one takes its slot); one that appears
    at sample SCRIPT_APPEARS and stands below the line where the car comes back to it"""
    i = np.arange(SCRIPT_LT)
    obs = np.zeros((3, SCRIPT_LT, 3))
    obs[0, :, 0], obs[0, :, 1], obs[0, :, 2] = 1.35 + 0.4 * Ts * i, 0.53, SCRIPT_RADIUS
    obs[1, :, 0], obs[1, :, 1], obs[1, :, 2] = 2.0, 0.94 - 0.8 * Ts * i, 0.1
    obs[2, :, 0], obs[2, :, 1], obs[2, :, 2] = 2.05, 0.22, 0.08
    obs[2, :SCRIPT_APPEARS] = (7.0, 7.0, 0.0)          # not there yet: whatever stands behind r == 0 is not read
    return obs


def script_scenes(nscenes):
    """(X0 [nscenes, 4], v_ref [nscenes], obs [nscenes, 3, SCRIPT_LT, 3]): scene s is the recorded scene moved as a whole
    by discs_common.scene_shifts()[s % NSHIFT] (scene 0: not moved); G = 1"""
    sh = D.scene_shifts()
    X0 = np.stack([SCRIPT_X0 + np.array([sh[s % D.NSHIFT][0], sh[s % D.NSHIFT][1], 0.0, 0.0]) for s in range(nscenes)])
    obs = np.stack([script_tracks() + np.array([sh[s % D.NSHIFT][0], sh[s % D.NSHIFT][1], 0.0]) for s in range(nscenes)])
    return X0, np.full(nscenes, SCRIPT_VREF), obs


def mirror_loop(O, model, N, X0, v_ref, obs, reach, G, T, cl, t0=0, wrap=False, shift=True, log=None):
    """Steps 1 to 6 of mpc_closed_loop_obstacles (no track) on the CPU checker, U0 = 0: the oracle's rollout, the restated
    selection and gather, discs_common.reference_solve (which starts every solve at U = 0, y = 0 and raises where it does
    not converge), the plant step x <- x_1 of the solved plan, the realised clearance.  Returns a dict of traj_x
    [B, T, nx], traj_u [B, T, 2], traj_sel [B, T, NDISC], traj_clear [B, T], margin [T]."""
    X0 = np.asarray(X0, dtype=np.float64)
    B, nx = X0.shape
    cfgs = [D.configs(O, model, N, v_ref=float(v_ref[b])) for b in range(B)]
    x, U = X0.copy(), np.zeros((B, 2 * N))
    out = dict(traj_x=np.zeros((B, T, nx)), traj_u=np.zeros((B, T, 2)), traj_sel=np.zeros((B, T, NDISC), dtype=np.int32),
               traj_clear=np.zeros((B, T)), margin=np.zeros(T))
    for t in range(T):
        ti = t0 + t + 1
        X = np.stack([O.rollout(cfgs[b][0], x[b], U[b]) for b in range(B)])
        sel, _, info = select_obstacles(X, G, obs, ti, reach, wrap)
        discs = gather_rows(sel, G, obs, ti, N, wrap)
        for b in range(B):
            U[b] = D.reference_solve(O, cfgs[b], x[b], cl, discs[b])[0]
        out["traj_u"][:, t] = U[:, :2]
        x = np.stack([O.rollout(cfgs[b][0], x[b], U[b])[0] for b in range(B)])
        if shift:
            U[:, :-2] = U[:, 2:].copy()
        out["traj_x"][:, t], out["traj_sel"][:, t], out["margin"][t] = x, sel, info["margin"]
        out["traj_clear"][:, t] = select_obstacles(x, G, obs, ti, np.inf, wrap)[1][:, 0]
        if log:
            log(f"step {t}: margin {info['margin']:.3e}, clear {out['traj_clear'][:, t].min():.6f}, sel {sel.reshape(-1).tolist()}, "
                f"x {x[0, :2]}")
    return out
