"""The checker of event-triggered holding in traffic (mpc_opponent_trigger, mpc_closed_loop_traffic_event): the rules of
include/mpc_hip.h restated in numpy with plain loops, on top of the restated selection and gather (tests/traffic_common.py),
the rule's bits (tests/obstacles_event_common.py: why_bits, held_inputs), the car trigger (tests/event_loop_common.py) and
the CPU checker of the discs (tests/discs_common.py: the oracle's rollout, reference_solve).  Shared by
tests/test_traffic_event_cpu.py, tests/test_gpu_traffic_event.py and tests/golden/make_traffic_event_golden.py."""
import numpy as np

import discs_common as D
import event_loop_common as EC
import obstacles_event_common as OE
import traffic_common as TC

NDISC = TC.NDISC
WHY_CAR, WHY_CLEAR, WHY_NEW = OE.WHY_CAR, OE.WHY_CLEAR, OE.WHY_NEW
held_start, held_inputs, held_rollout, why_bits = OE.held_start, OE.held_inputs, OE.held_rollout, OE.why_bits


# ----------------------------------------------------------------------------- the rules
def held_selection(X, held, G, radius, reach, want_margin=True):
    """(opp_chk [B, NDISC] int32, clear_chk [B, NDISC], margin [B]): per agent b the selection of traffic_common over the
    stages j < n_b = N - k_b of X [B, N, nx] and no others.  The count is b's own: the opponents' positions are read as X
    has them.  margin: as select_opponents' -- the gap between the last selected c and the first rejected one, and from the
    deciding candidates to reach^2 (inf where nothing could flip; want_margin=False: not worked out, inf)."""
    X = np.asarray(X, dtype=np.float64)
    radius = np.asarray(radius, dtype=np.float64)
    B, N = X.shape[0], X.shape[1]
    assert 1 <= G <= TC.SCENE_MAX and B % G == 0 and reach >= 0
    opp_chk = np.full((B, NDISC), -1, dtype=np.int32)
    clear_chk = np.full((B, NDISC), np.inf)
    margin = np.full(B, np.inf)
    r2 = float(np.float64(reach) * np.float64(reach))
    with np.errstate(all="ignore"):
        for b in range(B):
            Xw = X[:, :N - held_start(held[b], N)]
            cand, _ = TC.candidates(Xw, G, radius, reach, b)
            for j, (c, o) in enumerate(cand[:NDISC]):
                opp_chk[b, j], clear_chk[b, j] = o, c
            if not want_margin:
                continue
            if len(cand) > NDISC:
                margin[b] = min(margin[b], cand[NDISC][0] - cand[NDISC - 1][0])
            if np.isfinite(r2):
                s0 = (b // G) * G
                for o in range(s0, s0 + G):
                    c = None if o == b else TC.pair_clearance(Xw, b, o, radius[o])
                    if c is not None and (c >= r2 or len(cand) <= NDISC or (float(c), o) <= cand[NDISC - 1]):
                        margin[b] = min(margin[b], abs(float(c) - r2))
    return opp_chk, clear_chk, margin


def opponent_trigger(X, held, opp_plan, G, radius, reach, clear_thr, watch, fire_in=None):
    """(fire [B] int32, why [B] uint8, opp_chk, clear_chk, margin) -- mpc_opponent_trigger.  margin: over the agents with
    held > 0, the smallest margin of the held-window selection and (watch & 1) |clear_chk[b, 0] - clear_thr|."""
    assert clear_thr <= np.float64(reach) * np.float64(reach)
    opp_chk, clear_chk, m = held_selection(X, held, G, radius, reach)
    why = why_bits(held, opp_chk, clear_chk, opp_plan, clear_thr, watch, fire_in)
    margin = np.inf
    for b in np.flatnonzero(np.asarray(held) > 0):
        margin = min(margin, m[b])
        if watch & OE.WATCH_CLEAR and np.isfinite(clear_chk[b, 0]):
            margin = min(margin, abs(clear_chk[b, 0] - clear_thr))
    return (why != 0).astype(np.int32), why, opp_chk, clear_chk, margin


# ----------------------------------------------------------------------------- the recorded scene
# traffic_common's overtake scene with the slower car nearer and a short reach.  A held plan is blind to what the SELECTION
# left out, and the selection runs on the rollout of the plans before the solve.  So the rear car starts from a warm start
# that steers off the line (full throttle, full left): its rollout stays out of reach of the slower car, the plan of step 0
# is solved against nobody, drives straight along the line and, held, runs through the slower car.
EVENT_N = TC.OVERTAKE_N
EVENT_GAP = 0.30              # the slower car's lead over the rear car (overtake scene: 0.35)
EVENT_X0 = np.array([[1.0, 0.5, 0.0, 1.0], [1.0 + EVENT_GAP, 0.53, 0.0, 0.4], [3.5, 0.5, 0.0, 0.5]])
EVENT_VREF = TC.OVERTAKE_VREF
EVENT_RADIUS = TC.OVERTAKE_RADIUS
EVENT_RADII = np.array([0.07, EVENT_RADIUS, EVENT_RADIUS])   # of each car as an obstacle: the rear car is a small one -- the
#                               slower car, which a plan drives through from behind, has to move 0.04 aside, not 0.11 in eight stages
EVENT_REACH = 0.13            # reach^2 = 0.0169: the warm start's rollout comes no nearer than c = 0.020
EVENT_U0 = np.stack([np.tile([1.0, 0.32], EVENT_N), np.zeros(2 * EVENT_N), np.zeros(2 * EVENT_N)])
EVENT_MAX_HOLD = 8
EVENT_THR = 0.05              # the car trigger: without a disturbance the plant stays on its plan
EVENT_CLEAR_THR = -2e-3       # g = d^2 - r^2: a solved plan rides g = 0 to within alm_delta, MARGIN_MIN away from this
EVENT_W = np.ones(4)
EVENT_T = 24                  # steps of the recorded loop
EVENT_T_BLIND = 8             # steps of the loop that watches the car alone, up to the hold limit
MARGIN_MIN = TC.MARGIN_MIN


def event_scenes(nscenes):
    """(X0 [3 nscenes, 4], v_ref, radius, U0 [3 nscenes, 2N]): scene s is the recorded scene moved as a whole by
    discs_common.scene_shifts()[s % NSHIFT] (scene 0: not moved); G = 3"""
    sh = D.scene_shifts()
    X0 = np.concatenate([EVENT_X0 + np.array([sh[s % D.NSHIFT][0], sh[s % D.NSHIFT][1], 0.0, 0.0]) for s in range(nscenes)])
    return X0, np.tile(EVENT_VREF, nscenes), np.tile(EVENT_RADII, nscenes), np.tile(EVENT_U0, (nscenes, 1))


def event_loop(O, X0, v_ref, radius, U0, watch, T, log=None):
    """the mirror loop on recorded scenes"""
    return mirror_loop_event(O, 0, EVENT_N, X0, v_ref, radius, EVENT_REACH, 3, T, D.line_centerline(), EVENT_W, EVENT_THR,
                             EVENT_MAX_HOLD, EVENT_CLEAR_THR, watch, log=log, U0=U0)


# ----------------------------------------------------------------------------- the scenes of the loop tests
def loop_scene(model, B, G, seed):
    """(X0 [B, nx], v_ref [B], radius [B], shape [B, 4]): scenes of G cars in a row 0.28 .. 0.33 apart near the line y = 0.5
    of discs_common.line_centerline(), the rear ones faster -- within the horizon a rear car's plan runs into the plan of the
    car ahead --, but for the last (G >= 3), which drives 2 m ahead of the row and meets nobody: it re-plans for its own
    sake alone.  Radii 0.2 .. 0.24 (nobody inside a disc at the start), shape = [A, kx, ky, gain] of a car as a risk source"""
    rng = np.random.default_rng(seed)
    X0 = np.zeros((B, 6 if model else 4))
    for s in range(0, B, G):
        X0[s:s + G, 0] = 1.2 + np.cumsum(rng.uniform(0.28, 0.33, G))
        if G >= 3:
            X0[s + G - 1, 0] += 2.0
        X0[s:s + G, 1] = 0.5 + rng.uniform(-.04, .04, G)
        X0[s:s + G, 3] = 1.1 - 0.7 * np.arange(G) / max(G - 1, 1) + rng.uniform(-.03, .03, G)
    radius = rng.uniform(0.2, 0.24, B)
    shape = np.stack([rng.uniform(0.2, 0.4, B), 1.0 / (2.0 * rng.uniform(0.15, 0.25, B) ** 2), 1.0 / (2.0 * rng.uniform(0.05, 0.08, B) ** 2),
                      rng.uniform(0.1, 0.3, B)], 1)
    return X0, X0[:, 3].copy(), radius, shape


# ----------------------------------------------------------------------------- the mirror loop
def mirror_loop_event(O, model, N, X0, v_ref, radius, reach, G, T, cl, w, thr, max_hold, clear_thr, watch, shift=True, log=None,
                      solve=None, U0=None):
    """The ten steps of mpc_closed_loop_traffic_event (no disturbance, the plant on the controller's parameters) on the CPU
    checker, from the plans U0 [B, 2N] (None: zeros) and held = -1: the oracle's rollout, the restated triggers, selection
    and gather, discs_common.reference_solve for the agents that fire (it starts at U = 0, y = 0 and raises where it does
    not converge; `solve(b, cfgs, x, cl, discs)`: another solver, for the checks of this file's own logic).  Returns a dict
    of traj_x, traj_u, traj_opp, traj_chk (the held-window selection of the agents with held > 0, -1 elsewhere),
    traj_clear, traj_why, solved, held, opp_plan, solve_count and margin [T] (the smallest decision margin of the step: the
    full-window selection, the held-window selection, |clear_chk - clear_thr|, |dev2 - thr^2|)."""
    X0 = np.asarray(X0, dtype=np.float64)
    B, nx = X0.shape
    cfgs = [D.configs(O, model, N, v_ref=float(v_ref[b])) for b in range(B)]
    if solve is None:
        solve = lambda b, c, xb, cl_, d: D.reference_solve(O, c, xb, cl_, d)[0]      # noqa: E731
    x, xhat = X0.copy(), np.zeros_like(X0)
    U = np.zeros((B, 2 * N)) if U0 is None else np.array(U0, dtype=np.float64)
    held = np.full(B, -1, dtype=np.int32)
    opp_plan = np.full((B, NDISC), -1, dtype=np.int32)
    rows = np.zeros((B, N, NDISC, 3))
    out = dict(traj_x=np.zeros((B, T, nx)), traj_u=np.zeros((B, T, 2)), traj_opp=np.zeros((B, T, NDISC), dtype=np.int32),
               traj_clear=np.zeros((B, T)), traj_why=np.zeros((B, T), dtype=np.uint8), solved=np.zeros((B, T), dtype=np.uint8),
               margin=np.full(T, np.inf), solve_count=np.zeros(B, dtype=np.int32),
               traj_chk=np.full((B, T, NDISC), -1, dtype=np.int32))
    for t in range(T):
        fire_dev = np.zeros(B, dtype=np.int32)
        for b in range(B):                                                         # 1. the car trigger
            d2, f = EC.trigger(x[b].copy(), xhat[b], held[b], w, thr, max_hold)
            fire_dev[b] = f
            if 0 <= held[b] < max_hold and np.isfinite(thr) and thr > 0:
                out["margin"][t] = min(out["margin"][t], abs(d2 - thr * thr))
        # 2. what everybody will go on applying, 3. the rule, 4. the shift
        X = np.stack([held_rollout(lambda xb, Ub, c=cfgs[b][0]: O.rollout(c, xb, Ub), x[b], U[b], held[b]) for b in range(B)])
        fire, why, opp_chk, _, m_chk = opponent_trigger(X, held, opp_plan, G, radius, reach, clear_thr, watch, fire_dev)
        out["traj_chk"][held > 0, t] = opp_chk[held > 0]
        for b in np.flatnonzero(fire):
            if shift and held[b] > 0:
                U[b] = held_inputs(U[b], held[b]).ravel()
        opp, _, info = TC.select_opponents(X, G, radius, reach)                    # 5. everybody's selection
        new_rows = TC.gather_discs(X, opp, radius)
        for b in np.flatnonzero(fire):                                             # 6. the firing agents' rows, 7. their solves
            rows[b], opp_plan[b] = new_rows[b], opp[b]
        for b in np.flatnonzero(fire):
            U[b] = solve(b, cfgs[b], x[b], cl, rows[b])
            held[b], xhat[b] = 0, x[b]
            out["solve_count"][b] += 1
        for b in range(B):                                                         # 9. the step
            u = U[b, 2 * held[b]:2 * held[b] + 2].copy()
            x[b] = O.rollout(cfgs[b][0], x[b], u)[0]
            xhat[b] = O.rollout(cfgs[b][0], xhat[b], u)[0]
            held[b] += 1
            out["traj_u"][b, t] = u
        out["traj_x"][:, t], out["traj_opp"][:, t], out["traj_why"][:, t], out["solved"][:, t] = x, opp, why, fire
        out["margin"][t] = min(out["margin"][t], info["margin"], m_chk)
        out["traj_clear"][:, t] = TC.select_opponents(x, G, radius)[1][:, 0]        # 10. the realised clearance
        if log:
            log(f"step {t}: why {why.tolist()} held {held.tolist()} margin {out['margin'][t]:.3e} clear "
                f"{out['traj_clear'][:, t].min():.6f} opp {opp.reshape(-1).tolist()} chk {opp_chk.reshape(-1).tolist()}")
    out["held"], out["opp_plan"], out["U"], out["x"] = held, opp_plan, U, x
    return out
