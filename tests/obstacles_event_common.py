"""The checker of the event-triggered loop among scripted obstacles (mpc_rollout_held, mpc_obstacle_trigger,
mpc_closed_loop_obstacles_event): the rules of include/mpc_hip.h restated in numpy with plain loops, on top of the
restated selection and gather (tests/obstacles_common.py), the car trigger (tests/event_loop_common.py) and the CPU
checker of the discs (tests/discs_common.py: the oracle's rollout, reference_solve).  Shared by
tests/test_obstacles_event_cpu.py and tests/test_gpu_obstacles_event.py."""
import numpy as np

import discs_common as D
import event_loop_common as EC
import obstacles_common as OC

NDISC = OC.NDISC
WHY_CAR, WHY_CLEAR, WHY_NEW = 1, 2, 4        # bits of `why`: the car trigger, the clearance rule, the new-obstacle rule
WATCH_CLEAR, WATCH_NEW = 1, 2                # bits of `watch`


# ----------------------------------------------------------------------------- the rules
def held_start(held, N):
    """k_b: the first stage of the plan that is still to be applied"""
    return min(max(int(held), 0), N - 1)


def held_inputs(U, held):
    """the inputs an agent will go on applying, [N, 2]: u_{min(k + i, N - 1)} -- the in-place shift of the trigger"""
    N = U.shape[0] // 2
    k = held_start(held, N)
    return U.reshape(N, 2)[np.minimum(np.arange(N) + k, N - 1)]


def held_rollout(rollout, x, U, held):
    """X [N, nx] of one agent: rollout(x, U') with U' the plan shifted by the stages it has applied"""
    return rollout(x, held_inputs(U, held).ravel())


def held_selection(X, held, G, obs, ti, reach, wrap=False):
    """(sel_chk [B, NDISC] int32, clear_chk [B, NDISC], margin): per agent the selection of obstacles_common over the
    N - k_b stages its plan still holds and no others (the agent alone against its scene's tracks: agents are independent)"""
    X = np.asarray(X, dtype=np.float64)
    B, N = X.shape[0], X.shape[1]
    sel_chk = np.full((B, NDISC), -1, dtype=np.int32)
    clear_chk = np.full((B, NDISC), np.inf)
    margin = np.full(B, np.inf)
    for b in range(B):
        nst = N - held_start(held[b], N)
        sel, clear, info = OC.select_obstacles(X[b:b + 1, :nst], 1, obs[b // G:b // G + 1], ti, reach, wrap)
        sel_chk[b], clear_chk[b], margin[b] = sel[0], clear[0], info["margin"]
    return sel_chk, clear_chk, margin


def why_bits(held, sel_chk, clear_chk, sel_plan, clear_thr, watch, fire_in=None):
    """why [B] uint8: bit 0 the caller's fire; for held > 0, bit 1 = not clear_chk[b, 0] >= clear_thr (watch & 1), bit 2 =
    some sel_chk[b, j] >= 0 is not a member of the SET sel_plan[b] (watch & 2)"""
    B = len(held)
    assert 0 <= watch <= 3
    why = np.zeros(B, dtype=np.uint8)
    for b in range(B):
        w = WHY_CAR if fire_in is not None and fire_in[b] != 0 else 0
        if held[b] > 0:
            if watch & WATCH_CLEAR and not clear_chk[b, 0] >= clear_thr:
                w |= WHY_CLEAR
            plan = {int(o) for o in sel_plan[b]}
            if watch & WATCH_NEW and any(int(o) >= 0 and int(o) not in plan for o in sel_chk[b]):
                w |= WHY_NEW
        why[b] = w
    return why


def obstacle_trigger(X, held, sel_plan, G, obs, ti, reach, clear_thr, watch, fire_in=None, wrap=False):
    """(fire [B] int32, why [B] uint8, sel_chk, clear_chk, margin) -- mpc_obstacle_trigger.  margin: over the agents with
    held > 0, the smallest margin of the held-window selection and (watch & 1) |clear_chk[b, 0] - clear_thr|."""
    assert clear_thr <= np.float64(reach) * np.float64(reach)
    sel_chk, clear_chk, m = held_selection(X, held, G, obs, ti, reach, wrap)
    why = why_bits(held, sel_chk, clear_chk, sel_plan, clear_thr, watch, fire_in)
    margin = np.inf
    for b in np.flatnonzero(np.asarray(held) > 0):
        margin = min(margin, m[b])
        if watch & WATCH_CLEAR and np.isfinite(clear_chk[b, 0]):
            margin = min(margin, abs(clear_chk[b, 0] - clear_thr))
    return (why != 0).astype(np.int32), why, sel_chk, clear_chk, margin


# ----------------------------------------------------------------------------- the recorded scene
# A held plan meets only samples its own solve has met: what it can be blind to is a track the SELECTION left out, and the
# selection runs on the rollout of the plan before the solve.  So the scene starts from a warm start that steers off the line
# (U0 = full throttle, full left): its rollout is out of reach of both obstacles, the plan of step 0 is solved against
# nothing, drives straight along the line and, held, runs into the second obstacle at time 8.
SCRIPT_N = OC.SCRIPT_N
SCRIPT_X0 = OC.SCRIPT_X0                      # one kinematic car on discs_common.line_centerline(), v_ref = 1
SCRIPT_VREF = OC.SCRIPT_VREF
SCRIPT_U0 = np.tile([1.0, 0.32], SCRIPT_N)
SCRIPT_LT = 72
SCRIPT_REACH = 0.12
SCRIPT_APPEARS = 8            # A: the first sample at which the second obstacle is there
SCRIPT_NEW = (1.40, 0.47, 0.07)               # where it stands from then on: 0.03 beside the line, on the held plan's way
SCRIPT_MAX_HOLD = 8
SCRIPT_THR = 0.05             # the car trigger: without a disturbance the plant stays on its plan
SCRIPT_CLEAR_THR = -2e-3      # g = d^2 - r^2: a solved plan rides g = 0 to within alm_delta, MARGIN_MIN away from this
SCRIPT_W = np.ones(4)
SCRIPT_T = 48                 # steps of the recorded loop: the car has passed the slower obstacle
SCRIPT_T_BLIND = 8            # steps of the loop that watches the car alone, up to the hold limit: it is inside the disc then
MARGIN_MIN = OC.MARGIN_MIN


def script_tracks(Ts=0.05):
    """obs [2, SCRIPT_LT, 3] of one scene: a slower obstacle ahead (r = 0.14 at 0.4 m/s from x = 2.2, 0.03 beside the line),
    which the car passes; and one that is absent until sample SCRIPT_APPEARS and from then on stands at SCRIPT_NEW"""
    i = np.arange(SCRIPT_LT)
    obs = np.zeros((2, SCRIPT_LT, 3))
    obs[0, :, 0], obs[0, :, 1], obs[0, :, 2] = 2.2 + 0.4 * Ts * i, 0.53, OC.SCRIPT_RADIUS
    obs[1, :] = SCRIPT_NEW
    obs[1, :SCRIPT_APPEARS] = (7.0, 7.0, 0.0)          # not there yet: whatever stands behind r == 0 is not read
    return obs


def script_scenes(nscenes):
    """(X0 [nscenes, 4], v_ref [nscenes], obs [nscenes, 2, SCRIPT_LT, 3], U0 [nscenes, 2N]): scene s is the recorded scene
    moved as a whole by discs_common.scene_shifts()[s % NSHIFT] (scene 0: not moved); G = 1"""
    sh = D.scene_shifts()
    X0 = np.stack([SCRIPT_X0 + np.array([sh[s % D.NSHIFT][0], sh[s % D.NSHIFT][1], 0.0, 0.0]) for s in range(nscenes)])
    obs = np.stack([script_tracks() + np.array([sh[s % D.NSHIFT][0], sh[s % D.NSHIFT][1], 0.0]) for s in range(nscenes)])
    return X0, np.full(nscenes, SCRIPT_VREF), obs, np.tile(SCRIPT_U0, (nscenes, 1))


def script_loop(O, X0, v_ref, obs, U0, watch, T, log=None):
    """the mirror loop on recorded scenes"""
    return mirror_loop_event(O, 0, SCRIPT_N, X0, v_ref, obs, SCRIPT_REACH, 1, T, D.line_centerline(), SCRIPT_W, SCRIPT_THR,
                             SCRIPT_MAX_HOLD, SCRIPT_CLEAR_THR, watch, log=log, U0=U0)


def first_seen(res, s, o):
    """the first step at which track o is in agent s's held-window selection (traj_chk), or None"""
    hit = np.flatnonzero((res["traj_chk"][s] == o).any(1))
    return int(hit[0]) if hit.size else None


# ----------------------------------------------------------------------------- the mirror loop
def mirror_loop_event(O, model, N, X0, v_ref, obs, reach, G, T, cl, w, thr, max_hold, clear_thr, watch, t0=0, wrap=False,
                      shift=True, log=None, solve=None, U0=None):
    """The eleven steps of mpc_closed_loop_obstacles_event (no track, no disturbance, the plant on the controller's
    parameters) on the CPU checker, from the plans U0 [B, 2N] (None: zeros) and held = -1: the oracle's rollout, the restated triggers, selection and gather,
    discs_common.reference_solve for the agents that fire (it starts at U = 0, y = 0 and raises where it does not
    converge; `solve(b, cfgs, x, cl, discs)`: another solver, for the checks of this file's own logic).  Returns a dict of
    traj_x, traj_u, traj_sel, traj_chk (the held-window selection of the agents with held > 0, -1 elsewhere), traj_clear,
    traj_why, solved, held, sel_plan, solve_count and margin [T] (the smallest
    decision margin of the step: the full-window selection, the held-window selection, |clear_chk - clear_thr|,
    |dev2 - thr^2|)."""
    X0 = np.asarray(X0, dtype=np.float64)
    B, nx = X0.shape
    cfgs = [D.configs(O, model, N, v_ref=float(v_ref[b])) for b in range(B)]
    if solve is None:
        solve = lambda b, c, xb, cl_, d: D.reference_solve(O, c, xb, cl_, d)[0]      # noqa: E731
    x, xhat = X0.copy(), np.zeros_like(X0)
    U = np.zeros((B, 2 * N)) if U0 is None else np.array(U0, dtype=np.float64)
    held = np.full(B, -1, dtype=np.int32)
    sel_plan = np.full((B, NDISC), -1, dtype=np.int32)
    rows = np.zeros((B, N, NDISC, obs.shape[3]))
    out = dict(traj_x=np.zeros((B, T, nx)), traj_u=np.zeros((B, T, 2)), traj_sel=np.zeros((B, T, NDISC), dtype=np.int32),
               traj_clear=np.zeros((B, T)), traj_why=np.zeros((B, T), dtype=np.uint8), solved=np.zeros((B, T), dtype=np.uint8),
               margin=np.full(T, np.inf), solve_count=np.zeros(B, dtype=np.int32),
               traj_chk=np.full((B, T, NDISC), -1, dtype=np.int32))
    for t in range(T):
        ti = t0 + t + 1
        fire_dev = np.zeros(B, dtype=np.int32)
        for b in range(B):
            d2, f = EC.trigger(x[b].copy(), xhat[b], held[b], w, thr, max_hold)
            fire_dev[b] = f
            if 0 <= held[b] < max_hold and np.isfinite(thr) and thr > 0:
                out["margin"][t] = min(out["margin"][t], abs(d2 - thr * thr))
        X = np.stack([held_rollout(lambda xb, Ub, c=cfgs[b][0]: O.rollout(c, xb, Ub), x[b], U[b], held[b]) for b in range(B)])
        fire, why, sel_chk, _, m_chk = obstacle_trigger(X, held, sel_plan, G, obs, ti, reach, clear_thr, watch, fire_dev, wrap)
        out["traj_chk"][held > 0, t] = sel_chk[held > 0]
        for b in np.flatnonzero(fire):
            if shift and held[b] > 0:
                U[b] = held_inputs(U[b], held[b]).ravel()
        sel, _, info = OC.select_obstacles(X, G, obs, ti, reach, wrap)
        new_rows = OC.gather_rows(sel, G, obs, ti, N, wrap)
        for b in np.flatnonzero(fire):
            rows[b], sel_plan[b] = new_rows[b], sel[b]
            U[b] = solve(b, cfgs[b], x[b], cl, rows[b])
            held[b], xhat[b] = 0, x[b]
            out["solve_count"][b] += 1
        for b in range(B):
            u = U[b, 2 * held[b]:2 * held[b] + 2].copy()
            x[b] = O.rollout(cfgs[b][0], x[b], u)[0]
            xhat[b] = O.rollout(cfgs[b][0], xhat[b], u)[0]
            held[b] += 1
            out["traj_u"][b, t] = u
        out["traj_x"][:, t], out["traj_sel"][:, t], out["traj_why"][:, t], out["solved"][:, t] = x, sel, why, fire
        out["margin"][t] = min(out["margin"][t], info["margin"], m_chk)
        out["traj_clear"][:, t] = OC.select_obstacles(x, G, obs, ti, np.inf, wrap)[1][:, 0]
        if log:
            log(f"step {t}: why {why.tolist()} held {held.tolist()} margin {out['margin'][t]:.3e} clear "
                f"{out['traj_clear'][:, t].min():.6f} sel {sel.reshape(-1).tolist()} x {x[0, :2]}")
    out["held"], out["sel_plan"], out["U"], out["x"] = held, sel_plan, U, x
    return out
