"""Development script (not a pytest test, not bench.py): what event-triggered holding in the traffic loop saves in solves
and what its trigger costs per closed-loop step.

    python tools/dev/traffic_event_cost.py [B] [T] [reps] [--out FILE]

At B kinematic agents (default 65 536), N = 20, constr_mode CONSTR_DISCS at the default tolerances: copies of the recorded
scene of tests/traffic_event_common.py (the rear car on its warm start, the slower car 0.30 ahead, reach 0.13,
clear_thr -2e-3, thr 0.05, max_hold 8) with a fourth car far ahead, so that 65 536 agents are whole scenes (G = 4), every
scene moved by a small random shift; per-agent v_ref in a parameter table; `reps` passes alternating in one process after
one warm-up of each, host clock around blocking calls (the spread of the passes is printed with the median):
  (s) the two launches a step adds to closed_loop_traffic's -- rollout_held (step 2), opponent_trigger (step 3: the
      held-window selection and the rule; how many agents each rule fires is printed) -- and the full-window
      opponents_from_plans both loops make (step 5), each 20 launches per sample, the stream drained once;
  (a) closed_loop_traffic of this build, T steps (default 8: (a) takes seconds per step on this scene), shift on: every agent solved at every step;
  (b) closed_loop_traffic_event at thr = 0: the same solves (the bits of traj_x / traj_u are compared and printed), so
      (b) - (a) is the price of the event machinery per step;
  (c) closed_loop_traffic_event at thr = 0.05, max_hold = 8, watch = 3: solves per agent and step, ms per step, the steps
      with a solve and the smallest realised clearance beside (a)'s.
Prints; --out FILE appends the same lines to FILE (profiles/r23_traffic_event.txt keeps a run)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib
import discs_common as D
import traffic_event_common as TE

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path:
    args.remove(out_path)
B = int(args[0]) if len(args) > 0 else 65536
Tn = int(args[1]) if len(args) > 1 else 8
reps = int(args[2]) if len(args) > 2 else 2
N, G, LAUNCHES = TE.EVENT_N, 4, 20
assert torch.cuda.is_available(), "needs a HIP device (no timing exists without one)"
assert B % G == 0, "B must hold whole scenes of 4"
dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def say(line):
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def many(fn):
    def run():
        for _ in range(LAUNCHES):
            fn()
    return run


S = B // G
rng = np.random.default_rng(G)
scene = np.concatenate([TE.EVENT_X0, [[6.0, 0.5, 0.0, 0.5]]])
shift = np.stack([rng.uniform(-0.02, 0.02, S), rng.uniform(-0.005, 0.005, S), np.zeros(S), np.zeros(S)], 1)
X0 = (scene[None] + shift[:, None]).reshape(B, 4)
v_ref = np.tile(np.append(TE.EVENT_VREF, 0.5), S)
U0h = np.tile(np.concatenate([TE.EVENT_U0, np.zeros((1, 2 * N))]), (S, 1))
eng = mp.BatchedMPC(mp.default_config(mp.MODEL_KINEMATIC, N, constr_mode=mp.CONSTR_DISCS), dev)
ar = torch.arange(B, dtype=torch.int32, device=dev)
eng.set_agent_params(T(_lib.param_rows(eng.cfg, B, v_ref=v_ref)), ar)
x0, cl, U0, radius = T(X0), T(D.line_centerline()), T(U0h), T(np.tile(np.append(TE.EVENT_RADII, TE.EVENT_RADIUS), S))
table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
eng.set_agent_discs(table, ar)
fmt = lambda ts: " ".join("%.4f" % t for t in ts)
say("traffic_event_cost: library %s, B %d kinematic agents, N %d, G %d, T %d, %d alternating repetitions, %s"
    % (_lib.library_hash()[:16], B, N, G, Tn, reps, torch.cuda.get_device_name(0)))
held = T(rng.integers(1, 8, B), torch.int32)
plan = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
REACH, CTHR = TE.EVENT_REACH, TE.EVENT_CLEAR_THR

Ustraight = T(np.tile([1., 0.], (B, N)))
X = eng.rollout_held(x0, Ustraight, held)
steps = (("rollout_held (step 2)", many(lambda: eng.rollout_held(x0, Ustraight, held))),
         ("opponent_trigger (step 3)", many(lambda: eng.opponent_trigger(X, held, plan, G, radius, REACH, CTHR, 3))),
         ("opponents_from_plans, N stages (step 5)", many(lambda: eng.opponents_from_plans(X, G, radius, REACH))))
every = lambda: eng.closed_loop_traffic(x0, cl, U0, Tn, G, radius, REACH, shift=True, table=table)
event = lambda thr: (lambda: eng.closed_loop_traffic_event(x0, cl, U0, Tn, G, radius, TE.EVENT_W, thr, TE.EVENT_MAX_HOLD, reach=REACH,
                                                           clear_thr=CTHR, watch=3, shift=True, table=table))
for _, fn in steps:
    fn()
_, why1, _, _ = eng.opponent_trigger(X, held, plan, G, radius, REACH, CTHR, 3)
say("opponent_trigger on straight plans (U = [1, 0] x N), held 1 .. 7, opp_plan = none: clearance fires %d, new opponent %d of %d agents"
    % (int((why1 & 2).bool().sum()), int((why1 & 4).bool().sum()), B))
t1, ra = timed(every)                                                   # warm-up of each, and the bits
say("warm-up (a) %.2f s" % t1)
t1, rb = timed(event(0.0))
say("warm-up (b) %.2f s" % t1)
same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((ra.traj_x, rb.traj_x), (ra.traj_u, rb.traj_u)))
say("warm-up (c) %.2f s" % timed(event(TE.EVENT_THR))[0])
ts = [[] for _ in steps]
ta, tb, tc = [], [], []
for _ in range(reps):
    for acc, (_, fn) in zip(ts, steps):
        acc.append(timed(fn)[0])
    t2, ra = timed(every); ta.append(t2)
    tb.append(timed(event(0.0))[0])
    t3, r3 = timed(event(TE.EVENT_THR)); tc.append(t3)
for acc, (name, _) in zip(ts, steps):
    say("(s) %-40s s per %d %s -> median %.1f us each (host clock, allocation of the outputs included)"
        % (name, LAUNCHES, fmt(acc), 1e6 * np.median(acc) / LAUNCHES))
say("(a) closed_loop_traffic                        s %s -> median %.2f ms/step (spread %.2f); solves per agent and step 1; "
    "smallest realised clearance %.3e; failures %d"
    % (fmt(ta), 1e3 * np.median(ta) / Tn, 1e3 * (max(ta) - min(ta)) / Tn, float(ra.traj_clear.min()), int(ra.failures.sum())))
say("(b) closed_loop_traffic_event, thr = 0         s %s -> median %.2f ms/step (spread %.2f); same traj_x / traj_u bits: %s"
    % (fmt(tb), 1e3 * np.median(tb) / Tn, 1e3 * (max(tb) - min(tb)) / Tn, same))
say("(b) - (a), the event machinery: median - median %.3f ms/step = %.2f %% of (a)'s step"
    % (1e3 * (np.median(tb) - np.median(ta)) / Tn, 100 * (np.median(tb) / np.median(ta) - 1)))
say("(c) event loop, thr %.2f, max_hold %d, watch 3  s %s -> median %.2f ms/step; solves per agent and step %.3f; agents solved "
    "per step %s; smallest realised clearance %.3e; failures %d"
    % (TE.EVENT_THR, TE.EVENT_MAX_HOLD, fmt(tc), 1e3 * np.median(tc) / Tn, float(r3.solve_count.sum()) / (B * Tn),
       r3.solved.sum(0).tolist(), float(r3.traj_clear.min()), int(r3.failures.sum())))
eng.close()
