"""Development script (not a pytest test, not bench.py): what event-triggered holding among scripted obstacles saves in
solves and what its trigger costs per closed-loop step.

    python tools/dev/obstacles_event_cost.py [B] [T] [reps] [--out FILE]

At B kinematic agents (default 65 536), N = 20, constr_mode CONSTR_DISCS at the default tolerances, U0 = [1, 0] x N, the
straight centerline, synthetic states, scenes of (G, K) = (16, 16), tracks of Lt = 220 samples, reach 0.5; `reps` passes
alternating in one process after one warm-up of each, host clock around blocking calls (the spread of the passes is printed
with the median):
  (s) on obstacles that are present (r = 0.1, random straight paths through the agents' region): the two launches a step
      adds to closed_loop_obstacles' -- rollout_held (step 2), obstacle_trigger (step 3: the held-window selection and the
      rule; how many agents each rule fires is printed) -- and the full-window obstacles_select both loops make (step 6),
      each 20 launches per sample, the stream drained once;
  the loops run with every sample absent (r = 0), as tools/dev/obstacles_cost.py times its loop: the synthetic states are not
  placed with regard to the discs, and solves that start inside one run to their iteration limits (seconds per step, which
  says nothing about the loop); with the rows all zero the solves are closed_loop's --
  (a) closed_loop_obstacles, T steps (default 16), shift on: every agent solved at every step;
  (b) closed_loop_obstacles_event at thr = 0: the same solves (the bits of traj_x / traj_u are compared and printed), so
      (b) - (a) is the price of the event machinery per step -- trigger, held rollout, rule, shift, compaction, gather /
      scatter of the masked solve;
  (c) closed_loop_obstacles_event at thr = 0.05, max_hold = 8, watch = 3, no disturbance: solves per agent and step and ms
      per step -- what holding saves when nothing makes the rule fire.
Prints; --out FILE appends the same lines to FILE."""
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
from conftest import straight_centerline, synthetic_states

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path:
    args.remove(out_path)
B = int(args[0]) if len(args) > 0 else 65536
Tn = int(args[1]) if len(args) > 1 else 16
reps = int(args[2]) if len(args) > 2 else 3
N, LT, LAUNCHES, G, K, REACH = 20, 220, 20, 16, 16, 0.5
assert torch.cuda.is_available(), "needs a HIP device (no timing exists without one)"
assert B % G == 0, "B must hold whole scenes of 16"
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


eng = mp.BatchedMPC(mp.default_config(mp.MODEL_KINEMATIC, N, constr_mode=mp.CONSTR_DISCS), dev)
x0, cl, U0 = T(synthetic_states(0, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
eng.set_agent_discs(table, torch.arange(B, dtype=torch.int32, device=dev))
fmt = lambda ts: " ".join("%.4f" % t for t in ts)
say("obstacles_event_cost: library %s, B %d kinematic agents, N %d, G %d, K %d, Lt %d, T %d, %d alternating repetitions, %s"
    % (_lib.library_hash()[:16], B, N, G, K, LT, Tn, reps, torch.cuda.get_device_name(0)))
rng = np.random.default_rng(G)
S = B // G
p0 = np.stack([rng.uniform(0, 5, (S, K)), rng.uniform(-.3, .3, (S, K))], -1)
v = rng.uniform(-0.02, 0.02, (S, K, 2))
centres = p0[:, :, None, :] + np.arange(LT)[None, None, :, None] * v[:, :, None, :]
obs = T(_lib.obstacle_tracks(eng.cfg, centres=centres, radii=0.1))
absent = obs.clone()
absent[..., 2] = 0.0
held = T(rng.integers(1, 8, B), torch.int32)
plan = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
w = np.ones(4)

X = eng.rollout_held(x0, U0, held)
steps = (("rollout_held (step 2)", many(lambda: eng.rollout_held(x0, U0, held))),
         ("obstacle_trigger (step 3)", many(lambda: eng.obstacle_trigger(X, held, plan, G, obs, 1, REACH, -1e-3, 3))),
         ("obstacles_select, N stages (step 6)", many(lambda: eng.obstacles_select(X, G, obs, 1, REACH))))
every = lambda: eng.closed_loop_obstacles(x0, cl, U0, Tn, G, absent, REACH, shift=True, table=table)
event = lambda thr: (lambda: eng.closed_loop_obstacles_event(x0, cl, U0, Tn, G, absent, w, thr, 8, reach=REACH, clear_thr=-1e-3,
                                                             watch=3, shift=True, table=table))
for _, fn in steps:
    fn()
_, why1, _, _ = eng.obstacle_trigger(X, held, plan, G, obs, 1, REACH, -1e-3, 3)
say("obstacle_trigger on the present obstacles, held 1 .. 7, sel_plan = none: clearance fires %d, new obstacle %d of %d agents"
    % (int((why1 & 2).bool().sum()), int((why1 & 4).bool().sum()), B))
t1, ra = timed(every)                                                   # warm-up of each, and the bits
say("warm-up (a) %.2f s" % t1)
t1, rb = timed(event(0.0))
say("warm-up (b) %.2f s" % t1)
same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((ra.traj_x, rb.traj_x), (ra.traj_u, rb.traj_u)))
say("warm-up (c) %.2f s" % timed(event(0.05))[0])
ts = [[] for _ in steps]
ta, tb, tc = [], [], []
for _ in range(reps):
    for acc, (_, fn) in zip(ts, steps):
        acc.append(timed(fn)[0])
    ta.append(timed(every)[0]); tb.append(timed(event(0.0))[0])
    t3, r3 = timed(event(0.05)); tc.append(t3)
for acc, (name, _) in zip(ts, steps):
    say("(s) %-38s s per %d %s -> median %.1f us each (host clock, allocation of the outputs included)"
        % (name, LAUNCHES, fmt(acc), 1e6 * np.median(acc) / LAUNCHES))
say("(a) closed_loop_obstacles                      s %s -> median %.2f ms/step (spread %.2f)"
    % (fmt(ta), 1e3 * np.median(ta) / Tn, 1e3 * (max(ta) - min(ta)) / Tn))
say("(b) closed_loop_obstacles_event, thr = 0       s %s -> median %.2f ms/step (spread %.2f); same traj_x / traj_u bits: %s"
    % (fmt(tb), 1e3 * np.median(tb) / Tn, 1e3 * (max(tb) - min(tb)) / Tn, same))
say("(b) - (a), the event machinery: median - median %.3f ms/step = %.2f %% of (a)'s step"
    % (1e3 * (np.median(tb) - np.median(ta)) / Tn, 100 * (np.median(tb) / np.median(ta) - 1)))
say("(c) event loop, thr 0.05, max_hold 8, watch 3  s %s -> median %.2f ms/step; solves per agent and step %.3f (every step: 1); "
    "steps with a solve %s; failures %d (a: %d)"
    % (fmt(tc), 1e3 * np.median(tc) / Tn, float(r3.solve_count.sum()) / (B * Tn), r3.solved.any(0).to(torch.int32).tolist(),
       int(r3.failures.sum()), int(ra.failures.sum())))
eng.close()
