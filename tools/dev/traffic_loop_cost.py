"""Development script (not a pytest test, not bench.py): what the traffic selection and the traffic loop cost.

    python tools/dev/traffic_loop_cost.py [B] [T] [reps] [--out FILE]

At B kinematic agents (default 65 536), N = 20, constr_mode CONSTR_DISCS at the default tolerances, U0 = [1, 0] x N, the
straight centerline, synthetic states; for G = 16 and G = 64, `reps` passes alternating in one process after one warm-up of
each, host clock around blocking calls (the spread of the passes is printed with the median):
  (s) opponents_from_plans alone on the rollout of U0 (N stages; reach = +inf: every pair is a candidate) and on the states
      (one stage), 20 launches per sample, the stream drained once;
  (a) closed_loop on a bound table of zeros (radius 0: no disc acts), T steps (default 5), shift on;
  (b) closed_loop_traffic with radius 0 on the same table -- the gathered discs are vacuous, so the solves are the
      solves of (a): whether the bits of traj_x / traj_u / stats are equal is printed -- and (b) - (a) is the price of rollout,
      selection, gather and the clearance of every step.
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
Tn = int(args[1]) if len(args) > 1 else 5
reps = int(args[2]) if len(args) > 2 else 3
N, LAUNCHES = 20, 20
assert torch.cuda.is_available(), "needs a HIP device (no timing exists without one)"
assert B % 64 == 0, "B must hold whole scenes of 16 and of 64"
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


eng = mp.BatchedMPC(mp.default_config(mp.MODEL_KINEMATIC, N, constr_mode=mp.CONSTR_DISCS), dev)
x0, cl, U0 = T(synthetic_states(0, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
eng.set_agent_discs(table, torch.arange(B, dtype=torch.int32, device=dev))
radius = torch.zeros(B, dtype=torch.float64, device=dev)
X = eng.rollout(x0, U0)
fmt = lambda ts: " ".join("%.4f" % t for t in ts)
say("traffic_loop_cost: library %s, B %d kinematic agents, N %d, T %d, %d alternating repetitions, %s"
    % (_lib.library_hash()[:16], B, N, Tn, reps, torch.cuda.get_device_name(0)))


def many(fn):
    def run():
        for _ in range(LAUNCHES):
            fn()
    return run


plain = lambda: eng.closed_loop(x0, cl, U0, Tn, shift=True)
for G in (16, 64):
    sel_plans = many(lambda: eng.opponents_from_plans(X, G, radius))
    sel_now = many(lambda: eng.opponents_from_plans(x0, G, radius))
    traffic = lambda: eng.closed_loop_traffic(x0, cl, U0, Tn, G, radius, shift=True, table=table)
    ra, rb = plain(), traffic()                                         # warm-up of each, and the bits
    sel_plans(); sel_now()
    same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((ra[3], rb.traj_x), (ra[4], rb.traj_u), (ra[6], rb.stats)))
    assert not bool(table.reshape(B, N, 2, 3)[..., 2].any()) and bool((rb.traj_opp >= 0).all())
    ta, tb, tp, tn = [], [], [], []
    for _ in range(reps):
        ta.append(timed(plain)[0]); tb.append(timed(traffic)[0]); tp.append(timed(sel_plans)[0]); tn.append(timed(sel_now)[0])
    say("G = %d" % G)
    say("(s) opponents_from_plans, %d stages  s per %d launches %s -> median %.1f us each (host clock, allocation of the outputs included)"
        % (N, LAUNCHES, fmt(tp), 1e6 * np.median(tp) / LAUNCHES))
    say("(s) opponents_from_plans, 1 stage    s per %d launches %s -> median %.1f us each" % (LAUNCHES, fmt(tn), 1e6 * np.median(tn) / LAUNCHES))
    say("(a) closed_loop, zero table          s %s -> median %.2f ms/step (spread %.2f)"
        % (fmt(ta), 1e3 * np.median(ta) / Tn, 1e3 * (max(ta) - min(ta)) / Tn))
    say("(b) closed_loop_traffic, radius 0    s %s -> median %.2f ms/step (spread %.2f); same traj_x / traj_u / stats bits: %s"
        % (fmt(tb), 1e3 * np.median(tb) / Tn, 1e3 * (max(tb) - min(tb)) / Tn, same))
    say("(b) - (a), rollout + selection + gather + clearance: median - median %.3f ms/step = %.2f %% of (a)'s step"
        % (1e3 * (np.median(tb) - np.median(ta)) / Tn, 100 * (np.median(tb) / np.median(ta) - 1)))
eng.close()
