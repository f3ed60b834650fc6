"""Development script (not a pytest test, not bench.py): what the selection and the gather of the scripted obstacles cost
per closed-loop step, against the solve.

    python tools/dev/obstacles_cost.py [B] [T] [reps] [--out FILE]

At B kinematic agents (default 65 536), N = 20, constr_mode CONSTR_DISCS at the default tolerances, U0 = [1, 0] x N, the
straight centerline, synthetic states; for (G, K) = (16, 16) and (64, 64), tracks of Lt = 220 samples; `reps` passes
alternating in one process after one warm-up of each, host clock around blocking calls (the spread of the passes is
printed with the median):
  (s) obstacles_select on the rollout of U0 (N stages; reach = +inf) followed by discs_from_obstacles into the bound
      table, and obstacles_select on the states (one stage), 20 launches per sample, the stream drained once;
  (a) closed_loop on a bound table of zeros, T steps (default 5), shift on;
  (b) closed_loop_obstacles with every sample absent (r = 0) on the same table -- the gathered rows are zeros, so the
      solves are the solves of (a): whether the bits of traj_x / traj_u / stats are equal is printed -- and (b) - (a) is the
      price of rollout, selection, gather and the clearance of every step;
  (c) closed_loop_obstacles with the obstacles present (r = 0.1, random straight paths through the agents' region): the
      solves differ, the figure is for orientation only.
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
N, LT, LAUNCHES = 20, 220, 20
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


def many(fn):
    def run():
        for _ in range(LAUNCHES):
            fn()
    return run


eng = mp.BatchedMPC(mp.default_config(mp.MODEL_KINEMATIC, N, constr_mode=mp.CONSTR_DISCS), dev)
x0, cl, U0 = T(synthetic_states(0, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
table = torch.zeros(B, 6 * N, dtype=torch.float64, device=dev)
eng.set_agent_discs(table, torch.arange(B, dtype=torch.int32, device=dev))
X = eng.rollout(x0, U0)
fmt = lambda ts: " ".join("%.4f" % t for t in ts)
say("obstacles_cost: library %s, B %d kinematic agents, N %d, Lt %d, T %d, %d alternating repetitions, %s"
    % (_lib.library_hash()[:16], B, N, LT, Tn, reps, torch.cuda.get_device_name(0)))
plain = lambda: eng.closed_loop(x0, cl, U0, Tn, shift=True)
for G, K in ((16, 16), (64, 64)):
    rng = np.random.default_rng(G)
    S = B // G
    p0 = np.stack([rng.uniform(0, 5, (S, K)), rng.uniform(-.3, .3, (S, K))], -1)
    v = rng.uniform(-0.02, 0.02, (S, K, 2))
    centres = p0[:, :, None, :] + np.arange(LT)[None, None, :, None] * v[:, :, None, :]
    present = T(_lib.obstacle_tracks(eng.cfg, centres=centres, radii=0.1))
    absent = present.clone()
    absent[..., 2] = 0.0
    say("G = %d, K = %d: the obstacle table is %.1f MB (%.1f KB per scene)" % (G, K, present.numel() * 8 / 1e6, K * LT * 24 / 1e3))

    def sel_gather():
        sel, _ = eng.obstacles_select(X, G, present, 1)
        eng.discs_from_obstacles(sel, G, present, 1, out=table)
    step = many(sel_gather)
    sel_now = many(lambda: eng.obstacles_select(x0, G, present, 1))
    loop_absent = lambda: eng.closed_loop_obstacles(x0, cl, U0, Tn, G, absent, shift=True, table=table)
    loop_present = lambda: eng.closed_loop_obstacles(x0, cl, U0, Tn, G, present, 0.5, shift=True, table=table)
    step(); sel_now()
    table.zero_()
    ra, rb = plain(), loop_absent()                                     # warm-up of each, and the bits
    same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((ra[3], rb.traj_x), (ra[4], rb.traj_u), (ra[6], rb.stats)))
    assert not bool(table.any()) and bool((rb.traj_sel == -1).all())
    ta, tb, tc, ts, tn = [], [], [], [], []
    for _ in range(reps):
        table.zero_()
        ta.append(timed(plain)[0]); tb.append(timed(loop_absent)[0]); ts.append(timed(step)[0]); tn.append(timed(sel_now)[0])
    for _ in range(reps):
        tc.append(timed(loop_present)[0])
    say("(s) obstacles_select (%d stages) + discs_from_obstacles  s per %d %s -> median %.1f us a pair (host clock, allocation of the outputs included)"
        % (N, LAUNCHES, fmt(ts), 1e6 * np.median(ts) / LAUNCHES))
    say("(s) obstacles_select, 1 stage                            s per %d %s -> median %.1f us each" % (LAUNCHES, fmt(tn), 1e6 * np.median(tn) / LAUNCHES))
    say("(a) closed_loop, zero table                  s %s -> median %.2f ms/step (spread %.2f)"
        % (fmt(ta), 1e3 * np.median(ta) / Tn, 1e3 * (max(ta) - min(ta)) / Tn))
    say("(b) closed_loop_obstacles, all samples absent s %s -> median %.2f ms/step (spread %.2f); same traj_x / traj_u / stats bits: %s"
        % (fmt(tb), 1e3 * np.median(tb) / Tn, 1e3 * (max(tb) - min(tb)) / Tn, same))
    say("(b) - (a), rollout + selection + gather + clearance: median - median %.3f ms/step = %.2f %% of (a)'s step"
        % (1e3 * (np.median(tb) - np.median(ta)) / Tn, 100 * (np.median(tb) / np.median(ta) - 1)))
    say("(c) closed_loop_obstacles, obstacles present  s %s -> median %.2f ms/step (other solves than (a): orientation only)"
        % (fmt(tc), 1e3 * np.median(tc) / Tn))
eng.close()
