"""Development script (not a pytest test, not bench.py): what lap driving costs.

    python tools/dev/track_loop_cost.py [B] [T] [reps] [--out FILE]

At B kinematic agents (default 65 536), N = 20, default configuration, U0 = [1, 0] x N, w = 1, thr = 0.02, max_hold = 10,
shift = 1, T steps (default 20), three passes alternating in one process after one warm-up of each, host clock around
blocking calls:
  (a) closed_loop_event on the straight centerline, every agent on row 0 of a one-row table (cl_index of zeros);
  (b) closed_loop_track on the same centerline as a one-window open track (L = S): the same solves -- the bits of
      traj_x / traj_u / stats are asserted equal -- so (b) - (a) is the price of the select step;
  (c) closed_loop_track on the stadium (L = 388, stride 4, lead 10: R = 97 windows), the agents spread along it, the grid
      tables built once: the rows are spread over 97 centerline rows in place of one shared row, and K1b loses its LDS
      copy of the points -- another workload than (a) (curves, other states), so its time per SOLVE is the figure to
      read beside (a)'s, not its time per step.
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
from model_predictive_control_amd.tracks import stadium_track
from conftest import straight_centerline, synthetic_states

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path:
    args.remove(out_path)
B = int(args[0]) if len(args) > 0 else 65536
Tn = int(args[1]) if len(args) > 1 else 20
reps = int(args[2]) if len(args) > 2 else 3
N, thr, max_hold = 20, 0.02, 10
assert torch.cuda.is_available(), "needs a HIP device (no timing exists without one)"
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


cfg = mp.default_config(mp.MODEL_KINEMATIC, N)
eng = mp.BatchedMPC(cfg, dev)
w = np.ones(4)
U0 = T(np.tile([1., 0.], (B, N)))
dist = T(np.random.default_rng(17).normal(0, 4e-3, (B, Tn, 4)) * [1, 1, 0.5, 2])
say("track_loop_cost: library %s, B %d kinematic agents, N %d, T %d, thr %g, max_hold %d, %d alternating repetitions, %s"
    % (_lib.library_hash()[:16], B, N, Tn, thr, max_hold, reps, torch.cuda.get_device_name(0)))

# (a), (b): the straight centerline
Xs = T(synthetic_states(0, B, seed=21))
one = eng.track_windows(T(straight_centerline()), 4, 10, False)
zero = torch.zeros(B, dtype=torch.int32, device=dev)
event = lambda: eng.closed_loop_event(Xs, one.win, U0, Tn, w, thr, max_hold, shift=True, disturbance=dist, cl_index=zero)
track1 = lambda: eng.closed_loop_track(Xs, one, U0, Tn, w, thr, max_hold, zero, shift=True, disturbance=dist)

# (c): the stadium
st = stadium_track(10, 3, 0.1)
Ls = st.size // 2
rng = np.random.default_rng(13)
i = rng.integers(0, Ls, B)
tx, ty = st[(i + 1) % Ls] - st[i], st[Ls + (i + 1) % Ls] - st[Ls + i]
nrm = np.hypot(tx, ty)
d = rng.uniform(-.3, .3, B)
Xc = T(np.stack([st[i] - d * ty / nrm, st[Ls + i] + d * tx / nrm, np.arctan2(ty, tx) + rng.uniform(-.3, .3, B),
                 rng.uniform(.3, 1.5, B)], 1))
t_build, lap = timed(lambda: eng.track_windows(T(st), 4, 10, True))
ci0 = eng.track_locate(Xc, lap)
trackR = lambda: eng.closed_loop_track(Xc, lap, U0, Tn, w, thr, max_hold, ci0, shift=True, disturbance=dist)
say("(c) track_windows of the stadium (gather of %d windows + their grid tables, once): %.1f ms" % (lap.rows, 1e3 * t_build))

ra, rb, rc = event(), track1(), trackR()                               # warm-up of each, and the bits
same = (torch.equal(ra.traj_x.view(torch.int64), rb.traj_x.view(torch.int64)) and
        torch.equal(ra.traj_u.view(torch.int64), rb.traj_u.view(torch.int64)) and
        torch.equal(ra.stats.view(torch.int64), rb.stats.view(torch.int64)) and torch.equal(ra.solved, rb.solved))
assert same, "a one-window track must give the bits of closed_loop_event"
ta, tb, tc = [], [], []
for _ in range(reps):
    ta.append(timed(event)[0]); tb.append(timed(track1)[0]); tc.append(timed(trackR)[0])
sa, sc = float(ra.solved.float().sum()), float(rc.solved.float().sum())
fmt = lambda ts: " ".join("%.3f" % t for t in ts)
say("(a) closed_loop_event, one row         s %s -> median %.2f ms/step; agent-steps solved %.4f"
    % (fmt(ta), 1e3 * np.median(ta) / Tn, sa / (B * Tn)))
say("(b) closed_loop_track, one window      s %s -> median %.2f ms/step; same traj_x / traj_u / stats / solved bits: %s"
    % (fmt(tb), 1e3 * np.median(tb) / Tn, same))
say("(b) - (a), the select step: median - median %.3f ms/step = %.2f %% of (a)'s step"
    % (1e3 * (np.median(tb) - np.median(ta)) / Tn, 100 * (np.median(tb) / np.median(ta) - 1)))
say("(c) closed_loop_track, stadium R = %d   s %s -> median %.2f ms/step; agent-steps solved %.4f, solves not converged %d"
    % (lap.R, fmt(tc), 1e3 * np.median(tc) / Tn, sc / (B * Tn), int(rc.failures.sum())))
say("    per solved agent-step: (a) %.3f us, (c) %.3f us; agents on another row at the end of (c): %.3f"
    % (1e6 * np.median(ta) / sa, 1e6 * np.median(tc) / sc, float((rc.cl_index != ci0).float().mean())))
eng.close()
