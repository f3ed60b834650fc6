"""Development script (not a pytest test, not bench.py): what the event-triggered closed loop costs and saves.

    python tools/dev/event_loop_cost.py [B] [T] [reps] [--out FILE]

At B kinematic agents (default 65 536), N = 20, default configuration, straight centerline, U0 = [1, 0] x N, T steps
(default 40), runs alternating in one process after one warm-up of each, host clock around blocking calls:
  (a) closed_loop_event at thr = 0 (every agent solved at every step: mpc_closed_loop's arithmetic, checked here bit
      for bit) against mpc_closed_loop -- the difference is the price of trigger, compaction, gather, scatter and the
      extra host wait per step; the compaction / gather / scatter kernels are also timed alone with HIP events through
      solve_active on a mask of zeros (no solver kernels run);
  (b) closed_loop_event with a plant that accelerates 3 % less and has 10 % more friction than the controller's
      model (per-agent table, plant_index), w = 1, max_hold = 10, shift = 1, at thr = 0.01 and 0.03: time per step
      and the fraction of agent-steps solved, against thr = 0 under the same table.
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
Tn = int(args[1]) if len(args) > 1 else 40
reps = int(args[2]) if len(args) > 2 else 3
N = 20
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
X0, cl, U0 = T(synthetic_states(0, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
w = np.ones(4)
say("event_loop_cost: library %s, B %d kinematic agents, N %d, T %d, %d alternating repetitions, %s"
    % (_lib.library_hash()[:16], B, N, Tn, reps, torch.cuda.get_device_name(0)))

# ---- one blocking solve, for scale
eng.solve(X0, cl, U0)
ts = [timed(lambda: eng.solve(X0, cl, U0))[0] for _ in range(3)]
say("one blocking solve of the batch from U0: ms %s" % " ".join("%.1f" % (1e3 * t) for t in ts))

# ---- (a) thr = 0 against mpc_closed_loop
loop = lambda: eng.closed_loop(X0, cl, U0, Tn, shift=True)
event = lambda thr: (lambda: eng.closed_loop_event(X0, cl, U0, Tn, w, thr, 10, shift=True))
ref, ev = loop(), event(0.0)()                                   # warm-up of both, and the bits
same = torch.equal(ref[3], ev.traj_x) and torch.equal(ref[4], ev.traj_u) and torch.equal(ref[5], ev.failures)
tl, te = [], []
for _ in range(reps):
    tl.append(timed(loop)[0]); te.append(timed(event(0.0))[0])
say("(a) mpc_closed_loop        s %s  -> best %.1f ms/step" % (" ".join("%.3f" % t for t in tl), 1e3 * min(tl) / Tn))
say("(a) closed_loop_event thr=0 s %s  -> best %.1f ms/step; same traj_x / traj_u / failures bits: %s"
    % (" ".join("%.3f" % t for t in te), 1e3 * min(te) / Tn, same))
say("(a) price per step (best - best) %.2f ms = %.2f %% of mpc_closed_loop's step; median - median %.2f ms"
    % (1e3 * (min(te) - min(tl)) / Tn, 100 * (min(te) / min(tl) - 1), 1e3 * (np.median(te) - np.median(tl)) / Tn))
zeros = torch.zeros(B, dtype=torch.int32, device=dev)
ones = torch.ones(B, dtype=torch.int32, device=dev)
st = torch.zeros(B, 8, dtype=torch.float64, device=dev)
eng.solve_active(X0, cl, U0, zeros, stats=st, inplace=True)
tz = [timed(lambda: eng.solve_active(X0, cl, U0, zeros, stats=st, inplace=True))[0] for _ in range(20)]
say("(a) solve_active on a mask of zeros (trigger-free: count, list, gather, the count's copy and wait; no solver "
    "kernel): median %.3f ms, best %.3f ms per call (includes the centerline grid rebuild of the Python front end)"
    % (1e3 * np.median(tz), 1e3 * min(tz)))
Uc = U0.clone()
eng.solve_active(X0, cl, Uc, ones, stats=st, inplace=True)
t1 = [timed(lambda: eng.solve_active(X0, cl, U0.clone(), ones, stats=st, inplace=True))[0] for _ in range(3)]
say("(a) solve_active on a mask of ones: ms %s (the blocking solve above + gather + scatter of every row)"
    % " ".join("%.1f" % (1e3 * t) for t in t1))

# ---- (b) a mismatched plant
tab = T(_lib.param_rows(cfg, 2, accel=[2.0, 2.0 * 0.97], friction=[1.0, 1.1]))
eng.set_agent_params(tab, zeros, ones)
for thr in (0.0, 0.01, 0.03):
    event(thr)()
res = {thr: [] for thr in (0.0, 0.01, 0.03)}
frac = {}
for _ in range(reps):
    for thr in res:
        t, r = timed(event(thr))
        res[thr].append(t)
        frac[thr] = (float(r.solved.float().mean()), int(r.failures.sum()), float(r.solved[:, 1:].float().mean()))
for thr, ts in res.items():
    say("(b) plant accel x0.97 friction x1.1, thr %-5g s %s  -> best %.1f ms/step (%.2fx the thr = 0 loop's); agent-steps "
        "solved %.4f (after step 0: %.4f), solves not converged %d"
        % (thr, " ".join("%.3f" % t for t in ts), 1e3 * min(ts) / Tn, min(ts) / min(res[0.0]), frac[thr][0], frac[thr][2],
           frac[thr][1]))
eng.close()
