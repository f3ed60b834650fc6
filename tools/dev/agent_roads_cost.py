"""Development script (not a pytest test, not bench.py): what the road forms cost, and what a lane change does to the
iteration counts.

    python tools/dev/agent_roads_cost.py [B] [--package-root DIR]

At B agents (default 65 536), kinematic model N = 20, shared straight centerline, U0 = [1, 0] x N, the blocking solve
time of
  (a) no road table,
  (b) a road table of zero weights (P = B rows, the other words drawn at random; B = 65 536, N = 20: 84 MB) -- the same
      arithmetic as (a) bit for bit (asserted: U and the statistics are equal), so (b) / (a) is the price of the road
      forms: the rate and field forms on the handle's own zeros, four loads and four branches per stage,
  (c) the `change` scene of tests/road_common.py on every agent (off = 0 for k < 6, then -0.10; w_off = 5): another
      problem, reported with its iteration counts and compared with nothing.
--package-root DIR imports the package from another tree (the parent commit's, built there): a library without
mpc_set_agent_roads runs (a) alone, which is the base the three are set against in the same session.
One warm-up solve per variant, then three passes over the variants (so that they alternate), one timed blocking solve
each (host clock); the figure of a variant is the median of its three.  Then one more solve each in profile mode for
last_solve_info()'s per-kernel milliseconds."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--package-root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, ROOT)

import numpy as np
import torch

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib

args = [a for a in sys.argv[1:] if a.isdigit()]
B = int(args[0]) if args else 65536
model, N = 0, 20
dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)

rng = np.random.default_rng(0)
x = np.stack([rng.uniform(0, 5, B), rng.uniform(-.3, .3, B), rng.uniform(-.3, .3, B), rng.uniform(.3, 1.5, B)], 1)
cl = np.array([[i / 10 - 0.1, 0] for i in range(100)]).ravel(order="F")
X0, CL, U0 = T(x), T(cl), T(np.tile([1., 0.], (B, N)))
has_roads = hasattr(mp.BatchedMPC, "set_agent_roads")
print("library", _lib.LIB_PATH, _lib.library_hash()[:16], " model", model, " B", B, " N", N, " road table:", "yes" if has_roads else "no (base)")

cfg = mp.default_config(model, N, max_total_inner=1000, max_total_evals=4000)
cases = [("(a) no table", None, None)]
if has_roads:
    zero = np.zeros((B, N, _lib.NROAD))
    for i in (0, 2, 4, 6):
        zero[..., i] = rng.uniform(-1.0, 1.0, (B, N))
    change = _lib.road_rows(N, offset=np.where(np.arange(N) < 6, 0.0, -0.10), w_offset=5.0)
    cases += [("(b) zero weights, P = %d" % B, zero.reshape(B, -1), rng.permutation(B)),
              ("(c) lane change at stage 6", change.reshape(1, -1), np.zeros(B, dtype=np.int64))]


def timed(eng):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    U, lam, st = eng.solve(X0, CL, U0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, U, st


engs = []
for name, tab, idx in cases:                   # one engine per variant, so that the passes below only solve
    eng = mp.BatchedMPC(cfg, dev)
    keep = None
    if tab is not None:
        keep = (T(tab), T(idx, torch.int32))
        eng.set_agent_roads(*keep)
    eng.solve(X0, CL, U0)                      # warm-up
    engs.append((name, eng, keep, []))
res = {}
for _ in range(3):                             # the variants alternate
    for name, eng, _, times in engs:
        t, U, st = timed(eng)
        times.append(t)
        res[name] = (U, st)
base = float(np.median(engs[0][3]))
Ua, sta = res[cases[0][0]]
for name, eng, _, times in engs:
    eng.set_profile(True)
    eng.solve(X0, CL, U0)
    info = eng.last_solve_info()
    U, st = res[name]
    if name.startswith("(b)"):
        assert torch.equal(U, Ua) and torch.equal(st, sta), name + ": a table of zero weights must change no bit"
    print("%-32s ms %s  median/(a) %.3f  k solves/s %.1f  converged %.4f  inner mean %.1f  slowest %d  evals mean %.1f  rounds %d  solo agents %d"
          % (name, " ".join("%.1f" % (1e3 * t) for t in times), float(np.median(times)) / base, B / float(np.median(times)) / 1e3,
             float((st[:, 0] == 1).double().mean()), float(st[:, 2].mean()), int(st[:, 2].max()), float(st[:, 7].mean()),
             info["rounds"], info["solo_agents"]))
    print("      kernel ms (profile mode, one-stream sums): " +
          "  ".join("%s %.1f" % (k, v) for k, v in info["kernel_ms"].items()) + "  solo longest %.1f" % info["solo_longest_ms"], flush=True)
    eng.close()
