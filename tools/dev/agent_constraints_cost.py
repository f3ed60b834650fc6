"""Development script (not a pytest test, not bench.py): what the per-agent constraint table costs.

    python tools/dev/agent_constraints_cost.py [B]

At B agents (default 65 536) on BASELINE config 3's workload -- kinematic model, N = 40, lane band of halfwidth 0.05,
per-agent lane-change centerlines, U0 = [1, 0] x N (tools/dev/config3.py) -- the blocking solve time
  (a) without a table,
  (b) with a table whose rows all equal the handle's constraint data, P = 1 and P = 4 096 under random indices -- the
      same solve bit for bit (asserted here), so (b) / (a) is the price of the mechanism on identical arithmetic,
  (c) with four lane widths (0.05, 0.03, 0.04, 0.07; index b % 4): other problems, reported with their rounds and
      compared with nothing.
One warm-up solve per variant, then three passes over the variants (so that they alternate), one timed blocking solve
each (host clock); the figure of a variant is the median of its three.  Then one more solve each in profile mode for
last_solve_info()'s per-kernel milliseconds (HIP events, sampled every 8th round)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib
from model_predictive_control_amd.bezier_curves import lane_change_centerlines

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args and args[0].isdigit() else 65536
N = 40
P = min(4096, B)
dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)

cfg = mp.default_config(0, N, constr_mode=2, lane_halfwidth=0.05, max_total_inner=1000, max_total_evals=4000, Sigma0=10.0)
tabs = lane_change_centerlines(S=100)
rng = np.random.default_rng(0)
x = np.stack([rng.uniform(0, 2, B), rng.uniform(-.02, .02, B), rng.uniform(-.05, .05, B), rng.uniform(.5, 1.2, B)], 1)
X0, cl, ci = T(x), T(tabs), T(rng.integers(0, tabs.shape[0], B), torch.int32)
U0 = T(np.tile([1., 0.], (B, N)))
print("library", _lib.LIB_PATH, _lib.library_hash()[:16], " B", B, " N", N)


def timed(eng):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    U, lam, st = eng.solve(X0, cl, U0, cl_index=ci)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, U, lam, st


cases = [("(a) no table", None, None),
         ("(b) equal rows, P = 1", _lib.constraint_rows(cfg, 1), np.zeros(B, dtype=np.int64)),
         ("(b) equal rows, P = %d" % P, _lib.constraint_rows(cfg, P), rng.integers(0, P, B)),
         ("(c) four lane widths", _lib.constraint_rows(cfg, 4, lane_halfwidth=[0.05, 0.03, 0.04, 0.07]), np.arange(B) % 4)]
engs = []
for name, tab, idx in cases:                   # one engine per variant, so that the passes below only solve
    eng = mp.BatchedMPC(cfg, dev)
    keep = None
    if tab is not None:
        keep = (T(tab), T(idx, torch.int32))
        eng.set_agent_constraints(*keep)
    eng.solve(X0, cl, U0, cl_index=ci)         # warm-up
    engs.append((name, eng, keep, []))
res = {}
for _ in range(3):                             # the variants alternate
    for name, eng, _, times in engs:
        t, U, lam, st = timed(eng)
        times.append(t)
        res[name] = (U, lam, st)
base = float(np.median(engs[0][3]))
for name, eng, _, times in engs:
    eng.set_profile(True)
    eng.solve(X0, cl, U0, cl_index=ci)
    info = eng.last_solve_info()
    U, lam, st = res[name]
    same = all(torch.equal(p, q) for p, q in zip(res[name], res[cases[0][0]]))
    if name.startswith("(b)"):
        assert same, name + ": equal rows must give the bits of the solve without a table"
    print("%-28s ms %s  median/(a) %.3f  same bits as (a): %s  converged %.4f  inner mean %.1f  rounds %d  solo agents %d"
          % (name, " ".join("%.1f" % (1e3 * t) for t in times), float(np.median(times)) / base, same,
             float((st[:, 0] == 1).double().mean()), float(st[:, 2].mean()), info["rounds"], info["solo_agents"]))
    print("      kernel ms (profile mode, one-stream sums): " +
          "  ".join("%s %.1f" % (k, v) for k, v in info["kernel_ms"].items()) + "  solo longest %.1f" % info["solo_longest_ms"], flush=True)
    eng.close()
