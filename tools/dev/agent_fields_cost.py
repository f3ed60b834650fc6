"""Development script (not a pytest test, not bench.py): what the field forms cost, and what a soft obstacle does to the
iteration counts.

    python tools/dev/agent_fields_cost.py [B] [--pacejka]

At B agents (default 65 536), kinematic model N = 20 (--pacejka: Pacejka N = 12), shared straight centerline,
U0 = [1, 0] x N, the blocking solve time of
  (a) no table,
  (b) a field table with A = 0 in every source (P = 1 and P = B rows; B = 65 536, N = 20: 168 MB) -- the same arithmetic
      as (a) bit for bit (asserted: U and the statistics are equal), so (b) / (a) is the price of the field forms: the
      rate forms on the handle's own zero weights, one load and one branch per source and stage, the out-of-line exp
      never called,
  (c) one live source per stage 0.6 ahead of every agent, A = 0.3, sigma = (0.15, 0.06), and (d) both slots live with
      alpha = 0.5: other problems, reported with their iteration counts (mean inner iterations, the slowest agent) and
      compared with nothing -- (c) and (d) against (b) is what two exp calls per stage and the stiffer problem cost.
One warm-up solve per variant, then three passes over the variants (so that they alternate), one timed blocking solve
each (host clock); the figure of a variant is the median of its three.  Then one more solve each in profile mode for
last_solve_info()'s per-kernel milliseconds."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args and args[0].isdigit() else 65536
model = 1 if "--pacejka" in sys.argv else 0
N = 12 if model else 20
dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)

rng = np.random.default_rng(0)
cols = [rng.uniform(0, 5, B), rng.uniform(-.3, .3, B), rng.uniform(-.3, .3, B), rng.uniform(.3, 1.5, B)]
if model:
    cols += [rng.uniform(-.03, .03, B), rng.uniform(-.3, .3, B)]
x = np.stack(cols, 1)
cl = np.array([[i / 10 - 0.1, 0] for i in range(100)]).ravel(order="F")
X0, CL, U0 = T(x), T(cl), T(np.tile([1., 0.], (B, N)))
print("library", _lib.LIB_PATH, _lib.library_hash()[:16], " model", model, " B", B, " N", N)

cfg = mp.default_config(model, N, max_total_inner=1000, max_total_evals=4000)
def sources(P, live, alpha):
    """[P, N, 2, 8]: `live` of the two slots hold a source 0.6 (slot 1: 1.0) ahead of agent p and 0.03 beside its path"""
    tab = np.zeros((P, N, _lib.NFIELD, _lib.NFSRC))
    for j in range(live):
        tab[:, :, j, 0] = (x[:P, 0] + (0.6, 1.0)[j])[:, None]
        tab[:, :, j, 1] = (x[:P, 1] + (0.03, -0.03)[j])[:, None]
        tab[:, :, j, 2], tab[:, :, j, 4] = 1.0, 0.3
        tab[:, :, j, 5], tab[:, :, j, 6], tab[:, :, j, 7] = 1 / (2 * 0.15 ** 2), 1 / (2 * 0.06 ** 2), alpha
    return tab.reshape(P, -1)


ident = np.arange(B)
cases = [("(a) no table", None, None),
         ("(b) A = 0, P = 1", sources(1, 0, 0.0), np.zeros(B, dtype=np.int64)),
         ("(b) A = 0, P = %d" % B, sources(B, 0, 0.0), rng.permutation(B)),
         ("(c) one source per stage", sources(B, 1, 0.0), ident),
         ("(d) two sources, alpha = 0.5", sources(B, 2, 0.5), ident)]

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
        eng.set_agent_fields(*keep)
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
        assert torch.equal(U, Ua) and torch.equal(st, sta), name + ": a table of zeros must change no bit"
    print("%-32s ms %s  median/(a) %.3f  converged %.4f  inner mean %.1f  slowest %d  evals mean %.1f  rounds %d  solo agents %d"
          % (name, " ".join("%.1f" % (1e3 * t) for t in times), float(np.median(times)) / base,
             float((st[:, 0] == 1).double().mean()), float(st[:, 2].mean()), int(st[:, 2].max()), float(st[:, 7].mean()),
             info["rounds"], info["solo_agents"]))
    print("      kernel ms (profile mode, one-stream sums): " +
          "  ".join("%s %.1f" % (k, v) for k, v in info["kernel_ms"].items()) + "  solo longest %.1f" % info["solo_longest_ms"], flush=True)
    eng.close()
