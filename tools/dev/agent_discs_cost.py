"""Development script (not a pytest test, not bench.py): what the keep-out discs cost.

    python tools/dev/agent_discs_cost.py [B] [--parent-lib PATH]

At B agents (default 65 536), kinematic model, N = 20, shared straight centerline, U0 = [1, 0] x N, Sigma0 = 10, the
blocking solve time of
  (a) a handle of MPC_CONSTR_LANE with a half-width of 1e6 (the lane band is never active: m = N),
  (b) a handle of MPC_CONSTR_DISCS whose discs all have r = 0 (no disc is ever active: m = 2N), P = 1 and P = B rows --
      the same minimisation as (a) with twice the multipliers; controls compared on bench.DU_METRIC (the two problems
      differ in m, so their bits need not agree), (b) / (a) is the price of the disc forms against the cheapest
      constrained problem the library had,
  (c) one standing disc ahead of every agent on its line: another problem, reported with its rounds and compared with
      nothing.
One warm-up solve per variant, then three passes over the variants (so that they alternate), one timed blocking solve
each (host clock); the figure of a variant is the median of its three.  Then one more solve each in profile mode for
last_solve_info()'s per-kernel milliseconds.
--parent-lib: the headline against the parent's library is bench.py's business (MPC_LIB_PATH=PATH python bench.py ...,
run alternately with this build's); this script only prints the command."""
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
N = 20
dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
if "--parent-lib" in sys.argv:
    lib = sys.argv[sys.argv.index("--parent-lib") + 1]
    print("headline against the parent: alternate `python bench.py --gpus 1 --steps 5 --warmup 2` with and without MPC_LIB_PATH=%s" % lib)

common = dict(max_total_inner=1000, max_total_evals=4000, Sigma0=10.0)
rng = np.random.default_rng(0)
x = np.stack([rng.uniform(0, 5, B), rng.uniform(-.3, .3, B), rng.uniform(-.3, .3, B), rng.uniform(.3, 1.5, B)], 1)
cl = np.array([[i / 10 - 0.1, 0] for i in range(100)]).ravel(order="F")
X0, CL, U0 = T(x), T(cl), T(np.tile([1., 0.], (B, N)))
print("library", _lib.LIB_PATH, _lib.library_hash()[:16], " B", B, " N", N)

dcfg = mp.default_config(0, N, constr_mode=mp.CONSTR_DISCS, **common)
lcfg = mp.default_config(0, N, constr_mode=mp.CONSTR_LANE, lane_halfwidth=1e6, **common)
ahead = np.zeros((B, N, 2, 3))
ahead[:, :, 0, 0] = (x[:, 0] + 0.6)[:, None]; ahead[:, :, 0, 1] = (0.03 * np.sign(x[:, 1] + 1e-9))[:, None]; ahead[:, :, 0, 2] = 0.1
cases = [("(a) lane band, hw 1e6", lcfg, None, None),
         ("(b) discs r = 0, P = 1", dcfg, _lib.disc_rows(dcfg, 1), np.zeros(B, dtype=np.int64)),
         ("(b) discs r = 0, P = %d" % B, dcfg, _lib.disc_rows(dcfg, B), rng.permutation(B)),
         ("(c) a standing disc ahead", dcfg, ahead.reshape(B, -1), np.arange(B))]


def timed(eng):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    U, lam, st = eng.solve(X0, CL, U0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, U, lam, st


engs = []
for name, cfg, tab, idx in cases:              # one engine per variant, so that the passes below only solve
    eng = mp.BatchedMPC(cfg, dev)
    keep = None
    if tab is not None:
        keep = (T(tab), T(idx, torch.int32))
        eng.set_agent_discs(*keep)
    eng.solve(X0, CL, U0)                      # warm-up
    engs.append((name, eng, keep, []))
res = {}
for _ in range(3):                             # the variants alternate
    for name, eng, _, times in engs:
        t, U, lam, st = timed(eng)
        times.append(t)
        res[name] = (U, lam, st)
base = float(np.median(engs[0][3]))
Ua = res[cases[0][0]][0]
for name, eng, _, times in engs:
    eng.set_profile(True)
    eng.solve(X0, CL, U0)
    info = eng.last_solve_info()
    U, lam, st = res[name]
    du = ((U - Ua).abs().max(1).values / Ua.abs().max(1).values.clamp(min=1.0)).max().item()
    if name.startswith("(b)"):
        assert not bool(lam.any()), name + ": no disc may act"
        assert du <= 1e-5, name + ": vacuous discs must give the lane band's controls (bench.DU_METRIC)"
    print("%-28s ms %s  median/(a) %.3f  dU vs (a) %.2e  converged %.4f  inner mean %.1f  rounds %d  solo agents %d"
          % (name, " ".join("%.1f" % (1e3 * t) for t in times), float(np.median(times)) / base, du,
             float((st[:, 0] == 1).double().mean()), float(st[:, 2].mean()), info["rounds"], info["solo_agents"]))
    print("      kernel ms (profile mode, one-stream sums): " +
          "  ".join("%s %.1f" % (k, v) for k, v in info["kernel_ms"].items()) + "  solo longest %.1f" % info["solo_longest_ms"], flush=True)
    eng.close()
