"""Development script (not a pytest test, not bench.py): what the per-agent bounds table costs.

    python tools/dev/agent_bounds_cost.py [B]
    python tools/dev/agent_bounds_cost.py [B] --against OTHER/libmpc_hip.so

At B agents (default 65 536), kinematic N = 20 and Pacejka N = 12, default configuration, straight centerline,
U0 = [1, 0] x N: the blocking solve time
  (a) without a table,
  (b) with a table whose rows all equal the handle's box, P = 1 and P = 4 096 -- the same solve bit for bit
      (checked here), so (b) / (a) is the price of the mechanism on identical arithmetic,
  (c) with the distinct boxes of tests/test_gpu_agent_bounds.py's generator (seed 7), P = 4 096: other problems,
      reported with their rounds and compared with nothing.
One warm-up solve per variant, then three passes over the variants (so that they alternate), one timed blocking
solve each (host clock), then one more solve each in profile mode for last_solve_info()'s per-kernel milliseconds
(HIP events, sampled every 8th round).

--against: the no-table solve alone, of this build and of another build of the library (the parent commit's, through
MPC_LIB_PATH), each in child processes of its own that alternate -- other, this, other, this -- so that the spread of
the other build against itself is measured in the same call."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args and args[0].isdigit() else 65536
PROBLEMS = ((0, 20), (1, 12))

if "--against" in sys.argv:
    other = os.path.abspath(sys.argv[sys.argv.index("--against") + 1])
    best = {}
    for tag, lib in (("other", other), ("this", None), ("other", other), ("this", None)):
        env = dict(os.environ)
        env.pop("MPC_LIB_PATH", None)
        if lib:
            env["MPC_LIB_PATH"] = lib
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(B), "--no-table-only"], env=env, text=True,
                             stdout=subprocess.PIPE, timeout=600, check=True).stdout
        for ln in out.splitlines():
            print("[%s] %s" % (tag, ln), flush=True)
            if ln.startswith("NOTABLE"):
                _, model, ms = ln.split()[:3]
                best.setdefault((tag, model), []).append(float(ms))
    for model, _ in PROBLEMS:
        o, t = best[("other", str(model))], best[("this", str(model))]
        print("model %d  no table, best of three per process, ms:  other %s  this %s  |  this/other %.4f  other/other %.4f"
              % (model, " ".join("%.1f" % v for v in o), " ".join("%.1f" % v for v in t), min(t) / min(o), max(o) / min(o)))
    sys.exit(0)

import numpy as np
import torch

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib
from conftest import straight_centerline, synthetic_states

dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
P = min(4096, B)


def timed(eng, X0, cl, U0):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    U, _, st = eng.solve(X0, cl, U0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, U, st


if "--no-table-only" in sys.argv:
    print("library", _lib.LIB_PATH, _lib.library_hash()[:16])
    for model, N in PROBLEMS:
        eng = mp.BatchedMPC(mp.default_config(model, N), dev)
        X0, cl, U0 = T(synthetic_states(model, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
        eng.solve(X0, cl, U0)
        times = [timed(eng, X0, cl, U0)[0] for _ in range(3)]
        print("NOTABLE %d %.3f  (ms: %s)" % (model, 1e3 * min(times), " ".join("%.1f" % (1e3 * t) for t in times)))
        eng.close()
    sys.exit(0)

from test_gpu_agent_bounds import bound_rows, btable

for model, N in PROBLEMS:
    cfg = mp.default_config(model, N)
    X0, cl, U0 = T(synthetic_states(model, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
    rng = np.random.default_rng(0)
    cases = [("(a) no table", None, None),
             ("(b) equal rows, P = 1", _lib.bound_rows(cfg, 1), np.zeros(B, dtype=np.int64)),
             ("(b) equal rows, P = %d" % P, _lib.bound_rows(cfg, P), rng.integers(0, P, B)),
             ("(c) distinct rows, P = %d" % P, btable(bound_rows(P, 7)), rng.integers(0, P, B))]
    engs = []
    for name, tab, idx in cases:               # one engine per variant, so that the passes below only solve
        eng = mp.BatchedMPC(cfg, dev)
        keep = None
        if tab is not None:
            keep = (T(tab), T(idx, torch.int32))
            eng.set_agent_bounds(*keep)
        eng.solve(X0, cl, U0)                  # warm-up
        engs.append((name, eng, keep, []))
    res = {}
    for _ in range(3):                         # the variants alternate
        for name, eng, _, times in engs:
            t, U, st = timed(eng, X0, cl, U0)
            times.append(t)
            res[name] = (U, st)
    base = min(engs[0][3])
    for name, eng, _, times in engs:
        eng.set_profile(True)
        eng.solve(X0, cl, U0)
        info = eng.last_solve_info()
        U, st = res[name]
        same = torch.equal(U, res[cases[0][0]][0]) and torch.equal(st, res[cases[0][0]][1])
        print("model %d N %d B %d  %-28s ms %s  best/(a) %.3f  same bits as (a): %s  converged %.4f  inner mean %.1f  rounds %d  solo agents %d"
              % (model, N, B, name, " ".join("%.1f" % (1e3 * t) for t in times), min(times) / base, same,
                 float((st[:, 0] == 1).double().mean()), float(st[:, 2].mean()), info["rounds"], info["solo_agents"]))
        print("      kernel ms (profile mode, one-stream sums): " +
              "  ".join("%s %.1f" % (k, v) for k, v in info["kernel_ms"].items()) + "  solo longest %.1f" % info["solo_longest_ms"], flush=True)
        eng.close()
