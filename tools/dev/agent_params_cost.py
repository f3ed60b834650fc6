"""Development script (not a pytest test, not bench.py): what the per-agent parameter table costs.

    python tools/dev/agent_params_cost.py [B]

At B agents (default 65 536), kinematic N = 20 and Pacejka N = 12, default configuration, straight centerline,
U0 = [1, 0] x N: the blocking solve time
  (a) without a table,
  (b) with a table whose rows all equal the handle's values, P = 1 and P = 4 096 -- the same solve bit for bit
      (checked here), so (b) / (a) is the price of the mechanism on identical arithmetic,
  (c) with the distinct rows of tests/test_gpu_agent_params.py's generator (seed 1), P = 4 096.
One warm-up solve, then three timed solves each (host clock around a blocking solve), then one more solve in
profile mode for last_solve_info()'s per-kernel milliseconds (HIP events, sampled every 8th round)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import numpy as np
import torch

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib
from conftest import straight_centerline, synthetic_states
from test_gpu_agent_params import rows, table_of
from oracle import oracle as O

dev = torch.device("cuda:0")
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
P = min(4096, B)
O.build()

for model, N in ((0, 20), (1, 12)):
    cfg = mp.default_config(model, N)
    eng = mp.BatchedMPC(cfg, dev)
    X0, cl, U0 = T(synthetic_states(model, B, seed=21)), T(straight_centerline()), T(np.tile([1., 0.], (B, N)))
    rng = np.random.default_rng(0)
    cases = [("(a) no table", None, None),
             ("(b) equal rows, P = 1", _lib.param_rows(cfg, 1), np.zeros(B, dtype=np.int64)),
             ("(b) equal rows, P = %d" % P, _lib.param_rows(cfg, P), rng.integers(0, P, B)),
             ("(c) distinct rows, P = %d" % P, table_of(cfg, rows(O, model, P, 1)), rng.integers(0, P, B))]
    ref = None
    base = None
    for name, tab, idx in cases:
        keep = None
        if tab is None:
            eng.clear_agent_params()
        else:
            keep = (T(tab), T(idx, torch.int32))
            eng.set_agent_params(*keep)
        eng.set_profile(False)
        U, _, st = eng.solve(X0, cl, U0)                       # warm-up
        times = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            U, _, st = eng.solve(X0, cl, U0)
            torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
        eng.set_profile(True)
        eng.solve(X0, cl, U0)
        info = eng.last_solve_info()
        if ref is None:
            ref, base = (U, st), min(times)
        same = torch.equal(U, ref[0]) and torch.equal(st, ref[1])
        print("model %d N %d B %d  %-28s ms %s  best/(a) %.3f  same bits as (a): %s  converged %.4f  inner mean %.1f  rounds %d  solo agents %d"
              % (model, N, B, name, " ".join("%.1f" % (1e3 * t) for t in times), min(times) / base, same,
                 float((st[:, 0] == 1).double().mean()), float(st[:, 2].mean()), info["rounds"], info["solo_agents"]))
        print("      kernel ms (profile mode, one-stream sums): " +
              "  ".join("%s %.1f" % (k, v) for k, v in info["kernel_ms"].items()) + "  solo longest %.1f" % info["solo_longest_ms"], flush=True)
    eng.close()
