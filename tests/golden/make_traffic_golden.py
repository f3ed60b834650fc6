"""Writes tests/golden/traffic_reference.npz: the mirror loop of tests/traffic_common.py (the six steps of
mpc_closed_loop_traffic on the CPU checker: the frozen oracle's rollout, the restated selection, reference_solve) on the
overtake scene of tests/test_gpu_traffic_loop.py -- three kinematic cars, N = 20, G = 3, shift on, U0 = 0 --, NSCENE copies
moved by the small shifts of discs_common.scene_shifts(), T steps.  About a second per solve: recorded once.  While
recording, every step's selection margin must be at least traffic_common.MARGIN_MIN.

    OMP_NUM_THREADS=1 python tests/golden/make_traffic_golden.py [processes]     (one BLAS thread per process: two minutes on 8 cores)
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import discs_common as D  # noqa: E402
import traffic_common as TC  # noqa: E402

NSCENE, T = 16, 14


def one(s):
    from oracle import oracle as O
    X0, v_ref, radius = TC.overtake_scenes(NSCENE)
    sl = slice(3 * s, 3 * s + 3)
    res = TC.mirror_loop(O, 0, TC.OVERTAKE_N, X0[sl], v_ref[sl], radius[sl], TC.OVERTAKE_REACH, 3, T, D.line_centerline(),
                         log=((lambda m: print(m, flush=True)) if s == 0 else None))
    assert res["margin"].min() >= TC.MARGIN_MIN, (s, res["margin"])
    return res


def main():
    from oracle import oracle as O
    O.build()
    with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as pool:
        res = pool.map(one, range(NSCENE))
    X0, v_ref, radius = TC.overtake_scenes(NSCENE)
    out = {"shifts": D.scene_shifts(), "X0": X0, "v_ref": v_ref, "radius": radius}
    for k in ("traj_x", "traj_u", "traj_clear"):
        out[k] = np.concatenate([r[k] for r in res])
    out["traj_opp"] = np.concatenate([np.where(r["traj_opp"] >= 0, r["traj_opp"] + 3 * s, -1) for s, r in enumerate(res)]).astype(np.int32)
    out["margin"] = np.stack([r["margin"] for r in res])
    np.savez(os.path.join(HERE, "traffic_reference.npz"), **out)
    for k, v in out.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
