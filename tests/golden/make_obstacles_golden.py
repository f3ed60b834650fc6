"""Writes tests/golden/obstacles_reference.npz: the mirror loop of tests/obstacles_common.py (the steps of
mpc_closed_loop_obstacles on the CPU checker: the frozen oracle's rollout, the restated selection and gather,
reference_solve) on the recorded scene -- one kinematic car, N = 20, G = 1, three scripted obstacles, shift on, U0 = 0,
t0 = 0 --, NSCENE copies moved by the small shifts of discs_common.scene_shifts(), T steps.  About a second per solve:
recorded once.  While recording, every solve must converge (reference_solve raises where one does not) and every step's
selection margin must be at least obstacles_common.MARGIN_MIN.  The selection cases of the GPU test are checked against
the counts that test asserts (they come from a fixed seed and are not stored).

    OMP_NUM_THREADS=1 python tests/golden/make_obstacles_golden.py [processes] [--check]
    --check: compare with the committed file instead of writing it
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import discs_common as D  # noqa: E402
import obstacles_common as OC  # noqa: E402

NSCENE, T = 16, 14
PATH = os.path.join(HERE, "obstacles_reference.npz")


def one(s):
    from oracle import oracle as O
    X0, v_ref, obs = OC.script_scenes(NSCENE)
    res = OC.mirror_loop(O, 0, OC.SCRIPT_N, X0[s:s + 1], v_ref[s:s + 1], obs[s:s + 1], OC.SCRIPT_REACH, 1, T, D.line_centerline(),
                         log=((lambda m: print(m, flush=True)) if s == 0 else None))
    assert res["margin"].min() >= OC.MARGIN_MIN, (s, res["margin"])
    return res


def record(processes=4):
    from oracle import oracle as O
    O.build()
    with multiprocessing.Pool(processes) as pool:
        res = pool.map(one, range(NSCENE))
    X0, v_ref, obs = OC.script_scenes(NSCENE)
    out = {"shifts": D.scene_shifts(), "X0": X0, "v_ref": v_ref, "obs": obs}
    for k in ("traj_x", "traj_u", "traj_clear", "traj_sel"):
        out[k] = np.concatenate([r[k] for r in res])
    out["margin"] = np.stack([r["margin"] for r in res])
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    out = record(int(args[0]) if args else 4)
    if "--check" in sys.argv:
        ref = np.load(PATH)
        assert sorted(ref.files) == sorted(out)
        for k, v in out.items():
            assert np.array_equal(ref[k], v), k
        print("the committed file is reproduced")
        return
    np.savez(PATH, **out)
    for k, v in out.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
