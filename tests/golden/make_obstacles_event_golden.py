"""Writes tests/golden/obstacles_event_reference.npz: the mirror loop of tests/obstacles_event_common.py (the steps of
mpc_closed_loop_obstacles_event on the CPU checker: the frozen oracle's rollout, the restated triggers, selection and
gather, reference_solve) on the recorded scene -- one kinematic car, N = 20, G = 1, two scripted obstacles, shift on, a warm
start that steers off the line, t0 = 0, max_hold = 8 --, NSCENE copies moved by the small shifts of
discs_common.scene_shifts(): SCRIPT_T steps with both obstacle rules on, and SCRIPT_T_BLIND steps of the loop that watches
the car alone.  While recording, every solve must converge (reference_solve raises where one does not); every decision
margin of every step -- the selections, |clear_chk - clear_thr|, |c - reach^2|, |dev2 - thr^2| -- must be at least
MARGIN_MIN; the second obstacle must fire bit 1 or bit 2 at the first step at which it is in the held window, before the hold
limit; and the loop that watches the car alone must end deeper than half r^2 inside the second obstacle.

    OMP_NUM_THREADS=1 python tests/golden/make_obstacles_event_golden.py [processes] [--check]
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
import obstacles_event_common as OE  # noqa: E402

NSCENE = 16
PATH = os.path.join(HERE, "obstacles_event_reference.npz")


def check_scene(s, res, blind, r_new):
    """what the recording asserts of one scene, on the CPU reference alone"""
    assert res["margin"].min() >= OE.MARGIN_MIN, (s, res["margin"])
    assert blind["margin"].min() >= OE.MARGIN_MIN, (s, blind["margin"])
    t = OE.first_seen(res, 0, 1)
    assert t is not None and 1 <= t < OE.SCRIPT_MAX_HOLD and res["traj_why"][0, t] & 6, (s, t, res["traj_why"][0])
    assert res["solved"][0, 1:t].sum() == 0                                  # ... and no solve by the hold limit before it
    assert not (blind["traj_why"] & 6).any() and blind["solved"][0].tolist() == [1] + [0] * (OE.SCRIPT_T_BLIND - 1)
    assert blind["traj_clear"].min() < -0.5 * r_new ** 2, (s, blind["traj_clear"])
    assert res["solve_count"][0] < OE.SCRIPT_T and res["traj_clear"].min() > -1e-6, (s, res["traj_clear"].min())


def one(s):
    from oracle import oracle as O
    X0, v_ref, obs, U0 = OE.script_scenes(NSCENE)
    log = (lambda m: print(m, flush=True)) if s == 0 else None
    a = (X0[s:s + 1], v_ref[s:s + 1], obs[s:s + 1], U0[s:s + 1])
    res = OE.script_loop(O, *a, 3, OE.SCRIPT_T, log)
    blind = OE.script_loop(O, *a, 0, OE.SCRIPT_T_BLIND, log)
    check_scene(s, res, blind, OE.SCRIPT_NEW[2])
    return res, blind


def record(processes=4):
    from oracle import oracle as O
    O.build()
    with multiprocessing.Pool(processes) as pool:
        both = pool.map(one, range(NSCENE))
    X0, v_ref, obs, U0 = OE.script_scenes(NSCENE)
    out = {"shifts": D.scene_shifts(), "X0": X0, "v_ref": v_ref, "obs": obs, "U0": U0}
    for k in ("traj_x", "traj_u", "traj_clear", "traj_sel", "traj_chk", "traj_why", "solved", "solve_count"):
        out[k] = np.concatenate([r[k] for r, _ in both])
    out["margin"] = np.stack([r["margin"] for r, _ in both])
    for k in ("traj_x", "traj_clear", "solved"):
        out["blind_" + k] = np.concatenate([b[k] for _, b in both])
    out["blind_margin"] = np.stack([b["margin"] for _, b in both])
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
