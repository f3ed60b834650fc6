"""Writes tests/golden/traffic_event_reference.npz: the mirror loop of tests/traffic_event_common.py (the steps of
mpc_closed_loop_traffic_event on the CPU checker: the frozen oracle's rollout, the restated triggers, selection and gather,
reference_solve) on the recorded scene -- three kinematic cars, N = 20, G = 3, discs, shift on, max_hold = 8, the rear car
on a warm start that steers off the line --, NSCENE copies moved by the small shifts of discs_common.scene_shifts():
EVENT_T steps with both rules on, and EVENT_T_BLIND steps of the loop that watches the car alone.  While recording, every
solve must converge (reference_solve raises where one does not); every decision margin of every step -- the selections,
|clear_chk - clear_thr|, |c - reach^2|, |dev2 - thr^2| -- must be at least MARGIN_MIN; with both rules on the rear car must
fire bit 1 or bit 2 at step 1, before any solve by the hold limit, every car must solve at fewer than EVENT_T steps and no
car may end inside another; and in the loop that watches the car alone nobody fires a rule and the rear car ends deeper
than half r^2 inside the slower one.

    OMP_NUM_THREADS=1 python tests/golden/make_traffic_event_golden.py [processes] [--check]
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
import traffic_event_common as TE  # noqa: E402

NSCENE = 16
PATH = os.path.join(HERE, "traffic_event_reference.npz")


def check_scene(s, res, blind):
    """what the recording asserts of one scene, on the CPU reference alone (car 0: the rear car)"""
    assert res["margin"].min() >= TE.MARGIN_MIN, (s, res["margin"])
    assert blind["margin"].min() >= TE.MARGIN_MIN, (s, blind["margin"])
    assert (res["traj_opp"][:, 0] == -1).all(), (s, res["traj_opp"][:, 0])       # the plans of step 0 are solved against nobody
    assert res["traj_why"][0, 1] & 6, (s, res["traj_why"][0])
    assert (res["solve_count"] < TE.EVENT_T).all() and res["traj_clear"].min() > -1e-6, (s, res["solve_count"], res["traj_clear"].min())
    assert not (blind["traj_why"] & 6).any() and (blind["solved"] == np.eye(1, TE.EVENT_T_BLIND, dtype=np.uint8)).all()
    assert blind["traj_clear"][0, -1] < -0.5 * TE.EVENT_RADIUS ** 2, (s, blind["traj_clear"][0])


def one(s):
    from oracle import oracle as O
    X0, v_ref, radius, U0 = TE.event_scenes(NSCENE)
    log = (lambda m: print(m, flush=True)) if s == 0 else None
    sl = slice(3 * s, 3 * s + 3)
    a = (X0[sl], v_ref[sl], radius[sl], U0[sl])
    res = TE.event_loop(O, *a, 3, TE.EVENT_T, log)
    blind = TE.event_loop(O, *a, 0, TE.EVENT_T_BLIND, log)
    check_scene(s, res, blind)
    return res, blind


def record(processes=4, scenes=range(NSCENE)):
    from oracle import oracle as O
    O.build()
    with multiprocessing.Pool(processes) as pool:
        both = pool.map(one, scenes)
    X0, v_ref, radius, U0 = TE.event_scenes(NSCENE)
    out = {"shifts": D.scene_shifts(), "X0": X0, "v_ref": v_ref, "radius": radius, "U0": U0}

    def glob(s, a):      # a scene's agent indices -> the batch's
        return np.where(a >= 0, a + 3 * s, -1).astype(np.int32)
    for k in ("traj_x", "traj_u", "traj_clear", "traj_why", "solved", "solve_count"):
        out[k] = np.concatenate([r[k] for r, _ in both])
    for k in ("traj_opp", "traj_chk"):
        out[k] = np.concatenate([glob(s, r[k]) for s, (r, _) in zip(scenes, both)])
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
