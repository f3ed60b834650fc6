"""Writes tests/golden/discs_reference.npz: the reference solves (tests/discs_common.py reference_solve: an ALM loop in
numpy around scipy's L-BFGS-B, on the frozen oracle's evaluations) of the three keep-out-disc scenes of
tests/test_gpu_agent_discs.py, each with the NSHIFT small shifts of the discs that the 64 agents of the test cycle
through.  Several seconds per solve: recorded once, re-derived in part by tests/test_agent_discs_cpu.py.

    python tests/golden/make_discs_golden.py [processes]
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import discs_common as D  # noqa: E402


def one(job):
    from oracle import oracle as O
    name, p = job
    model, N, x0, scene = D.SCENES[name]
    U, lam, outer = D.reference_solve(O, D.configs(O, model, N), x0, D.line_centerline(), scene(N, D.scene_shifts()[p]))
    return name, p, U, lam, outer


def main():
    from oracle import oracle as O
    O.build()
    jobs = [(name, p) for name in D.SCENES for p in range(D.NSHIFT)]
    with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as pool:
        res = pool.map(one, jobs)
    out = {"shifts": D.scene_shifts()}
    for name in D.SCENES:
        mine = sorted((r for r in res if r[0] == name), key=lambda r: r[1])
        out["U_" + name] = np.stack([r[2] for r in mine])
        out["lam_" + name] = np.stack([r[3] for r in mine])
        out["outer_" + name] = np.array([r[4] for r in mine])
    np.savez(os.path.join(HERE, "discs_reference.npz"), **out)
    for k, v in out.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
