"""Writes tests/golden/rates_reference.npz: the reference solves of tests/rate_common.py (scipy's L-BFGS-B finished by
projected Newton steps, on the frozen oracle's evaluations plus the numpy move penalty; around it the ALM loop of
tests/discs_common.py on the disc scene) for the two scenes of tests/test_gpu_agent_rates.py, 16 agents each, at the
weights rate_common.WEIGHTS.  Seconds per solve: recorded once, re-derived in part by tests/test_agent_rates_cpu.py.

    python tests/golden/make_rates_golden.py [processes]
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import discs_common as D  # noqa: E402
import rate_common as R  # noqa: E402


def one(job):
    from oracle import oracle as O
    scene, wi, b = job
    w = R.WEIGHTS[wi]
    cl = D.line_centerline()
    if scene == "kin":
        X0, up = R.scene_agents(0)
        cfg = O.default_config(0, 20, constr_mode=O.CONSTR_NONE)
        U = R.reference_solve(O, cfg, X0[b], cl, np.array([w[0], w[1], up[b, 0], up[b, 1]]))
        return scene, wi, b, U, np.zeros(0), 0
    X0, discs, up = R.disc_scene_agents()
    U, lam, outer = R.reference_solve_discs(O, D.configs(O, 0, 20), X0[b], cl, discs[b], np.array([w[0], w[1], up[b, 0], up[b, 1]]))
    return scene, wi, b, U, lam, outer


def main():
    from oracle import oracle as O
    O.build()
    jobs = [(s, wi, b) for s in ("kin", "moving") for wi in range(len(R.WEIGHTS)) for b in range(R.NAGENT)]
    with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as pool:
        res = pool.map(one, jobs)
    out = {"weights": np.array(R.WEIGHTS), "u_prev_kin": R.scene_agents(0)[1], "u_prev_moving": R.disc_scene_agents()[2]}
    for s in ("kin", "moving"):
        for wi in range(len(R.WEIGHTS)):
            mine = sorted((r for r in res if r[0] == s and r[1] == wi), key=lambda r: r[2])
            out[f"U_{s}_{wi}"] = np.stack([r[3] for r in mine])
            if s == "moving":
                out[f"lam_{s}_{wi}"] = np.stack([r[4] for r in mine])
                out[f"outer_{s}_{wi}"] = np.array([r[5] for r in mine])
    np.savez(os.path.join(HERE, "rates_reference.npz"), **out)
    for k, v in out.items():
        print(k, v.shape)
    X0, discs, _ = R.disc_scene_agents()
    c0 = D.configs(O, 0, 20)[0]
    for wi in range(len(R.WEIGHTS)):
        print("routes round the discs, weights", R.WEIGHTS[wi], [R.route(O, c0, X0[b], out[f"U_moving_{wi}"][b], discs[b]) for b in range(R.NAGENT)])
    for wi in range(len(R.WEIGHTS)):
        print("first drive of agent 0, kin, weights", R.WEIGHTS[wi], out[f"U_kin_{wi}"][0, 0])


if __name__ == "__main__":
    main()
