"""Writes tests/golden/roads_reference.npz: the reference solves of tests/road_common.py (scipy's L-BFGS-B restarted and
finished by projected Newton steps, on the frozen oracle's evaluations plus the numpy road cost; on the disc handle inside
the ALM loop of tests/discs_common.py) for the scenes of tests/test_gpu_agent_roads.py: `change`, `edges`, `brake` and
`pacejka` over the 16 shifts of discs_common.scene_shifts() on unconstrained handles, `disc_road` over the first 4.  Every
agent is solved from three starts (field_common.starts: U = 0, tile(1, 0), a random point of the whole input box); the
spread between them and the projected-gradient residual are recorded, and no file is written in which a spread exceeds
1e-8: a scene that fails is changed, not skipped at test time.  The unshifted scenes are also solved without the table
(`base_*`): what the effect sizes are measured against.  Last, the mirror of the host loop in which a lane change
commanded at sample 8 advances through 6 steps of roads_from_script, solve and rollout (road_common.mirror_script_loop):
its realised states and its last plan (`script_*`).

    python tests/golden/make_roads_golden.py [processes]
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import discs_common as D  # noqa: E402
import road_common as W  # noqa: E402

SPREAD_MAX = 1e-8


def one(job):
    from oracle import oracle as O
    name, b, si = job
    model, N, x0, row, discs = W.scene_row(name, D.scene_shifts()[b])
    cl = D.line_centerline()
    mach = W.machine(O, model, N)
    if si < 0:                                                   # the scene without the table (the discs alone), from U = 0
        U = W.reference_solve(O, mach[0], mach, x0, cl, None) if discs is None else D.reference_solve(O, mach[:2], x0, cl, discs)[0]
        return job, U, np.zeros(0), 0, 0.0, 0.0
    U0 = W.starts(N, b)[si]
    if discs is None:
        U = W.reference_solve(O, mach[0], mach, x0, cl, row, U0)
        return job, U, np.zeros(0), 0, W.projected_gradient(O, mach[0], mach, x0, cl, U, row), 0.0
    U, lam, outer = W.reference_solve_discs(O, mach, x0, cl, discs, row, U0)
    viol, res = W.disc_conditions(O, mach, x0, cl, U, discs, lam, row)
    return job, U, lam, outer, res, viol


def main():
    from oracle import oracle as O
    O.build()
    jobs = [("disc_road", b, si) for b in range(W.DISC_SHIFTS) for si in range(3)]
    jobs += [(s, b, si) for s in W.NONE_SCENES for b in range(D.NSHIFT) for si in range(3)]
    jobs += [(s, 0, -1) for s in W.SCENES]
    with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as pool:
        res = {r[0]: r[1:] for r in pool.map(one, jobs, chunksize=1)}
    out = {"shifts": D.scene_shifts()}
    for s, (model, N, x0, handle) in W.SCENES.items():
        nb = W.DISC_SHIFTS if handle == "discs" else D.NSHIFT
        U = np.stack([np.stack([res[(s, b, si)][0] for si in range(3)]) for b in range(nb)])      # [nb, 3, 2N]
        spread = np.abs(U - U[:, :1]).max((1, 2))
        out[f"U_{s}"] = U[:, 0]                                  # the start U = 0, as the solver is started
        out[f"spread_{s}"] = spread
        out[f"pg_{s}"] = np.array([[res[(s, b, si)][3] for si in range(3)] for b in range(nb)]).max(1)
        out[f"base_{s}"] = res[(s, 0, -1)][0]
        mach = W.machine(O, model, N)
        Xr, Xb = O.rollout(mach[0], x0, U[0, 0]), O.rollout(mach[0], x0, out[f"base_{s}"])
        msg = (f"{s}: end of the plan y {Xr[-1, 1]:.3f} (without the table {Xb[-1, 1]:.3f}), speed {W.speed(Xr)[-1]:.3f} "
               f"({W.speed(Xb)[-1]:.3f}); spread between starts {spread.max():.1e}, residual at most {out[f'pg_{s}'].max():.1e}")
        if handle == "discs":
            lam = np.stack([np.stack([res[(s, b, si)][1] for si in range(3)]) for b in range(nb)])
            out[f"lam_{s}"] = lam[:, 0]
            out[f"lamspread_{s}"] = np.abs(lam - lam[:, :1]).max((1, 2))
            out[f"outer_{s}"] = np.array([res[(s, b, 0)][2] for b in range(nb)])
            out[f"viol_{s}"] = np.array([[res[(s, b, si)][4] for si in range(3)] for b in range(nb)]).max(1)
            msg += (f"; active multipliers {[int((l != 0).sum()) for l in lam[:, 0]]}, outer {out[f'outer_{s}'].tolist()}, spread in "
                    f"lambda {out[f'lamspread_{s}'].max():.1e}, violation at most {out[f'viol_{s}'].max():.1e}, controls "
                    f"{np.abs(U[0, 0] - out[f'base_{s}']).max():.3f} from the solve of the discs alone")
        print(msg)
        if spread.max() > SPREAD_MAX:
            raise SystemExit(f"{s}: the spread between starts {spread.max():.2e} exceeds {SPREAD_MAX:g}: change the scene")
    tx, plan = W.mirror_script_loop(O)
    out["script_traj_x"], out["script_last_plan"] = tx, plan
    print(f"lane change in time (command at sample {W.SCRIPT_AT}): realised |y - 0.5| per step "
          f"{np.array2string(np.abs(tx[:, 1] - 0.5), precision=4)}; the last plan ends at y {plan[-1, 1]:.4f}")
    assert plan[-1, 1] - 0.5 > 0.05 and np.abs(tx[:, 1] - 0.5).max() < 0.05
    np.savez(os.path.join(HERE, "roads_reference.npz"), **out)
    for k, v in out.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
