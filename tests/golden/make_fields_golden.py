"""Writes tests/golden/fields_reference.npz: the reference solves of tests/field_common.py (scipy's L-BFGS-B restarted and
finished by projected Newton steps, on the frozen oracle's evaluations plus the numpy risk field; on LANE handles inside
the ALM loop of tests/discs_common.py) for the scenes of tests/test_gpu_agent_fields.py: `standing`, `moving`, `pacejka`
over the 16 shifts of discs_common.scene_shifts() on unconstrained handles, `standing` and `pacejka` with
lane_halfwidth = 0.10 over the first 4.  Every agent is solved from three starts (field_common.starts: U = 0, tile(1, 0), a
random point of the whole input box); the spread between them is recorded, and no file is written in which a NONE-handle
agent's spread exceeds 1e-8: a scene that fails is changed, not skipped at test time (field_common.SOURCE_Y says how these
were).  Then the mirror loop of mpc_closed_loop_traffic_field on the CPU checker (field_common.mirror_loop): three cars,
the rear one passing the slow one, two shifted scenes, 14 steps; the selection margin of every step is asserted.

    python tests/golden/make_fields_golden.py [processes]
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import discs_common as D  # noqa: E402
import field_common as F  # noqa: E402

NONE_SCENES = ("standing", "moving", "pacejka")
LANE_SCENES = ("standing", "pacejka")
SPREAD_MAX = 1e-8


def one(job):
    from oracle import oracle as O
    kind, name, b, si = job
    model, N, x0, row = F.scene_row(name, D.scene_shifts()[b], lane=kind == "lane")
    cl = D.line_centerline()
    cfgs = F.machine(O, model, N)
    U0 = F.starts(N, b)[si]
    if kind == "none":
        cfg = O.default_config(model, N, constr_mode=O.CONSTR_NONE)
        U = F.reference_solve(O, cfg, cfgs, x0, cl, row, U0)
        _, g = F.psi(O, cfg, cfgs, x0, cl, U, row)
        pg = np.abs(U - np.clip(U - g, np.tile([-1.0, -0.32], N), np.tile([1.0, 0.32], N))).max()
        dev = np.abs(O.rollout(cfg, x0, U)[:, 1] - 0.5).max()
        return job, U, np.zeros(0), 0, pg, dev
    cfg = O.default_config(model, N, constr_mode=O.CONSTR_LANE, lane_halfwidth=F.LANE_HW)
    U, lam, outer = F.reference_solve_lane(O, cfg, cfgs, x0, cl, row, U0)
    viol, res = F.lane_conditions(O, cfg, cfgs, x0, cl, U, row, lam, F.LANE_HW)
    return job, U, lam, outer, res, viol


def mirror(s):
    """scene s of field_common.traffic_scenes() through the mirror loop, alone (agents of different scenes never meet)"""
    from oracle import oracle as O
    X0, v_ref, radius, shape = F.traffic_scenes()
    sl = slice(3 * s, 3 * s + 3)
    return F.mirror_loop(O, F.TRAFFIC_N, X0[sl], v_ref[sl], radius[sl], shape[sl], F.TRAFFIC_REACH, 3, F.TRAFFIC_T, D.line_centerline())


def main():
    from oracle import oracle as O
    O.build()
    jobs = [("none", s, b, si) for s in NONE_SCENES for b in range(D.NSHIFT) for si in range(3)]
    jobs += [("lane", s, b, si) for s in LANE_SCENES for b in range(F.LANE_SHIFTS) for si in range(3)]
    with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as pool:
        res = {r[0]: r[1:] for r in pool.map(one, jobs, chunksize=1)}
    out = {"shifts": D.scene_shifts(), "source": np.array([F.SOURCE["A"], *F.SOURCE["sigma"]]), "lane_hw": np.array(F.LANE_HW)}
    for kind, scenes, nb in (("none", NONE_SCENES, D.NSHIFT), ("lane", LANE_SCENES, F.LANE_SHIFTS)):
        for s in scenes:
            U = np.stack([np.stack([res[(kind, s, b, si)][0] for si in range(3)]) for b in range(nb)])      # [nb, 3, 2N]
            spread = np.abs(U - U[:, :1]).max((1, 2))
            out[f"U_{kind}_{s}"] = U[:, 0]                           # the start U = 0, as the solver is started
            out[f"spread_{kind}_{s}"] = spread
            fig = np.array([[res[(kind, s, b, si)][3] for si in range(3)] for b in range(nb)])
            oth = np.array([[res[(kind, s, b, si)][4] for si in range(3)] for b in range(nb)])
            if kind == "none":
                out[f"pg_{kind}_{s}"], out[f"dev_{kind}_{s}"] = fig.max(1), oth[:, 0]
                print(f"{kind} {s}: largest sideways deviation {oth.max():.3f}, spread between starts {spread.max():.1e}, "
                      f"projected gradient at most {fig.max():.1e}")
                if spread.max() > SPREAD_MAX:
                    raise SystemExit(f"{kind} {s}: the spread between starts {spread.max():.2e} exceeds {SPREAD_MAX:g}: change the scene")
            else:
                lam = np.stack([np.stack([res[(kind, s, b, si)][1] for si in range(3)]) for b in range(nb)])
                out[f"lam_{kind}_{s}"] = lam[:, 0]
                out[f"lamspread_{kind}_{s}"] = np.abs(lam - lam[:, :1]).max((1, 2))
                out[f"outer_{kind}_{s}"] = np.array([res[(kind, s, b, 0)][2] for b in range(nb)])
                print(f"{kind} {s}: active multipliers {[int((l != 0).sum()) for l in lam[:, 0]]}, outer {out[f'outer_{kind}_{s}'].tolist()}, "
                      f"spread between starts {spread.max():.1e} in U, {out[f'lamspread_{kind}_{s}'].max():.1e} in lambda; "
                      f"Lagrangian residual at most {fig.max():.1e}, violation at most {oth.max():.1e}")
    X0, v_ref, radius, shape = F.traffic_scenes()
    with multiprocessing.Pool(F.TRAFFIC_SCENES) as pool:
        mir = pool.map(mirror, range(F.TRAFFIC_SCENES))
    out.update(traffic_X0=X0, traffic_v_ref=v_ref, traffic_radius=radius, traffic_shape=shape)
    for k in ("traj_x", "traj_u", "traj_opp", "traj_clear"):
        out["traffic_" + k] = np.concatenate([m[k] for m in mir])
    for s in range(1, F.TRAFFIC_SCENES):                    # the selection restated per scene: global agent indices
        sel = out["traffic_traj_opp"][3 * s:3 * s + 3]
        sel[sel >= 0] += 3 * s
    out["traffic_margin"] = np.stack([m["margin"] for m in mir])
    tx = out["traffic_traj_x"]
    passed = [int(np.argmax(tx[3 * s, :, 0] > tx[3 * s + 1, :, 0])) for s in range(F.TRAFFIC_SCENES)]
    print(f"traffic: selection margin at least {out['traffic_margin'].min():.3e}; the rear car is past the slow one at steps {passed}, "
          f"{np.abs(tx[0::3, :, 1] - X0[0::3, None, 1]).max():.3f} beside its line at most; smallest clearance {out['traffic_traj_clear'].min():.4f}")
    assert out["traffic_margin"].min() >= 1e-3 and all(p > 0 for p in passed)
    np.savez(os.path.join(HERE, "fields_reference.npz"), **out)
    for k, v in out.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
