"""What the GPU tests of the per-agent tables share (tests/test_gpu_agent_params.py, tests/test_gpu_agent_bounds.py,
tests/test_gpu_agent_constraints.py, tests/test_gpu_agent_tables.py): tensors from arrays, the oracle run with every
agent's own configuration, the assertions of tests/test_gpu_parity.py for the same quantities, and the generators of
the parameter and box rows.  The order of the generators' draws is part of the tests: these rows were checked with the
oracle alone."""
import numpy as np
import torch

from conftest import straight_centerline, synthetic_states

from model_predictive_control_amd import _lib


def T(a, dev, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def kwl(kw):
    """ctypes-friendly copy of a row's overrides."""
    return {k: (list(v) if hasattr(v, "__len__") else float(v)) for k, v in kw.items()}


def by_row(idx, P, fn):
    """fn(p, sel) -> tuple of arrays for the agents sel (those with row p); the tuples scattered back into batch order."""
    B = len(idx)
    outs = None
    for p in range(P):
        sel = np.nonzero(idx == p)[0]
        if sel.size == 0:
            continue
        res = fn(p, sel)
        if outs is None:
            outs = [None if r is None else np.empty((B,) + np.asarray(r).shape[1:]) for r in res]
        for o, r in zip(outs, res):
            if o is not None:
                o[sel] = r
    return outs


def problem(model, N, B, seed=21):
    return synthetic_states(model, B, seed=seed), straight_centerline(), np.tile([1., 0.], (B, N))


def oracle_solve(O, model, N, overrides, X0, cl, U0, **common):
    """overrides[b]: the configuration overrides of agent b (dicts; agents that share one are solved in one batch).
    Returns (U, stats, lambda or None)."""
    B = len(overrides)
    keys = [repr(sorted((k, np.asarray(v).tolist()) for k, v in o.items())) for o in overrides]
    U = np.empty((B, U0.shape[1])); st = np.empty((B, 8)); lam = None
    for key in sorted(set(keys)):
        sel = np.array([b for b in range(B) if keys[b] == key])
        ocfg = O.default_config(model, N, **{**common, **kwl(overrides[sel[0]])})
        Us, ls, ss = O.solve_batch(ocfg, X0[sel], cl, U0[sel])
        U[sel], st[sel] = Us, ss
        if ls.shape[1]:
            lam = np.empty((B, ls.shape[1])) if lam is None else lam
            lam[sel] = ls
    return U, st, lam


def assert_tight(U, st, Uo, sto):
    """The assertions of test_solve_matches_oracle_tight_tolerance (alm_eps = 1e-10)."""
    conv = (st[:, 0] == 1) & (sto[:, 0] == 1)
    assert conv.mean() >= 0.97
    assert np.mean((st[:, 0] == 1) == (sto[:, 0] == 1)) >= 0.98
    scale = np.maximum(1.0, np.abs(Uo).max(1))
    d = np.abs(U - Uo).max(1) / scale                                     # bench.DU_METRIC
    match = conv & (d <= 1e-5)
    assert match.sum() >= 0.97 * conv.sum()
    other = conv & ~match
    assert np.all(np.abs(st[other, 6] - sto[other, 6]) > 1e-9)            # the others sit at distinct minima
    assert np.median(np.abs(U - Uo).max(1)[match]) <= 1e-7
    assert np.allclose(st[match, 6], sto[match, 6], rtol=1e-10, atol=1e-12)


def assert_reference_tolerance(U, st, Uo, sto):
    """The assertions of test_solve_reference_tolerance_statistics (alm_eps = 1e-6)."""
    assert np.all(st[:, 0] == 1) and np.all(sto[:, 0] == 1)
    assert np.allclose(st[:, 6], sto[:, 6], rtol=0, atol=1e-9)
    assert np.abs(U - Uo).max() <= 2e-4
    assert abs(st[:, 2].mean() - sto[:, 2].mean()) <= 0.05 * sto[:, 2].mean()
    assert np.all(st[:, 1] == sto[:, 1])
    assert np.all(st[:, 4] <= 1e-6)


# ----------------------------------------------------------------------------- the rows of the tests
def param_rows_of(O, model, P, seed):
    """Parameter row p as the override of the oracle's configuration AND the content of table row p (row 0: the
    defaults)."""
    rng = np.random.default_rng(seed)
    base = O.default_config(model, 12)
    out = []
    for p in range(P):
        veh = np.array(list(base.veh))
        if model == 0:
            veh[1] *= rng.uniform(.8, 1.25); veh[2] *= rng.uniform(.8, 1.25)
            kw = dict(veh=veh, accel=base.accel * rng.uniform(.75, 1.25), friction=base.friction * rng.uniform(.7, 1.3),
                      v_ref=rng.uniform(.6, 1.4), cost_w=np.array(list(base.cost_w)) * rng.uniform(.7, 1.4, 6))
        else:
            veh[1] *= rng.uniform(.9, 1.1); veh[2] *= rng.uniform(.9, 1.1)
            veh[7] *= rng.uniform(.85, 1.2); veh[8] *= rng.uniform(.85, 1.2)
            veh[11:17] *= rng.uniform(.9, 1.1, 6)
            veh[17] *= rng.uniform(.85, 1.15); veh[18:22] *= rng.uniform(.8, 1.2, 4)
            kw = dict(veh=veh, v_ref=rng.uniform(.7, 1.3), cost_w=np.array(list(base.cost_w)) * rng.uniform(.7, 1.4, 6))
        out.append({} if p == 0 else kw)
    return out


def box_rows_of(P, seed):
    """Box row p as the override of the oracle's configuration AND the content of table row p."""
    rng = np.random.default_rng(seed)
    out = [dict(u_lb=[-1.0, -0.32], u_ub=[1.0, 0.32])]          # row 0: the handle's box
    for _ in range(1, P):
        lb_d = -rng.uniform(.2, 1.0); ub_d = rng.uniform(.35, 1.0)
        s_lo = -rng.uniform(.08, .32); s_hi = rng.uniform(.08, .32)
        out.append(dict(u_lb=[lb_d, s_lo], u_ub=[ub_d, s_hi]))
    return out


def table_of(cfg, rws, make=_lib.param_rows, fields=_lib.PARAM_FIELDS):
    """[P, width] host table of the rows: the handle's row with the overrides of each row (parameters; the constraint
    table with make=_lib.constraint_rows, fields=_lib.CONSTR_FIELDS)."""
    tab = make(cfg, len(rws))
    for p, kw in enumerate(rws):
        for k, v in kw.items():
            off, width = fields[k]
            tab[p, off:off + width] = v
    return tab
