"""CPU tests of the per-agent field table (mpc_set_agent_fields): the checker of tests/field_common.py has the gradient of
its own psi, the term is what the header says on numbers worked by hand, the header declares the API and the library
exports it, the default row is zeros, the host-side table builder puts its arguments in the documented columns, the
gather rule has a numpy mirror, and the front ends carry the new entry points.  No compute call is made here."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import discs_common as D
import field_common as F

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


# ----------------------------------------------------------------------------- the checker
CASES = [(0, N, mode) for mode in ("none", "state_sq", "lane") for N in (1, 2, 12, 20)] + [(1, 12, "none")]


@pytest.mark.parametrize("model,N,mode", CASES)
def test_checker_gradient_agrees_with_central_differences(O, model, N, mode):
    """within 1e-7 relative to ||grad psi|| (h = 1e-6; measured 8.7e-10 kinematic N = 20, 4.4e-9 Pacejka N = 12): a source
    with alpha = 0.5 rotated by 0.1 rad beside the path, a second one further on, so that the term is a visible part of the
    gradient (asserted)"""
    rng = np.random.default_rng(7 + N)
    kw = dict(none=dict(constr_mode=O.CONSTR_NONE), state_sq=dict(constr_mode=O.CONSTR_STATE_SQ),
              lane=dict(constr_mode=O.CONSTR_LANE, lane_halfwidth=0.05))[mode]
    cfg = O.default_config(model, N, **kw)
    cfgs = F.machine(O, model, N)
    x0 = D.X0_PAC if model else D.X0_KIN
    cl = D.line_centerline()
    U = np.tile([0.6, 0.0], N) + rng.uniform(-.3, .3, 2 * N) * np.tile([1.0, 0.3], N)
    row = F.source_rows(N, (1.2, 0.53), 0.1, 0.3, (0.15, 0.06), 0.5, second=((1.5, 0.46), -0.3, 0.2, (0.2, 0.08), -0.4))
    m = O.m(cfg)
    y = rng.uniform(-1.0, 1.0, m) if m else None
    Sig = 10 ** rng.uniform(0, 2, m) if m else None
    p, g = F.psi(O, cfg, cfgs, x0, cl, U, row, y, Sig)
    p0, g0 = O.psi(cfg, x0, cl, U, y, Sig)
    t, tg = F.field_term(O, cfgs, x0, cl, U, row)
    assert p == p0 + t and t > 0 and np.linalg.norm(tg) > 1e-2 * np.linalg.norm(g)
    fd = F.psi_fd_grad(O, cfg, cfgs, x0, cl, U, row, y, Sig)
    err = np.abs(fd - g).max() / np.linalg.norm(g)
    print(f"model {model} N {N} {mode}: checker vs central differences {err:.2e}")
    assert err <= 1e-7


def test_term_by_hand():
    """one source on numbers whose products are exact: frame (c, s) = (0.6, 0.8), kx = 2, ky = 4, alpha = 0.5"""
    X = np.array([[1.5, 0.75, 0.0, 1.0]])
    row = np.zeros((1, F.NFIELD, F.NFSRC))
    row[0, 0] = [1.0, 0.5, 0.6, 0.8, 0.25, 2.0, 4.0, 0.5]
    row[0, 1] = [9.0, 9.0, 1.0, 0.0, 0.0, 1.0, 1.0, 3.0]               # A = 0: nothing, whatever the rest says
    V, w = F.field_values(X, row)
    a, l = 0.6 * 0.5 + 0.8 * 0.25, 0.6 * 0.25 - 0.8 * 0.5               # 0.5, -0.25
    E = 2 * a * a + 4 * l * l + 0.5 * a
    assert np.isclose(a, 0.5) and np.isclose(l, -0.25) and np.isclose(E, 1.0)
    assert np.isclose(V[0, 0], 0.25 * np.exp(-1.0), rtol=1e-15) and V[0, 1] == 0.0
    ga, gl = -V[0, 0] * (2 * 2 * a + 0.5), -V[0, 0] * (2 * 4 * l)
    assert np.allclose(w[0], [0.6 * ga - 0.8 * gl, 0.8 * ga + 0.6 * gl], rtol=1e-15)
    # the gradient of V by differences of V itself
    h = 1e-6
    for i in range(2):
        e = np.zeros(4); e[i] = h
        fd = (F.field_values(X + e, row)[0].sum() - F.field_values(X - e, row)[0].sum()) / (2 * h)
        assert abs(fd - w[0, i]) <= 1e-9
    assert not F.field_values(X, np.zeros((1, F.NFIELD, F.NFSRC)))[0].any()


# ----------------------------------------------------------------------------- the API
def test_header_declares_and_library_exports_the_fields_api(L):
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert re.search(r"#define\s+MPC_NFIELD\s+2\b", hdr) and re.search(r"#define\s+MPC_NFSRC\s+8\b", hdr)
    assert re.search(r"#define\s+MPC_FIELD_ROW\(N\)\s+\(MPC_NFIELD \* MPC_NFSRC \* \(N\)\)", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mpc_default_fields\s*\(\s*const\s+mpc_config\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+mpc_set_agent_fields\s*\(\s*mpc_handle\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    for name in ("mpc_default_fields", "mpc_set_agent_fields", "mpc_fields_from_plans", "mpc_closed_loop_traffic_field"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert (_lib.NFIELD, _lib.NFSRC) == (2, 8) == (mp.NFIELD, mp.NFSRC) and _lib.NFIELD == _lib.NDISC
    assert _lib.field_row(20) == 320 == mp.field_row(20) and _lib.field_row(1) == 16
    assert 65536 * _lib.field_row(20) * 8 == 167772160                      # the 168 MB the header names
    assert len(L.mpc_default_fields.argtypes) == 2
    assert L.mpc_set_agent_fields.argtypes == L.mpc_set_agent_rates.argtypes == L.mpc_set_agent_discs.argtypes
    assert L.mpc_fields_from_plans.argtypes == L.mpc_discs_from_plans.argtypes
    # mpc_closed_loop_traffic's arguments with `shape` beside `radius`
    t, f = L.mpc_closed_loop_traffic.argtypes, L.mpc_closed_loop_traffic_field.argtypes
    assert len(f) == len(t) + 1 and f[:6] == t[:6] and f[6] is C.c_void_p and f[7:] == t[6:]
    # the operation order is part of the contract
    assert "E = ((kx a) a + (ky l) l) + alpha a" in hdr and "V = A exp(-E)" in hdr and "168 MB" in hdr


def test_null_arguments_return_codes_not_exceptions(L):
    E_ARG = -1
    cfg = mp.default_config(0, 2)
    row = (C.c_double * 32)(*([1.0] * 32))
    assert L.mpc_default_fields(None, row) == E_ARG and b"mpc_default_fields" in L.mpc_last_error()
    assert L.mpc_default_fields(C.byref(cfg), None) == E_ARG
    assert L.mpc_default_fields(C.byref(cfg), row) == 0 and list(row) == [0.0] * 32
    assert L.mpc_set_agent_fields(None, None, 0, None, 0) == E_ARG
    assert b"mpc_set_agent_fields" in L.mpc_last_error()
    assert L.mpc_set_agent_fields(None, C.c_void_p(8), 1, C.c_void_p(8), 1) == E_ARG   # (nothing is dereferenced)
    assert L.mpc_fields_from_plans(None, 1, None, None, None, None, None) == E_ARG
    assert L.mpc_closed_loop_traffic_field(None, 4, 1, 0, 2, C.c_void_p(8), C.c_void_p(8), 1.0, *([None] * 13)) == E_ARG
    # the scene arguments are checked without a device, as mpc_closed_loop_traffic checks them
    assert L.mpc_closed_loop_traffic_field(None, 5, 1, 0, 2, C.c_void_p(8), C.c_void_p(8), 1.0, *([None] * 13)) == E_ARG
    assert b"whole number of scenes" in L.mpc_last_error()


def test_field_rows(L):
    N = 12
    assert not _lib.default_fields(mp.default_config(1, N)).any() and _lib.default_fields(mp.default_config(1, N)).shape == (16 * N,)
    tab = _lib.field_rows(np.broadcast_to([1.55, 0.53], (1, N, 2, 2)), 0.0, [0.3, 0.0], 0.15, 0.06)
    assert tab.shape == (1, N, 2, 8) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
    assert np.array_equal(tab[0, 3, 0], [1.55, 0.53, 1.0, 0.0, 0.3, 1 / (2 * 0.15 ** 2), 1 / (2 * 0.06 ** 2), 0.0])
    assert tab[0, :, 1, 4].tolist() == [0.0] * N
    P = 3
    rng = np.random.default_rng(0)
    ce = rng.uniform(0, 2, (P, N, 2, 2)); hd = rng.uniform(-1, 1, (P, N, 2)); A = rng.uniform(0, 1, (P, 1, 2))
    sx, sy, al = rng.uniform(0.1, 0.3, (P, N, 2)), 0.07, rng.uniform(-1, 1, (P, N, 2))
    tab = _lib.field_rows(ce, hd, A, sx, sy, al)
    assert tab.shape == (P, N, 2, 8) and np.array_equal(tab[..., :2], ce) and np.array_equal(tab[..., 2], np.cos(hd))
    assert np.array_equal(tab[..., 3], np.sin(hd)) and np.array_equal(tab[..., 4], np.broadcast_to(A, (P, N, 2)))
    assert np.array_equal(tab[..., 5], 1 / (2 * sx * sx)) and (tab[..., 6] == 1 / (2 * 0.07 * 0.07)).all() and np.array_equal(tab[..., 7], al)
    one = _lib.field_rows([1.2, 0.53], 0.1, [0.3, 0.0], 0.15, 0.06, 0.5)                               # a point, every stage: N = 1 row
    assert one.shape == (1, 1, 2, 8)
    ref = F.source_rows(N, (1.2, 0.53), 0.1, 0.3, (0.15, 0.06), 0.5)                                     # the checker's layout
    assert np.array_equal(np.broadcast_to(one, (1, N, 2, 8))[0, :, 0], ref[:, 0]) and not one[..., 1, 4].any() and not ref[:, 1].any()
    assert mp.field_rows is _lib.field_rows and mp.default_fields is _lib.default_fields
    for bad in (dict(A=-1e-3), dict(A=float("nan")), dict(sigma_x=0.0), dict(sigma_y=-0.1), dict(alpha=float("inf")),
                dict(heading=float("nan")), dict(centres=[1.0, 2.0, 3.0]), dict(centres=[[float("inf"), 0.0]]),
                dict(A=np.zeros(3)), dict(heading=np.zeros((2, 3, 2)), A=np.zeros((3, 3, 2)))):
        kw = dict(centres=[1.0, 0.5], heading=0.0, A=0.3, sigma_x=0.15, sigma_y=0.06, alpha=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib.field_rows(**kw)


def test_gather_mirror():
    """the numpy mirror of mpc_fields_from_plans: copies, the frame of the opponent's heading, the skew from the speed
    difference, zeros for an unused slot and an opponent out of range"""
    rng = np.random.default_rng(5)
    B, N, nx = 5, 3, 4
    X = rng.uniform(0.5, 2.0, (B, N, nx))
    shape = rng.uniform(0.1, 1.0, (B, 4))
    opp = np.array([[1, 2], [0, -1], [7, 3], [4, 4], [-1, -1]], dtype=np.int32)
    tab = F.gather(X, opp, shape)
    assert tab.shape == (B, N, 2, 8)
    assert np.array_equal(tab[0, :, 1, 0], X[2, :, 0]) and np.array_equal(tab[0, :, 1, 1], X[2, :, 1])
    assert np.array_equal(tab[0, :, 0, 2], np.cos(X[1, :, 2])) and np.array_equal(tab[0, :, 0, 3], np.sin(X[1, :, 2]))
    assert np.array_equal(tab[0, :, 0, 4:7], np.broadcast_to(shape[1, :3], (N, 3)))
    assert np.array_equal(tab[3, :, 0, 7], shape[4, 3] * (X[3, :, 3] - X[4, :, 3]))
    assert not tab[1, :, 1].any() and not tab[2, :, 0].any() and not tab[4].any() and tab[2, :, 1].any()
    # a table the gather made passes the binder's row rule whenever shape does: A, kx, ky copied, alpha != 0 only with kx > 0
    assert (tab[..., 4:7] >= 0).all()


def test_front_ends_carry_the_new_entry_points():
    from model_predictive_control_amd.controller import MPCController
    for name in ("set_agent_fields", "clear_agent_fields", "fields_from_plans", "closed_loop_traffic_field"):
        assert callable(getattr(mp.BatchedMPC, name))
    assert isinstance(inspect.getattr_static(mp.BatchedMPC, "agent_fields_bound"), property)
    assert list(inspect.signature(mp.BatchedMPC.set_agent_fields).parameters) == ["self", "table", "index"]
    assert list(inspect.signature(mp.BatchedMPC.fields_from_plans).parameters) == ["self", "X", "opp", "shape", "out"]
    par = list(inspect.signature(mp.BatchedMPC.closed_loop_traffic_field).parameters)
    ref = list(inspect.signature(mp.BatchedMPC.closed_loop_traffic).parameters)
    assert par == ref[:ref.index("radius") + 1] + ["shape"] + ref[ref.index("radius") + 1:]
    for fn in (MPCController.solve, MPCController.step):
        par = inspect.signature(fn).parameters
        assert "fields" in par and "field_index" in par
        assert par["fields"].default is None and par["field_index"].default is None
    code = ("import sys; sys.path.insert(0, %r); import model_predictive_control_amd as mp; "
            "from model_predictive_control_amd import controller; "
            "assert not any('oracle' in m for m in sys.modules), 'oracle imported'; "
            "assert mp.field_rows([1.0, 0.5], 0.0, [0.3, 0.0], 0.15, 0.06).shape == (1, 1, 2, 8)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ----------------------------------------------------------------------------- the recorded reference solves
def test_golden_file_meets_its_own_conditions(O):
    """tests/golden/fields_reference.npz as tests/golden/make_fields_golden.py writes it: all scenes and shifts there, the
    three starts of every NONE-handle agent (the third drawn in the whole input box) within 1e-8 of each other (the maker
    refuses to write otherwise), projected
    gradients at rounding level, the source does push the plan off the line (0.05 and more), the LANE scenes have active
    multipliers; and agent 0 of the standing scene solved again here is the recorded one"""
    from conftest import GOLDEN
    ref = np.load(os.path.join(GOLDEN, "fields_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts()) and float(ref["lane_hw"]) == F.LANE_HW == 0.10
    assert np.array_equal(ref["source"], [0.3, 0.15, 0.06])
    for name in ("standing", "moving", "pacejka"):
        N = D.SCENES[name][1]
        assert ref[f"U_none_{name}"].shape == (D.NSHIFT, 2 * N)
        assert ref[f"spread_none_{name}"].max() <= 1e-8 and ref[f"pg_none_{name}"].max() <= 1e-10
        assert ref[f"dev_none_{name}"].min() > 0.05
    for name in ("standing", "pacejka"):
        N = D.SCENES[name][1]
        assert ref[f"U_lane_{name}"].shape == (F.LANE_SHIFTS, 2 * N) and ref[f"lam_lane_{name}"].shape == (F.LANE_SHIFTS, N)
        assert (ref[f"lam_lane_{name}"] != 0).any(1).all() and ref[f"spread_lane_{name}"].max() <= 2.5e-5
    model, N, x0, row = F.scene_row("standing")
    assert row[:, 1, 4].tolist() == [0.0] * N and (row[:, 0, 4] == 0.3).all()
    cfg = O.default_config(model, N, constr_mode=O.CONSTR_NONE)
    U = F.reference_solve(O, cfg, F.machine(O, model, N), x0, D.line_centerline(), row)
    assert np.abs(U - ref["U_none_standing"][0]).max() <= 1e-10
    # the whole box, as the issue words the third start
    s = np.stack([F.starts(N, b)[2] for b in range(D.NSHIFT)]).reshape(-1, 2)
    assert s[:, 0].min() < -0.9 and s[:, 0].max() > 0.9 and s[:, 1].min() < -0.29 and s[:, 1].max() > 0.29
    # the mirror loop of the traffic loop: two scenes of three cars, the rear one past the slow one before the end, a selection
    # margin no 1e-4 state difference flips
    B, Tn = 3 * F.TRAFFIC_SCENES, F.TRAFFIC_T
    assert np.array_equal(ref["traffic_X0"], F.traffic_scenes()[0]) and ref["traffic_traj_x"].shape == (B, Tn, 4)
    assert ref["traffic_traj_opp"].shape == (B, Tn, F.NFIELD) and ref["traffic_margin"].min() >= 1e-3
    tx = ref["traffic_traj_x"]
    assert (tx[0::3, -1, 0] > tx[1::3, -1, 0]).all() and (tx[0::3, 0, 0] < tx[1::3, 0, 0]).all()
    assert (ref["traffic_traj_opp"][3:, :, 0][ref["traffic_traj_opp"][3:, :, 0] >= 0] >= 3).all()      # global indices
