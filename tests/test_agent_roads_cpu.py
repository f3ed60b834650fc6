"""CPU tests of the per-agent road table (mpc_set_agent_roads): the checker of tests/road_common.py has the gradient of its
own psi, the term is what the header says on numbers worked by hand, the header declares the API and the library exports
it, the default row is zeros, the host-side table builder puts its arguments in the documented columns and refuses what
the binder refuses, mpc_roads_from_script has a numpy mirror, the recorded reference solves meet their own conditions, and
the front ends carry the new entry points.  No compute call is made here."""
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
import rate_common as R
import road_common as W

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


# ----------------------------------------------------------------------------- the checker
def _live_row(N):
    """every part active at every stage on a car 0.12 beside the line y = 0.5 (e about -0.12: below lo) -- and, on the
    second half of the horizon, on the other side of a band moved under it (above hi)"""
    k = np.arange(N)
    lo = np.where(k < N // 2, -0.05, -0.30)
    hi = np.where(k < N // 2, 0.05, -0.20)
    return W.rows(N, offset=0.04, w_offset=3.0, lo=lo, w_lo=40.0, hi=hi, w_hi=30.0, v_target=0.9, w_speed=2.0)


@pytest.mark.parametrize("model,N,mode", [(0, 20, "none"), (0, 20, "state_sq"), (0, 20, "lane"), (0, 1, "none"), (0, 2, "lane"),
                                          (1, 12, "none"), (1, 12, "lane")])
def test_checker_gradient_agrees_with_central_differences(O, model, N, mode):
    """within 1e-7 relative to ||grad psi|| (h = 1e-6), every part of the term active and a visible part of the gradient
    (asserted)"""
    rng = np.random.default_rng(11 + N)
    kw = dict(none=dict(constr_mode=O.CONSTR_NONE), state_sq=dict(constr_mode=O.CONSTR_STATE_SQ),
              lane=dict(constr_mode=O.CONSTR_LANE, lane_halfwidth=0.05))[mode]
    cfg = O.default_config(model, N, **kw)
    mach = W.machine(O, model, N)
    x0 = R.X0_PAC if model else R.X0_KIN
    cl = D.line_centerline()
    U = np.tile([0.6, 0.0], N) + rng.uniform(-.3, .3, 2 * N) * np.tile([1.0, 0.3], N)
    row = _live_row(N)
    m = O.m(cfg)
    y = rng.uniform(-1.0, 1.0, m) if m else None
    Sig = 10 ** rng.uniform(0, 2, m) if m else None
    p, g = W.psi(O, cfg, mach, x0, cl, U, row, y, Sig)
    p0, g0 = O.psi(cfg, x0, cl, U, y, Sig)
    t, tg = W.road_term(O, mach, x0, cl, U, row)
    assert p == p0 + t and t > 0 and np.linalg.norm(tg) > 1e-2 * np.linalg.norm(g)
    e = O.constraints(mach[2], x0, cl, U)
    X = O.rollout(mach[0], x0, U)
    assert np.allclose(e, -(X[:, 1] - 0.5), atol=1e-14)                    # the sign: positive to the right
    assert (e[:max(1, N // 2)] < -0.05).all() and (N < 4 or (e[N // 2:] > -0.20).all())     # below lo, then above hi
    fd = W.psi_fd_grad(lambda u: W.psi(O, cfg, mach, x0, cl, u, row, y, Sig, want_grad=False)[0], U)
    err = np.abs(fd - g).max() / np.linalg.norm(g)
    print(f"model {model} N {N} {mode}: checker vs central differences {err:.2e}")
    assert err <= 1e-7


def test_checker_beside_the_other_tables(O):
    """the rate, field and disc terms add up with the road term: psi is the sum, the gradient agrees with differences"""
    import field_common as F
    N, model = 20, 0
    rng = np.random.default_rng(3)
    mach = W.machine(O, model, N)
    x0, cl = R.X0_KIN, D.line_centerline()
    U = np.tile([0.6, 0.0], N) + rng.uniform(-.3, .3, 2 * N) * np.tile([1.0, 0.3], N)
    row, rate = _live_row(N), np.array([0.3, 2.0, 0.1, -0.05])
    fld = F.source_rows(N, (1.3, 0.6), 0.1, 0.3, (0.15, 0.06), 0.5)
    p, g = W.psi(O, mach[0], mach, x0, cl, U, row, rate_row=rate, field_row=fld)
    assert np.isclose(p, O.psi(mach[0], x0, cl, U)[0] + W.road_term(O, mach, x0, cl, U, row, False)[0] + R.rate_term(U, rate, False)[0] +
                      F.field_term(O, mach[:2], x0, cl, U, fld, False)[0], rtol=1e-14)
    fd = W.psi_fd_grad(lambda u: W.psi(O, mach[0], mach, x0, cl, u, row, rate_row=rate, field_row=fld, want_grad=False)[0], U)
    assert np.abs(fd - g).max() / np.linalg.norm(g) <= 1e-7
    discs = D.scene_standing(N)
    yv, Sg = rng.uniform(-1, 0, 2 * N), 10 ** rng.uniform(0, 2, 2 * N)
    p, _, g, _ = W.psi_discs(O, mach, x0, cl, U, discs, yv, Sg, row, rate)
    fd = W.psi_fd_grad(lambda u: W.psi_discs(O, mach, x0, cl, u, discs, yv, Sg, row, rate, False)[0], U)
    assert np.abs(fd - g).max() / np.linalg.norm(g) <= 1e-7


def test_term_by_hand():
    """numbers whose products are exact; a part with weight 0 adds nothing whatever the word beside it says"""
    X = np.array([[1.0, 0.5, 0.0, 0.75], [1.1, 0.5, 0.0, 0.5], [1.2, 0.5, 0.0, 1.0]])
    e = np.array([0.25, -0.5, 0.125])
    row = np.array([[0.0, 2.0, 9.0, 0.0, 0.125, 4.0, 0.25, 8.0],           # target and upper edge: 2 / 16 + 4 / 64, speed 8 / 4
                    [9.0, 0.0, -0.25, 16.0, 9.0, 0.0, 9.0, 0.0],           # lower edge alone: 16 / 16
                    [0.125, 2.0, 0.0, 4.0, 0.25, 4.0, 1.0, 2.0]])          # inside the road, on every target: nothing
    t, de, dv = W.road_values(e, X, row)
    assert t == (0.125 + 0.0625 + 2.0) + 1.0 + 0.0
    assert de.tolist() == [2 * 2 * 0.25 + 2 * 4 * 0.125, 2 * 16 * -0.25, 0.0] and dv.tolist() == [2 * 8 * 0.5, 0.0, 0.0]
    assert W.road_values(e, X, np.zeros((3, 8)))[0] == 0.0
    Xp = np.array([[1.0, 0.5, 0.0, 0.6, 0.8, 0.0]])                        # Pacejka: sp = 1
    assert W.road_values(e[:1], Xp, W.rows(1, v_target=0.5, w_speed=4.0))[0] == 1.0


# ----------------------------------------------------------------------------- the API
def test_header_declares_and_library_exports_the_roads_api(L):
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert re.search(r"#define\s+MPC_NROAD\s+8\b", hdr) and re.search(r"#define\s+MPC_ROAD_ROW\(N\)\s+\(MPC_NROAD \* \(N\)\)", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mpc_default_roads\s*\(\s*const\s+mpc_config\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+mpc_set_agent_roads\s*\(\s*mpc_handle\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    for name in ("mpc_default_roads", "mpc_set_agent_roads", "mpc_roads_from_script"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.NROAD == 8 == mp.NROAD == W.NROAD
    assert len(L.mpc_default_roads.argtypes) == 2 and len(L.mpc_roads_from_script.argtypes) == 9
    assert L.mpc_set_agent_roads.argtypes == L.mpc_set_agent_fields.argtypes == L.mpc_set_agent_rates.argtypes
    # the layout, the operation order, the sign and the degenerate centerline are part of the contract
    for text in ("[off, w_off, lo, w_lo, hi, w_hi, v_tgt, w_v]", "e = ((x[0] - nx) wy - (x[1] - ny) wx) / nrm", "t = e - off,  a = w_off t",
                 "POSITIVE TO THE RIGHT", "nrm == 0", "not even a signed zero"):
        assert text in hdr, text
    src = open(os.path.join(ROOT, "model_predictive_control_amd", "csrc", "mpc_device.hpp")).read()
    assert "void road_term(" in src and "constexpr int NROAD = 8" in src


def test_null_arguments_return_codes_not_exceptions(L):
    E_ARG = -1
    cfg = mp.default_config(0, 2)
    row = (C.c_double * 16)(*([1.0] * 16))
    assert L.mpc_default_roads(None, row) == E_ARG and b"mpc_default_roads" in L.mpc_last_error()
    assert L.mpc_default_roads(C.byref(cfg), None) == E_ARG
    assert L.mpc_default_roads(C.byref(cfg), row) == 0 and list(row) == [0.0] * 16
    bad = mp.default_config(0, 2)
    bad.N = 0
    assert L.mpc_default_roads(C.byref(bad), row) == E_ARG and b"out of range" in L.mpc_last_error()
    assert L.mpc_set_agent_roads(None, None, 0, None, 0) == E_ARG
    assert b"mpc_set_agent_roads" in L.mpc_last_error()
    assert L.mpc_set_agent_roads(None, C.c_void_p(8), 1, C.c_void_p(8), 1) == E_ARG     # (nothing is dereferenced)
    p = C.c_void_p(8)
    assert L.mpc_roads_from_script(None, 1, 4, 0, 0, p, p, p, None) == E_ARG and b"null handle" in L.mpc_last_error()
    for args, why in (((-1, 4, 0, 0, p, p, p), b"negative batch"), ((1, 0, 0, 0, p, p, p), b"Lt must be >= 1"),
                      ((1, 4, 0, -1, p, p, p), b"ti must be >= 0"), ((1, 4, 0, 0, None, p, p), b"null script"),
                      ((1, 4, 0, 0, p, None, p), b"null script"), ((1, 4, 0, 0, p, p, None), b"null script")):
        assert L.mpc_roads_from_script(None, *args, None) == E_ARG
        assert b"mpc_roads_from_script" in L.mpc_last_error() and why in L.mpc_last_error(), (args, L.mpc_last_error())


def test_road_rows(L):
    N = 12
    d = _lib.default_roads(mp.default_config(1, N))
    assert not d.any() and d.shape == (8 * N,) and mp.road_rows is _lib.road_rows and mp.default_roads is _lib.default_roads
    tab = _lib.road_rows(N)
    assert tab.shape == (1, N, 8) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"] and not tab.any()
    tab = _lib.road_rows(N, offset=-0.1, w_offset=5.0, lo=-0.05, w_lo=50.0, hi=0.05, w_hi=40.0, v_target=0.8, w_speed=2.0)
    assert tab.shape == (1, N, 8) and all(np.array_equal(r, [-0.1, 5.0, -0.05, 50.0, 0.05, 40.0, 0.8, 2.0]) for r in tab[0])
    P = 3
    rng = np.random.default_rng(0)
    off, wv = rng.uniform(-1, 1, (P, N)), rng.uniform(0, 1, (P, 1))
    vt = np.linspace(0.8, 0.3, N)
    tab = _lib.road_rows(N, offset=off, w_offset=1.0, v_target=vt, w_speed=wv)
    assert tab.shape == (P, N, 8) and np.array_equal(tab[..., 0], off) and (tab[..., 1] == 1.0).all()
    assert np.array_equal(tab[..., 6], np.broadcast_to(vt, (P, N))) and np.array_equal(tab[..., 7], np.broadcast_to(wv, (P, N)))
    assert not tab[..., 2:6].any()
    assert np.array_equal(_lib.road_rows(N, lo=W.rows(N, lo=-0.05)[:, 2], w_lo=50.0, hi=0.05, w_hi=50.0)[0],
                          W.rows(N, lo=-0.05, w_lo=50.0, hi=0.05, w_hi=50.0))                  # the checker's layout
    # lo > hi is refused only where both edges are on
    assert _lib.road_rows(N, lo=0.1, w_lo=1.0, hi=0.0).shape == (1, N, 8)
    assert _lib.road_rows(N, lo=0.1, hi=0.0, w_hi=1.0).shape == (1, N, 8)
    for bad in (dict(w_offset=-1e-3), dict(w_lo=-1.0), dict(w_hi=-1.0), dict(w_speed=-1.0), dict(offset=float("nan")),
                dict(v_target=float("inf")), dict(w_lo=float("nan")), dict(lo=0.1, w_lo=1.0, hi=0.0, w_hi=1.0),
                dict(offset=np.zeros(N + 1)), dict(offset=np.zeros((2, N)), lo=np.zeros((3, N))), dict(offset=np.zeros((1, 1, N)))):
        with pytest.raises(ValueError):
            _lib.road_rows(N, **bad)
    with pytest.raises(ValueError):
        _lib.road_rows(0)


def test_script_mirror():
    """the numpy mirror of mpc_roads_from_script: stage k gets sample min(ti + k, Lt - 1), or (ti + k) mod Lt with wrap"""
    rng = np.random.default_rng(5)
    Ps, Lt, N = 3, 7, 5
    script = rng.uniform(0, 1, (Ps, Lt, 8))
    idx = np.array([2, 0, 0, 1])
    w = W.script_window(script, idx, 0, N)
    assert w.shape == (4, N, 8) and np.array_equal(w[0], script[2, :N]) and np.array_equal(w[2], script[0, :N])
    w = W.script_window(script, idx, 4, N)                                  # runs off the end: the last sample is held
    assert np.array_equal(w[3, :3], script[1, 4:7]) and np.array_equal(w[3, 3], script[1, 6]) and np.array_equal(w[3, 4], script[1, 6])
    assert (W.script_window(script, idx, 100, N) == script[idx][:, -1:]).all()
    w = W.script_window(script, idx, 4, N, wrap=True)
    assert np.array_equal(w[3, :3], script[1, 4:7]) and np.array_equal(w[3, 3:], script[1, 0:2])
    assert np.array_equal(W.script_window(script, idx, 7 * 9 + 2, N, wrap=True), W.script_window(script, idx, 2, N, wrap=True))


def test_front_ends_carry_the_new_entry_points():
    from model_predictive_control_amd.controller import MPCController
    for name in ("set_agent_roads", "clear_agent_roads", "roads_from_script"):
        assert callable(getattr(mp.BatchedMPC, name))
    assert isinstance(inspect.getattr_static(mp.BatchedMPC, "agent_roads_bound"), property)
    assert list(inspect.signature(mp.BatchedMPC.set_agent_roads).parameters) == ["self", "table", "index"]
    assert list(inspect.signature(mp.BatchedMPC.roads_from_script).parameters) == ["self", "script", "index", "ti", "wrap", "out"]
    assert list(inspect.signature(_lib.road_rows).parameters) == ["N", "offset", "w_offset", "lo", "w_lo", "hi", "w_hi", "v_target", "w_speed"]
    for fn in (MPCController.solve, MPCController.step):
        par = inspect.signature(fn).parameters
        names = list(par)
        assert par["roads"].default is None and par["road_index"].default is None
        assert names[names.index("roads"):names.index("roads") + 3] == ["roads", "road_index", "fields"]
    for name in ("NROAD", "default_roads", "road_rows"):
        assert name in mp.__all__
    code = ("import sys; sys.path.insert(0, %r); import model_predictive_control_amd as mp; "
            "from model_predictive_control_amd import controller; "
            "assert not any('oracle' in m for m in sys.modules), 'oracle imported'; "
            "assert mp.road_rows(4, w_offset=1.0).shape == (1, 4, 8)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ----------------------------------------------------------------------------- the recorded reference solves
def test_golden_file_meets_its_own_conditions(O):
    """tests/golden/roads_reference.npz as tests/golden/make_roads_golden.py writes it: all scenes and shifts there, the
    three starts of every agent (the third drawn in the whole input box) within 1e-8 of each other (the maker refuses to
    write otherwise), residuals at rounding level, and the effects the scenes are there to show, with margins: `change`
    ends more than 0.05 off the line where the plan without the table stays on it; `edges` and `pacejka` end nearer the
    line than without the table and within 0.01 of the road's edge; `brake` ends below 0.6 where the plan without the table
    is above 0.9; `disc_road` has active multipliers and controls more than 0.05 from the solve of the discs alone.  Agent 0
    of `change` solved again here is the recorded one, and so is the mirror loop of the lane change commanded in time."""
    from conftest import GOLDEN
    ref = np.load(os.path.join(GOLDEN, "roads_reference.npz"))
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    cl = D.line_centerline()
    end = {}
    for name, (model, N, x0, handle) in W.SCENES.items():
        nb = W.DISC_SHIFTS if handle == "discs" else D.NSHIFT
        assert ref[f"U_{name}"].shape == (nb, 2 * N) and ref[f"base_{name}"].shape == (2 * N,)
        assert ref[f"spread_{name}"].max() <= 1e-8 and ref[f"pg_{name}"].max() <= 1e-9, (name, ref[f"spread_{name}"].max(), ref[f"pg_{name}"].max())
        c0 = W.machine(O, model, N)[0]
        Xr, Xb = O.rollout(c0, x0, ref[f"U_{name}"][0]), O.rollout(c0, x0, ref[f"base_{name}"])
        end[name] = (Xr[-1, 1], Xb[-1, 1], W.speed(Xr)[-1], W.speed(Xb)[-1])
        print(name, "end of the plan: y %.4f (without %.4f), speed %.4f (without %.4f)" % end[name])
    assert end["change"][0] - 0.5 > 0.05 and abs(end["change"][1] - 0.5) < 0.005
    for name in ("edges", "pacejka"):
        assert 0.5 < end[name][0] < 0.5 + W.EDGE_HALF + 0.01 and end[name][1] > end[name][0] + 0.02
    assert end["brake"][2] < 0.6 and end["brake"][3] > 0.9
    assert ref["lam_disc_road"].shape == (W.DISC_SHIFTS, 2 * 20) and (ref["lam_disc_road"] != 0).any(1).all()
    assert ref["viol_disc_road"].max() <= 1e-8 and ref["lamspread_disc_road"].max() <= 1e-6
    assert np.abs(ref["U_disc_road"][0] - ref["base_disc_road"]).max() > 0.05
    model, N, x0, row, _ = W.scene_row("change")
    assert (row[:W.CHANGE_AT, 0] == 0.0).all() and (row[W.CHANGE_AT:, 0] == -0.10).all() and (row[:, 1] == 5.0).all()
    mach = W.machine(O, model, N)
    U = W.reference_solve(O, mach[0], mach, x0, cl, row)
    assert np.abs(U - ref["U_change"][0]).max() <= 1e-10
    # the lane change commanded in time: the mirror loop run again here is the record; before the command (sample 8) the six
    # realised states move towards the new lane step by step and stay nearer the old one, the last plan ends nearer the new
    tx, plan = W.mirror_script_loop(O)
    assert ref["script_traj_x"].shape == (W.SCRIPT_T, 4) and ref["script_last_plan"].shape == (20, 4)
    assert np.abs(tx - ref["script_traj_x"]).max() <= 1e-10 and np.abs(plan - ref["script_last_plan"]).max() <= 1e-10
    off = tx[:, 1] - 0.5
    assert (np.diff(off) > 0).all() and 0 < off[0] < 0.01 and off[-1] < 0.03 and plan[-1, 1] - 0.5 > 0.05
    s = W.lane_change_script()
    assert s.shape == (1, W.SCRIPT_LT, 8) and (s[0, :W.SCRIPT_AT, 0] == 0).all() and (s[0, W.SCRIPT_AT:, 0] == -0.10).all()
    # the whole box, as the third start is worded
    s = np.stack([W.starts(N, b)[2] for b in range(D.NSHIFT)]).reshape(-1, 2)
    assert s[:, 0].min() < -0.9 and s[:, 0].max() > 0.9 and s[:, 1].min() < -0.29 and s[:, 1].max() > 0.29
