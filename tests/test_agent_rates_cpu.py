"""CPU tests of the per-agent rate table (mpc_set_agent_rates): the checker of tests/rate_common.py has the gradient of its
own psi, the header declares the API, the library exports it with the argument types of the other setters, the default
row is zeros, the host-side table builder puts its arguments in the documented columns and refuses what the binder
refuses, and the front ends carry the new entry points.  No compute call is made here."""
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

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


# ----------------------------------------------------------------------------- the checker
@pytest.mark.parametrize("model,N,mode", [(0, 20, "none"), (1, 12, "none"), (0, 1, "none"), (0, 2, "none"), (0, 20, "state_sq"),
                                          (0, 20, "lane")])
def test_checker_gradient_agrees_with_central_differences(O, model, N, mode):
    """within 1e-6 relative to ||grad psi||, the bar of the issue; weights (0.5, 5.0) and a u_prev away from u_0, so that the
    term is a visible part of the gradient (asserted)"""
    rng = np.random.default_rng(3 + N)
    kw = dict(none=dict(constr_mode=O.CONSTR_NONE), state_sq=dict(constr_mode=O.CONSTR_STATE_SQ),
              lane=dict(constr_mode=O.CONSTR_LANE, lane_halfwidth=0.05))[mode]
    cfg = O.default_config(model, N, **kw)
    x0 = R.X0_PAC if model else R.X0_KIN
    cl = D.line_centerline()
    U = np.tile([0.6, 0.0], N) + rng.uniform(-.3, .3, 2 * N) * np.tile([1.0, 0.3], N)
    row = np.array([0.5, 5.0, -0.4, 0.2])
    m = O.m(cfg)
    y = rng.uniform(-1.0, 1.0, m) if m else None
    Sig = 10 ** rng.uniform(0, 2, m) if m else None
    p, g = R.psi(O, cfg, x0, cl, U, row, y, Sig)
    p0, g0 = O.psi(cfg, x0, cl, U, y, Sig)
    t, tg = R.rate_term(U, row)
    assert p == p0 + t and t > 0 and np.linalg.norm(tg) > 1e-2 * np.linalg.norm(g)
    fd = R.psi_fd_grad(O, cfg, x0, cl, U, row, y, Sig)
    err = np.abs(fd - g).max() / np.linalg.norm(g)
    print(f"model {model} N {N} {mode}: checker vs central differences {err:.2e}")
    assert err <= 1e-6


def test_term_by_hand():
    """N = 2 written out in binary fractions (every operation exact); zero weights give an exact zero whatever u_prev is"""
    U = np.array([0.5, 0.125, -0.25, 0.375])
    row = np.array([2.0, 3.0, 1.0, -0.125])
    t, g = R.rate_term(U, row)
    e0, e1 = np.array([-0.5, 0.25]), np.array([-0.75, 0.25])
    assert t == 2 * 0.25 + 3 * 0.0625 + 2 * 0.5625 + 3 * 0.0625 == 2.0
    assert np.array_equal(g, np.concatenate([2 * row[:2] * e0 - 2 * row[:2] * e1, 2 * row[:2] * e1]))
    assert np.array_equal(g, [1.0, 0.0, -3.0, 1.5])
    t1, g1 = R.rate_term(U[:2], row)                     # N = 1: u_{-1} alone, no successor
    assert t1 == 2 * 0.25 + 3 * 0.0625 and np.array_equal(g1, 2 * row[:2] * e0)
    t0, g0 = R.rate_term(U, np.array([0.0, 0.0, 0.7, -0.3]))
    assert t0 == 0.0 and not g0.any()


# ----------------------------------------------------------------------------- the API
def test_header_declares_and_library_exports_the_rates_api(L):
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert re.search(r"#define\s+MPC_NRATE\s+4\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mpc_default_rates\s*\(\s*const\s+mpc_config\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+mpc_set_agent_rates\s*\(\s*mpc_handle\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    for name in ("mpc_default_rates", "mpc_set_agent_rates"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.NRATE == 4 and mp.NRATE == 4
    assert len(L.mpc_default_rates.argtypes) == 2
    assert L.mpc_set_agent_rates.argtypes == L.mpc_set_agent_bounds.argtypes == L.mpc_set_agent_discs.argtypes
    assert L.mpc_set_agent_rates.argtypes[2] is C.c_int and L.mpc_set_agent_rates.argtypes[4] is C.c_int
    # the operation order is part of the contract
    assert "t_i = w_i e_i" in hdr and "P == B" in hdr


def test_null_arguments_return_codes_not_exceptions(L):
    E_ARG = -1
    row = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    cfg = mp.default_config(0, 20)
    assert L.mpc_default_rates(None, row) == E_ARG and b"mpc_default_rates" in L.mpc_last_error()
    assert L.mpc_default_rates(C.byref(cfg), None) == E_ARG
    assert L.mpc_default_rates(C.byref(cfg), row) == 0 and list(row) == [0.0] * 4
    assert L.mpc_set_agent_rates(None, None, 0, None, 0) == E_ARG
    assert b"mpc_set_agent_rates" in L.mpc_last_error()
    assert L.mpc_set_agent_rates(None, C.c_void_p(8), 1, C.c_void_p(8), 1) == E_ARG   # (nothing is dereferenced)
    assert L.mpc_set_agent_rates(None, C.c_void_p(8), 1, None, 1) == E_ARG


def test_rate_rows(L):
    assert list(_lib.default_rates(mp.default_config(1, 12))) == [0.0] * 4
    tab = _lib.rate_rows(0.1, 1.0)
    assert tab.shape == (1, 4) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"] and list(tab[0]) == [0.1, 1.0, 0.0, 0.0]
    tab = _lib.rate_rows(0.5, 5.0, [0.3, -0.1])
    assert list(tab[0]) == [0.5, 5.0, 0.3, -0.1]
    P = 5
    rng = np.random.default_rng(0)
    wd, wl, up = rng.uniform(0, 1, P), rng.uniform(0, 5, P), rng.uniform(-.3, .3, (P, 2))
    tab = _lib.rate_rows(wd, wl, up)
    assert tab.shape == (P, 4) and np.array_equal(tab[:, 0], wd) and np.array_equal(tab[:, 1], wl) and np.array_equal(tab[:, 2:], up)
    tab = _lib.rate_rows(0.0, wl)                                        # a scalar beside [P]: every row's
    assert tab.shape == (P, 4) and not tab[:, 0].any() and np.array_equal(tab[:, 1], wl) and not tab[:, 2:].any()
    tab = _lib.rate_rows(0.2, 0.3, up)
    assert tab.shape == (P, 4) and (tab[:, 0] == 0.2).all() and np.array_equal(tab[:, 2:], up)
    assert mp.rate_rows is _lib.rate_rows and mp.default_rates is _lib.default_rates
    for bad in (dict(w_d=-1e-3, w_delta=1.0), dict(w_d=0.1, w_delta=float("nan")), dict(w_d=float("inf"), w_delta=0.0),
                dict(w_d=0.1, w_delta=1.0, u_prev=[0.0, float("inf")]), dict(w_d=0.1, w_delta=1.0, u_prev=[float("nan"), 0.0]),
                dict(w_d=0.1, w_delta=1.0, u_prev=[0.0, 0.0, 0.0]), dict(w_d=np.zeros(3), w_delta=np.zeros(4)),
                dict(w_d=np.zeros(3), w_delta=1.0, u_prev=np.zeros((2, 2))), dict(w_d=np.zeros((2, 2)), w_delta=1.0),
                dict(w_d=np.zeros(0), w_delta=1.0)):
        with pytest.raises(ValueError):
            _lib.rate_rows(**bad)


def test_front_ends_carry_the_new_entry_points():
    from model_predictive_control_amd.controller import MPCController
    for name in ("set_agent_rates", "clear_agent_rates"):
        assert callable(getattr(mp.BatchedMPC, name))
    assert isinstance(inspect.getattr_static(mp.BatchedMPC, "agent_rates_bound"), property)
    assert list(inspect.signature(mp.BatchedMPC.set_agent_rates).parameters) == ["self", "table", "index"]
    for fn in (MPCController.solve, MPCController.step):
        par = inspect.signature(fn).parameters
        assert "rates" in par and "rate_index" in par
        assert par["rates"].default is None and par["rate_index"].default is None
        assert list(par)[:len(inspect.signature(fn).parameters) - 2][-2:] == ["discs", "disc_index"]   # behind the older kinds
    code = ("import sys; sys.path.insert(0, %r); import model_predictive_control_amd as mp; "
            "from model_predictive_control_amd import controller; "
            "assert not any('oracle' in m for m in sys.modules), 'oracle imported'; "
            "assert mp.rate_rows([0.1, 0.2], 1.0).shape == (2, 4)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])
