"""CPU tests of the per-agent parameter table (mpc_set_agent_params): the header declares it, the library exports
it, the default row is the configuration's, the host-side table builder puts overrides in the documented columns, and
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

import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_table_api(L):
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert re.search(r"#define\s+MPC_NPARAM\s+31\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("mpc_default_params", "mpc_set_agent_params"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.NPARAM == 31 and mp.NPARAM == 31
    # the documented columns cover the row exactly once
    cols = sorted(_lib.PARAM_FIELDS.values())
    assert cols == [(0, 22), (22, 1), (23, 1), (24, 1), (25, 6)] and sum(w for _, w in cols) == _lib.NPARAM


@pytest.mark.parametrize("model", [0, 1])
def test_default_row_is_the_configuration(L, O, model):
    """mpc_default_params(mpc_default_config(model, N)) == the oracle's independent default table, field for field."""
    N = 12 if model else 20
    row = _lib.default_params(mp.default_config(model, N))
    ocfg = O.default_config(model, N)
    assert row.shape == (31,) and row.dtype == np.float64
    assert list(row[0:22]) == list(ocfg.veh)
    assert row[22] == ocfg.accel and row[23] == ocfg.friction and row[24] == ocfg.v_ref
    assert list(row[25:31]) == list(ocfg.cost_w)
    # overrides of the configuration show up in the row
    veh = [float(i + 1) for i in range(22)]
    cfg = mp.default_config(model, N, veh=veh, accel=3.5, friction=0.25, v_ref=1.75, cost_w=[6, 5, 4, 3, 2, 1])
    row = _lib.default_params(cfg)
    assert list(row) == veh + [3.5, 0.25, 1.75, 6, 5, 4, 3, 2, 1]


def test_null_arguments_return_codes_not_exceptions(L):
    E_ARG = -1
    row = (C.c_double * 31)()
    cfg = mp.default_config(0, 20)
    assert L.mpc_default_params(None, row) == E_ARG and b"mpc_default_params" in L.mpc_last_error()
    assert L.mpc_default_params(C.byref(cfg), None) == E_ARG
    assert L.mpc_default_params(C.byref(cfg), row) == 0
    assert L.mpc_set_agent_params(None, None, 0, None, None, 0) == E_ARG
    assert b"mpc_set_agent_params" in L.mpc_last_error()
    assert L.mpc_set_agent_params(None, C.c_void_p(8), 1, C.c_void_p(8), None, 1) == E_ARG   # (nothing is dereferenced)


def test_param_rows(L):
    cfg = mp.default_config(1, 12, v_ref=1.25)
    base = _lib.default_params(cfg)
    P = 5
    tab = _lib.param_rows(cfg, P)
    assert tab.shape == (P, 31) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(tab[p], base) for p in range(P))
    rng = np.random.default_rng(0)
    veh = np.tile(base[:22], (P, 1)); veh[1:] *= rng.uniform(.8, 1.2, (P - 1, 22))
    cw = np.tile(base[25:], (P, 1)); cw[1:] *= rng.uniform(.8, 1.2, (P - 1, 6))
    vr = np.array([1.25, .7, .8, .9, 1.1]); ac = np.array([2.0, 1.5, 1.6, 1.7, 1.8]); fr = np.array([1.0, .7, .8, .9, 1.3])
    tab = _lib.param_rows(cfg, P, veh=veh, cost_w=cw, v_ref=vr, accel=ac, friction=fr)
    assert np.array_equal(tab[0], base)                                   # row 0 untouched by identity overrides
    assert np.array_equal(tab[:, 0:22], veh) and np.array_equal(tab[:, 25:31], cw)
    assert np.array_equal(tab[:, 22], ac) and np.array_equal(tab[:, 23], fr) and np.array_equal(tab[:, 24], vr)
    # one value for every row
    tab = _lib.param_rows(cfg, 3, v_ref=0.5, cost_w=[1, 2, 3, 4, 5, 6])
    assert np.array_equal(tab[:, 24], [0.5] * 3) and np.array_equal(tab[:, 25:], np.tile([1., 2, 3, 4, 5, 6], (3, 1)))
    assert np.array_equal(tab[:, :24], np.tile(base[:24], (3, 1)))
    assert mp.param_rows is _lib.param_rows
    for bad in (dict(mass=[1.0] * P), dict(veh=np.zeros((P, 21))), dict(cost_w=np.zeros((P + 1, 6))), dict(v_ref=np.zeros(P + 1)),
                dict(accel=np.zeros((P, 1)))):
        with pytest.raises(ValueError):
            _lib.param_rows(cfg, P, **bad)
    with pytest.raises(ValueError):
        _lib.param_rows(cfg, 0)


def test_front_ends_carry_the_new_entry_points():
    from model_predictive_control_amd.controller import MPCController
    for name in ("set_agent_params", "clear_agent_params"):
        assert callable(getattr(mp.BatchedMPC, name))
    assert isinstance(inspect.getattr_static(mp.BatchedMPC, "agent_params_bound"), property)
    assert list(inspect.signature(mp.BatchedMPC.set_agent_params).parameters) == ["self", "table", "index", "plant_index"]
    for fn in (MPCController.solve, MPCController.step):
        par = inspect.signature(fn).parameters
        assert "params" in par and "param_index" in par
        assert par["params"].default is None and par["param_index"].default is None
    # the package imports without a GPU and without the oracle
    code = ("import sys; sys.path.insert(0, %r); import model_predictive_control_amd as mp; "
            "from model_predictive_control_amd import controller; "
            "assert not any('oracle' in m for m in sys.modules), 'oracle imported'; "
            "assert mp.param_rows(mp.default_config(0, 20), 2).shape == (2, 31)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])
