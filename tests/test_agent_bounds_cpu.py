"""CPU tests of the per-agent bounds table (mpc_set_agent_bounds): the header declares it, the library exports it, the
default row is the configuration's box, the host-side table builder puts overrides in the documented columns, the
front ends carry the new entry points, and the code object holds the per-agent-box form of every step kernel with the
resources and the argument layout the shared form has.  No compute call is made here."""
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
from codeobj_common import STEP_LEAN_TARGS, _waves_by_vgprs, built_library_kernels, step_form, step_forms
from model_predictive_control_amd import _lib

STEP_LDS_BYTES = 264                              # s_req[64] + s_next (+ padding), as the shared kernel
LEAN_WAVES_PER_SIMD = 5                           # the shared lean kernel's target, and this one's


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_bounds_api(L):
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert re.search(r"#define\s+MPC_NBOUND\s+4\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mpc_default_bounds\s*\(\s*const\s+mpc_config\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+mpc_set_agent_bounds\s*\(\s*mpc_handle\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    for name in ("mpc_default_bounds", "mpc_set_agent_bounds"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.NBOUND == 4 and mp.NBOUND == 4
    assert len(L.mpc_default_bounds.argtypes) == 2 and len(L.mpc_set_agent_bounds.argtypes) == 5
    assert L.mpc_set_agent_bounds.argtypes[2] is C.c_int and L.mpc_set_agent_bounds.argtypes[4] is C.c_int


@pytest.mark.parametrize("model", [0, 1])
def test_default_row_is_the_configurations_box(L, O, model):
    N = 12 if model else 20
    row = _lib.default_bounds(mp.default_config(model, N))
    ocfg = O.default_config(model, N)
    assert row.shape == (4,) and row.dtype == np.float64
    assert list(row) == [ocfg.u_lb[0], ocfg.u_lb[1], ocfg.u_ub[0], ocfg.u_ub[1]] == [-1.0, -0.32, 1.0, 0.32]
    cfg = mp.default_config(model, N, u_lb=[-0.6, -0.11], u_ub=[0.7, float("inf")])
    assert list(_lib.default_bounds(cfg)) == [-0.6, -0.11, 0.7, float("inf")]


def test_null_arguments_return_codes_not_exceptions(L):
    E_ARG = -1
    row = (C.c_double * 4)()
    cfg = mp.default_config(0, 20)
    assert L.mpc_default_bounds(None, row) == E_ARG and b"mpc_default_bounds" in L.mpc_last_error()
    assert L.mpc_default_bounds(C.byref(cfg), None) == E_ARG
    assert L.mpc_default_bounds(C.byref(cfg), row) == 0
    assert L.mpc_set_agent_bounds(None, None, 0, None, 0) == E_ARG
    assert b"mpc_set_agent_bounds" in L.mpc_last_error()
    assert L.mpc_set_agent_bounds(None, C.c_void_p(8), 1, C.c_void_p(8), 1) == E_ARG   # (nothing is dereferenced)
    assert L.mpc_set_agent_bounds(None, C.c_void_p(8), 1, None, 1) == E_ARG


def test_bound_rows(L):
    cfg = mp.default_config(1, 12, u_lb=[-0.9, -0.3], u_ub=[0.8, 0.25])
    base = _lib.default_bounds(cfg)
    assert list(base) == [-0.9, -0.3, 0.8, 0.25]
    P = 5
    tab = _lib.bound_rows(cfg, P)
    assert tab.shape == (P, 4) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(tab[p], base) for p in range(P))
    rng = np.random.default_rng(0)
    lb = -rng.uniform(.1, 1, (P, 2)); ub = rng.uniform(.1, 1, (P, 2))
    tab = _lib.bound_rows(cfg, P, u_lb=lb, u_ub=ub)
    assert np.array_equal(tab[:, 0:2], lb) and np.array_equal(tab[:, 2:4], ub)
    tab = _lib.bound_rows(cfg, 3, u_ub=[0.5, 0.2])
    assert np.array_equal(tab, np.tile([-0.9, -0.3, 0.5, 0.2], (3, 1)))
    assert mp.bound_rows is _lib.bound_rows and mp.default_bounds is _lib.default_bounds
    for bad in (dict(u_lb=np.zeros((P, 3))), dict(u_ub=np.zeros((P + 1, 2))), dict(u_lb=np.zeros(3))):
        with pytest.raises(ValueError):
            _lib.bound_rows(cfg, P, **bad)
    with pytest.raises(ValueError):
        _lib.bound_rows(cfg, 0)


def test_front_ends_carry_the_new_entry_points():
    from model_predictive_control_amd.controller import MPCController
    for name in ("set_agent_bounds", "clear_agent_bounds"):
        assert callable(getattr(mp.BatchedMPC, name))
    assert isinstance(inspect.getattr_static(mp.BatchedMPC, "agent_bounds_bound"), property)
    assert list(inspect.signature(mp.BatchedMPC.set_agent_bounds).parameters) == ["self", "table", "index"]
    for fn in (MPCController.solve, MPCController.step):
        par = inspect.signature(fn).parameters
        assert "bounds" in par and "bound_index" in par
        assert par["bounds"].default is None and par["bound_index"].default is None
        assert "params" in par and "param_index" in par
    code = ("import sys; sys.path.insert(0, %r); import model_predictive_control_amd as mp; "
            "from model_predictive_control_amd import controller; "
            "assert not any('oracle' in m for m in sys.modules), 'oracle imported'; "
            "assert mp.bound_rows(mp.default_config(0, 20), 2).shape == (2, 4)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ------------------------------------------------------------------ the code object (tests/codeobj_common.py)
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return built_library_kernels(tmp_path_factory)


def test_lean_box_step_kernel_fits_the_shared_kernels_target(L, kernels):
    k = step_form(kernels, STEP_LEAN_TARGS, "BoxTab")       # step_kernel<1, -1, false, BoxTab>: exactly one
    assert k[".sgpr_spill_count"] == 0
    assert k[".vgpr_spill_count"] == 0
    assert k[".private_segment_fixed_size"] == 0
    assert k[".group_segment_fixed_size"] == STEP_LDS_BYTES
    assert k[".vgpr_count"] <= 512 // LEAN_WAVES_PER_SIMD // 8 * 8          # 96
    assert _waves_by_vgprs(k[".vgpr_count"] + k.get(".agpr_count", 0)) >= LEAN_WAVES_PER_SIMD
    assert k[".max_flat_workgroup_size"] == 256
    # ... which is what the host sizes the LDS copy of the history for (the plan has no box form of its own)
    for n, M in ((24, 12), (40, 20)):
        P, lds, wps = C.c_int(), C.c_int(), C.c_int()
        assert L.mpc_step_lds_plan(n, M, 0, 1, 0, C.byref(P), C.byref(lds), C.byref(wps)) == 0
        assert wps.value == LEAN_WAVES_PER_SIMD


def test_every_step_kernel_has_a_box_form_with_the_shared_argument_layout(kernels):
    shared, box = step_forms(kernels), step_forms(kernels, "BoxTab")
    assert len(shared) == 8 and len(box) == 8
    # the same eight <NE, MC, HASM>
    assert [t for t, _ in shared] == [t for t, _ in box]
    for (_, sn), (_, bn) in zip(shared, box):
        s, k = kernels[sn], kernels[bn]
        cfg, ws, bt = k[".args"][0], k[".args"][1], k[".args"][2]
        assert cfg[".value_kind"] == ws[".value_kind"] == bt[".value_kind"] == "by_value"
        assert cfg[".offset"] == 0 and cfg[".size"] % 8 == 0
        assert ws[".offset"] == cfg[".size"]                                  # KernArgs::W_OFF
        assert (cfg[".size"], ws[".size"]) == (s[".args"][0][".size"], s[".args"][1][".size"])
        assert bt[".offset"] == ws[".offset"] + ws[".size"] and bt[".size"] == 16   # KernArgs::T_OFF: two pointers
        assert k[".group_segment_fixed_size"] == s[".group_segment_fixed_size"]
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
