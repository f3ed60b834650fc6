"""CPU tests of the per-agent constraint table (mpc_set_agent_constraints): the header declares it, the library exports
it, the default row is the configuration's constraint data, the host-side table builder puts overrides in the documented
columns, the front ends carry the new entry points, and the code object holds a constraint form of every constrained
(HASM) step kernel with the resources of the form it derives from.  No compute call is made here."""
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
from codeobj_common import _waves_by_vgprs, built_library_kernels, step_forms
from model_predictive_control_amd import _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_constraints_api(L):
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert re.search(r"#define\s+MPC_NCONSTR\s+19\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mpc_default_constraints\s*\(\s*const\s+mpc_config\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+mpc_set_agent_constraints\s*\(\s*mpc_handle\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    for name in ("mpc_default_constraints", "mpc_set_agent_constraints"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.NCONSTR == 19 and mp.NCONSTR == 19
    assert _lib.CONSTR_FIELDS == {"g_off": (0, 6), "D_lb": (6, 6), "D_ub": (12, 6), "lane_halfwidth": (18, 1)}
    assert len(L.mpc_default_constraints.argtypes) == 2 and len(L.mpc_set_agent_constraints.argtypes) == 5
    assert L.mpc_set_agent_constraints.argtypes[2] is C.c_int and L.mpc_set_agent_constraints.argtypes[4] is C.c_int


@pytest.mark.parametrize("model", [0, 1])
def test_default_row_is_the_configurations_constraint_data(L, O, model):
    N = 12 if model else 20
    row = _lib.default_constraints(mp.default_config(model, N))
    ocfg = O.default_config(model, N)
    assert row.shape == (19,) and row.dtype == np.float64
    assert list(row) == list(ocfg.g_off) + list(ocfg.D_lb) + list(ocfg.D_ub) + [ocfg.lane_halfwidth]
    assert list(row[:6]) == [20, 1, 1, 2, 1, 0.1] and np.all(row[6:12] == -np.inf) and np.all(row[12:18] == np.inf)
    assert row[18] == 0.15
    kw = dict(g_off=[18, 0.9, 1.1, 0.5, 1.2, 0.2], D_lb=[-np.inf, -1, -2, -0.4, -np.inf, -3], D_ub=[0, 0.5, np.inf, 0.01, 0, 1],
              lane_halfwidth=0.04)
    got = _lib.default_constraints(mp.default_config(model, N, constr_mode=1, **kw))
    oc = O.default_config(model, N, constr_mode=1, **kw)
    assert list(got) == kw["g_off"] + kw["D_lb"] + kw["D_ub"] + [0.04]
    assert list(got) == list(oc.g_off) + list(oc.D_lb) + list(oc.D_ub) + [oc.lane_halfwidth]


def test_null_arguments_return_codes_not_exceptions(L):
    E_ARG = -1
    row = (C.c_double * 19)()
    cfg = mp.default_config(0, 20)
    assert L.mpc_default_constraints(None, row) == E_ARG and b"mpc_default_constraints" in L.mpc_last_error()
    assert L.mpc_default_constraints(C.byref(cfg), None) == E_ARG
    assert L.mpc_default_constraints(C.byref(cfg), row) == 0
    assert L.mpc_set_agent_constraints(None, None, 0, None, 0) == E_ARG
    assert b"mpc_set_agent_constraints" in L.mpc_last_error()
    assert L.mpc_set_agent_constraints(None, C.c_void_p(8), 1, C.c_void_p(8), 1) == E_ARG   # (nothing is dereferenced)
    assert L.mpc_set_agent_constraints(None, C.c_void_p(8), 1, None, 1) == E_ARG


def test_constraint_rows(L):
    cfg = mp.default_config(1, 12, constr_mode=1, g_off=[20, 1, 1, 0.5, 1, 0.1], D_lb=[-np.inf] * 6, D_ub=[0.0] * 6,
                            lane_halfwidth=0.05)
    base = _lib.default_constraints(cfg)
    assert list(base) == [20, 1, 1, 0.5, 1, 0.1] + [-np.inf] * 6 + [0.0] * 6 + [0.05]
    P = 5
    tab = _lib.constraint_rows(cfg, P)
    assert tab.shape == (P, 19) and tab.dtype == np.float64 and tab.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(tab[p], base) for p in range(P))
    rng = np.random.default_rng(0)
    off = rng.uniform(.1, 2, (P, 6)); lb = -rng.uniform(.1, 1, (P, 6)); ub = rng.uniform(.1, 1, (P, 6)); hw = rng.uniform(.02, .1, P)
    tab = _lib.constraint_rows(cfg, P, g_off=off, D_lb=lb, D_ub=ub, lane_halfwidth=hw)
    assert np.array_equal(tab[:, 0:6], off) and np.array_equal(tab[:, 6:12], lb) and np.array_equal(tab[:, 12:18], ub)
    assert np.array_equal(tab[:, 18], hw)
    tab = _lib.constraint_rows(cfg, 3, D_ub=[0.5, 0.2, 0.1, 0.0, 0.3, 0.4], lane_halfwidth=0.07)     # one value: every row
    assert np.array_equal(tab, np.tile(list(base[:12]) + [0.5, 0.2, 0.1, 0.0, 0.3, 0.4, 0.07], (3, 1)))
    # the kinematic model has four states: nx leading entries are enough, the others keep the configuration's
    kcfg = mp.default_config(0, 20, constr_mode=1)
    tab = _lib.constraint_rows(kcfg, 2, g_off=[[1, 2, 3, 4], [5, 6, 7, 8]])
    assert np.array_equal(tab[:, 0:4], [[1, 2, 3, 4], [5, 6, 7, 8]]) and np.array_equal(tab[:, 4:6], [[1, 0.1]] * 2)
    assert mp.constraint_rows is _lib.constraint_rows and mp.default_constraints is _lib.default_constraints
    for bad in (dict(g_off=np.zeros((P, 3))), dict(D_ub=np.zeros((P + 1, 6))), dict(D_lb=np.zeros(5)),
                dict(lane_halfwidth=np.zeros(P + 1))):
        with pytest.raises(ValueError):
            _lib.constraint_rows(cfg, P, **bad)
    with pytest.raises(ValueError):
        _lib.constraint_rows(cfg, 0)


def test_front_ends_carry_the_new_entry_points():
    from model_predictive_control_amd.controller import MPCController
    for name in ("set_agent_constraints", "clear_agent_constraints"):
        assert callable(getattr(mp.BatchedMPC, name))
    assert isinstance(inspect.getattr_static(mp.BatchedMPC, "agent_constraints_bound"), property)
    assert list(inspect.signature(mp.BatchedMPC.set_agent_constraints).parameters) == ["self", "table", "index"]
    for fn in (MPCController.solve, MPCController.step):
        par = inspect.signature(fn).parameters
        assert "constraints" in par and "constraint_index" in par
        assert par["constraints"].default is None and par["constraint_index"].default is None
        assert "params" in par and "param_index" in par and "bounds" in par and "bound_index" in par
    code = ("import sys; sys.path.insert(0, %r); import model_predictive_control_amd as mp; "
            "from model_predictive_control_amd import controller; "
            "assert not any('oracle' in m for m in sys.modules), 'oracle imported'; "
            "assert mp.constraint_rows(mp.default_config(0, 20), 2).shape == (2, 19)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ------------------------------------------------------------------ the code object (tests/codeobj_common.py)
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return built_library_kernels(tmp_path_factory, skip=False)    # (these register and occupancy checks never skip)


def _waves(k):
    return min(8, _waves_by_vgprs(k[".vgpr_count"] + k.get(".agpr_count", 0)))


def test_every_constrained_step_kernel_has_its_constraint_forms(kernels):
    """step_kernel<NE, MC, true> -> step_kernel<NE, MC, true, ConTab>, step_kernel<NE, MC, true, BoxTab> ->
    step_kernel<NE, MC, true, BoxTab, ConTab>: no scratch, no spilled vector register, no more spilled scalars and no more
    vector registers than the form it derives from, its LDS, and -- by registers (512 per SIMD lane, blocks of 8) --
    exactly its waves per SIMD."""
    for box in ((), ("BoxTab",)):
        parents = [(t, n) for t, n in step_forms(kernels, *box) if t.endswith("Lb1E")]      # HASM
        cons = step_forms(kernels, *box, "ConTab")
        assert len(parents) == 4 and len(cons) == 4
        # the same four <NE, MC>, and a constraint form of a constrained kernel alone
        assert [t for t, _ in parents] == [t for t, _ in cons]
        for (_, pn), (_, cn) in zip(parents, cons):
            p, k = kernels[pn], kernels[cn]
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
            assert k[".sgpr_spill_count"] <= p[".sgpr_spill_count"], (cn, k[".sgpr_spill_count"], p[".sgpr_spill_count"])
            assert k[".vgpr_count"] <= p[".vgpr_count"], (cn, k[".vgpr_count"], p[".vgpr_count"])
            assert _waves(k) == _waves(p), (cn, k[".vgpr_count"], p[".vgpr_count"])
            assert k[".group_segment_fixed_size"] == p[".group_segment_fixed_size"]
            assert k[".max_flat_workgroup_size"] == 256
            # the argument layout KernArgs reads: DevCfg, Workspace, the tables (two pointers each), then the list
            # pointers the constraint forms read again behind their loop (KernArgs::tail)
            args, pargs = k[".args"], p[".args"]
            assert (args[0][".size"], args[1][".size"]) == (pargs[0][".size"], pargs[1][".size"])
            assert args[1][".offset"] == args[0][".size"]                     # KernArgs::W_OFF
            ntab = len(box) + 1
            for j in range(ntab):
                t = args[2 + j]
                assert t[".value_kind"] == "by_value" and t[".size"] == 16
                assert t[".offset"] == args[1][".offset"] + args[1][".size"] + 16 * j   # KernArgs::T_OFF, KernArgs::tab
            for j in range(3):
                t = args[2 + ntab + j]
                assert t[".value_kind"] == "global_buffer" and t[".size"] == 8
                assert t[".offset"] == args[1][".offset"] + args[1][".size"] + 16 * ntab + 8 * j


def test_the_k1_kernels_and_the_persistent_kernel_have_constraint_forms(kernels):
    """By their mangled names: <..., PA = true, ConTab> and, for the persistent kernel, <..., PA = true, BoxTab, ConTab>."""
    k1 = "Lb1EJNS_6ConTabEEE"
    count = lambda pre, tail: sum(1 for n in kernels if n.startswith("_ZN3mpc" + pre + "I") and tail in n)
    assert count("12stage_kernel", k1) == 4            # two models x shared / per-agent centerline
    assert count("20stage_adjoint_kernel", k1) == 2    # the kinematic model's fused K1b + K1c
    assert count("16solo_eval_kernel", k1) == 2        # the wave evaluation
    assert count("11solo_kernel", "Lb0ELb1EJNS_6BoxTabENS_6ConTabEEE") == 6   # two models x three history variants, never the lookahead
    # ... and in no other form: every kernel that names the ConTab in its template arguments is one of these 4 + 2 + 2 + 6
    # = 14 or one of the step kernel's 4 + 4 constraint forms (test_every_constrained_step_kernel_has_its_constraint_forms)
    assert sum(1 for n in kernels if "JNS_6ConTabEE" in n or "ENS_6ConTabEEE" in n) == 14 + 8
