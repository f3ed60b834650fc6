"""CPU test of the step kernel's occupancy target: the wave-per-agent step kernel of the benchmark's problem
(step_kernel<1, -1, false>) is compiled for five waves per SIMD -- at most 96 VGPRs (512 / 5, in granules of 8), no
spills, no scratch, 264 B of static LDS -- and the host sizes the LDS copy of the L-BFGS history (P pairs) so that the
same number of its workgroups share a CU's 160 KiB of LDS (mpc_step_lds_plan exposes that computation).  The code
object's metadata is read by tests/codeobj_common.py; skips when the LLVM tools are absent."""
import ctypes as C

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

from codeobj_common import STEP_LEAN_TARGS, _waves_by_vgprs, built_library_kernels, step_form
from model_predictive_control_amd import _lib

STEP_LDS_BYTES = 264          # s_req[64] + s_next (+ padding): the history copy is dynamic LDS, sized at launch
LEAN_WAVES_PER_SIMD = 5
CU_LDS = 160 * 1024
LDS_GRANULE = 512


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return built_library_kernels(tmp_path_factory)


def test_lean_step_kernel_fits_its_target(kernels):
    k = step_form(kernels, STEP_LEAN_TARGS)
    assert k[".sgpr_spill_count"] == 0
    assert k[".vgpr_spill_count"] == 0
    assert k[".private_segment_fixed_size"] == 0
    assert k[".vgpr_count"] <= 512 // LEAN_WAVES_PER_SIMD // 8 * 8          # 96
    assert _waves_by_vgprs(k[".vgpr_count"] + k.get(".agpr_count", 0)) >= LEAN_WAVES_PER_SIMD
    assert k[".group_segment_fixed_size"] == STEP_LDS_BYTES


def _plan(L, n, M, m=0, chain=0, lds_pairs=0):
    P, lds, wps = C.c_int(), C.c_int(), C.c_int()
    assert L.mpc_step_lds_plan(n, M, m, chain, lds_pairs, C.byref(P), C.byref(lds), C.byref(wps)) == 0
    return P.value, lds.value, wps.value


def _wg_per_cu(lds):
    per_wg = -(-(lds + STEP_LDS_BYTES) // LDS_GRANULE) * LDS_GRANULE
    return CU_LDS // per_wg


@pytest.mark.parametrize("n, M", [(24, 12), (40, 20), (80, 40)])
def test_history_copy_leaves_room_for_the_target(L, n, M):
    # n = 24: Pacejka N = 12 (all 12 pairs fit); n = 40: the benchmark (N = 20); n = 80: BASELINE config 3 (two
    # elements per lane, three waves per SIMD)
    for chain in (0, 1):
        P, lds, wps = _plan(L, n, M, chain=chain)
        assert 1 <= P <= M
        assert wps == (LEAN_WAVES_PER_SIMD if n <= 64 else 3)
        assert lds >= 4 * 2 * P * n * 8
        assert _wg_per_cu(lds) >= wps, (n, M, chain, P, lds)
    if n == 24:
        assert P == M
    if n == 40:
        assert P == 12


def test_lds_pairs_override(L):
    # MPC_LDS_PAIRS (the GPU suite forces 3) still decides P, clamped to [1, M]
    assert _plan(L, 40, 20, lds_pairs=3)[0] == 3
    assert _plan(L, 40, 20, lds_pairs=99)[0] == 20
    assert _plan(L, 40, 20, m=40)[0] == 20           # state constraints: the whole history, two waves per SIMD
    assert _plan(L, 40, 20, m=40)[2] == 2
