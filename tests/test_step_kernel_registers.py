"""CPU test of the step kernel's register budget, read from the AMDGPU metadata of the built library's gfx950 code
object: the wave-per-agent step kernel of the benchmark's problem (step_kernel<1, -1, false>) spills no scalar or
vector registers, uses no scratch and stays within the 128 VGPRs of four waves per SIMD.  Every step kernel reads
its DevCfg and Workspace from the argument segment at fixed offsets (KernArgs in mpc_solver.hpp): the code object's
argument layout must be the one that code assumes.  Skips when the LLVM tools that read a code object are absent."""
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

from codeobj_common import built_library_kernels

pytest.importorskip("yaml")

STEP_LEAN = "_ZN3mpc11step_kernelILi1ELin1ELb0EEEvNS_6DevCfgENS_9WorkspaceEPiS3_S3_iiii"
STEP_LDS_BYTES = 264   # s_req[64] + s_next (+ padding): the history copy is dynamic LDS, sized at launch


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return built_library_kernels(tmp_path_factory)


def test_lean_step_kernel_does_not_spill(kernels):
    k = kernels[STEP_LEAN]
    assert k[".sgpr_spill_count"] == 0
    assert k[".vgpr_spill_count"] == 0
    assert k[".private_segment_fixed_size"] == 0          # no scratch
    assert k[".vgpr_count"] <= 128                        # four waves per SIMD (512 / 4)
    assert k[".group_segment_fixed_size"] <= STEP_LDS_BYTES


def test_step_kernels_argument_layout(kernels):
    steps = [k for n, k in kernels.items() if n.startswith("_ZN3mpc11step_kernel")]
    assert len(steps) >= 8
    for k in steps:
        cfg, ws = k[".args"][0], k[".args"][1]
        assert cfg[".value_kind"] == "by_value" and ws[".value_kind"] == "by_value"
        assert cfg[".offset"] == 0
        assert cfg[".size"] % 8 == 0 and ws[".offset"] == cfg[".size"]   # KernArgs::W_OFF
