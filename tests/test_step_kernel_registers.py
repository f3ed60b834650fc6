"""CPU test of the step kernel's register budget, read from the AMDGPU metadata of the built library's gfx950 code
object: the wave-per-agent step kernel of the benchmark's problem (step_kernel<1, -1, false>) spills no scalar or
vector registers, uses no scratch and stays within the 128 VGPRs of four waves per SIMD.  Every step kernel reads
its DevCfg and Workspace from the argument segment at fixed offsets (KernArgs in mpc_solver.hpp): the code object's
argument layout must be the one that code assumes.  Skips when the LLVM tools that read a code object are absent."""
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

from codeobj_common import STEP_LEAN_TARGS, built_library_kernels, step_form, step_forms

pytest.importorskip("yaml")

STEP_LDS_BYTES = 264   # s_req[64] + s_next (+ padding): the history copy is dynamic LDS, sized at launch


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return built_library_kernels(tmp_path_factory)


def test_lean_step_kernel_does_not_spill(kernels):
    k = step_form(kernels, STEP_LEAN_TARGS)
    assert [a[".value_kind"] for a in k[".args"][:9]] == ["by_value"] * 2 + ["global_buffer"] * 3 + ["by_value"] * 4
    assert k[".sgpr_spill_count"] == 0
    assert k[".vgpr_spill_count"] == 0
    assert k[".private_segment_fixed_size"] == 0          # no scratch
    assert k[".vgpr_count"] <= 128                        # four waves per SIMD (512 / 4)
    assert k[".group_segment_fixed_size"] <= STEP_LDS_BYTES


def test_step_kernels_argument_layout(kernels):
    forms = [step_forms(kernels, *t) for t in ((), ("BoxTab",), ("ConTab",), ("BoxTab", "ConTab"))]
    assert [len(f) for f in forms] == [8, 8, 4, 4]
    steps = [kernels[n] for f in forms for _, n in f]
    assert len(steps) == sum(1 for n in kernels if n.startswith("_ZN3mpc11step_kernelI"))    # no form but these
    for k in steps:
        cfg, ws = k[".args"][0], k[".args"][1]
        assert cfg[".value_kind"] == "by_value" and ws[".value_kind"] == "by_value"
        assert cfg[".offset"] == 0
        assert cfg[".size"] % 8 == 0 and ws[".offset"] == cfg[".size"]   # KernArgs::W_OFF
