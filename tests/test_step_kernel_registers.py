"""CPU test of the step kernel's register budget, read from the AMDGPU metadata of the built library's gfx950 code
object: the wave-per-agent step kernel of the benchmark's problem (step_kernel<1, -1, false>) spills no scalar or
vector registers, uses no scratch and stays within the 128 VGPRs of four waves per SIMD.  Every step kernel reads
its DevCfg and Workspace from the argument segment at fixed offsets (KernArgs in mpc_solver.hpp): the code object's
argument layout must be the one that code assumes.  Skips when the LLVM tools that read a code object are absent."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

from model_predictive_control_amd import _lib

yaml = pytest.importorskip("yaml")

STEP_LEAN = "_ZN3mpc11step_kernelILi1ELin1ELb0EEEvNS_6DevCfgENS_9WorkspaceEPiS3_S3_iiii"
STEP_LDS_BYTES = 264   # s_req[64] + s_next (+ padding): the history copy is dynamic LDS, sized at launch


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    missing = [n for n, p in tools.items() if p is None]
    if missing:
        pytest.skip("needs " + ", ".join(missing))
    _lib.build()
    d = tmp_path_factory.mktemp("codeobj")
    fatbin, co = str(d / "fatbin.bin"), str(d / "gfx950.o")
    subprocess.check_call([tools["llvm-objcopy"], "--dump-section=.hip_fatbin=" + fatbin, _lib.LIB_PATH, str(d / "x")])
    subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + fatbin,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([tools["llvm-readelf"], "--notes", co], text=True)
    doc = notes[notes.index("---"):notes.index("\n...", notes.index("---"))]
    meta = yaml.safe_load(doc)
    return {k[".name"]: k for k in meta["amdhsa.kernels"]}


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
