"""CPU test of the kinematic persistent kernel's resources: the benchmark's instantiation (solo_kernel<KIN, 1, -1, false,
false>: one element per lane, L-BFGS history in LDS, no lookahead, no per-agent table) is compiled against 256 registers
-- two waves per SIMD (mpc_solo.hpp SoloOcc) -- and spills; the two-half form of its evaluation (solo_halves) must not
cost it a wave or more scratch than the 656 B per lane it needed before that form existed (profiles/r19_solo_dual.txt).
The code object's metadata is read by tests/codeobj_common.py; skips when the LLVM tools are absent."""
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

from codeobj_common import _waves_by_vgprs, built_library_kernels

SOLO_KIN = "_ZN3mpc11solo_kernelILi0ELi1ELin1ELb0ELb0EJEEE"   # the mangled name begins with the template arguments
SOLO_KIN_WAVES_PER_SIMD = 2
SOLO_KIN_SCRATCH_BEFORE = 656
# A first build of the two-half form met the bound above with 608 B and was slower than the kernel before it: the serial
# recursion of the rollouts reloaded a spilled sixteen-register tuple of the DevCfg three times per stage (4 340 lane
# reads in the kernel against 2 465 before).  solo_eval therefore hands the rollouts h, friction, N, lf, lr as scalar
# registers of their own (the empty asm on its DevCfg copy), which gave 560 B and 2 564 lane reads.  Which scalars the
# allocator spills is the compiler's choice, so a build that falls back to the slow allocation must show up: it is
# known by its scratch, which is the slow build's or more.
SOLO_KIN_SCRATCH_SLOW_BUILD = 608


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return built_library_kernels(tmp_path_factory)


def test_kinematic_persistent_kernel_keeps_its_waves_and_its_scratch(kernels):
    names = [n for n in kernels if n.startswith(SOLO_KIN)]
    assert len(names) == 1, names
    k = kernels[names[0]]
    print({f: k[f] for f in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")})
    assert _waves_by_vgprs(k[".vgpr_count"] + k.get(".agpr_count", 0)) >= SOLO_KIN_WAVES_PER_SIMD
    assert k[".private_segment_fixed_size"] <= SOLO_KIN_SCRATCH_BEFORE


def test_rollout_scalars_stay_out_of_the_spilled_tuples(kernels):
    """560 B per lane when this was written; at the 608 B of the slow first build or above, the recursion's scalars are
    back in a spilled tuple (see SOLO_KIN_SCRATCH_SLOW_BUILD) and the kernel needs measuring again."""
    k = kernels[[n for n in kernels if n.startswith(SOLO_KIN)][0]]
    assert k[".private_segment_fixed_size"] < SOLO_KIN_SCRATCH_SLOW_BUILD
