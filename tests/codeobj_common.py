"""The reader of the built library's gfx950 code object (shared by the CPU tests that check a kernel's registers,
spills, LDS or argument layout, and by tools/dev/codeobj_diff.py): the AMDGPU metadata of every kernel, as the LLVM
tools of the ROCm installation print it.  No GPU needed."""
import os
import re
import shutil
import subprocess

TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")


def _tool(name):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    return p if os.access(p, os.X_OK) else shutil.which(name)


def kernel_metadata(lib_path, workdir):
    """{mangled kernel name: its metadata map} of the gfx950 code object bundled in `lib_path` (needs PyYAML and TOOLS;
    scratch files go to `workdir`)."""
    import yaml
    fatbin, co = os.path.join(workdir, "fatbin.bin"), os.path.join(workdir, "gfx950.o")
    subprocess.check_call([_tool("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fatbin, lib_path, os.path.join(workdir, "x")])
    subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fatbin,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([_tool("llvm-readelf"), "--notes", co], text=True)
    doc = notes[notes.index("---"):notes.index("\n...", notes.index("---"))]
    return {k[".name"]: k for k in yaml.safe_load(doc)["amdhsa.kernels"]}


def built_library_kernels(tmp_path_factory, skip=True):
    """What a test module's `kernels` fixture returns: kernel_metadata of the library, built first if it is stale.
    Without PyYAML or one of TOOLS the tests that use it skip (skip=False: fail -- a skip would drop them without notice)."""
    import pytest
    from model_predictive_control_amd import _lib
    missing = [n for n in TOOLS if _tool(n) is None]
    if skip:
        pytest.importorskip("yaml")
        if missing:
            pytest.skip("needs " + ", ".join(missing))
    assert not missing, "needs " + ", ".join(missing)
    _lib.build()
    return kernel_metadata(_lib.LIB_PATH, str(tmp_path_factory.mktemp("codeobj")))


STEP_LEAN_TARGS = "Li1ELin1ELb0E"      # <NE, MC, HASM> = <1, -1, false>: the benchmark problem's step kernel


def step_forms(kernels, *tables):
    """The instantiations step_kernel<NE, MC, HASM, tables...> in `kernels` (`tables`: struct names, the whole pack in
    its order; none: the empty pack), by their mangled names: [(mangled <NE, MC, HASM>, kernel name)], sorted."""
    pack = "J" + "".join("NS_%d%sE" % (len(t), t) for t in tables) + "EEE"      # J <pack> E, template arguments E, name E
    rx = re.compile(r"_ZN3mpc11step_kernelI(Li\d+ELin?\d+ELb[01]E)" + pack + "v")
    return sorted((m.group(1), n) for n in kernels for m in [rx.match(n)] if m)


def step_form(kernels, targs, *tables):
    """The metadata of the one step_kernel<targs, tables...>."""
    found = [n for t, n in step_forms(kernels, *tables) if t == targs]
    assert len(found) == 1, (targs, tables, found)
    return kernels[found[0]]


def _waves_by_vgprs(vgprs):
    """waves per SIMD that `vgprs` unified registers allow: 512 per SIMD lane, allocated in blocks of 8"""
    return 512 // (-(-vgprs // 8) * 8)
