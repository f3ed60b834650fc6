"""Compares the gfx950 code-object metadata of two builds of libmpc_hip.so, kernel by kernel.

    python tools/dev/codeobj_diff.py OLD.so NEW.so

For every kernel present in both: registers (vector, accumulator, scalar), spill counts, scratch and static LDS
bytes must be equal; differences are listed.  Kernels only in NEW (the per-agent instantiations) are listed with
the same figures and the waves per SIMD their registers allow (512 unified registers per SIMD lane on gfx950,
allocated in blocks of 8; at most 8 waves).  A kernel that gained a trailing `false` template argument (the
per-agent flag at its default) is matched with the old kernel of the same name without it, and a box or constraint
form of step_kernel or prox_kernel with the kernel of a name of its own that it was (old_name).  No GPU needed.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
from codeobj_common import _tool, kernel_metadata  # noqa: E402  (the reader the CPU tests use)

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(lib):
    """{demangled kernel name: metadata}"""
    with tempfile.TemporaryDirectory() as d:
        ks = list(kernel_metadata(lib, d).values())
    filt = _tool("llvm-cxxfilt") or _tool("c++filt")
    names = subprocess.check_output([filt] + [k[".name"] for k in ks], text=True).split("\n")
    return {old_name(re.sub(r"\(.*$", "", nm).replace("void ", "").replace("mpc::", "")): k for k, nm in zip(ks, names)}


def old_name(nm):
    """A box or constraint form of step_kernel or prox_kernel by the name it had as a kernel of its own, so that the two
    spellings match: step_kernel<1, 0, true, BoxTab, ConTab> was step_kernel_box_con<1, 0>, prox_kernel<BoxTab> prox_box_kernel."""
    m = re.fullmatch(r"(step|prox)_kernel<(.*?)(?:, )?(BoxTab)?(?:, )?(ConTab)?>", nm)
    if not m:
        return nm
    k, args, box, con = m.groups()
    sfx = "_box" * bool(box) + "_con" * bool(con)
    if con:
        args = args[:-len(", true")]
    return (k + "_kernel" + sfx if k == "step" else k + sfx + "_kernel") + ("<%s>" % args if args else "")


def waves(k):
    regs = k[".vgpr_count"]           # (the unified count: accumulator registers included)
    regs = max(8, (regs + 7) // 8 * 8)
    return min(8, 512 // regs)


def fmt(k):
    return "vgpr %3d  agpr %3d  sgpr %3d  spill v/s %3d/%3d  scratch %4d B  LDS %5d B" % tuple(k[x] for x in KEYS)


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    same, diff, added = 0, [], []
    for nm, k in sorted(new.items()):
        o = old.get(nm)
        if o is None:
            o = old.get(re.sub(r", false>$", ">", nm)) or old.get(re.sub(r"<false>$", "", nm))
        if o is None:
            added.append((nm, k))
        elif all(o[x] == k[x] for x in KEYS):
            same += 1
        else:
            diff.append((nm, o, k))
    gone = [nm for nm in old if nm not in new and not any(
        re.sub(r", false>$", ">", n2) == nm or re.sub(r"<false>$", "", n2) == nm for n2 in new)]
    print("kernels: %d old, %d new; %d in both with identical figures, %d in both that differ, %d only new, %d only old"
          % (len(old), len(new), same, len(diff), len(added), len(gone)))
    for nm, o, k in diff:
        print("DIFFERS %s\n   old %s\n   new %s" % (nm, fmt(o), fmt(k)))
    for nm in gone:
        print("ONLY OLD %s" % nm)
    for nm, k in added:
        print("NEW %-62s %s  -> %d waves/SIMD" % (nm, fmt(k), waves(k)))


if __name__ == "__main__":
    main()
