"""The layouts of the handle's device allocations (csrc/mpc_arena.hpp), walked on host memory: tests/handle_layout_main.hip
measures each arena, mallocs exactly the measured size, places the pointers and writes every block to its full extent,
under the address and undefined-behaviour sanitizers; this module checks what it prints.  No GPU needed.

The program is built by hipcc for host and device (the kernel headers that define the real structs leave a host-only
build without its code object at link time); the sanitizers instrument the host side alone, and nothing is preloaded.

What the workspace must keep is written out here independently of the header, from the order the arrays have always been
carved in: the agent-major rows xk gk q xn xe ge xe2 ge2 [n], S Y [M n], Sig Sig_old e1 e2 yhx yhxn yhe [max(m, 1)],
rec [64], each times Bp = B rounded up to 64; the four slot arrays trajx [(N + 1) nx], useq [2 N], stage_L [N],
jac [N (nx (nx + 1) + 2)], each times St = 2 Bp + 64 (MAX_GROUPS + 1); then the ints lists [4 Bp], agent_of [St],
counts [8 MAX_GROUPS], the 64-bit totals [16] and the ints solo_ctr [2 MAX_GROUPS]."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GROUPS, REC, NDISC = 8, 64, 2
BATCHES = (1, 63, 64, 65, 130, 4096)


def issue_cases():
    for nx, N in itertools.product((4, 6), (1, 20, 64)):
        for M, m, B in itertools.product((1, N, 64), (0, N, nx * N, NDISC * N), BATCHES):
            yield nx, N, M, m, B


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(the finished process, its cases): a case is (key, {arena: (bytes, [(block, offset, bytes, element size)])})"""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path_factory.mktemp("layout") / "handle_layout_main")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "handle_layout_main.hip")])
    p = subprocess.run([exe], capture_output=True, text=True)
    cases = []
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] in ("case", "grid"):
            cases.append(((f[0],) + tuple(int(v) for v in f[1:]), {}))
        elif f[0] == "arena":
            blocks = cases[-1][1].setdefault(f[1], (int(f[2]), []))[1]
        else:
            assert f[0] == "blk", line
            blocks.append((f[1], int(f[2]), int(f[3]), int(f[4])))
    return p, cases


def test_sanitizers_report_nothing(run):
    p, cases = run
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-4000:])
    have = {key[1:] for key, _ in cases if key[0] == "case"}
    assert have == set(issue_cases())
    for _, arenas in cases:
        assert all(blocks for _, blocks in arenas.values())


def test_blocks_are_disjoint_aligned_and_inside(run):
    for key, arenas in run[1]:
        for arena, (size, blocks) in arenas.items():
            end = 0
            for name, off, nbytes, elem in sorted(blocks, key=lambda b: b[1]):
                assert off >= end, (key, arena, name, "overlaps the block before it")
                assert off % elem == 0 and nbytes > 0, (key, arena, name)
                end = off + nbytes
            assert end <= size, (key, arena, end, size)


def parent_workspace(nx, N, M, m, B):
    """([(array, offset, bytes)] in the parent's carve order, the parent's allocation formula)"""
    Bp = (B + 63) // 64 * 64
    St = 2 * Bp + 64 * (MAX_GROUPS + 1)
    n, m1, JS = 2 * N, max(m, 1), nx * (nx + 1) + 2
    rows = [(a, n) for a in "xk gk q xn xe ge xe2 ge2".split()] + [("S", M * n), ("Y", M * n)]
    rows += [(a, m1) for a in "Sig Sig_old e1 e2 yhx yhxn yhe".split()] + [("rec", REC)]
    slots = [("trajx", (N + 1) * nx), ("useq", 2 * N), ("stage_L", N), ("jac", N * JS)]
    sized = [(a, 8 * k * Bp) for a, k in rows] + [(a, 8 * k * St) for a, k in slots]
    sized += [("lists", 4 * 4 * Bp), ("agent_of", 4 * St), ("counts", 4 * 8 * MAX_GROUPS), ("totals", 8 * 16), ("solo_ctr", 4 * 2 * MAX_GROUPS)]
    table, off = [], 0
    for a, nbytes in sized:
        table.append((a, off, nbytes))
        off += nbytes
    nd = 8 * n + 2 * M * n + 7 * m1 + REC
    nscr = (N + 1) * nx + 2 * N + N + N * JS
    return table, (nd * 8 + 4 * 4) * Bp + nscr * 8 * St + 4 * St + 8 * 4 * MAX_GROUPS + 256 + 64 + 256


def test_workspace_keeps_the_parents_offsets_and_fits_its_size(run):
    seen = 0
    for key, arenas in run[1]:
        if key[0] != "case":
            continue
        size, blocks = arenas["workspace"]
        table, parent_bytes = parent_workspace(*key[1:])
        assert [(name, off, nbytes) for name, off, nbytes, _ in blocks] == table, key
        assert table[-1][1] + table[-1][2] <= size <= parent_bytes, (key, size, parent_bytes)
        seen += 1
    assert seen >= len(set(issue_cases()))
