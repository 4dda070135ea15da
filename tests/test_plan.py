"""The launch geometry rules of csrc/nk_plan.hpp (res_plan, st_plan, red_blocks, wide_blocks) against their
restatements: test_hip_resident_variants.py's `sweep_plan` / `sweep_applies`, test_hip_resident_tail.py's
`tail_plan`, and the oracle's dr_sweep_applies, tile counts and block counts (oracle/nk_oracle.c, which keeps its
own text of every rule).  The GPU tests compare results bit for bit, which only holds while these agree; here they
are compared directly, on the CPU.

A small program includes the header (it needs no HIP), is built with g++ -- under the address and
undefined-behaviour sanitizers where the toolchain links them -- and answers one query per line with the product's
default knobs (`ResKnobs{}`, `StKnobs{}`; the tail group's configured size is the one knob the queries set).
"""
import itertools
import os
import subprocess
import tempfile

import pytest

import _nkpath  # noqa: F401
import test_hip_resident_tail as tt
import test_hip_resident_variants as tv
from oracle import oracle as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "newtonkrylov.jl_amd", "csrc")

SRC = r"""
#include <cstdio>
#include "nk_plan.hpp"
int main() {
    char kind;
    long long a, b, c, d, e;
    while (std::scanf(" %c %lld %lld %lld %lld %lld", &kind, &a, &b, &c, &d, &e) == 6) {
        if (kind == 'R') {  // n np G rl_max tail
            nk::ResKnobs K;
            K.tail = (int)e;
            const nk::ResPlan P = nk::res_plan(a, (int)b, (int)c, (int)d, -1, false, 0, K);
            std::printf("%d %d %d %d %d\n", (int)P.applies, P.rv, P.rl, (int)P.full, P.tg);
        } else if (kind == 'S') {  // dim nx ny nz blk: a residual launch, zero boundaries
            nk::StShape S{};
            S.dim = (int)a; S.nx = b; S.ny = c; S.nz = d; S.blk = e != 0; S.mode = nk::MODE_RES;
            const nk::StPlan P = nk::st_plan(S, nk::StKnobs{});
            std::printf("%d %d %d %d %d\n", P.grid, P.nparts, P.vec, P.rows, P.tiles_x);
        } else {  // B n
            std::printf("%d %d\n", nk::red_blocks(a, nk::kMaxRedBlocks), nk::wide_blocks(a, nk::kRedCap - 2));
        }
    }
    return 0;
}
"""

GS, RLS, NPS = (256, 128, 64, 8), (39, 8, 0), (1, 2, 64, 65)
TAILS = (0, 8, 16, 24, 64)


def sweep_ns(G):
    """The vector lengths of the sweep checks on G blocks: every shape of the two resident test files, and
    n = 2 (256 G w + d) around every whole-slot count w up to 130, each also odd (n + 1)."""
    cases = tv.CASES + [tv.THRESHOLD_BELOW] + tt.CASES
    shapes = [(c.nx, c.ny) for c in cases] + [tv.EDGE_SHAPE] + [s for s, _ in tv.SUITE_SHAPES] + tt.KBENCH_SHAPES
    ns = [nx * ny for nx, ny in shapes]
    ns += [2 * (256 * G * w + d) for w in range(131) for d in (0, 1, 255, 256, 257)]
    return sorted({m for n in ns for m in (n, n + 1) if m > 0})


SWEEP_QUERIES = [(n, np_, G, rl, t) for G in GS for rl in RLS for np_ in NPS for n in sweep_ns(G) for t in TAILS]
ST1 = [(1, n, 1, 1, 0) for n in (1, 255, 256, 257, 1000, 10000)]
ST2 = [(2, nx, ny, 1, 0) for nx in (1, 2, 63, 64, 511, 512, 513, 1000, 4096, 16384)
       for ny in (1, 5, 7, 8, 9, 37, 1000, 2048, 4096, 16384, 600000)]
ST3 = [(3, nx, ny, nz, blk) for nx in (16, 64, 127, 128, 130, 256, 512) for ny in (1, 3, 4, 12, 94, 256)
       for nz in (1, 10, 15, 16, 17, 64, 81, 512) for blk in (0, 1)]
RED_PER, RED_CAP, WIDE_PER, WIDE_CAP = 2048, 2048, 1024, 16382  # elements per block and the cap of either rule
BLOCK_NS = sorted({1, 2 ** 25 + 1} | {cap * per + d for per, cap in ((RED_PER, RED_CAP), (WIDE_PER, WIDE_CAP))
                                      for d in (-per, -1, 0, 1)})


@pytest.fixture(scope="module")
def answers():
    """Build the program once and put every query to it in one run: {query line: its integers}."""
    lines = ["R %d %d %d %d %d" % q for q in SWEEP_QUERIES] + ["S %d %d %d %d %d" % q for q in ST1 + ST2 + ST3]
    lines += ["B %d 0 0 0 0" % n for n in BLOCK_NS]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "plan.cpp"), os.path.join(d, "plan")
        with open(src, "w") as f:
            f.write(SRC)
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src]
        if subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"],
                          capture_output=True).returncode != 0:
            subprocess.run(base, check=True)  # no sanitizer runtimes to link here
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return {q: tuple(int(v) for v in o.split()) for q, o in zip(lines, out)}


def test_sweep_plan_matches_the_restatements(answers):
    """(applies, rv, rl, full) is `sweep_applies` / `sweep_plan`'s, tg is `tail_plan`'s, for every n, G, LDS limit,
    pass count and configured tail of the grid."""
    applied = set()
    for n, np_, G, rl_max, tail in SWEEP_QUERIES:
        applies, rv, rl, full, tg = answers["R %d %d %d %d %d" % (n, np_, G, rl_max, tail)]
        assert bool(applies) == tv.sweep_applies(n, np_, G, rl_max), (n, np_, G, rl_max)
        if applies:
            assert (rv, rl, bool(full)) == tv.sweep_plan(n, G, rl_max)[:3], (n, np_, G, rl_max)
            assert tg == tt.tail_plan(n, tail, G, rl_max), (n, np_, G, rl_max, tail)
            applied.add((rv, bool(full), tg > 0))
    # the grid reaches every instantiated rv, full and streamed, with and without a tail
    assert {a[0] for a in applied} == set(tv.RV_SET)
    assert {a[1:] for a in applied} == {(True, True), (True, False), (False, False)}


def test_sweep_applies_as_in_the_oracle(answers):
    """`applies` is dr_sweep_applies under oc_set_devred(on, G, rl_max)."""
    L = oc.lib()
    try:
        for G, rl_max in itertools.product(GS, RLS):
            L.oc_set_devred(1, G, rl_max)
            for np_ in NPS:
                for n in sweep_ns(G):
                    got = answers["R %d %d %d %d %d" % (n, np_, G, rl_max, TAILS[0])][0]
                    assert got == L.oc_dr_sweep_applies(n, np_), (n, np_, G, rl_max)
    finally:
        oc.set_devred(False)


def test_stencil_grids_match_the_oracle_tile_counts(answers):
    """st_plan's grid (and, march tiles handing on one partial each, nparts) is the oracle's tile count in 1D, 2D
    -- up to ny = 600000, where the reduction slot's capacity sets the rows -- and 3D, slabs and blocks."""
    L = oc.lib()
    for q in ST1 + ST2 + ST3:
        dim, nx, ny, nz, blk = q
        want = (L.oc_dr_tile_parts1d(nx, None, None, None) if dim == 1
                else L.oc_dr_tile_parts2d(nx, ny, None, None, None) if dim == 2
                else L.oc_dr_tile_parts3d(nx, ny, nz, blk, None, None, None))
        grid, nparts = answers["S %d %d %d %d %d" % q][:2]
        assert grid == nparts == want, q
    # ny = 600000 at 16384 columns: 32 tiles across, rows set by the capacity of kRedCap - 2 partials
    grid, _, vec, rows, tiles_x = answers["S 2 16384 600000 1 0"]
    assert (vec, tiles_x) == (2, 32) and rows == -(-600000 * 32 // WIDE_CAP) > 32 and grid == 32 * -(-600000 // rows)


def test_block_counts_match_the_oracle(answers):
    """red_blocks and wide_blocks at n = 1, around each rule's cap, and at 2^25 + 1."""
    L = oc.lib()
    for n in BLOCK_NS:
        assert answers["B %d 0 0 0 0" % n] == (L.oc_dr_red_blocks(n), L.oc_dr_wide_blocks(n)), n
    assert answers["B 1 0 0 0 0"] == (1, 1)
    assert answers["B %d 0 0 0 0" % (RED_PER * RED_CAP - 1)] == (RED_CAP, RED_PER * RED_CAP // WIDE_PER)
    assert answers["B %d 0 0 0 0" % (2 ** 25 + 1)] == (RED_CAP, WIDE_CAP)
