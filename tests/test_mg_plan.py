"""The multigrid's host-only rules of csrc/nk_mg_plan.hpp against their restatements: the level plans (mg_plan,
mg_plan_semi, mg_plan_slabs) against `plan`, `plan_semi` and `slab_levels` of the multigrid test files, the level-list
validation, which transfer kernels a level pair runs (mg_xfer) and when their index products fit 32 bits, the integer
transfer weights (mg_rax_t, mg_pax_t: the functions the kernels call) against the restatement's 1D matrices, the
one-ghost-plane property of equal slabs, the grid of the row-shaped kernels (mg_rows) and the coarse tail's rule.

A small program includes the header (it needs no HIP), is built with g++ -- under the address and
undefined-behaviour sanitizers where the toolchain links them -- and answers one query per line.
"""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _nkpath  # noqa: F401
import test_hip_multigrid as tm
import test_hip_multigrid_dist as td
import test_hip_multigrid_semi as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "newtonkrylov.jl_amd", "csrc")

SRC = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "nk_mg_plan.hpp"
using namespace nk;
static void levels_out(int L, const int64_t (*ext)[3]) {
    std::printf("%d", L);
    for (int l = 0; l < L; ++l) std::printf(" %" PRId64 " %" PRId64 " %" PRId64, ext[l][0], ext[l][1], ext[l][2]);
    std::printf("\n");
}
template <typename I>
static bool same_weights(int nf, int nc) {
    for (int j = 0; j < nc; ++j) {
        const MgAx a = mg_rax_t<I>(nf, nc, j), b = mg_rax_t<int64_t>(nf, nc, j);
        if (a.lo != b.lo || a.cnt != b.cnt || a.D != b.D) return false;
        for (int t = 0; t < 4; ++t)
            if (a.w[t] != b.w[t]) return false;
    }
    for (int i = 0; i < nf; ++i) {
        const MgPx a = mg_pax_t<I>(nf, nc, i), b = mg_pax_t<int64_t>(nf, nc, i);
        if (a.j != b.j || a.w != b.w) return false;
    }
    return true;
}
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const char kind = line[0];
        std::vector<long long> v;
        const char* s = line.c_str() + 1;
        for (char* end = nullptr;; s = end) {
            const long long x = std::strtoll(s, &end, 10);
            if (end == s) break;
            v.push_back(x);
        }
        int64_t ext[kMgMaxLevels + 1][3];
        if (kind == 'P' || kind == 'S') {  // nx ny nz max_levels: mg_plan / mg_plan_semi (h = 1 / (n + 1), k = 1, tau = 1/2)
            const int64_t n[3] = {v[0], v[1], v[2]};
            double h[3], k[3] = {1.0, 1.0, 1.0};
            for (int a = 0; a < 3; ++a) h[a] = n[a] == 1 ? 1.0 : 1.0 / (double)(n[a] + 1);
            levels_out(kind == 'P' ? mg_plan(n, (int)v[3], ext) : mg_plan_semi(n, h, k, 0.5, (int)v[3], ext), ext);
        } else if (kind == 'D') {  // nx ny nz nranks max_levels: mg_plan_slabs, "L ax extents" or "0 why"
            const int64_t n[3] = {v[0], v[1], v[2]};
            int ax = 0;
            const char* why = nullptr;
            const int L = mg_plan_slabs(n, (int)v[3], (int)v[4], ext, &ax, &why);
            if (L == 0) std::printf("0 %s\n", why);
            else { std::printf("%d ", ax); levels_out(L, ext); }
        } else if (kind == 'V') {  // n0x n0y n0z nlevels extents...: mg_levels_why
            const int64_t n0[3] = {v[0], v[1], v[2]};
            std::vector<int64_t> given(v.begin() + 4, v.end());
            given.resize(std::max<size_t>(given.size(), 3), 0);
            char buf[128];
            const char* why = mg_levels_why(n0, given.data(), (int)v[3], buf);
            std::printf("%s\n", why ? why : "ok");
        } else if (kind == 'X') {  // fine extents, coarse extents: mg_xfer
            const int nf[3] = {(int)v[0], (int)v[1], (int)v[2]}, nc[3] = {(int)v[3], (int)v[4], (int)v[5]};
            const MgXfer t = mg_xfer(nf, nc);
            std::printf("%d %d %d\n", t.mask, (int)t.s32, (int)t.general);
        } else if (kind == 'E') {  // nf nc: the 32-bit weights are the 64-bit ones
            std::printf("%d\n", (int)same_weights<int32_t>((int)v[0], (int)v[1]));
        } else if (kind == 'W') {  // nf nc: every mg_rax_t (lo cnt w0 w1 w2 w3 D), then every mg_pax_t (j w)
            const int nf = (int)v[0], nc = (int)v[1];
            for (int j = 0; j < nc; ++j) {
                const MgAx a = mg_rax_t<int64_t>(nf, nc, j);
                std::printf("%d %d %d %d %d %d %d ", a.lo, a.cnt, a.w[0], a.w[1], a.w[2], a.w[3], a.D);
            }
            for (int i = 0; i < nf; ++i) {
                const MgPx p = mg_pax_t<int64_t>(nf, nc, i);
                std::printf("%d %a ", p.j, p.w);
            }
            std::printf("\n");
        } else if (kind == 'G') {  // ranks m_f: the rows (1-based, global) a rank's coarse / fine rows reach, against its slab
            const int R = (int)v[0], mf = (int)v[1], mc = mf / 2, nf = R * mf, nc = R * mc;
            long long rlo = 1 << 30, rhi = -(1 << 30), plo = 1 << 30, phi = -(1 << 30), cnt = 1 << 30;
            for (int j = 0; j < nc; ++j) {
                const MgAx a = mg_rax_t<int64_t>(nf, nc, j);
                const long long r = j / mc;
                rlo = std::min(rlo, (a.lo + 1) - r * mf);                     // >= 0: not before the lower ghost row
                rhi = std::max(rhi, (a.lo + a.cnt) - ((r + 1) * mf + 1));     // <= 0: not after the upper ghost row
                cnt = std::min<long long>(cnt, a.cnt);
            }
            for (int i = 0; i < nf; ++i) {
                const MgPx p = mg_pax_t<int64_t>(nf, nc, i);  // coarse rows p.j and p.j + 1 (1-based)
                const long long r = i / mf;
                plo = std::min(plo, p.j - r * mc);
                phi = std::max(phi, (p.j + 1) - ((r + 1) * mc + 1));
            }
            std::printf("%lld %lld %lld %lld %lld\n", rlo, rhi, cnt, plo, phi);
        } else if (kind == 'O') {  // nx rows: mg_rows
            const MgRows g = mg_rows((int)v[0], v[1]);
            std::printf("%d %d %d\n", g.gx, g.gy, g.lbx);
        } else if (kind == 'T') {  // nlevels extents...: mg_tail_plan
            const int L = (int)v[0];
            for (int l = 0; l < L; ++l)
                for (int a = 0; a < 3; ++a) ext[l][a] = v[1 + 3 * l + a];
            const MgTailPlan T = mg_tail_plan(ext, L);
            std::printf("%d %zu\n", T.first, T.lds);
        } else {  // K: the constants
            std::printf("%d %d %d %zu %d %d\n", kMgMaxLevels, kMgTailLevels, kMgTailPoints, kMgTailLds, kRedCap, kBlock);
        }
    }
    return 0;
}
"""


def pad(e):
    return tuple((list(e) + [1, 1])[:3])


# ------------------------------------------------------------------------------------ the cases
SLAB_CASES = ([((48, 8), 8, 0), ((40, 12), 3, 0), ((20, 24, 8), 2, 0), ((48, 8), 8, 2)]
              + [(s[:-1] + (s[-1] // R,), R, 0) for _, s, R in td.CASES.values()]
              + [(local, R, ml) for local, R in [((4096, 512), 8), ((130, 40), 5), ((7, 64), 2), ((3, 3, 32), 4), ((17, 13, 6), 3)]
                 for ml in (0, 1, 2, 3, 9)])
SLAB_REFUSALS = [((48, 7), 8, "odd number of planes"), ((20, 24, 9), 2, "odd number of planes"), ((48,), 2, "1D grids"),
                 ((48, 8), 1, "at least 2 ranks"), ((48, 8), 0, "at least 2 ranks")]
ONE_RANK_PLANS = [tm.plan(s) for s in tm.PLAN_SHAPES] + [ts.plan_semi(s) for s in ts.PLAN_ALL]
SLAB_PLANS = [(td.slab_levels(local, R, ml), R) for local, R, ml in SLAB_CASES]
PLANS = ONE_RANK_PLANS + [lv for lv, _ in SLAB_PLANS]
# a level list describes a whole grid: the one-rank plans, and the slab plans in global extents (a local slab may halve
# 2 rows to 1, which no list may: its global axis has nranks times as many)
LISTS = ONE_RANK_PLANS + [[e[:-1] + (R * e[-1],) for e in lv] for lv, R in SLAB_PLANS]
# level pairs with an axis whose index products come close to, or pass, 2^31 (sqrt(2^31) = 46340.95), kept axes of 8 points
LONG_AXES = (46340, 46341, 65534, 2 ** 20)
LONG_PAIRS = [p for n in LONG_AXES for p in (((n, 8, 1), (n // 2, 8, 1)), ((8, n, 1), (8, n // 2, 1)), ((n, 8, 8), (n // 2, 8, 4)),
                                             ((8, 8, n), (4, 8, n // 2)), ((n, n, 1), (n // 2, n, 1)))]
PAIRS = sorted({(pad(f), pad(c)) for lv in PLANS for f, c in zip(lv, lv[1:])} | set(LONG_PAIRS))
# the malformed lists test_create_levels_rejections gives the device: (grid, list, the reason)
NEITHER = "level 1 of the level list: an axis is neither kept nor n / 2 of an axis of more than 3 points"
COUNT = "the level list has fewer than 1 or more than 32 levels"
BAD_LISTS = [((96, 12), [(48, 12), (24, 12)], "level 0 of the level list is not the problem's grid"),
             ((96, 12), [(96, 12), (48, 5)], NEITHER),
             ((96, 12), [(96, 12), (48, 12), (48, 12)], "level 2 of the level list coarsens no axis"),
             ((96, 12), [(96, 12), (192, 12)], NEITHER),
             ((96, 12), [], COUNT),
             ((96, 12), [(96, 12)] * 33, COUNT),
             ((96, 3), [(96, 3), (48, 1)], NEITHER)]
WEIGHT_AXES = [(n, n // 2) for n in range(4, 131)] + [(n, n) for n in range(4, 131)]
ROW_NX = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 4096, 2 ** 20)
ROW_ROWS = (1, 7, 8, 9, 10 ** 3, 10 ** 6, 2 ** 31 - 1)


def q_plan(kind, shape, ml=0):
    return "%s %d %d %d %d" % ((kind,) + pad(shape) + (ml,))


def q_slabs(local, R, ml=0):
    return "D %d %d %d %d %d" % (pad(local) + (R, ml))


def q_list(grid, lv):
    return "V %d %d %d %d " % (pad(grid) + (len(lv),)) + " ".join(str(n) for e in lv for n in pad(e))


def q_xfer(f, c):
    return "X %d %d %d %d %d %d" % (f + c)


def q_tail(lv):
    return "T %d " % len(lv) + " ".join(str(n) for e in lv for n in pad(e))


@pytest.fixture(scope="module")
def ask():
    """Build the program once and put every query to it in one run: {query line: its answer line}."""
    lines = [q_plan("P", s) for s in tm.PLAN_SHAPES] + [q_plan("S", s) for s in ts.PLAN_ALL]
    lines += [q_slabs(*c) for c in SLAB_CASES] + [q_slabs(local, R) for local, R, _ in SLAB_REFUSALS]
    lines += [q_list(lv[0], lv) for lv in LISTS] + [q_list(g, lv) for g, lv, _ in BAD_LISTS]
    lines += [q_xfer(f, c) for f, c in PAIRS] + [q_tail(lv) for lv in PLANS]
    lines += ["W %d %d" % a for a in WEIGHT_AXES]
    lines += ["G %d %d" % (R, mf) for R in range(2, 17) for mf in range(2, 65, 2)]
    lines += ["O %d %d" % (nx, rows) for nx in ROW_NX for rows in ROW_ROWS] + ["K"]
    lines = sorted(set(lines))
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "mg_plan.cpp"), os.path.join(d, "mg_plan")
        with open(src, "w") as f:
            f.write(SRC)
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src]
        if subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"],
                          capture_output=True).returncode != 0:
            subprocess.run(base, check=True)  # no sanitizer runtimes to link here

        def run(qs):
            p = subprocess.run([exe], input="\n".join(qs) + "\n", capture_output=True, text=True)
            assert p.returncode == 0, p.stderr[-3000:]
            out = p.stdout.splitlines()
            assert len(out) == len(qs)
            return dict(zip(qs, out))

        answers = run(lines)
        # the 32-bit weights only where mg_xfer says they fit (anywhere else the products would overflow): a second run
        s32 = sorted({"E %d %d" % (f[a], c[a]) for f, c in PAIRS if answers[q_xfer(f, c)].split()[1] == "1"
                      for a in range(3) if f[a] != c[a]})
        answers.update(run(s32))
        answers["s32 axes"] = s32
    return answers


def levels_of(answer, dim, skip=1):
    v = [int(t) for t in answer.split()]
    assert len(v) == skip + 3 * v[skip - 1]
    return [tuple(v[skip + 3 * l:skip + 3 * l + dim]) for l in range(v[skip - 1])]


# ------------------------------------------------------------------------------------ plans
def test_plans_match_the_restatements(ask):
    for s in tm.PLAN_SHAPES:
        assert levels_of(ask[q_plan("P", s)], len(s)) == tm.plan(s), s
    for s in ts.PLAN_ALL:
        assert levels_of(ask[q_plan("S", s)], len(s)) == ts.plan_semi(s), s
    for local, R, ml in SLAB_CASES:
        got = ask[q_slabs(local, R, ml)]
        assert int(got.split()[0]) == len(local) - 1, (local, R, ml)  # the slab axis: the slowest one
        assert levels_of(got, len(local), 2) == td.slab_levels(local, R, ml), (local, R, ml)
    for local, R, why in SLAB_REFUSALS:
        got = ask[q_slabs(local, R)]
        assert got.startswith("0 ") and why in got, (local, R, got)


def test_level_list_validation(ask):
    """Every plan is a valid list for its own grid; the malformed lists are refused with the reasons nk_mg_create_levels
    has always given."""
    for lv in LISTS:
        assert ask[q_list(lv[0], lv)] == "ok", lv
    for grid, lv, why in BAD_LISTS:
        assert ask[q_list(grid, lv)] == why, (grid, lv)


# ------------------------------------------------------------------------------------ transfer kernels
def products(nf, nc):
    """the largest magnitude of every product mg_rax_t / mg_pax_t form along an axis n_f -> n_c, over all its points
    (numpy int64: the values stay below 2^42)"""
    F, Cc = nf + 1, nc + 1
    J = np.arange(1, nc + 1, dtype=np.int64)
    lo = np.maximum(((J - 1) * F) // Cc + 1, 1)
    big = [(J - 1) * F, (J + 1) * F, J * F] + [(lo + t) * Cc for t in range(4)]
    big += [np.abs((lo + t) * Cc - J * F) for t in range(4)]
    big.append(np.arange(1, nf + 1, dtype=np.int64) * Cc)
    return max(int(b.max()) for b in big)


def test_transfer_kernel_rule(ask):
    seen = set()
    for f, c in PAIRS:
        mask, s32, general = (int(t) for t in ask[q_xfer(f, c)].split())
        coarsened = [a for a in range(3) if f[a] != c[a]]
        used = [a for a in range(3) if f[a] > 1]
        want_general = not coarsened or coarsened == used or all(f[a] <= 3 for a in range(3) if f[a] == c[a])
        assert bool(general) == want_general, (f, c)
        assert mask == (0 if general else sum(1 << a for a in coarsened)), (f, c)
        if general:
            assert not s32  # (the general kernels have one index width, 64 bits)
        if s32:
            for a in coarsened:
                assert products(f[a], c[a]) < 2 ** 31, (f, c, a)
        seen.add((bool(general), bool(s32)))
    assert seen == {(True, False), (False, True), (False, False)}
    # the long axes fall on both sides: 46340 and 46341 fit, 65534 and 2^20 do not
    for n, fits in zip(LONG_AXES, (1, 1, 0, 0)):
        assert ask[q_xfer((n, 8, 1), (n // 2, 8, 1))] == "1 %d 0" % fits, n
    # on every axis a 32-bit instantiation runs, its weights are the 64-bit ones field for field
    assert len(ask["s32 axes"]) >= 8
    for q in ask["s32 axes"]:
        assert ask[q] == "1", q


def test_weights_are_the_restatements_matrices(ask):
    """mg_pax_t's (j, w) rows are prolong_1d's rows bit for bit; mg_rax_t's integer weights are the columns of P times
    n_f + 1 (integers: P's entries are r / (n_f + 1) and 1 - r / (n_f + 1), rounded once or twice, so the product lies
    within 1e-9 of its integer), over exactly P's nonzero pattern, and D is their sum."""
    for nf, nc in WEIGHT_AXES:
        t = ask["W %d %d" % (nf, nc)].split()
        P = tm.prolong_1d(nf, nc, np.float64)
        rax, pax = t[:7 * nc], t[7 * nc:]
        assert len(pax) == 2 * nf
        got = np.zeros((nf, nc))
        for i in range(nf):
            j, w = int(pax[2 * i]), float.fromhex(pax[2 * i + 1])
            if 0 <= j - 1 < nc:
                got[i, j - 1] += 1 - w
            if 0 <= j < nc:
                got[i, j] += w
        np.testing.assert_array_equal(got, P, err_msg=str((nf, nc)))
        for j in range(nc):
            lo, cnt, w0, w1, w2, w3, D = (int(x) for x in rax[7 * j:7 * j + 7])
            w = [w0, w1, w2, w3]
            assert 1 <= cnt <= 4 and w[cnt:] == [0] * (4 - cnt) and D == sum(w), (nf, nc, j)
            col = P[:, j] * (1 if nf == nc else nf + 1)  # (an axis that is kept: the identity, weight 1)
            assert list(np.flatnonzero(col)) == list(range(lo, lo + cnt)), (nf, nc, j)
            assert np.max(np.abs(col[lo:lo + cnt] - w[:cnt])) < 1e-9 and all(x > 0 for x in w[:cnt]), (nf, nc, j)


def test_one_ghost_plane_is_enough_for_equal_slabs(ask):
    """test_hip_multigrid_dist.py's loop on the functions themselves: with the transfer stencils of the GLOBAL extents,
    every fine row a coarse row of rank r gathers lies in r m_f .. (r + 1) m_f + 1 and every coarse row a fine row
    interpolates from in r m_c .. (r + 1) m_c + 1 (1-based), for 2 <= ranks <= 16 and even m_f <= 64."""
    for R in range(2, 17):
        for mf in range(2, 65, 2):
            rlo, rhi, cnt, plo, phi = (int(t) for t in ask["G %d %d" % (R, mf)].split())
            assert rlo >= 0 and rhi <= 0 and cnt >= 1 and plo >= 0 and phi <= 0, (R, mf)


# ------------------------------------------------------------------------------------ grids and the tail
def test_row_grid(ask):
    max_levels, tail_levels, tail_points, tail_lds, red_cap, block = (int(t) for t in ask["K"].split())
    for nx in ROW_NX:
        for rows in ROW_ROWS:
            gx, gy, lbx = (int(t) for t in ask["O %d %d" % (nx, rows)].split())
            assert 4 <= 2 ** lbx <= 64, (nx, rows)
            assert gx * 2 ** lbx >= nx > (gx - 1) * 2 ** lbx, (nx, rows)
            assert 1 <= gy <= 65535, (nx, rows)
            if gx <= red_cap - 2:
                assert gx * gy <= red_cap - 2, (nx, rows)
            # the smallest block extent that covers a short row, and no more blocks along y than eight rows per thread need
            assert 2 ** lbx == min(64, max(4, 2 ** math.ceil(math.log2(nx)))), (nx, rows)
            assert gy <= -(-rows // (8 * (block >> lbx))), (nx, rows)


def test_tail_rule(ask):
    max_levels, tail_levels, tail_points, tail_lds, red_cap, block = (int(t) for t in ask["K"].split())
    assert (max_levels, tail_levels, tail_points, tail_lds) == (32, 12, 1024, 5 * 8 * 2047)
    firsts = set()
    for lv in PLANS:
        n = [int(np.prod(e)) for e in lv]
        first = next((l for l in range(len(lv)) if n[l] <= tail_points and len(lv) - l <= tail_levels), len(lv))
        got = tuple(int(t) for t in ask[q_tail(lv)].split())
        assert got == (first, 5 * 8 * sum(n[first:])), lv
        assert got[1] <= tail_lds, lv
        firsts.add(0 if first == 0 else (1 if first < len(lv) else 2))
    assert firsts == {0, 1, 2}  # the whole cycle in the tail, a proper tail, none
