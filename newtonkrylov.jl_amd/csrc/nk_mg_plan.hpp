// nk_mg_plan.hpp -- the multigrid's host-only rules as pure functions: the level plans (mg_plan, mg_plan_semi,
// mg_plan_slabs), the validation of a caller's level list, which transfer kernels a level pair runs (mg_xfer), the
// grid of the row-shaped kernels (mg_rows), the coarse tail's first level and LDS, the ghost-plane size of a slab
// level, and the integer weight formulas of the transfers (mg_rax_t, mg_pax_t), which the kernels of nk_mg.hip call
// as they stand here.  Numbers in, a plan out: nothing touches a device, so every rule is callable -- and tested --
// on the CPU (tests/test_mg_plan.py, against the tests' restatements).  No HIP header: this file compiles with a
// plain host compiler.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "nk_plan.hpp"

// the weight formulas run on the device as well
#ifdef __HIPCC__
#define NK_MG_HD __host__ __device__ __forceinline__
#else
#define NK_MG_HD inline
#endif

namespace nk {

constexpr int kMgMaxLevels = 32;
constexpr int kMgTailLevels = 12;      // 1024 -> 2 points in 1D is 10 levels
constexpr int kMgTailPoints = 1024;    // first tail level: at most this many points (5 arrays x < 2 x 1024 x 8 B = 80 KiB LDS)
constexpr int kMgTailThreads = 1024;
// LDS of the tail: its levels at least halve, so they hold at most 2 kMgTailPoints - 1 points, five arrays each
constexpr size_t kMgTailLds = 5 * sizeof(double) * (2 * kMgTailPoints - 1);
constexpr int kMgMinmaxBlocks = 64;

// ---------------------------------------------------------------- level plans
// the level extents (all integer arithmetic)
inline int mg_plan(const int64_t n0[3], int max_levels, int64_t (*ext)[3]) {
    int64_t n[3] = {n0[0], n0[1], n0[2]};
    int L = 0;
    for (;;) {
        for (int a = 0; a < 3; ++a) ext[L][a] = n[a];
        ++L;
        if (L == kMgMaxLevels || (max_levels > 0 && L >= max_levels)) break;
        if (n[0] <= 3 && n[1] <= 3 && n[2] <= 3) break;
        for (int a = 0; a < 3; ++a)
            if (n[a] > 3) n[a] /= 2;
    }
    return L;
}

// The semicoarsened plan.  On every level only the axes whose coupling c_a = |k_a| / h_a² is at least tau times
// the strongest one are halved (point Jacobi smooths the error along those; the weakly coupled axes wait until the
// level is isotropic).  Double precision, in this order (the tests restate it): L_a = (n_a^0 + 1) h_a^0,
// c_a = |k_a| ((n_a + 1) / L_a)² over the axes of more than 3 points.  The axis of c_max always qualifies, so every
// level at least halves its points.
inline int mg_plan_semi(const int64_t n0[3], const double h[3], const double k[3], double tau, int max_levels, int64_t (*ext)[3]) {
    int64_t n[3] = {n0[0], n0[1], n0[2]};
    double len[3];
    for (int a = 0; a < 3; ++a) len[a] = (double)(n0[a] + 1) * h[a];
    int L = 0;
    for (;;) {
        for (int a = 0; a < 3; ++a) ext[L][a] = n[a];
        ++L;
        if (L == kMgMaxLevels || (max_levels > 0 && L >= max_levels)) break;
        if (n[0] <= 3 && n[1] <= 3 && n[2] <= 3) break;
        double cc[3] = {0.0, 0.0, 0.0}, cmax = 0.0;
        for (int a = 0; a < 3; ++a)
            if (n[a] > 3) {
                const double q = (double)(n[a] + 1) / len[a];
                cc[a] = std::fabs(k[a]) * (q * q);
                cmax = std::fmax(cmax, cc[a]);
            }
        const double bar = tau * cmax;
        for (int a = 0; a < 3; ++a)
            if (n[a] > 3 && cc[a] >= bar) n[a] /= 2;
    }
    return L;
}

// The plan of a slab-distributed grid in LOCAL extents (equal slabs of the slowest axis: every rank holds n0,
// the global extent of that axis is nranks n0[ax]).  It is mg_plan of the global grid cut after L_d levels: level
// l + 1 exists only while the local slab extent m_l is even, then m_{l+1} = m_l / 2 (the global nranks m_l >= 4 is
// halved by mg_plan's rule as well; the other axes are whole on every rank).  *ax = the slab axis (1: y, 2: z).
// Returns 0 with *why set where no distributed hierarchy exists.
inline int mg_plan_slabs(const int64_t n0[3], int nranks, int max_levels, int64_t (*ext)[3], int* ax, const char** why) {
    *why = nullptr;
    *ax = n0[2] > 1 ? 2 : 1;
    if (nranks < 2) *why = "a slab plan needs at least 2 ranks";
    else if (n0[1] == 1 && n0[2] == 1) *why = "1D grids are not distributed (2D y-slabs and 3D z-slabs only)";
    else if (n0[*ax] % 2 != 0) *why = "slabs of an odd number of planes cannot be coarsened";
    else if ((int64_t)nranks * n0[*ax] >= ((int64_t)1 << 31)) *why = "at most 2^31 - 1 planes along the slab axis";
    if (*why) return 0;
    int64_t g[3] = {n0[0], n0[1], n0[2]};
    g[*ax] *= nranks;
    int Ld = 1;
    for (int64_t ml = n0[*ax]; ml % 2 == 0; ml /= 2) ++Ld;
    if (max_levels > 0) Ld = std::min(Ld, max_levels);
    const int L = mg_plan(g, Ld, ext);  // (L == Ld: the global slab axis stays above 3 points while m_l is even)
    for (int l = 0; l < L; ++l) ext[l][*ax] /= nranks;
    return L;
}

// The plan of a periodic grid (neighbours wrap, n_a >= 3 per used axis).  The levels are nested -- coarse point j is
// fine point 2 j -- so an axis can be halved only while it is even, and n_a / 2 >= 3 must remain: an axis is halvable
// when n_a is even and n_a >= 6.  Level l + 1 halves every halvable axis and keeps the others; the plan ends when no
// axis is halvable.  Extents (3, 4 or 5) 2^k coarsen all the way down; an odd axis is never coarsened.
inline bool mg_per_halvable(int64_t n) { return n % 2 == 0 && n >= 6; }
// null where a periodic hierarchy exists on the grid n0 of `dim` used axes (the first dim ones), else the reason.
// dim = 0: taken from the extents -- the axes up to the last one of more than one point (a plan query has no kind)
inline const char* mg_plan_per_why(const int64_t n0[3], int dim) {
    if (dim == 0) dim = n0[2] > 1 ? 3 : (n0[1] > 1 ? 2 : 1);
    for (int a = 0; a < 3; ++a)
        if (a < dim ? n0[a] < 3 : n0[a] != 1) return "a periodic axis needs at least 3 points (and an unused one has 1)";
    return nullptr;
}
inline int mg_plan_per(const int64_t n0[3], int max_levels, int64_t (*ext)[3]) {
    int64_t n[3] = {n0[0], n0[1], n0[2]};
    int L = 0;
    for (;;) {
        for (int a = 0; a < 3; ++a) ext[L][a] = n[a];
        ++L;
        if (L == kMgMaxLevels || (max_levels > 0 && L >= max_levels)) break;
        if (!mg_per_halvable(n[0]) && !mg_per_halvable(n[1]) && !mg_per_halvable(n[2])) break;
        for (int a = 0; a < 3; ++a)
            if (mg_per_halvable(n[a])) n[a] /= 2;
    }
    return L;
}

// A caller's level list (nlevels x 3 extents) for the grid n0: null where it is a hierarchy -- level 0 is the grid,
// every later level keeps each axis or halves one of more than 3 points, and coarsens at least one -- else the reason
// (a literal, or written into buf where it names the level)
inline const char* mg_levels_why(const int64_t n0[3], const int64_t* given, int nlevels, char (&buf)[128]) {
    if (nlevels < 1 || nlevels > kMgMaxLevels) return "the level list has fewer than 1 or more than 32 levels";
    for (int a = 0; a < 3; ++a)
        if (given[a] != n0[a]) return "level 0 of the level list is not the problem's grid";
    for (int l = 1; l < nlevels; ++l) {
        bool coarsened = false;
        for (int a = 0; a < 3; ++a) {
            const int64_t v = given[3 * l + a], f = given[3 * (l - 1) + a];
            if (v == f) continue;
            if (!(f > 3 && v == f / 2)) {
                std::snprintf(buf, sizeof(buf), "level %d of the level list: an axis is neither kept nor n / 2 of an axis of more than 3 points", l);
                return buf;
            }
            coarsened = true;
        }
        if (!coarsened) {
            std::snprintf(buf, sizeof(buf), "level %d of the level list coarsens no axis", l);
            return buf;
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------- launches
// Which transfer kernels a level pair runs.  mask = the coarsened axes when they are a proper subset of the used ones
// (a semicoarsened level: the k_mg_*_m instantiation of that mask), 0 = the general kernels (every used axis
// coarsened).  s32: the index products of mg_rax_t / mg_pax_t along the coarsened axes fit 32 bits.
struct MgXfer {
    int mask;
    bool s32;
    bool general;
};
inline MgXfer mg_xfer(const int nf[3], const int nc[3]) {
    int mask = 0, used = 0;
    bool s32 = true;
    for (int a = 0; a < 3; ++a) {
        if (nf[a] > 1) used |= 1 << a;
        if (nf[a] != nc[a]) {
            mask |= 1 << a;
            s32 = s32 && (int64_t)(nf[a] + 4) * (nc[a] + 2) < ((int64_t)1 << 31);
        }
    }
    // axes of at most 3 points that stay as they are while every other one is coarsened: also the general kernels
    bool rest_small = true;
    for (int a = 0; a < 3; ++a)
        if (nf[a] == nc[a] && nf[a] > 3) rest_small = false;
    if (mask == 0 || mask == used || rest_small) return MgXfer{0, false, true};
    return MgXfer{mask, s32, false};
}

// grid of the row-shaped kernels for rows of nx points: 2^lbx = the block's extent along x (4 .. 64, the smallest
// that covers a short row), about eight rows per thread, at most kRedCap - 2 blocks as the streaming kernels
struct MgRows {
    int gx, gy, lbx;
};
inline MgRows mg_rows(int nx, int64_t rows) {
    int lbx = 6;
    while (lbx > 2 && (1 << (lbx - 1)) >= nx) --lbx;
    const int64_t gx = ((int64_t)nx + (1 << lbx) - 1) >> lbx, rpb = kBlock >> lbx;
    int64_t gy = (rows + 8 * rpb - 1) / (8 * rpb);
    gy = std::min<int64_t>(gy, std::max<int64_t>(1, (kRedCap - 2) / gx));
    gy = std::min<int64_t>(gy, 65535);
    return MgRows{(int)gx, (int)gy, lbx};
}

// the coarse tail of a plan: its first level -- the first of at most kMgTailPoints points with at most kMgTailLevels
// levels from it on; nlev: none -- and the LDS its levels take (five arrays each)
struct MgTailPlan {
    int first;
    size_t lds;
};
inline MgTailPlan mg_tail_plan(const int64_t (*ext)[3], int nlev) {
    MgTailPlan T{nlev, 0};
    for (int l = 0; l < nlev; ++l) {
        const int64_t n = ext[l][0] * ext[l][1] * ext[l][2];
        if (T.first == nlev && n <= kMgTailPoints && nlev - l <= kMgTailLevels) T.first = l;
        if (T.first < nlev) T.lds += 5 * sizeof(double) * (size_t)n;
    }
    return T;
}

// doubles of the one ghost plane before and after a slab level's arrays (slab_ax 1: a row, 2: an xy plane; 0: one rank)
inline int64_t mg_ghost(const int64_t ext[3], int slab_ax) { return slab_ax ? ext[0] * (slab_ax == 2 ? ext[1] : 1) : 0; }

// ---------------------------------------------------------------- transfer weights
// one axis of R = D^-1 P^T for coarse point j (0-based): the fine points lo .. lo + cnt - 1 with integer weights
// w = (n_f + 1) - |I (n_c + 1) - J (n_f + 1)| (I, J 1-based) and their sum D; an axis that was not coarsened is
// the identity
struct MgAx {
    int lo, cnt, w[4], D;
};
// I: the integer type of the products, which reach n_f^2 / 2: 64-bit in general (an axis may have more than 65534
// points), 32-bit where mg_xfer has checked that they fit (the same integers either way)
template <typename I>
NK_MG_HD MgAx mg_rax_t(int nf, int nc, int j) {
    MgAx a{j, 1, {1, 0, 0, 0}, 1};
    if (nf == nc) return a;
    const I J = j + 1, F = nf + 1, Cc = nc + 1;
    I lo = ((J - 1) * F) / Cc + 1, hi = ((J + 1) * F - 1) / Cc;
    lo = lo < 1 ? 1 : lo;
    hi = hi > nf ? nf : hi;
    hi = hi > lo + 3 ? lo + 3 : hi;  // the open interval has length 2 (n_f + 1) / (n_c + 1) <= 4: at most 4 points
    a.lo = (int)(lo - 1);
    a.cnt = (int)(hi - lo + 1);
    a.D = 0;
    for (int t = 0; t < 4; ++t) {
        const I d = (lo + t) * Cc - J * F;
        a.w[t] = t < a.cnt ? (int)(F - (d < 0 ? -d : d)) : 0;
        a.D += a.w[t];
    }
    return a;
}

// one axis of P for fine point i (0-based): coarse points j - 1 and j (0-based; outside 0 .. n_c - 1: the
// boundary, 0) with weights 1 - w and w, w = (q mod (n_f + 1)) / (n_f + 1), q = (i + 1) (n_c + 1), j = q / (n_f + 1)
struct MgPx {
    int j;
    double w;
};
template <typename I>
NK_MG_HD MgPx mg_pax_t(int nf, int nc, int i) {
    if (nf == nc) return MgPx{i + 1, 0.0};
    const I q = (I)(i + 1) * (nc + 1), F = nf + 1;  // q reaches n_f^2 / 2 (I as in mg_rax_t)
    return MgPx{(int)(q / F), (double)(q % F) / (double)F};
}

// ---------------------------------------------------------------- periodic transfers (nested levels, n_f = 2 n_c)
// one coarsened axis of R = D^-1 P^T for coarse point j: the fine points m = (2 j - 1) mod n_f, c = 2 j and
// p = (2 j + 1) mod n_f with the integer weights 1, 2, 1 (D = 4).  n_f is even, so only m wraps (at j = 0);
// 32-bit indices, the wrap a compare-and-select
struct MgPerR {
    int m, c, p;
};
NK_MG_HD MgPerR mg_per_rax(int nf, int j) {
    const int c = 2 * j;
    return MgPerR{j > 0 ? c - 1 : nf - 1, c, c + 1};
}
// an axis that was kept: the identity -- mg_restrict_per reads c alone there and divides by 1 (m and p only keep the
// type of the three axes the same)
NK_MG_HD MgPerR mg_per_rkeep(int j) { return MgPerR{j, j, j}; }

// one coarsened axis of P for fine point i: e_f[i] = (1 - w) e_c[j0] + w e_c[j1]; an even i takes e_c[i / 2] (w = 0,
// j1 is not read), an odd one w = 1/2 between j0 = (i - 1) / 2 and j1 = ((i + 1) / 2) mod n_c
struct MgPerP {
    int j0, j1;
    double w;
};
NK_MG_HD MgPerP mg_per_pax(int nc, int i) {
    const int j0 = i >> 1, j1 = j0 + 1 < nc ? j0 + 1 : 0;
    return (i & 1) ? MgPerP{j0, j1, 0.5} : MgPerP{j0, j0, 0.0};
}
NK_MG_HD MgPerP mg_per_pkeep(int i) { return MgPerP{i, i, 0.0}; }

}  // namespace nk
