// nk_mg.hip -- geometric multigrid preconditioner (NK_PRECOND_MG) for the stencil Jacobians
//   A_l = Σ_a k_a δ²_a(h_a^l) + diag(s_l)      (Bratu: k = 1, s_0 = λ exp(u); heat: k = θ a Δt, s_0 = -1).
// One V-cycle from x = 0 per application: weighted Jacobi smoothing, coarse operators rediscretised on the
// non-nested grids n_{l+1} = n_l / 2, linear prolongation P, restriction R = D^-1 P^T as a gather (no
// atomics: every application is bit-identical).  The per-point arithmetic lives in device functions on
// plain pointers, shared by the per-level kernels (global memory) and the coarse tail (k_mg_tail: every
// level of at most kMgTailPoints points, all of them in one work-group's LDS, one launch).  The level extents are a
// plan: mg_plan halves every axis of more than 3 points, mg_plan_semi only the strongly coupled ones (anisotropic
// grids and coefficients), nk_mg_create_levels takes any such list; the transfers between two levels that coarsen a
// proper subset of the axes run kernels instantiated on that subset (k_mg_restrict_m / k_mg_prolong_m).  On a
// distributed context the hierarchy lives on equal slabs of the slowest axis: mg_plan_slabs cuts mg_plan's levels where
// the local slab extent stops being even, the level arrays carry one ghost plane per side, and the same kernels run in
// their slab instantiation (AX = the slab axis; 0: one rank) with the context's ghost-plane exchange between them --
// the one-rank cycle of the global grid, bit for bit.  A periodic grid (NK_BC_PERIODIC, the heat kinds, one rank) has a
// hierarchy of its own: nested levels (mg_plan_per: an axis is halved while it is even and >= 6), neighbours that wrap
// (the PER instantiations of the device functions, the per-level kernels and the tail) and transfers with fixed
// footprints (k_mg_restrict_p / k_mg_prolong_p).  One text per expression: the device functions and the per-level
// kernels are templates on AX, and mg_pick turns the runtime AX, RED, MASK, S32 and OUT into the instantiation a
// launcher runs.  The host-only rules (plans, level-list validation, kernel choice, grids, the tail's extent, the
// transfers' integer weights) are nk_mg_plan.hpp, which a CPU test calls.  DESIGN.md §10.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "nk_device.hpp"
#include "nk_mg_plan.hpp"

namespace nk {
namespace {

struct MgLv {
    int nx, ny, nz, n;
    double cx, cy, cz;  // k_a / h_a^2 (0 along an unused axis)
};
// A distributed hierarchy: the level's rows along the slowest axis are split over the ranks (equal slabs); every level
// array carries one ghost plane before and after its interior, which the separate-launch exchange fills with the
// neighbours' boundary planes (zero, as allocated, on the physical side of the first and last rank).  AX = the slab
// axis (1: y of a 2D grid, 2: z of a 3D grid; 0: one rank).  L holds the LOCAL extents.  Along AX the device functions
// read the ghost plane where the one-rank form substitutes 0 -- the same value -- and the transfers take their weights
// from the GLOBAL row and the GLOBAL extents; only the memory row is local.
struct MgSl {
    int ngf, ngc;  // global extents of the fine / coarse level along the slab axis
    int of, oc;    // this rank's first global row (0-based) on the fine / coarse level
};

// Σ_a c_a (x_- + x_+) at point i, zero Dirichlet boundary.  Along AX the neighbours are the ghost planes, read as they
// are (the local extent along AX may be 1); a y-slab grid is 2D.  PER (one rank, AX = 0): a periodic grid -- the
// neighbours wrap (point 0's lower neighbour is point n_a - 1), the same sums in the same order
template <int AX = 0, bool PER = false>
__device__ __forceinline__ double mg_off(const MgLv& L, const double* x, int i) {
    const int ix = i % L.nx, t = i / L.nx, iy = t % L.ny, iz = t / L.ny;
    if constexpr (PER) {
        const double xm = x[ix > 0 ? i - 1 : i + (L.nx - 1)], xp = x[ix + 1 < L.nx ? i + 1 : i - (L.nx - 1)];
        double o = L.cx * (xm + xp);
        if (L.ny > 1) {
            const int wy = L.nx * (L.ny - 1);
            const double ym = x[iy > 0 ? i - L.nx : i + wy], yp = x[iy + 1 < L.ny ? i + L.nx : i - wy];
            o = o + L.cy * (ym + yp);
        }
        if (L.nz > 1) {
            const int pl = L.nx * L.ny, wz = pl * (L.nz - 1);
            const double zm = x[iz > 0 ? i - pl : i + wz], zp = x[iz + 1 < L.nz ? i + pl : i - wz];
            o = o + L.cz * (zm + zp);
        }
        return o;
    }
    const double xm = ix > 0 ? x[i - 1] : 0.0, xp = ix + 1 < L.nx ? x[i + 1] : 0.0;
    double o = L.cx * (xm + xp);
    if (AX == 1 || L.ny > 1) {
        const double ym = AX == 1 || iy > 0 ? x[i - L.nx] : 0.0, yp = AX == 1 || iy + 1 < L.ny ? x[i + L.nx] : 0.0;
        o = o + L.cy * (ym + yp);
    }
    if (AX == 2 || (AX == 0 && L.nz > 1)) {
        const int pl = L.nx * L.ny;
        const double zm = AX == 2 || iz > 0 ? x[i - pl] : 0.0, zp = AX == 2 || iz + 1 < L.nz ? x[i + pl] : 0.0;
        o = o + L.cz * (zm + zp);
    }
    return o;
}
// weighted Jacobi x <- x + ω (b - A x) / diag, written on 1 / diag alone:
//   x <- (1 - ω) x + ω ((b - Σ_a c_a (x_- + x_+)) / diag);   from x = 0: x = ω (b / diag)
__device__ __forceinline__ double mg_sweep0_pt(double omega, const double* b, const double* idg, int i) {
    return omega * (idg[i] * b[i]);
}
template <int AX = 0, bool PER = false>
__device__ __forceinline__ double mg_sweep_pt(const MgLv& L, double omega, double om1, const double* x, const double* b,
                                              const double* idg, int i) {
    const double t = b[i] - mg_off<AX, PER>(L, x, i);
    return om1 * x[i] + omega * (idg[i] * t);
}
template <int AX = 0, bool PER = false>
__device__ __forceinline__ double mg_resid_pt(const MgLv& L, const double* x, const double* b, const double* dg, int i) {
    return b[i] - (mg_off<AX, PER>(L, x, i) + dg[i] * x[i]);
}

// the transfers' weights along one axis: mg_rax_t / mg_pax_t of nk_mg_plan.hpp, here with 64-bit products
__device__ __forceinline__ MgAx mg_rax(int nf, int nc, int j) { return mg_rax_t<int64_t>(nf, nc, j); }
// the gather of one coarse point from its three axes, and the final division
__device__ __forceinline__ double mg_restrict_ax(const MgLv& Lf, const MgAx& ax, const MgAx& ay, const MgAx& az, const double* r) {
    double acc = 0.0;
    for (int c = 0; c < az.cnt; ++c)
        for (int b = 0; b < ay.cnt; ++b) {
            const double wyz = (double)az.w[c] * (double)ay.w[b];
            const int row = ((az.lo + c) * Lf.ny + (ay.lo + b)) * Lf.nx + ax.lo;
            for (int a = 0; a < ax.cnt; ++a) acc = fma(wyz * (double)ax.w[a], r[row + a], acc);
        }
    return acc / ((double)az.D * (double)ay.D * (double)ax.D);
}
// slabs: the weights along AX come from the global row and extents, then lo shifts to the memory row (-1 and the
// slab's extent are the ghost planes)
template <int AX = 0>
__device__ __forceinline__ double mg_restrict_pt(const MgLv& Lf, const MgLv& Lc, const double* r, int j, const MgSl& S = MgSl{}) {
    const int jx = j % Lc.nx, t = j / Lc.nx, jy = t % Lc.ny, jz = t / Lc.ny;
    const MgAx ax = mg_rax(Lf.nx, Lc.nx, jx);
    MgAx ay = AX == 1 ? mg_rax(S.ngf, S.ngc, S.oc + jy) : mg_rax(Lf.ny, Lc.ny, jy);
    MgAx az = AX == 2 ? mg_rax(S.ngf, S.ngc, S.oc + jz) : mg_rax(Lf.nz, Lc.nz, jz);
    if constexpr (AX != 0) {
        MgAx& as = AX == 1 ? ay : az;
        as.lo -= S.of;
        // one ghost plane suffices for equal slabs (tests/test_mg_plan.py checks it exhaustively); a row beyond it
        // is never read
        if (as.lo < -1 || as.lo + as.cnt - 1 > (AX == 1 ? Lf.ny : Lf.nz)) return NAN;
    }
    return mg_restrict_ax(Lf, ax, ay, az, r);
}

__device__ __forceinline__ MgPx mg_pax(int nf, int nc, int i) { return mg_pax_t<int64_t>(nf, nc, i); }
// the interpolation of one fine point from its three axes.  MASK (bit a: axis a is coarsened) = 7 is the general form,
// in which an axis that was not coarsened is the identity through its weights 1 and 0; an axis outside MASK is known
// to be the identity, and its zero-weight neighbour is neither read nor added: the same value (a term 0 * e of a
// finite e only decides the sign of a zero result).  The coarse rows in memory are 0 .. extent - 1, and -1 .. extent
// along the slab axis AX (its ghost planes).  A slab form takes the four bounds by value (mg_prolong_pt), the one-rank
// form reads the level's extents in place: the other way round either kernel compiles to some 25 instructions more
template <int MASK, int AX = 0>
__device__ __forceinline__ double mg_prolong_ax(const MgLv& Lc, const MgPx& px, const MgPx& py, const MgPx& pz, const double* e,
                                                int ylo = 0, int yhi = 0, int zlo = 0, int zhi = 0) {
    constexpr bool CX = (MASK & 1) != 0, CY = (MASK & 2) != 0, CZ = (MASK & 4) != 0;
    double vz[2] = {0.0, 0.0};
    for (int c = 0; c < (CZ ? 2 : 1); ++c) {
        const int jz = pz.j - 1 + c;
        double vy[2] = {0.0, 0.0};
        for (int b = 0; b < (CY ? 2 : 1); ++b) {
            const int jy = py.j - 1 + b;
            double lo = 0.0, hi = 0.0;
            if (AX == 0 ? jz >= 0 && jz < Lc.nz && jy >= 0 && jy < Lc.ny : jz >= zlo && jz < zhi && jy >= ylo && jy < yhi) {
                const int row = (jz * Lc.ny + jy) * Lc.nx;
                if (px.j - 1 >= 0) lo = e[row + px.j - 1];
                if (CX && px.j < Lc.nx) hi = e[row + px.j];
            }
            vy[b] = CX ? (1.0 - px.w) * lo + px.w * hi : lo;
        }
        vz[c] = CY ? (1.0 - py.w) * vy[0] + py.w * vy[1] : vy[0];
    }
    return CZ ? (1.0 - pz.w) * vz[0] + pz.w * vz[1] : vz[0];
}
template <int AX = 0>
__device__ __forceinline__ double mg_prolong_pt(const MgLv& Lf, const MgLv& Lc, const double* e, int i, const MgSl& S = MgSl{}) {
    const int ix = i % Lf.nx, t = i / Lf.nx, iy = t % Lf.ny, iz = t / Lf.ny;
    const MgPx px = mg_pax(Lf.nx, Lc.nx, ix);
    MgPx py = AX == 1 ? mg_pax(S.ngf, S.ngc, S.of + iy) : mg_pax(Lf.ny, Lc.ny, iy);
    MgPx pz = AX == 2 ? mg_pax(S.ngf, S.ngc, S.of + iz) : mg_pax(Lf.nz, Lc.nz, iz);
    if (AX == 1) py.j -= S.oc;
    if (AX == 2) pz.j -= S.oc;
    return mg_prolong_ax<7, AX>(Lc, px, py, pz, e, AX == 1 ? -1 : 0, AX == 1 ? Lc.ny + 1 : Lc.ny, AX == 2 ? -1 : 0,
                                AX == 2 ? Lc.nz + 1 : Lc.nz);
}

// The periodic transfers (nested levels; mg_per_rax / mg_per_pax of nk_mg_plan.hpp give the wrapped indices).  cx, cy,
// cz: the axis is coarsened -- compile-time constants in the row-shaped kernels, level data in the tail.  nxf / plf and
// nxc / plc: a row and an xy plane of the source level.
// R: per coarsened axis (r_m + r_p) + 2 r_c, the x axis innermost, then one division by D = 4 per coarsened axis (a
// power of two).  A fixed order, and a constant r comes back exactly: (s + s) + 2 s = 4 s
__device__ __forceinline__ double mg_restrict_per(int nxf, int plf, bool cx, bool cy, bool cz, const MgPerR& ax, const MgPerR& ay,
                                                  const MgPerR& az, const double* r) {
    auto line = [&](int base) { return cx ? fma(2.0, r[base + ax.c], r[base + ax.m] + r[base + ax.p]) : r[base + ax.c]; };
    auto plane = [&](int base) {
        return cy ? fma(2.0, line(base + ay.c * nxf), line(base + ay.m * nxf) + line(base + ay.p * nxf)) : line(base + ay.c * nxf);
    };
    const double v = cz ? fma(2.0, plane(az.c * plf), plane(az.m * plf) + plane(az.p * plf)) : plane(az.c * plf);
    return v / ((cx ? 4.0 : 1.0) * (cy ? 4.0 : 1.0) * (cz ? 4.0 : 1.0));
}
// P: per coarsened axis e[j0] at an even fine index, (1 - w) e[j0] + w e[j1] (w = 1/2) at an odd one
__device__ __forceinline__ double mg_prolong_per(int nxc, int plc, bool cx, bool cy, bool cz, const MgPerP& px, const MgPerP& py,
                                                 const MgPerP& pz, const double* e) {
    auto line = [&](int base) {
        double v = e[base + px.j0];
        if (cx && px.w != 0.0) v = (1.0 - px.w) * v + px.w * e[base + px.j1];
        return v;
    };
    auto plane = [&](int base) {
        double v = line(base + py.j0 * nxc);
        if (cy && py.w != 0.0) v = (1.0 - py.w) * v + py.w * line(base + py.j1 * nxc);
        return v;
    };
    double v = plane(pz.j0 * plc);
    if (cz && pz.w != 0.0) v = (1.0 - pz.w) * v + pz.w * plane(pz.j1 * plc);
    return v;
}
// one point of either, for the tail
__device__ __forceinline__ double mg_restrict_per_pt(const MgLv& Lf, const MgLv& Lc, const double* r, int j) {
    const int jx = j % Lc.nx, t = j / Lc.nx, jy = t % Lc.ny, jz = t / Lc.ny;
    const bool cx = Lf.nx != Lc.nx, cy = Lf.ny != Lc.ny, cz = Lf.nz != Lc.nz;
    return mg_restrict_per(Lf.nx, Lf.nx * Lf.ny, cx, cy, cz, cx ? mg_per_rax(Lf.nx, jx) : mg_per_rkeep(jx),
                           cy ? mg_per_rax(Lf.ny, jy) : mg_per_rkeep(jy), cz ? mg_per_rax(Lf.nz, jz) : mg_per_rkeep(jz), r);
}
__device__ __forceinline__ double mg_prolong_per_pt(const MgLv& Lf, const MgLv& Lc, const double* e, int i) {
    const int ix = i % Lf.nx, t = i / Lf.nx, iy = t % Lf.ny, iz = t / Lf.ny;
    const bool cx = Lf.nx != Lc.nx, cy = Lf.ny != Lc.ny, cz = Lf.nz != Lc.nz;
    return mg_prolong_per(Lc.nx, Lc.nx * Lc.ny, cx, cy, cz, cx ? mg_per_pax(Lc.nx, ix) : mg_per_pkeep(ix),
                          cy ? mg_per_pax(Lc.ny, iy) : mg_per_pkeep(iy), cz ? mg_per_pax(Lc.nz, iz) : mg_per_pkeep(iz), e);
}

// ------------------------------------------------------------------------------ per-level kernels (AX: one rank or slabs)
__global__ __launch_bounds__(kBlock) void k_mg_sweep0(int n, double omega, double* x, const double* b,
                                                     const double* __restrict__ idg) {
    NK_CHUNKED(i, n) x[i] = mg_sweep0_pt(omega, b, idg, (int)i);
}
// xn must not alias x (the ping-pong pair); b is only read at the point written
template <int AX, bool PER>
__global__ __launch_bounds__(kBlock) void k_mg_sweep(MgLv L, double omega, double om1, double* xn, const double* __restrict__ x,
                                                    const double* b, const double* __restrict__ idg) {
    NK_CHUNKED(i, L.n) xn[i] = mg_sweep_pt<AX, PER>(L, omega, om1, x, b, idg, (int)i);
}
// The sweep that writes the cycle's result z: the same per-point arithmetic times sigma (+-1: exact), and with RED the
// partials of <b, z> (b = the cycle's input v, read at the point written anyway) in a fixed order, no atomics
template <bool RED>
__global__ __launch_bounds__(kBlock) void k_mg_sweep0_z(int n, double omega, double sigma, double* z, const double* b,
                                                       const double* __restrict__ idg, double* __restrict__ part, int fin) {
    __shared__ double sh[kShN];
    double acc = 0.0;
    NK_CHUNKED(i, n) {
        const double bi = b[i];
        const double zi = sigma * mg_sweep0_pt(omega, b, idg, (int)i);
        z[i] = zi;
        if (RED) acc = fma(bi, zi, acc);
    }
    if (RED) publish(acc, part, fin, sh);
}
template <int AX, bool PER, bool RED>
__global__ __launch_bounds__(kBlock) void k_mg_sweep_z(MgLv L, double omega, double om1, double sigma, double* z,
                                                      const double* __restrict__ x, const double* b, const double* __restrict__ idg,
                                                      double* __restrict__ part, int fin) {
    __shared__ double sh[kShN];
    double acc = 0.0;
    NK_CHUNKED(i, L.n) {
        const double bi = b[i];
        const double zi = sigma * mg_sweep_pt<AX, PER>(L, omega, om1, x, b, idg, (int)i);
        z[i] = zi;
        if (RED) acc = fma(bi, zi, acc);
    }
    if (RED) publish(acc, part, fin, sh);
}
template <int AX, bool PER>
__global__ __launch_bounds__(kBlock) void k_mg_resid(MgLv L, double* __restrict__ r, const double* __restrict__ x,
                                                    const double* __restrict__ b, const double* __restrict__ dg) {
    NK_CHUNKED(i, L.n) r[i] = mg_resid_pt<AX, PER>(L, x, b, dg, (int)i);
}
// (S is read by the slab forms only)
template <int AX>
__global__ __launch_bounds__(kBlock) void k_mg_restrict(MgLv Lf, MgLv Lc, MgSl S, double* __restrict__ bc,
                                                       const double* __restrict__ r) {
    NK_CHUNKED(j, Lc.n) bc[j] = mg_restrict_pt<AX>(Lf, Lc, r, (int)j, S);
}
template <int AX>
__global__ __launch_bounds__(kBlock) void k_mg_prolong(MgLv Lf, MgLv Lc, MgSl S, double* __restrict__ x,
                                                      const double* __restrict__ e) {
    NK_CHUNKED(i, Lf.n) x[i] = x[i] + mg_prolong_pt<AX>(Lf, Lc, e, (int)i, S);
}
// The transfers between two levels of a semicoarsened plan, instantiated on the set MASK of coarsened axes (a proper
// subset of the used axes; all of them is the kernel above).  The block is 2^lbx points of a grid row by
// kBlock >> lbx rows: a thread keeps its x index, so the x axis' weights are computed once and then reused down the
// rows it walks, a wave reads and writes whole contiguous row segments (x coarsened: up to four contiguous fine
// points per coarse point; y or z coarsened: two to four whole rows), and the axes outside MASK cost no index
// arithmetic at all.  Per point the same device functions, fma order and final division as the general kernels.
// S32: the index products fit 32 bits.
template <int MASK, bool S32>
__global__ __launch_bounds__(kBlock) void k_mg_restrict_m(MgLv Lf, MgLv Lc, int lbx, double* __restrict__ bc,
                                                         const double* __restrict__ r) {
    using I = typename std::conditional<S32, int32_t, int64_t>::type;
    const int jx = (int)(blockIdx.x << lbx) + (int)(threadIdx.x & ((1u << lbx) - 1));
    if (jx >= Lc.nx) return;
    const MgAx ax = (MASK & 1) ? mg_rax_t<I>(Lf.nx, Lc.nx, jx) : MgAx{jx, 1, {1, 0, 0, 0}, 1};
    const int64_t rows = (int64_t)Lc.ny * Lc.nz, rpb = kBlock >> lbx;
    for (int64_t row = blockIdx.y * rpb + (threadIdx.x >> lbx); row < rows; row += gridDim.y * rpb) {
        const int jy = (int)(row % Lc.ny), jz = (int)(row / Lc.ny);
        const MgAx ay = (MASK & 2) ? mg_rax_t<I>(Lf.ny, Lc.ny, jy) : MgAx{jy, 1, {1, 0, 0, 0}, 1};
        const MgAx az = (MASK & 4) ? mg_rax_t<I>(Lf.nz, Lc.nz, jz) : MgAx{jz, 1, {1, 0, 0, 0}, 1};
        bc[row * Lc.nx + jx] = mg_restrict_ax(Lf, ax, ay, az, r);
    }
}
template <int MASK, bool S32>
__global__ __launch_bounds__(kBlock) void k_mg_prolong_m(MgLv Lf, MgLv Lc, int lbx, double* __restrict__ x,
                                                        const double* __restrict__ e) {
    using I = typename std::conditional<S32, int32_t, int64_t>::type;
    const int ix = (int)(blockIdx.x << lbx) + (int)(threadIdx.x & ((1u << lbx) - 1));
    if (ix >= Lf.nx) return;
    const MgPx px = (MASK & 1) ? mg_pax_t<I>(Lf.nx, Lc.nx, ix) : MgPx{ix + 1, 0.0};
    const int64_t rows = (int64_t)Lf.ny * Lf.nz, rpb = kBlock >> lbx;
    for (int64_t row = blockIdx.y * rpb + (threadIdx.x >> lbx); row < rows; row += gridDim.y * rpb) {
        const int iy = (int)(row % Lf.ny), iz = (int)(row / Lf.ny);
        const MgPx py = (MASK & 2) ? mg_pax_t<I>(Lf.ny, Lc.ny, iy) : MgPx{iy + 1, 0.0};
        const MgPx pz = (MASK & 4) ? mg_pax_t<I>(Lf.nz, Lc.nz, iz) : MgPx{iz + 1, 0.0};
        const int64_t i = row * Lf.nx + ix;
        x[i] = x[i] + mg_prolong_ax<MASK>(Lc, px, py, pz, e);
    }
}
// The transfers of a periodic hierarchy, instantiated on the set MASK of coarsened axes (any non-empty set: an axis
// that is odd or too short is kept while the others are halved).  Row-shaped on mg_rows' grid like the _m kernels: a
// thread keeps its x index (its wrapped x indices are computed once), a wave reads and writes whole contiguous row
// segments, kept axes cost no index arithmetic.  The levels are nested, so the footprints are fixed (3 / 2 points per
// coarsened axis) and all indices are 32-bit (a level has fewer than 2^31 points); wraps are compare-and-select.  The
// row's (y, z) is divided out once per thread and then stepped: no integer division per point.
struct MgRowIt {
    int row, y, z, step, sy, sz;
};
__device__ __forceinline__ MgRowIt mg_row_first(int ny, int lbx) {
    const int rpb = kBlock >> lbx, row = (int)blockIdx.y * rpb + (int)(threadIdx.x >> lbx), step = (int)gridDim.y * rpb;
    return MgRowIt{row, row % ny, row / ny, step, step % ny, step / ny};
}
__device__ __forceinline__ void mg_row_next(MgRowIt& it, int ny) {
    it.row += it.step;
    it.y += it.sy;
    it.z += it.sz;
    if (it.y >= ny) {
        it.y -= ny;
        ++it.z;
    }
}
template <int MASK>
__global__ __launch_bounds__(kBlock) void k_mg_restrict_p(MgLv Lf, MgLv Lc, int lbx, double* __restrict__ bc,
                                                         const double* __restrict__ r) {
    constexpr bool CX = (MASK & 1) != 0, CY = (MASK & 2) != 0, CZ = (MASK & 4) != 0;
    const int jx = (int)(blockIdx.x << lbx) + (int)(threadIdx.x & ((1u << lbx) - 1));
    if (jx >= Lc.nx) return;
    const MgPerR ax = CX ? mg_per_rax(Lf.nx, jx) : mg_per_rkeep(jx);
    const int rows = Lc.ny * Lc.nz, plf = Lf.nx * Lf.ny;
    for (MgRowIt it = mg_row_first(Lc.ny, lbx); it.row < rows; mg_row_next(it, Lc.ny)) {
        const MgPerR ay = CY ? mg_per_rax(Lf.ny, it.y) : mg_per_rkeep(it.y);
        const MgPerR az = CZ ? mg_per_rax(Lf.nz, it.z) : mg_per_rkeep(it.z);
        bc[it.row * Lc.nx + jx] = mg_restrict_per(Lf.nx, plf, CX, CY, CZ, ax, ay, az, r);
    }
}
template <int MASK>
__global__ __launch_bounds__(kBlock) void k_mg_prolong_p(MgLv Lf, MgLv Lc, int lbx, double* __restrict__ x,
                                                        const double* __restrict__ e) {
    constexpr bool CX = (MASK & 1) != 0, CY = (MASK & 2) != 0, CZ = (MASK & 4) != 0;
    const int ix = (int)(blockIdx.x << lbx) + (int)(threadIdx.x & ((1u << lbx) - 1));
    if (ix >= Lf.nx) return;
    const MgPerP px = CX ? mg_per_pax(Lc.nx, ix) : mg_per_pkeep(ix);
    const int rows = Lf.ny * Lf.nz, plc = Lc.nx * Lc.ny;
    for (MgRowIt it = mg_row_first(Lf.ny, lbx); it.row < rows; mg_row_next(it, Lf.ny)) {
        const MgPerP py = CY ? mg_per_pax(Lc.ny, it.y) : mg_per_pkeep(it.y);
        const MgPerP pz = CZ ? mg_per_pax(Lc.nz, it.z) : mg_per_pkeep(it.z);
        const int i = it.row * Lf.nx + ix;
        x[i] = x[i] + mg_prolong_per(Lc.nx, plc, CX, CY, CZ, px, py, pz, e);
    }
}
// set-up: diag = dsum + s (dsum = Σ_a -2 c_a, summed in axis order on the host) and 1 / diag
// the ignition kinds' s_0 (nk_mg_set_jacobian): the argument m = α u_n + (1 - α) u of G_Midpoint!'s exp, mixed as the
// stencils mix it, and s = coef exp(.) - 1 in place on the exponentials
__global__ __launch_bounds__(kBlock) void k_mg_ign_mix(int n, double alpha, const double* __restrict__ un, const double* __restrict__ u,
                                                      double* __restrict__ m) {
    NK_CHUNKED(i, n) m[i] = alpha * un[i] + (1.0 - alpha) * u[i];
}
__global__ __launch_bounds__(kBlock) void k_mg_ign_s(int n, double coef, double* __restrict__ s) {
    NK_CHUNKED(i, n) s[i] = coef * s[i] - 1.0;
}

__global__ __launch_bounds__(kBlock) void k_mg_diag(int n, double dsum, const double* __restrict__ s, double* __restrict__ dg,
                                                   double* __restrict__ idg) {
    NK_CHUNKED(i, n) {
        const double d = dsum + s[i];
        dg[i] = d;
        idg[i] = 1.0 / d;
    }
}
// set-up: per-block minimum and maximum of the diagonal (NaN counts as a failure: part = {NaN-safe -inf, +inf})
__global__ __launch_bounds__(kBlock) void k_mg_minmax(int n, const double* __restrict__ dg, double* __restrict__ part) {
    __shared__ double smin[kBlock], smax[kBlock];
    double lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    NK_CHUNKED(i, n) {
        const double d = dg[i];
        bad = bad || !(d == d);
        lo = fmin(lo, d);
        hi = fmax(hi, d);
    }
    if (bad) { lo = -INFINITY; hi = INFINITY; }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = smin[0];
        part[2 * blockIdx.x + 1] = smax[0];
    }
}

// ------------------------------------------------------------------------------ the coarse tail
// Levels t .. L - 1 (the first with at most kMgTailPoints points) in one work-group: each level's five arrays
// (the ping-pong pair xa / xb, b, 1 / diag, diag) live in LDS, a barrier between sweeps.  The x of a level after
// k sweeps is in xa for odd k, xb for even k (the first sweep, from zero, writes xa).
struct MgTail {
    int nlev, nu, cs;
    double omega, om1;
    MgLv lv[kMgTailLevels];
    int off[kMgTailLevels];  // first double of the level's arrays in LDS
    const double* dg[kMgTailLevels];
    const double* idg[kMgTailLevels];
    const double* b;  // right-hand side of the tail's first level
    double* x;        // its result
};

template <bool PER>
__device__ __forceinline__ void mg_tail_sweeps(const MgLv& L, double omega, double om1, double* xa, double* xb, const double* b,
                                               const double* idg, int done, int sweeps) {
    for (int s = 0; s < sweeps; ++s, ++done) {
        if (done == 0) {
            for (int i = threadIdx.x; i < L.n; i += kMgTailThreads) xa[i] = mg_sweep0_pt(omega, b, idg, i);
        } else {
            const double* x = (done & 1) ? xa : xb;
            double* xn = (done & 1) ? xb : xa;
            for (int i = threadIdx.x; i < L.n; i += kMgTailThreads) xn[i] = mg_sweep_pt<0, PER>(L, omega, om1, x, b, idg, i);
        }
        __syncthreads();
    }
}

// OUT = 0: the cycle as it is.  OUT = 1: level 0 is the tail's first level and the closing loop writes sigma x.
// OUT = 2: that, and <b, z> from the LDS copy of b into the one partial part[0].  PER: a periodic hierarchy, from the
// same device functions on the LDS pointers.
template <int OUT, bool PER>
__global__ __launch_bounds__(kMgTailThreads) void k_mg_tail(MgTail T, double sigma, double* part, int fin) {
    extern __shared__ double mg_lds[];
#define MG_XA(l) (mg_lds + T.off[l])
#define MG_XB(l) (mg_lds + T.off[l] + T.lv[l].n)
#define MG_B(l) (mg_lds + T.off[l] + 2 * T.lv[l].n)
#define MG_IDG(l) (mg_lds + T.off[l] + 3 * T.lv[l].n)
#define MG_DG(l) (mg_lds + T.off[l] + 4 * T.lv[l].n)
    for (int l = 0; l < T.nlev; ++l)
        for (int i = threadIdx.x; i < T.lv[l].n; i += kMgTailThreads) {
            MG_IDG(l)[i] = T.idg[l][i];
            MG_DG(l)[i] = T.dg[l][i];
            if (l == 0) MG_B(0)[i] = T.b[i];
        }
    __syncthreads();
    // descent
    for (int l = 0; l < T.nlev; ++l) {
        const MgLv& L = T.lv[l];
        const bool last = l == T.nlev - 1;
        mg_tail_sweeps<PER>(L, T.omega, T.om1, MG_XA(l), MG_XB(l), MG_B(l), MG_IDG(l), 0, last ? T.cs : T.nu);
        if (last) break;
        const double* x = (T.nu & 1) ? MG_XA(l) : MG_XB(l);
        double* r = (T.nu & 1) ? MG_XB(l) : MG_XA(l);
        for (int i = threadIdx.x; i < L.n; i += kMgTailThreads) r[i] = mg_resid_pt<0, PER>(L, x, MG_B(l), MG_DG(l), i);
        __syncthreads();
        const MgLv& Lc = T.lv[l + 1];
        for (int j = threadIdx.x; j < Lc.n; j += kMgTailThreads) MG_B(l + 1)[j] = PER ? mg_restrict_per_pt(L, Lc, r, j) : mg_restrict_pt(L, Lc, r, j);
        __syncthreads();
    }
    // ascent
    for (int l = T.nlev - 2; l >= 0; --l) {
        const MgLv& L = T.lv[l];
        const MgLv& Lc = T.lv[l + 1];
        const int kc = (l + 1 == T.nlev - 1) ? T.cs : 2 * T.nu;  // sweeps level l + 1 has seen
        const double* e = (kc & 1) ? MG_XA(l + 1) : MG_XB(l + 1);
        double* x = (T.nu & 1) ? MG_XA(l) : MG_XB(l);
        for (int i = threadIdx.x; i < L.n; i += kMgTailThreads) x[i] = x[i] + (PER ? mg_prolong_per_pt(L, Lc, e, i) : mg_prolong_pt(L, Lc, e, i));
        __syncthreads();
        mg_tail_sweeps<PER>(L, T.omega, T.om1, MG_XA(l), MG_XB(l), MG_B(l), MG_IDG(l), T.nu, T.nu);
    }
    const int k0 = T.nlev == 1 ? T.cs : 2 * T.nu;
    const double* x0 = (k0 & 1) ? MG_XA(0) : MG_XB(0);
    if (OUT == 0) {
        for (int i = threadIdx.x; i < T.lv[0].n; i += kMgTailThreads) T.x[i] = x0[i];
    } else {
        __shared__ double sh[kShN];
        double acc = 0.0;
        for (int i = threadIdx.x; i < T.lv[0].n; i += kMgTailThreads) {
            const double zi = sigma * x0[i];
            T.x[i] = zi;
            if (OUT == 2) acc = fma(MG_B(0)[i], zi, acc);
        }
        if (OUT == 2) publish<kMgTailThreads>(acc, part, fin, sh);
    }
#undef MG_XA
#undef MG_XB
#undef MG_B
#undef MG_IDG
#undef MG_DG
}

}  // namespace
}  // namespace nk

using namespace nk;

struct nk_mg {
    nk_ctx* c = nullptr;
    nk_problem prob{};       // the geometry it was created for
    int dim = 1;
    int nlev_alloc = 0;      // levels of the plan
    int nlev = 0;            // levels in use (set-up may truncate)
    int nlev_spd = 0;        // ... in SPD form: it also ends before the first level whose diagonal has the other sign
    bool spd = false;        // SPD form (nk_mg_set_spd): z = sigma V(v), sigma = the sign of the level-0 diagonal
    double sigma = 1.0;
    int tail = 0;            // first level of the one-launch coarse tail (== nlev_alloc: none)
    int nu = 2, cs = 8;
    double omega = 0.0;
    bool ready = false;      // an operator has been set
    bool user_op = false;    // ... by nk_mg_set_operator: the caller's, not refreshed from a Jacobian by the Newton loop
    MgLv lv[kMgMaxLevels];
    double len[3] = {0, 0, 0};  // L_a = (n_a^0 + 1) h_a^0
    double h0[3] = {0, 0, 0};
    // per level (device): ping-pong pair, right-hand side (level 0: the caller's v), s, diag, 1 / diag
    double *xa[kMgMaxLevels] = {}, *xb[kMgMaxLevels] = {}, *b[kMgMaxLevels] = {}, *s[kMgMaxLevels] = {},
           *dg[kMgMaxLevels] = {}, *idg[kMgMaxLevels] = {};
    double* part = nullptr;  // set-up: kMgMinmaxBlocks (min, max) pairs per level
    // a distributed hierarchy (slabs of the slowest axis): lv holds the local extents
    int slab_ax = 0;              // 0: one rank; 1 / 2: the slab axis (y of a 2D grid, z of a 3D grid)
    int ng[kMgMaxLevels] = {};    // global extent of the level along the slab axis (nranks x the local one)
    int64_t ghost[kMgMaxLevels] = {};  // doubles of the ghost plane before and after xa, xb, b, s (0: one rank)
    // a periodic hierarchy (NK_BC_PERIODIC, one rank): nested levels of mg_plan_per, the PER kernels
    bool per = false;
};

namespace {

// compile-time dispatch: f(std::integral_constant<T, V>{}) for the V of the list that v equals, so that a generic
// lambda names the kernel instantiation of a runtime AX, RED, MASK, S32 or OUT in one launch expression
template <typename T, T... Vs, typename F>
void mg_pick(T v, F&& f) {
    (void)((v == Vs && (f(std::integral_constant<T, Vs>{}), true)) || ...);
}

int mg_launch_sweep0(nk_mg* m, int l, double* x, const double* b) {
    const MgLv& L = m->lv[l];
    return launch(m->c, "mg_sweep0", 24.0 * L.n, [&] {
        hipLaunchKernelGGL(k_mg_sweep0, dim3(wide_blocks(L.n)), dim3(kBlock), 0, m->c->stream, L.n, m->omega, x, b, m->idg[l]);
    });
}
// slabs: the ghost planes of level l's array x from the neighbour ranks (the context's separate-launch exchange)
int mg_exchange(nk_mg* m, int l, const double* x) {
    nk_problem lp = m->prob;
    lp.nx = m->lv[l].nx;
    lp.ny = m->lv[l].ny;
    lp.nz = m->lv[l].nz;
    return halo_exchange(m->c, &lp, x);
}
MgSl mg_slab(const nk_mg* m, int l) {
    const int mf = m->slab_ax == 1 ? m->lv[l].ny : m->lv[l].nz, mc = m->slab_ax == 1 ? m->lv[l + 1].ny : m->lv[l + 1].nz;
    return MgSl{m->ng[l], m->ng[l + 1], m->c->rank * mf, m->c->rank * mc};
}
int mg_launch_sweep(nk_mg* m, int l, double* xn, const double* x, const double* b) {
    const MgLv& L = m->lv[l];
    if (m->slab_ax) NK_TRY(mg_exchange(m, l, x));
    return launch(m->c, "mg_sweep", 32.0 * L.n, [&] {
        if (m->per)
            hipLaunchKernelGGL((k_mg_sweep<0, true>), dim3(wide_blocks(L.n)), dim3(kBlock), 0, m->c->stream, L, m->omega,
                               1.0 - m->omega, xn, x, b, m->idg[l]);
        else
            mg_pick<int, 0, 1, 2>(m->slab_ax, [&](auto AX) {
                hipLaunchKernelGGL((k_mg_sweep<AX.value, false>), dim3(wide_blocks(L.n)), dim3(kBlock), 0, m->c->stream, L, m->omega,
                                   1.0 - m->omega, xn, x, b, m->idg[l]);
            });
    });
}
// the residual of level l's x into r (slabs: x's ghost planes first)
int mg_launch_resid(nk_mg* m, int l, double* r, const double* x, const double* b) {
    const MgLv& L = m->lv[l];
    if (m->slab_ax) NK_TRY(mg_exchange(m, l, x));
    return launch(m->c, "mg_resid", 32.0 * L.n, [&] {
        if (m->per)
            hipLaunchKernelGGL((k_mg_resid<0, true>), dim3(wide_blocks(L.n)), dim3(kBlock), 0, m->c->stream, L, r, x, b, m->dg[l]);
        else
            mg_pick<int, 0, 1, 2>(m->slab_ax, [&](auto AX) {
                hipLaunchKernelGGL((k_mg_resid<AX.value, false>), dim3(wide_blocks(L.n)), dim3(kBlock), 0, m->c->stream, L, r, x, b,
                                   m->dg[l]);
            });
    });
}
// how the cycle's last launch writes z: times sigma, with the partials of <v, z> into *red when given
struct MgOut {
    double sigma;
    Red* red;
    bool plain() const { return sigma == 1.0 && !red; }
};
// the level-0 sweep that writes z (x == nullptr: the pointwise first sweep).  The fused reduction streams on a
// red_blocks grid like the other reductions every block of a consumer sums (k_axpy_sumsq), 16 B/pt less than
// mg_sweep + dot together (neither b nor z is read a second time)
int mg_launch_sweep_z(nk_mg* m, double* z, const double* x, const double* b, const MgOut& o) {
    const MgLv& L = m->lv[0];
    nk_ctx* c = m->c;
    const int g = o.red ? red_blocks(L.n) : wide_blocks(L.n);
    int fin = 0;
    double* part = o.red ? red_out(c, g, o.red, &fin) : nullptr;
    const char* name = x ? (o.red ? "mg_sweep_dot" : "mg_sweep") : (o.red ? "mg_sweep0_dot" : "mg_sweep0");
    if (x && m->slab_ax) NK_TRY(mg_exchange(m, 0, x));
    return launch(c, name, (x ? 32.0 : 24.0) * L.n, [&] {
        mg_pick<bool, false, true>(o.red != nullptr, [&](auto RED) {
            if (!x)
                hipLaunchKernelGGL(k_mg_sweep0_z<RED.value>, dim3(g), dim3(kBlock), 0, c->stream, L.n, m->omega, o.sigma, z, b,
                                   m->idg[0], part, fin);
            else if (m->per)
                hipLaunchKernelGGL((k_mg_sweep_z<0, true, RED.value>), dim3(g), dim3(kBlock), 0, c->stream, L, m->omega,
                                   1.0 - m->omega, o.sigma, z, x, b, m->idg[0], part, fin);
            else
                mg_pick<int, 0, 1, 2>(m->slab_ax, [&](auto AX) {
                    hipLaunchKernelGGL((k_mg_sweep_z<AX.value, false, RED.value>), dim3(g), dim3(kBlock), 0, c->stream, L, m->omega,
                                       1.0 - m->omega, o.sigma, z, x, b, m->idg[0], part, fin);
                });
        });
    });
}
// `sweeps` sweeps on level l after `done` earlier ones; the x so far is *cur (unused when done == 0), the sweeps
// ping-pong between xa / xb and the last one writes `final` when given (level 0: the cycle's z, written as `out`
// says).  *cur = where x is afterwards.
int mg_sweeps(nk_mg* m, int l, const double* b, int done, int sweeps, double** cur, double* final, const MgOut& out) {
    for (int s = 0; s < sweeps; ++s, ++done) {
        const bool last = final && s == sweeps - 1;
        double* dst = last ? final : (*cur == m->xa[l] ? m->xb[l] : m->xa[l]);
        if (last && !out.plain()) NK_TRY(mg_launch_sweep_z(m, dst, done == 0 ? nullptr : *cur, b, out));
        else if (done == 0) NK_TRY(mg_launch_sweep0(m, l, dst, b));
        else NK_TRY(mg_launch_sweep(m, l, dst, *cur, b));
        *cur = dst;
    }
    return NK_OK;
}

// Which transfer kernels the level pair l, l + 1 runs: nk_mg_plan.hpp's rule on the one-rank extents (slabs: the
// slab forms of the general kernels).  The names of the profiler classes carry the mask: mg_restrict_x, mg_prolong_yz, ...
MgXfer mg_xfer(const nk_mg* m, int l) {
    // the kernel-variant bench build can force the general kernels under the mask's class name, to time both on the
    // same level pair
    static const bool generic = NK_TUNE("NK_MG_GENERIC", 0) != 0;
    const MgLv &Lf = m->lv[l], &Lc = m->lv[l + 1];
    const int nf[3] = {Lf.nx, Lf.ny, Lf.nz}, nc[3] = {Lc.nx, Lc.ny, Lc.nz};
    MgXfer t = m->slab_ax ? MgXfer{0, false, true} : nk::mg_xfer(nf, nc);
    t.general = t.general || generic;
    return t;
}
const char* const kMgRestrictName[7] = {"mg_restrict",    "mg_restrict_x",  "mg_restrict_y", "mg_restrict_xy",
                                        "mg_restrict_z",  "mg_restrict_xz", "mg_restrict_yz"};
const char* const kMgSetupName[7] = {"mg_setup_restrict",    "mg_setup_restrict_x",  "mg_setup_restrict_y", "mg_setup_restrict_xy",
                                     "mg_setup_restrict_z",  "mg_setup_restrict_xz", "mg_setup_restrict_yz"};
const char* const kMgProlongName[7] = {"mg_prolong",   "mg_prolong_x",  "mg_prolong_y", "mg_prolong_xy",
                                       "mg_prolong_z", "mg_prolong_xz", "mg_prolong_yz"};

// The transfers: the general kernel in its AX form (slabs: the source's ghost planes first), or the instantiation on
// the mask of a semicoarsened level pair.  setup: the restriction of s during set-up (a profiler class of its own)
// a periodic level pair: the set of coarsened axes (never empty: every level of mg_plan_per halves an axis)
int mg_per_mask(const MgLv& Lf, const MgLv& Lc) { return (Lf.nx != Lc.nx ? 1 : 0) | (Lf.ny != Lc.ny ? 2 : 0) | (Lf.nz != Lc.nz ? 4 : 0); }

int mg_restrict(nk_mg* m, int l, double* bc, const double* r, bool setup) {
    const MgLv &Lf = m->lv[l], &Lc = m->lv[l + 1];
    if (m->per) {
        const MgRows g = mg_rows(Lc.nx, (int64_t)Lc.ny * Lc.nz);
        return launch(m->c, setup ? "mg_setup_restrict_per" : "mg_restrict_per", 8.0 * Lf.n + 8.0 * Lc.n, [&] {
            mg_pick<int, 1, 2, 3, 4, 5, 6, 7>(mg_per_mask(Lf, Lc), [&](auto MASK) {
                hipLaunchKernelGGL(k_mg_restrict_p<MASK.value>, dim3(g.gx, g.gy), dim3(kBlock), 0, m->c->stream, Lf, Lc, g.lbx, bc, r);
            });
        });
    }
    if (m->slab_ax) NK_TRY(mg_exchange(m, l, r));
    const MgXfer t = mg_xfer(m, l);
    const MgSl S = mg_slab(m, l);
    const MgRows g = mg_rows(Lc.nx, (int64_t)Lc.ny * Lc.nz);
    return launch(m->c, (setup ? kMgSetupName : kMgRestrictName)[t.mask], 8.0 * Lf.n + 8.0 * Lc.n, [&] {
        if (t.general)
            mg_pick<int, 0, 1, 2>(m->slab_ax, [&](auto AX) {
                hipLaunchKernelGGL(k_mg_restrict<AX.value>, dim3(wide_blocks(Lc.n)), dim3(kBlock), 0, m->c->stream, Lf, Lc, S, bc, r);
            });
        else
            mg_pick<int, 1, 2, 3, 4, 5, 6>(t.mask, [&](auto MASK) {
                mg_pick<bool, false, true>(t.s32, [&](auto S32) {
                    hipLaunchKernelGGL((k_mg_restrict_m<MASK.value, S32.value>), dim3(g.gx, g.gy), dim3(kBlock), 0, m->c->stream, Lf,
                                       Lc, g.lbx, bc, r);
                });
            });
    });
}
int mg_prolong(nk_mg* m, int l, double* x, const double* e) {
    const MgLv &Lf = m->lv[l], &Lc = m->lv[l + 1];
    if (m->per) {
        const MgRows g = mg_rows(Lf.nx, (int64_t)Lf.ny * Lf.nz);
        return launch(m->c, "mg_prolong_per", 16.0 * Lf.n + 8.0 * Lc.n, [&] {
            mg_pick<int, 1, 2, 3, 4, 5, 6, 7>(mg_per_mask(Lf, Lc), [&](auto MASK) {
                hipLaunchKernelGGL(k_mg_prolong_p<MASK.value>, dim3(g.gx, g.gy), dim3(kBlock), 0, m->c->stream, Lf, Lc, g.lbx, x, e);
            });
        });
    }
    if (m->slab_ax) NK_TRY(mg_exchange(m, l + 1, e));
    const MgXfer t = mg_xfer(m, l);
    const MgSl S = mg_slab(m, l);
    const MgRows g = mg_rows(Lf.nx, (int64_t)Lf.ny * Lf.nz);
    return launch(m->c, kMgProlongName[t.mask], 16.0 * Lf.n + 8.0 * Lc.n, [&] {
        if (t.general)
            mg_pick<int, 0, 1, 2>(m->slab_ax, [&](auto AX) {
                hipLaunchKernelGGL(k_mg_prolong<AX.value>, dim3(wide_blocks(Lf.n)), dim3(kBlock), 0, m->c->stream, Lf, Lc, S, x, e);
            });
        else
            mg_pick<int, 1, 2, 3, 4, 5, 6>(t.mask, [&](auto MASK) {
                mg_pick<bool, false, true>(t.s32, [&](auto S32) {
                    hipLaunchKernelGGL((k_mg_prolong_m<MASK.value, S32.value>), dim3(g.gx, g.gy), dim3(kBlock), 0, m->c->stream, Lf,
                                       Lc, g.lbx, x, e);
                });
            });
    });
}

int mg_free(nk_mg* m) {
    for (int l = 0; l < kMgMaxLevels; ++l) {
        for (double* q : {m->xa[l], m->xb[l], m->b[l], m->s[l]})
            if (q) (void)hipFree(q - m->ghost[l]);
        for (double* q : {m->dg[l], m->idg[l]})
            if (q) (void)hipFree(q);
    }
    if (m->part) (void)hipFree(m->part);
    delete m;
    return NK_OK;
}

// slabs: pos[l] / neg[l] of this rank's rows -> of the whole level, through the context's cross-rank sum.  Every rank
// adds 1 (positive) + 64 (negative) per level (at most kMbRanks = 32 < 64 ranks: no carry), four levels of 12 bits to
// a scalar (exact in a double); a level is positive / negative when the count is nranks.  One host sync per scalar.
int mg_agree(nk_mg* m, bool* pos, bool* neg) {
    nk_ctx* c = m->c;
    for (int l0 = 0; l0 < m->nlev_alloc; l0 += 4) {
        double code = 0.0, f = 1.0;
        for (int l = l0; l < l0 + 4 && l < m->nlev_alloc; ++l, f *= 4096.0) code += f * ((pos[l] ? 1.0 : 0.0) + (neg[l] ? 64.0 : 0.0));
        Red r{};
        int fin = 0;
        double* part = red_out(c, 1, &r, &fin);
        r.fin = nullptr;  // nothing was folded: the one partial is the value
        c->hpin[1] = code;
        NK_HIP(c, hipMemcpyAsync(part, c->hpin + 1, sizeof(double), hipMemcpyHostToDevice, c->stream));
        double sum = 0.0;
        NK_TRY(host_scalar(c, r, 0, &sum));
        int64_t S = (int64_t)sum;
        for (int l = l0; l < l0 + 4 && l < m->nlev_alloc; ++l, S /= 4096) {
            pos[l] = (S % 64) == c->nranks;
            neg[l] = ((S / 64) % 64) == c->nranks;
        }
    }
    return NK_OK;
}

// diag and 1 / diag of every level from k and s_0 (already in m->s[0]); level 0's from nk_jacobian_diag when
// `jac` (bit-identical to J's own diagonal); then the sign check that may truncate the hierarchy
int mg_setup(nk_mg* m, const double k[3], const nk_problem* jac, const double* u) {
    nk_ctx* c = m->c;
    for (int l = 0; l < m->nlev_alloc; ++l) {
        MgLv& L = m->lv[l];
        int ext[3] = {L.nx, L.ny, L.nz};
        if (m->slab_ax) ext[m->slab_ax] = m->ng[l];  // the spacing of the global grid
        double cc[3] = {0.0, 0.0, 0.0}, dsum = 0.0;
        for (int a = 0; a < m->dim; ++a) {
            // periodic: the period n_a^0 h_a^0 stays, so h_a^l = h_a^0 (n_a^0 / n_a^l), an exact power of two
            const int n0a = a == 0 ? m->lv[0].nx : (a == 1 ? m->lv[0].ny : m->lv[0].nz);
            const double h = l == 0 ? m->h0[a] : (m->per ? m->h0[a] * (double)(n0a / ext[a]) : m->len[a] / (double)(ext[a] + 1));
            cc[a] = k[a] / (h * h);
            dsum = a == 0 ? -2.0 * cc[a] : dsum + -2.0 * cc[a];
        }
        L.cx = cc[0]; L.cy = cc[1]; L.cz = cc[2];
        if (l > 0) NK_TRY(mg_restrict(m, l - 1, m->s[l], m->s[l - 1], true));
        if (l == 0 && jac) {
            NK_TRY(launch_jdiag(c, jac, m->dg[0], u, 0));
            NK_TRY(launch_jdiag(c, jac, m->idg[0], u, 1));
        } else {
            NK_TRY(launch(c, "mg_setup_diag", 24.0 * L.n, [&] {
                hipLaunchKernelGGL(k_mg_diag, dim3(wide_blocks(L.n)), dim3(kBlock), 0, c->stream, L.n, dsum, m->s[l], m->dg[l],
                                   m->idg[l]);
            }));
        }
        const int g = std::min(kMgMinmaxBlocks, wide_blocks(L.n));
        NK_TRY(launch(c, "mg_setup_minmax", 8.0 * L.n, [&] {
            hipLaunchKernelGGL(k_mg_minmax, dim3(g), dim3(kBlock), 0, c->stream, L.n, m->dg[l], m->part + 2 * kMgMinmaxBlocks * l);
        }));
    }
    std::vector<double> part((size_t)2 * kMgMinmaxBlocks * m->nlev_alloc);
    NK_HIP(c, hipMemcpyAsync(part.data(), m->part, part.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    NK_HIP(c, hipStreamSynchronize(c->stream));
    // per level: the whole diagonal is positive / negative (and finite)
    bool pos[kMgMaxLevels], neg[kMgMaxLevels];
    for (int l = 0; l < m->nlev_alloc; ++l) {
        const int g = std::min(kMgMinmaxBlocks, wide_blocks(m->lv[l].n));
        double lo = INFINITY, hi = -INFINITY;
        for (int b = 0; b < g; ++b) {
            lo = std::fmin(lo, part[(size_t)2 * (kMgMinmaxBlocks * l + b)]);
            hi = std::fmax(hi, part[(size_t)2 * (kMgMinmaxBlocks * l + b) + 1]);
        }
        const bool finite = !(std::isinf(lo) || std::isinf(hi));
        pos[l] = finite && lo > 0.0;
        neg[l] = finite && hi < 0.0;
    }
    // slabs: of the whole level, not of this rank's rows -- every rank must keep the same levels (and sigma), or the
    // ranks that keep more wait in their exchanges for one that never arrives
    if (m->slab_ax) NK_TRY(mg_agree(m, pos, neg));
    int ok = 0, ok_spd = 0;
    bool neg0 = false;
    for (; ok < m->nlev_alloc; ++ok) {
        if (!(pos[ok] || neg[ok])) break;
        // the SPD form's hierarchy: the leading levels whose diagonal has level 0's sign (a mixed one is not definite)
        if (ok == 0) neg0 = neg[0];
        if (ok_spd == ok && neg[ok] == neg0) ok_spd = ok + 1;
    }
    m->ready = false;
    if (ok == 0) return fail(c, NK_E_ARG, "multigrid: the diagonal of the operator changes sign, vanishes or is not finite");
    m->nlev = ok;
    m->nlev_spd = ok_spd;
    m->sigma = neg0 ? -1.0 : 1.0;
    m->ready = true;
    return NK_OK;
}

// the plan ABI's shared argument check and copy-out (the first `cap` levels; *nlevels is the plan's count)
bool mg_plan_args(const int64_t* n, int32_t max_levels, const int64_t* extents, int32_t cap, const int32_t* nlevels) {
    return n && nlevels && n[0] >= 1 && n[1] >= 1 && n[2] >= 1 && max_levels >= 0 && cap >= 0 && (cap == 0 || extents);
}
int mg_plan_out(const int64_t (*ext)[3], int L, int64_t* extents, int32_t cap, int32_t* nlevels) {
    for (int l = 0; l < L && l < cap; ++l)
        for (int a = 0; a < 3; ++a) extents[3 * l + a] = ext[l][a];
    *nlevels = L;
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_mg_plan(const int64_t n[3], int32_t max_levels, int64_t* extents, int32_t cap, int32_t* nlevels) {
    if (!mg_plan_args(n, max_levels, extents, cap, nlevels)) return NK_E_ARG;
    int64_t ext[kMgMaxLevels][3];
    return mg_plan_out(ext, mg_plan(n, max_levels, ext), extents, cap, nlevels);
}

int nk_mg_plan_periodic(const int64_t n[3], int32_t max_levels, int64_t* extents, int32_t cap, int32_t* nlevels) {
    if (!mg_plan_args(n, max_levels, extents, cap, nlevels) || mg_plan_per_why(n, 0)) return NK_E_ARG;
    int64_t ext[kMgMaxLevels][3];
    return mg_plan_out(ext, mg_plan_per(n, max_levels, ext), extents, cap, nlevels);
}

int nk_mg_plan_slabs(const int64_t n_local[3], int32_t nranks, int32_t max_levels, int64_t* extents, int32_t cap,
                     int32_t* nlevels) {
    if (!mg_plan_args(n_local, max_levels, extents, cap, nlevels)) return NK_E_ARG;
    int64_t ext[kMgMaxLevels][3];
    int ax = 0;
    const char* why = nullptr;
    const int L = mg_plan_slabs(n_local, nranks, max_levels, ext, &ax, &why);
    return L == 0 ? NK_E_ARG : mg_plan_out(ext, L, extents, cap, nlevels);
}

int nk_mg_plan_semi(const int64_t n[3], const double h[3], const double k[3], double threshold, int32_t max_levels,
                    int64_t* extents, int32_t cap, int32_t* nlevels) {
    if (!h || !mg_plan_args(n, max_levels, extents, cap, nlevels)) return NK_E_ARG;
    if (!(threshold == 0.0 || (threshold > 0.0 && threshold <= 1.0))) return NK_E_ARG;
    double kk[3] = {1.0, 1.0, 1.0};
    for (int a = 0; a < 3; ++a) {
        if (n[a] == 1) continue;  // an unused axis: neither h nor k is read
        if (k) kk[a] = k[a];
        if (!std::isfinite(kk[a]) || kk[a] == 0.0 || !std::isfinite(h[a]) || !(h[a] > 0.0)) return NK_E_ARG;
    }
    const double hh[3] = {n[0] == 1 ? 1.0 : h[0], n[1] == 1 ? 1.0 : h[1], n[2] == 1 ? 1.0 : h[2]};
    int64_t ext[kMgMaxLevels][3];
    return mg_plan_out(ext, mg_plan_semi(n, hh, kk, threshold == 0.0 ? 0.5 : threshold, max_levels, ext), extents, cap, nlevels);
}

}  // extern "C"

namespace {

// the hierarchy on the level extents `given` (nlevels of them; validated here), or on mg_plan's when null
int mg_create(nk_ctx* c, const nk_problem* p, const nk_mg_opts* opts, const int64_t* given, int32_t nlevels, nk_mg** out) {
    if (!c || !p || !out) return NK_E_ARG;
    if (!stencil_kind(p->kind))
        return fail(c, NK_E_ARG, "multigrid: built-in stencil kinds only (a user residual's coefficients are unknown; "
                                 "give them with nk_mg_set_operator on a built-in kind's grid)");
    // periodic boundaries: the heat kinds on one rank, on mg_plan_per's nested levels
    const bool per = p->bc == NK_BC_PERIODIC;
    if (p->bc != NK_BC_ZERO && !per) return fail(c, NK_E_ARG, "multigrid: bc_zero! or bc_periodic! (unknown bc)");
    if (per && !kind_of(p->kind).periodic)
        return fail(c, NK_E_ARG, "multigrid: periodic boundaries are implemented for the heat kinds only (this kind is bc_zero! only)");
    if (per && c->nranks != 1)
        return fail(c, NK_E_ARG, "multigrid: periodic boundaries are not implemented on a distributed context");
    if (per && given)
        return fail(c, NK_E_ARG, "multigrid: periodic boundaries are not implemented with a level list (semicoarsening)");
    // a distributed context: equal slabs of the slowest axis.  Every refusal depends on values all
    // ranks hold alike (kind, bc, process grid, local extents -- equal by precondition -- and options), and comes
    // before the first exchange is enqueued
    const bool dist = c->nranks != 1;
    if (dist && (c->px * c->py > 1 || block_self(c)))
        return fail(c, NK_E_ARG, "multigrid: slabs only on a distributed context (3D blocks are not implemented)");
    const Kind K = kind_of(p->kind);
    if (dist && K.dim == 1) return fail(c, NK_E_ARG, "multigrid: 1D kinds are not implemented on a distributed context");
    if (dist && !K.ranks)
        return fail(c, NK_E_ARG, K.ignition ? "multigrid: the ignition kinds run on one rank (a distributed context is not implemented for them)"
                                            : "multigrid: NK_BRATU3D runs on one rank (a distributed context is not implemented for it)");
    if (dist && given)
        return fail(c, NK_E_ARG, "multigrid: a level list (semicoarsening) is not implemented on a distributed context");
    Geo g;
    NK_TRY(geometry(c, p, &g));
    if (g.n >= ((int64_t)1 << 31)) return fail(c, NK_E_ARG, "multigrid: at most 2^31 - 1 points");
    const int nu = opts && opts->nu ? opts->nu : 2, cs = opts && opts->coarse_sweeps ? opts->coarse_sweeps : 8;
    const double omega = opts && opts->omega != 0.0 ? opts->omega : 2.0 * g.dim / (2.0 * g.dim + 1.0);
    if (nu < 1 || cs < 1 || !(omega > 0.0) || (opts && opts->max_levels < 0))
        return fail(c, NK_E_ARG, "multigrid: nu >= 1, coarse_sweeps >= 1, omega > 0, max_levels >= 0");
    const int64_t n0[3] = {p->nx, p->ny, p->nz};
    const double h[3] = {p->hx, p->hy, p->hz};
    int64_t ext[kMgMaxLevels][3];
    int nlev = 0, slab_ax = 0;
    if (given) {
        char buf[128];
        if (const char* why = mg_levels_why(n0, given, nlevels, buf)) return fail(c, NK_E_ARG, std::string("multigrid: ") + why);
        std::copy(given, given + 3 * nlevels, &ext[0][0]);
        nlev = nlevels;
    } else if (dist) {
        const char* why = nullptr;
        nlev = mg_plan_slabs(n0, c->nranks, opts ? opts->max_levels : 0, ext, &slab_ax, &why);
        if (nlev == 0) return fail(c, NK_E_ARG, std::string("multigrid on a distributed context: ") + why);
    } else if (per) {
        if (const char* why = mg_plan_per_why(n0, g.dim)) return fail(c, NK_E_ARG, std::string("multigrid on a periodic grid: ") + why);
        nlev = mg_plan_per(n0, opts ? opts->max_levels : 0, ext);
    } else {
        nlev = mg_plan(n0, opts ? opts->max_levels : 0, ext);
    }
    nk_mg* m = new nk_mg();
    m->per = per;
    m->c = c;
    m->prob = *p;
    m->dim = g.dim;
    m->nu = nu;
    m->cs = cs;
    m->omega = omega;
    m->nlev_alloc = nlev;
    m->slab_ax = slab_ax;
    for (int a = 0; a < 3; ++a) {
        m->h0[a] = h[a];
        // slabs: the length of the global grid along the slab axis, as the one-rank hierarchy of that grid has it
        m->len[a] = (double)((a == slab_ax && dist ? c->nranks * n0[a] : n0[a]) + 1) * h[a];
    }
    // (a distributed hierarchy has no tail: every level runs the per-level kernels, with exchanges between them)
    const MgTailPlan tail = dist ? MgTailPlan{nlev, 0} : mg_tail_plan(ext, nlev);
    m->tail = tail.first;
    for (int l = 0; l < m->nlev_alloc; ++l) {
        MgLv& L = m->lv[l];
        L.nx = (int)ext[l][0]; L.ny = (int)ext[l][1]; L.nz = (int)ext[l][2];
        L.n = L.nx * L.ny * L.nz;
        L.cx = L.cy = L.cz = 0.0;
        const size_t bytes = sizeof(double) * (size_t)L.n;
        bool ok = true;
        // slabs: xa, xb, s, b carry one ghost plane before and after the interior, zero from here on where no
        // neighbour writes it (the physical side of the first and last rank: the Dirichlet boundary)
        const int64_t gh = mg_ghost(ext[l], slab_ax);
        if (dist) m->ng[l] = (int)(c->nranks * ext[l][slab_ax]);
        m->ghost[l] = gh;
        auto with_ghosts = [&](double** q) {
            double* base = nullptr;
            const size_t all = bytes + 2 * sizeof(double) * (size_t)gh;
            if (hipMalloc(&base, all) != hipSuccess) return false;
            if (gh && hipMemsetAsync(base, 0, all, c->stream) != hipSuccess) {
                (void)hipFree(base);
                return false;
            }
            *q = base + gh;
            return true;
        };
        for (double** q : {&m->xa[l], &m->xb[l], &m->s[l]}) ok = ok && with_ghosts(q);
        for (double** q : {&m->dg[l], &m->idg[l]}) ok = ok && hipMalloc(q, bytes) == hipSuccess;
        if (l > 0) ok = ok && with_ghosts(&m->b[l]);
        if (!ok) {
            (void)hipGetLastError();
            mg_free(m);
            return fail(c, NK_E_NOMEM, "multigrid: out of device memory for the hierarchy");
        }
    }
    if (hipMalloc(&m->part, sizeof(double) * 2 * kMgMinmaxBlocks * (size_t)m->nlev_alloc) != hipSuccess) {
        mg_free(m);
        return fail(c, NK_E_NOMEM, "multigrid: out of device memory");
    }
    if (m->tail < m->nlev_alloc) {
        // the same limit for every hierarchy (a per-hierarchy value could lower it under an earlier, larger tail)
        hipError_t e = tail.lds <= kMgTailLds ? hipSuccess : hipErrorInvalidValue;
        for (const void* f : {reinterpret_cast<const void*>(k_mg_tail<0, false>), reinterpret_cast<const void*>(k_mg_tail<1, false>),
                              reinterpret_cast<const void*>(k_mg_tail<2, false>), reinterpret_cast<const void*>(k_mg_tail<0, true>),
                              reinterpret_cast<const void*>(k_mg_tail<1, true>), reinterpret_cast<const void*>(k_mg_tail<2, true>)})
            if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMgTailLds);
        if (e != hipSuccess) {
            mg_free(m);
            return fail(c, NK_E_HIP, std::string("multigrid: LDS for the coarse tail: ") + hipGetErrorString(e));
        }
    }
    m->nlev = m->nlev_spd = m->nlev_alloc;
    *out = m;
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_mg_create(nk_ctx* c, const nk_problem* p, const nk_mg_opts* opts, nk_mg** out) {
    return mg_create(c, p, opts, nullptr, 0, out);
}

int nk_mg_create_levels(nk_ctx* c, const nk_problem* p, const nk_mg_opts* opts, const int64_t* extents, int32_t nlevels,
                        nk_mg** out) {
    if (!extents) return NK_E_ARG;
    return mg_create(c, p, opts, extents, nlevels, out);
}

int nk_mg_level_extents(nk_mg* m, int64_t* extents, int32_t cap, int32_t* nlevels) {
    if (!m || !nlevels || cap < 0 || (cap > 0 && !extents)) return NK_E_ARG;
    const int L = m->spd ? m->nlev_spd : m->nlev;
    for (int l = 0; l < L && l < cap; ++l) {
        extents[3 * l] = m->lv[l].nx;
        extents[3 * l + 1] = m->lv[l].ny;
        extents[3 * l + 2] = m->lv[l].nz;
    }
    *nlevels = L;
    return NK_OK;
}

int nk_mg_destroy(nk_mg* m) {
    if (!m) return NK_OK;
    (void)hipStreamSynchronize(m->c->stream);
    return mg_free(m);
}

int nk_mg_levels(nk_mg* m, int32_t* nlevels) {
    if (!m || !nlevels) return NK_E_ARG;
    *nlevels = m->spd ? m->nlev_spd : m->nlev;
    return NK_OK;
}

int nk_mg_set_spd(nk_mg* m, int32_t on) {
    if (!m) return NK_E_ARG;
    m->spd = on != 0;
    return NK_OK;
}

int nk_mg_get_spd(nk_mg* m, int32_t* on) {
    if (!m || !on) return NK_E_ARG;
    *on = m->spd ? 1 : 0;
    return NK_OK;
}

int nk_mg_set_operator(nk_mg* m, const double k[3], const double* s_dev, double s_const) {
    if (!m || !k) return NK_E_ARG;
    nk_ctx* c = m->c;
    if (s_dev) NK_TRY(launch_copy(c, m->lv[0].n, m->s[0], s_dev));
    else NK_TRY(launch_fill(c, m->lv[0].n, m->s[0], s_const));
    m->user_op = true;
    return mg_setup(m, k, nullptr, nullptr);
}

int nk_mg_set_jacobian(nk_mg* m, const nk_problem* p, const double* u) {
    if (!m || !p || !u) return NK_E_ARG;
    nk_ctx* c = m->c;
    if (p->kind != m->prob.kind || p->nx != m->prob.nx || p->ny != m->prob.ny || p->nz != m->prob.nz || p->hx != m->prob.hx ||
        (m->dim >= 2 && p->hy != m->prob.hy) || (m->dim == 3 && p->hz != m->prob.hz) || p->bc != m->prob.bc)
        return fail(c, NK_E_ARG, "multigrid: the problem does not match the hierarchy's (kind, grid, spacings, bc)");
    double k[3] = {0.0, 0.0, 0.0};
    const int64_t n = m->lv[0].n;
    if (kind_of(p->kind).ignition) {
        // J = θ Δt (a L + λ diag(exp(m))) - I: k_a = θ a Δt as for the heat kinds, s = θ Δt λ exp(m) - 1 with m = u
        // (G_Midpoint!: α u_n + (1 - α) u).  s turns positive where θ Δt λ exp(m) > 1 (near blow-up): the diagonal then
        // changes sign on some level and mg_setup truncates the hierarchy there, as for Bratu above the fold
        const int sch = kind_of(p->kind).scheme;
        const double theta = sch == 1 ? 1.0 - p->alpha : (sch == 2 ? 0.5 : 1.0);
        if (!p->un) return fail(c, NK_E_ARG, "ignition problem needs u_n");
        for (int a = 0; a < m->dim; ++a) k[a] = theta * p->a * p->dt;
        const double* arg = u;
        if (sch == 1) {  // (a level-0 work vector holds m: no cycle runs during the setup)
            NK_TRY(launch(c, "mg_setup_mix", 24.0 * n, [&] {
                hipLaunchKernelGGL(k_mg_ign_mix, dim3(wide_blocks(n)), dim3(kBlock), 0, c->stream, (int)n, p->alpha, p->un, u, m->xa[0]);
            }));
            arg = m->xa[0];
        }
        NK_TRY(launch_exp(c, n, m->s[0], arg));  // the stencils' own correctly rounded exp
        const double coef = (sch == 2 ? p->dt / 2.0 : p->dt) * (sch == 1 ? 1.0 - p->alpha : 1.0) * p->lambda;
        NK_TRY(launch(c, "mg_setup_s", 16.0 * n, [&] {
            hipLaunchKernelGGL(k_mg_ign_s, dim3(wide_blocks(n)), dim3(kBlock), 0, c->stream, (int)n, coef, m->s[0]);
        }));
    } else if (kind_of(p->kind).heat) {
        const int sch = kind_of(p->kind).scheme;
        const double theta = sch == 1 ? 1.0 - p->alpha : (sch == 2 ? 0.5 : 1.0);
        for (int a = 0; a < m->dim; ++a) k[a] = theta * p->a * p->dt;
        NK_TRY(launch_fill(c, n, m->s[0], -1.0));
    } else {  // NK_BRATU1D / 2D / 3D: the Laplacian plus s = λ exp(u)
        for (int a = 0; a < m->dim; ++a) k[a] = 1.0;
        NK_TRY(launch_exp(c, n, m->s[0], u));  // the stencils' own correctly rounded exp
        NK_TRY(launch_scal(c, n, p->lambda, m->s[0]));
    }
    m->user_op = false;
    return mg_setup(m, k, p, u);
}

}  // extern "C"

// the Newton loop's refresh before each solve: J(u)'s coefficients, unless the caller set the operator itself
int nk::mg_refresh(nk_mg* m, const nk_problem* p, const double* u) {
    if (!m) return NK_E_ARG;
    if (m->user_op) return m->ready ? NK_OK : fail(m->c, NK_E_STATE, "multigrid: no operator set");
    return nk_mg_set_jacobian(m, p, u);
}

// one V-cycle in the form that is set; red (optional): the partials of <v, z> from the launch that writes z
int nk::mg_apply_red(nk_mg* m, double* z, const double* v, Red* red) {
    if (!m || !z || !v) return NK_E_ARG;
    nk_ctx* c = m->c;
    if (!m->ready) return fail(c, NK_E_STATE, "multigrid: no operator set (nk_mg_set_jacobian / nk_mg_set_operator)");
    const int L = m->spd ? m->nlev_spd : m->nlev;
    const MgOut out{m->spd ? m->sigma : 1.0, red};
    const int G = std::min(m->tail, L);  // levels 0 .. G - 1 run per-level kernels, G .. L - 1 the tail launch
    double* cur[kMgMaxLevels] = {};
    // descent
    for (int l = 0; l < G; ++l) {
        const double* b = l == 0 ? v : m->b[l];
        if (l == L - 1) {  // the coarsest level, too large for the tail
            NK_TRY(mg_sweeps(m, l, b, 0, m->cs, &cur[l], l == 0 ? z : nullptr, out));
            break;
        }
        NK_TRY(mg_sweeps(m, l, b, 0, m->nu, &cur[l], nullptr, out));
        double* r = cur[l] == m->xa[l] ? m->xb[l] : m->xa[l];
        NK_TRY(mg_launch_resid(m, l, r, cur[l], b));
        NK_TRY(mg_restrict(m, l, m->b[l + 1], r, false));
    }
    if (G < L) {
        MgTail T{};
        T.nlev = L - G;
        T.nu = m->nu;
        T.cs = m->cs;
        T.omega = m->omega;
        T.om1 = 1.0 - m->omega;
        double pts = 0.0;
        size_t lds = 0;
        for (int l = G; l < L; ++l) {
            T.lv[l - G] = m->lv[l];
            T.off[l - G] = (int)(lds / sizeof(double));
            T.dg[l - G] = m->dg[l];
            T.idg[l - G] = m->idg[l];
            pts += m->lv[l].n;
            lds += 5 * sizeof(double) * (size_t)m->lv[l].n;
        }
        T.b = G == 0 ? v : m->b[G];
        T.x = G == 0 ? z : m->xa[G];
        cur[G] = T.x;
        // the tail writes z itself when level 0 is in it: times sigma, and <v, z> as its one partial
        const int mode = (G == 0 && !out.plain()) ? (red ? 2 : 1) : 0;
        int fin = 0;
        double* part = mode == 2 ? red_out(c, 1, red, &fin) : nullptr;
        NK_TRY(launch(c, mode == 2 ? "mg_tail_dot" : "mg_tail", 16.0 * pts + 16.0 * m->lv[G].n, [&] {
            mg_pick<int, 0, 1, 2>(mode, [&](auto OUT) {
                mg_pick<bool, false, true>(m->per, [&](auto PER) {
                    hipLaunchKernelGGL((k_mg_tail<OUT.value, PER.value>), dim3(1), dim3(kMgTailThreads), lds, c->stream, T,
                                       mode ? out.sigma : 1.0, part, fin);
                });
            });
        }));
    }
    // ascent
    for (int l = std::min(G, L - 1) - 1; l >= 0; --l) {
        NK_TRY(mg_prolong(m, l, cur[l], cur[l + 1]));
        NK_TRY(mg_sweeps(m, l, l == 0 ? v : m->b[l], m->nu, m->nu, &cur[l], l == 0 ? z : nullptr, out));
    }
    return NK_OK;
}

bool nk::mg_is_spd(const nk_mg* m) { return m && m->spd; }

extern "C" {

int nk_mg_apply(nk_mg* m, double* z, const double* v) { return mg_apply_red(m, z, v, nullptr); }

int nk_mg_apply_dot(nk_mg* m, double* z, const double* v, double* vz) {
    if (!m || !z || !v || !vz) return NK_E_ARG;
    nk_ctx* c = m->c;
    Red r{};
    NK_TRY(mg_apply_red(m, z, v, &r));
    return host_scalar(c, r, 0, vz);
}

}  // extern "C"
