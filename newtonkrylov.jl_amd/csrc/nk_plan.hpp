// nk_plan.hpp -- launch geometry as pure host code: the grid sizes of the streaming kernels, the
// resident MGS sweep's residency rule (res_plan) and the stencils' tile rule (st_plan).  Numbers in, a
// plan out: nothing here touches a device, so the rules are callable -- and tested -- on the CPU
// (tests/test_plan.py, against the oracle's and the tests' restatements).  The launchers
// (launch_mgs_sweep in nk_resident.hip, launch_stencil_ex in nk_kernels.hip) fill the knobs from NK_TUNE
// and dispatch on the plan.  No HIP header: this file compiles with a plain host compiler.
#pragma once

#include <algorithm>
#include <cstdint>

namespace nk {

constexpr int kBlock = 256;          // threads per block for every streaming kernel (4 waves of 64)
constexpr int kMaxRedBlocks = 2048;  // partial sums per reduction (8 blocks per CU on 256 CUs)
constexpr int kRedCap = 16384;       // doubles per slot (a stencil launch may have more blocks)
constexpr int kTileCap = 1 << 19;    // one-shot stencil tiles per launch (per-tile partials before the group fold)
constexpr int kTileParts = 1024;     // partials a one-shot stencil launch hands on (tiles folded in groups)
constexpr int kResMax = 64;          // resident sweep: passes per launch (reorthogonalisation: 2k)
constexpr int kResThreads = 256;     // resident sweep: threads per block = double2 elements per slot
// tail-group size of a fully resident sweep (LDS slots; 0 = off): -DNK_RES_TAIL_DEFAULT=g for a `make variant`
// A/B of the product build; the kbench build reads NK_RES_TAIL instead.
#ifndef NK_RES_TAIL_DEFAULT
#define NK_RES_TAIL_DEFAULT 24
#endif
constexpr int kResTail = NK_RES_TAIL_DEFAULT;
#ifndef NK_F0R_DEFAULT  // (product variant builds for A/B: 0 never, 2 every FD launch, 3 no 3D F0R)
#define NK_F0R_DEFAULT 1
#endif

// MODE_TRIAL: the residual at the trial point w = fma(s, v, u) of a line search (nk_residual_trial): the field is
// loaded and cooked as MODE_JFD's, the value is MODE_RES's
enum Mode { MODE_RES = 0, MODE_JEXACT = 1, MODE_JFD = 2, MODE_TRIAL = 3 };

// ---------------------------------------------------------------- streaming grids
// grid size of streaming reductions: >= 4 double2 per thread, at most `cap` (kMaxRedBlocks) blocks
inline int red_blocks(int64_t n, int cap) {
    int64_t g = (n + 2LL * kBlock * 4 - 1) / (2LL * kBlock * 4);
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// Grid of the streaming kernels whose partials (if any) only a one-block finaliser reads: up to
// `cap` (kRedCap - 2) blocks, >= 2 double2 per thread.  Many short-lived blocks stream faster than a
// grid of 8 per CU looping over block chunks (tools/stream_probe.py: a plain copy 5.0 -> 6.2 TB/s;
// k_update_x -9 % on heat 8192^2, profiles/r02/ab_redblocks.log).  Reductions consumed by every
// block of the next kernel (dot, sumsq, the MGS chain) keep red_blocks: each consumer block sums
// all the partials.
inline int wide_blocks(int64_t n, int cap) {
    int64_t g = (n + 2LL * kBlock * 2 - 1) / (2LL * kBlock * 2);
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// ---------------------------------------------------------------- resident MGS sweep
// the kernel-variant build's tuning knobs (NK_RES_*); default-constructed: the product
struct ResKnobs {
    int rl = -1, rv = -1;  // LDS / register slots instead of the rule's (< 0: the rule)
    int nts = 1, pre = 1;  // load policy of the rv = 89 variants: streamed remainder non-temporal, prefetched batches of 4
    int vout = 1;          // V_{k+1} straight from the registers at full residency
    int strided = 0, mirror = 0;
    int tail = kResTail;
    int ntc = -1, mall_mb = 244;  // streamed slots whose V_{i+1} loads cached (< 0: what the Infinity Cache has room for)
    int jv = 0;                   // the fused Jv phase
};

struct ResPlan {
    bool applies;    // false: the caller falls back to the per-pass chain (nothing else is set)
    int rv, rl;      // register and LDS slots per thread
    int tg;          // tail group: the last tg LDS slots
    bool full;       // all of q is resident; else part of it streams through memory
    bool keep_vout;  // the sweep can store V_{k+1} = q / ||q|| instead of q
    int ntc, strided, mirror;
    int xv;          // kernel-variant bench: the variant a caller's rv = 1000 + xv names, else -1
    double bytes, dram;  // the profile's algorithmic and unique-DRAM byte models
};

// n doubles in np passes on G blocks with at most rl_max LDS slots; rv_req >= 0: the caller's register
// slots (1000 + v: kernel variant v with 89); want_vout: the caller offers a V_{k+1}; jv_nx: the row
// length of a fused Jv's grid, 0 without one
inline ResPlan res_plan(int64_t n, int np, int G, int rl_max, int rv_req, bool want_vout, int64_t jv_nx, const ResKnobs& K) {
    ResPlan P{};
    P.xv = -1;
    if (np < 1 || np > kResMax || (n & 1)) return P;
    // fused Jv phase (kbench build only): at one wave per SIMD its ~190 fp64 VALU instructions per
    // point pair (IEEE divisions, two exp) do not hide behind the loads: 791 us per Arnoldi step vs
    // 619 + 124 us for the sweep and a separate Jv kernel (-1.7 % end to end, 4096^2)
    const bool jv = jv_nx != 0;
    if (jv && (!K.jv || !want_vout || jv_nx % 2 != 0)) return P;
    // every block's chunk must hold its rv + rl resident slots in full (the kernel does not predicate them)
    const int64_t n2 = n >> 1;
    const int64_t ns = (n2 + kResThreads - 1) / kResThreads;
    const int64_t whole = ns / G - (n2 % kResThreads != 0 ? 1 : 0);  // the last block's last slot may be partial
    if (whole < 1) return P;
    const int slots = (int)std::min<int64_t>(whole, 1 << 20);
    int rl = std::min(slots, K.rl >= 0 ? std::min(K.rl, rl_max) : rl_max);  // LDS first
    const bool explicit_rv = rv_req >= 0 || K.rv >= 0;  // a caller's choice skips the benefit test below
    int rv = rv_req;
    if (rv >= 1000) {  // kernel-variant bench: 1000 + {0: 89 slots, batches of 4 + prefetch across the hand-off; 1: same, no prefetch; 2: alternating slot order; 3: V_i cached; 4: V_{i+1} non-temporal; 5: streamed remainder non-temporal (NTS); 6: 0 + 5; 8: batches of 2 + prefetch (batches of 6 + prefetch spill); 9 / 10: 0 with LDS slots in batches of 8 / 6; 11: 0 with alternate passes starting on the top LDS group (prefetched across the hand-off)}
        P.xv = rv - 1000;
        rv = 89;
    }
    if (rv < 0) rv = K.rv >= 0 ? K.rv : slots - rl;  // registers hold what the LDS cannot
    // the instantiated register-slot counts (25 + 39 LDS slots = 64: a 4096 x 2048 slab, 4096^2 on two GPUs)
    constexpr int kRv[] = {89, 64, 48, 32, 25, 16, 0};
    int pick = 0;
    for (int r : kRv)
        if (r <= rv && r <= slots) {
            pick = r;
            break;
        }
    if (P.xv < 0) rv = pick;
    else if (rv > slots) return P;
    rl = std::min(rl, slots - rv);
    if (P.xv == 11 && rl < 4) P.xv = 0;  // ALT + prefetch starts on the top LDS group of 4
    // worth it from two passes on (a one-pass sweep only adds q's load + store) while a tenth of q
    // or more is resident (tools/kbench_res.py per pass vs the chain: 4096^2 1.28x at k = 2,
    // 1.8x from k = 16; 2 x 4096^2 (half resident) 1.40-1.52x; 8192^2 (a quarter) 1.16-1.18x;
    // 512^3 (an eighth) 1.06-1.09x -- with the streamed remainder non-temporal; 1.01x at 512^3
    // without it, hence a fifth then)
    const int64_t chunk = std::max<int64_t>(1, ns / G);
    const double frac = (double)(rv + rl) / (double)chunk;  // resident fraction of q
    if (!explicit_rv && (np < 2 || frac < (K.nts ? 0.1 : 0.2))) return P;
    // V_{k+1} straight from the registers only when all of q is resident (no streamed slot; a
    // partial last slot is streamed)
    const bool full = n2 % kResThreads == 0 && (ns + G - 1) / G <= rv + rl;
    const bool keep_vout = full && K.vout;
    if (jv && (!keep_vout || (rv != 0 && rv != 89) || (rv > 0 && rl < 16))) return P;  // fused Jv: full residency, instantiated rv, LDS staging
    P.applies = true;
    P.rv = rv;
    P.rl = rl;
    P.full = full;
    P.keep_vout = keep_vout;
    // slots interleaved across the blocks (kbench): a different partition of the partial sums
    const bool exact = n2 % kResThreads == 0 && ns % G == 0 && ns / G == rv + rl;  // every block exactly full
    P.strided = K.strided && exact;
    P.mirror = K.mirror && !P.strided && exact;
    // tail group: only where all of q is resident -- the streamed remainder follows the
    // LDS slots in the chain of partial sums and loads between the tail's two phases -- and never
    // with the alternating slot orders (kbench variants 2 and 11), which end a pass elsewhere
    P.tg = full && P.xv != 2 && P.xv != 11 ? std::max(0, std::min(K.tail, rl)) : 0;
    // NTS: the Infinity Cache (256 MB) keeps the resident part's V_{i+1} (4 KB per block and slot) for
    // its re-read as the next pass's V_i; the room left (244 MB of it) goes to the first streamed slots
    // of every block, whose V_{i+1} then loads cached: half resident 129.3 -> 120.2 us per pass, a
    // quarter 313.1 -> 300.1 (profiles/r02/ab_ntc.log; 128 slots, past the room, thrash)
    const double slot = 4096.0 * G;  // one slot of V across the grid, bytes
    const double room = 1e6 * K.mall_mb - slot * (rv + rl);
    P.ntc = K.ntc >= 0 ? K.ntc : (room > 0 ? (int)(room / slot) : 0);
    // algorithmic bytes: the resident fraction f of q is loaded once (or computed by the fused Jv
    // from u, V_k, F0, V_1), stored once (q or V_{k+1}) and each pass reads V_i (+ V_{i+1}); the
    // streamed rest reads and writes q in every pass as well (k_mgs_pass's 32 / 24 B/pt)
    const double f = std::min(1.0, (double)G * (rv + rl) * kResThreads / (double)(n >> 1));
    const double per_res = (jv ? 5.0 : 2.0) + 2.0 * np - 1.0, per_str = 4.0 * np - 1.0;  // doubles per point
    P.bytes = 8.0 * (double)n * (f * per_res + (1.0 - f) * per_str);
    // unique-DRAM model: V_{i+1}, read again as the next pass's V_i, counted once (the Infinity Cache
    // serves the second read at best): np + 2 doubles per resident point (q in, V_1..V_np, q / V_{k+1}
    // out), 3 np for a streamed point (q read and written every pass, each V once)
    P.dram = 8.0 * (double)n * (f * ((jv ? 5.0 : 2.0) + np) + (1.0 - f) * (3.0 * np));
    return P;
}

// ---------------------------------------------------------------- stencil tiles
// the kernel-variant build's tuning knobs (NK_ST_*, NK_ST3_*, NK_F0R, NK_TILE_PARTS); default-constructed: the product
struct StKnobs {
    int vec_pref = 2;
    int blocks = 1024, min_rows = 8, max_rows = 32;  // 2D: tiles aimed at, rows per tile
    int oneshot = 0;
    int lds3 = 1, nw3 = 4;
    int blocks3 = 8192, min_planes = 16;  // 3D: tiles aimed at, planes per z-chunk
    int zalt = 0, ymarch = 0, ym_rows = 64;
    int f0r = NK_F0R_DEFAULT;
    int tile_parts = kTileParts;
};

// what a stencil launch is asked for
struct StShape {
    int dim;  // 1, 2, 3
    int64_t nx, ny, nz;
    bool per, blk;      // periodic; 3D blocks (x / y ghost faces)
    int mode;           // Mode
    bool heat;          // a heat kind (else Bratu)
    int scheme;         // 0 G_Euler!, 1 G_Midpoint!, 2 G_Trapezoid!
    bool vstore, vdot;  // V_k is stored by a dot launch; that dot has a partner other than V_k itself
    int rows_override, fast;  // the kernel-variant bench's rows / planes per tile and variant bits (0, 0: the product)
    bool f0r;           // the caller's F0 is exactly this library's F(u)
};

struct StPlan {
    int vec, tiles_x, tiles_y, rows, grid;
    int lin, tile2;            // 2D, kbench: tiles in address order; rows of a one-shot tile (0: the row march)
    int lds3, nw, zalt, ym;    // 3D: k_st3l, rows per tile, tile order, y-march
    int f0r;                   // FD: F0 recomputed from u
    int group, nparts;         // tiles per partial handed on (one-shot tiles: > 1), partials of the launch
};

inline StPlan st_plan(const StShape& S, const StKnobs& K) {
    StPlan P{};
    const int fast = S.fast;
    P.vec = 1;
    P.grid = 1;
    if (S.dim == 1) {
        P.grid = (int)((S.nx + kBlock - 1) / kBlock);
    } else if (S.dim == 2) {
        P.vec = (S.nx % 2 == 0) ? 2 : 1;
        if (((fast & 4) || K.vec_pref == 4) && S.nx % 4 == 0 && !S.per) P.vec = 4;
        P.tiles_x = (int)((S.nx + kBlock * P.vec - 1) / (kBlock * P.vec));
        // rows per tile: about 1024 tiles, between 8 and 32 rows (4096^2: 32-row tiles, FD Jv 121.3 ->
        // 114.8 us and +0.6 % on the bench, profiles/r02/ab_st_blocks.log; 8192^2 heat: 32 rows are
        // as fast as 64 for the FD Jv and 3 % faster for the residual, kbench_st2d_8192.log), and
        // never more tiles than the reduction slot holds partials
        int64_t rows = (S.ny * P.tiles_x + K.blocks - 1) / K.blocks;
        if (rows > K.max_rows) rows = K.max_rows;
        if (rows < K.min_rows) rows = K.min_rows;
        const int64_t cap_rows = (S.ny * P.tiles_x + (kRedCap - 3)) / (kRedCap - 2);
        if (rows < cap_rows) rows = cap_rows;
        if (S.rows_override > 0) rows = S.rows_override;
        if (rows > S.ny) rows = S.ny;
        P.rows = (int)rows;
        P.tiles_y = (int)((S.ny + rows - 1) / rows);
        P.grid = P.tiles_x * P.tiles_y;
        P.lin = (fast & 2048) ? 1 : 0;  // kbench: tiles in address order
        // kbench only: one-shot LDS tiles (k_st2t: 8 rows x 128 columns, no march, tiles in address
        // order, block partials folded by k_tile_fold) for the FD operator (NK_ST_ONESHOT=1), or for any
        // mode with fast bits 8192 / 16384 / 32768 (8 / 4 / 16 rows); 262144 forces the march.  8-12 %
        // faster than the march in isolation (profiles/r03/ab_tile8.log, ab_oneshot_fold2.log), but not in
        // the bench (ab_oneshot4.log): the product keeps the march.
        P.tile2 = (fast & 8192) ? 8 : ((fast & 16384) ? 4 : ((fast & 32768) ? 16 : 0));
        if (!P.tile2 && K.oneshot && S.mode == MODE_JFD && P.vec == 2 && !(fast & (262144 | 4 | 2048)) &&
            S.rows_override <= 0 && !(K.oneshot == 2 && S.scheme == 2))
            P.tile2 = 8;
        // fast bit 131072 with a one-shot tile: 256 columns wide (VEC 4), 8 or 4 rows
        if (P.tile2 && (fast & 131072) && S.nx % 4 == 0 && !S.per && !(P.tile2 == 16)) {
            P.vec = 4;
            P.tiles_x = (int)((S.nx + 255) / 256);
            P.tiles_y = (int)((S.ny + P.tile2 - 1) / P.tile2);
            P.grid = P.tiles_x * P.tiles_y;
        } else if (P.tile2 && P.vec == 2) {
            const int tx1 = (int)((S.nx + 127) / 128), ty1 = (int)((S.ny + P.tile2 - 1) / P.tile2);
            if ((int64_t)tx1 * ty1 <= kTileCap) {
                P.tiles_x = tx1;
                P.tiles_y = ty1;
                P.grid = P.tiles_x * P.tiles_y;
            } else {
                P.tile2 = 0;  // beyond the per-tile partial buffer: the row march
            }
        } else {
            P.tile2 = 0;
        }
    } else {
        P.vec = (S.nx % 2 == 0) ? 2 : 1;
        // rows per 3D tile and the y-neighbour path (k_st3d loads, k_st3l LDS); fast bits 8 / 16 select
        // k_st3l with 4 / 8 rows (kernel-variant bench), NK_ST3_LDS / NK_ST3_NW likewise
        // k_st3l with 4-row tiles is the default: +6-16 % over k_st3d on every 3D kind / mode at 512^3
        // and at config 5's 512^2 x 64 slab (profiles/r02/kbench_st3l.log)
        P.lds3 = (fast & 24) ? 1 : K.lds3;
        P.nw = P.lds3 ? ((fast & 8) ? 4 : ((fast & 16) ? 8 : (K.nw3 == 4 ? 4 : 8))) : 4;
        if (S.blk) {  // 3D blocks: k_st3l with 4-row tiles (the kernel-variant build's other forms have no faces)
            P.lds3 = 1;
            P.nw = 4;
        }
        P.tiles_x = (int)((S.nx + 64 * P.vec - 1) / (64 * P.vec));
        P.tiles_y = (int)((S.ny + P.nw - 1) / P.nw);
        // about 8192 tiles: shorter z-marches keep y-adjacent tiles in step (L2 reuse of the halo rows)
        int64_t planes = ((int64_t)S.nz * P.tiles_x * P.tiles_y + K.blocks3 - 1) / K.blocks3;
        // at least 16 planes: (16 + 2) / 16 z-halo re-reads (blocks: one chunk size on every rank -- the
        // in-launch exchange numbers x / y patches by chunk)
        if (planes < K.min_planes || S.blk) planes = K.min_planes;
        if (S.rows_override > 0) planes = S.rows_override;
        if (planes > S.nz) planes = S.nz;
        P.rows = (int)planes;
        P.grid = P.tiles_x * P.tiles_y * (int)((S.nz + planes - 1) / planes);
        // k_st3l tile order / march direction (tile3_of; kbench only: 1 whole tile columns per XCD band with
        // odd z-chunks marching down, 2 plane-major + odd chunks down, 3 chunk pairs): within +-3 % of the
        // plane-major order, upward marches (0, the product) -- profiles/r03/ab_zalt*.log
        P.zalt = (P.lds3 && !(fast & 65536) && !S.blk) ? K.zalt : 0;  // kbench fast bit 65536: the plane-major order
        // the y-march (k_st3y, kbench NK_ST3_YMARCH=1: slabs short along z; NK_ST3Y_ROWS rows per chunk):
        // tiles of nw planes x 64 vec columns marching a chunk of rows
        P.ym = (P.lds3 && (K.ymarch || (fast & 524288)) && S.rows_override <= 0 && !P.zalt && !S.blk) ? 1 : 0;  // (bit 2^19: the y-march)
        if (P.ym) {
            const int64_t r = std::min<int64_t>(std::max(1, K.ym_rows), S.ny);
            P.rows = (int)r;
            P.tiles_y = (int)((S.ny + r - 1) / r);
            P.grid = P.tiles_x * P.tiles_y * (int)((S.nz + P.nw - 1) / P.nw);
        }
    }
    // FD with F0 recomputed from u (2D, VEC <= 2: k_st2d<..., F0R>; 3D heat: k_st3l<..., F0R>, not
    // with NK_F0R=3 (A/B)); never with the `fast` reciprocals,
    // which would change F(u) against the residual kernel that stored F0.  NK_F0R: 1 (default) for the
    // heat kinds, whose F(u) costs a few flops (8192^2 FD Jv 728 -> 612 us, bench +3.3 %), and for
    // Bratu's Jv launches that also store V_k (fused normalisation): they move enough bytes to hide the
    // second exp per point (config-4 slab Jv 277 -> 246 us, V_1 step 248 -> 227 us, bench +1.2 %),
    // while the plain Jv + dot (116 -> 122 us) and the restart residual (110 -> 126 us) do not
    // (profiles/r02/ab_f0r_bratu.log); 2 for every Bratu launch too; 0 never
    // 3D: the F0R kernel needs 145 VGPRs (3 waves per SIMD instead of 4), which pays only where the
    // field is cheap and the kernel moves the most bytes: G_Euler!'s Jv with a dot partner (512^3
    // FD Jv + V_k store 1400 -> 1198 us), not the V_1 = r0 / beta step, not midpoint / trapezoid
    // (profiles/r02/ab_f0r3.log)
    const bool dotvs = S.vstore && !S.vdot;
    const bool f0r = K.f0r && S.f0r && S.mode == MODE_JFD && P.vec <= 2 && !(fast & 1) &&
                     ((S.dim == 2 && (K.f0r >= 2 || S.heat || S.vstore)) ||
                      (S.dim == 3 && P.lds3 && K.f0r != 3 && (K.f0r >= 2 || (S.heat && S.scheme == 0 && !dotvs))));
    P.f0r = f0r ? 1 : 0;
    // partials handed on: one per tile, one-shot tiles in groups of about kTileParts
    P.group = 1;
    P.nparts = P.grid;
    if (P.tile2 && P.grid > K.tile_parts) {
        P.group = (P.grid + K.tile_parts - 1) / K.tile_parts;
        P.nparts = (P.grid + P.group - 1) / P.group;
    }
    return P;
}

}  // namespace nk
