// nk_resident.hip -- the resident MGS sweep: one Arnoldi step's whole modified-Gram-Schmidt
// orthogonalisation (np passes + ||q||, optionally V_{k+1} = q / ||q|| and the FD Jv before it) as
// ONE launch of one block per CU, with q held in registers and LDS ("Resident MGS
// sweep"), and its kernel-variant bench hook (nkb_mgs_res, tools/kbench_res.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "nk_device.hpp"

namespace nk {
namespace {
// ------------------------------------------------------------------------------ resident MGS sweep
// One Arnoldi step's whole MGS sweep (np passes + h_{k+1,k} = ||q||) in ONE launch, with q held
// on chip: one block per CU owns a contiguous chunk of q; its first RV x 256 double2 live in
// registers, the next rl x 256 in LDS, only the rest streams through memory.  A pass then reads
// V_i and V_{i+1} (16 B/pt; V_{i+1} is re-read as the next pass's V_i from the Infinity Cache)
// instead of q, V_i, V_{i+1} and the q write-back (32 B/pt).  Per-element arithmetic is exactly
// k_mgs_pass's (q = fma(-h, V_i, q); acc = fma(V_{i+1}, q, acc)); only the partition of the
// partial sums differs, and it is fixed, so results stay run-to-run bit reproducible.
// Between passes every block needs h = Σ_b partial_b: each block publishes its partial as two
// self-validating {tag:32 | half:32} granules (cdna_hip_programming.md §6 G16, R2 -- the data is
// the flag, no fence) into a parity-double-buffered slot, then polls all G partials and sums them
// in block order -- the same tree in every block, so every block holds the bit-identical h.
// Double buffering is enough: a block can write pass t+2's granule only after reading everyone's
// pass t+1 granule, i.e. after everyone finished reading pass t's.  Every spin is bounded.
// Requires all G blocks co-resident: G = #CUs, 1 block per CU (the LDS share forces it).
// (kResMax passes per launch, kResThreads, the tail group's size kResTail and the residency rule: nk_plan.hpp)
#ifdef NK_KBENCH
int g_res_tail_hook = -1;     // nkb_mgs_res_tail: the tail size of its launches (overrides NK_RES_TAIL), -1 = none
int g_res_tail_launched = 0;  // A.tg of the last launch
#endif
struct ResArgs {
    const double* V[kResMax + 1];  // pass t: V_i = V[t], V_{i+1} = V[t + 1]
    double* q;
    double* vout;  // non-null (full residency only): store V_{k+1} = q / ||q|| here instead of q
    double* col;   // h of every pass, ||q|| at [np]
    double* colh;  // pinned host mirror
    const double* red_in;  // partials of h of the first pass (the Jv's <V_1, q>)
    uint64_t* gran;        // 2 parities x G blocks x 2 granules
    int* err;              // pinned host flag: a poll timed out
    int noxchg;            // kbench build only (NK_RES_NOXCHG=1, timing probe): skip the exchange -- WRONG results
    int ntc;               // NTS: the first ntc streamed slots of a block load V_{i+1} cached (Infinity Cache room)
    int nwc;               // kernel-variant build: resident slots s >= nwc load V_{i+1} non-temporally (ldw_s)
    int poll1;             // 1: one polling wave (NK_RES_POLL1, default 1), 2: four staggered polling waves, 0: every thread polls one partial
    int strided;           // slots interleaved across blocks (every block exactly full: no streamed remainder)
    int mirror;            // kbench: odd blocks map slot s to the chunk's slot S-1-s (every block exactly full)
    uint64_t* tstamp;      // kernel-variant bench only: per pass and block, wall clock at pass end and after the hand-off
    int senders;           // cross-rank: blocks [0, senders) each send this rank's sum to every rank (identical bits)
    // fused FD Jv (2D Bratu): q = (F(u + eps V_k) - F0) / eps computed into the registers, with the
    // partials of <V_1, q> -- instead of loading the q a separate Jv kernel wrote
    const double *ju, *jv, *jf0, *jaux;
    double jeps, jlam, jhx2, jhy2;
    int64_t jnx;
    int jv_on;
    int64_t n2;            // double2 elements
    int np, red_len, rl;
    int tg;                // tail group: the last tg of the rl LDS slots are updated first and dotted last in every pass
    unsigned tag0, mb0, spin;
};

template <int RV>
struct ResState {
    dx2 r[RV];
};

// `budget`: this thread's remaining polls for the whole launch (a stuck grid drains in bounded time)
// t: the exchange's index in this launch (tags, parity and mailbox epochs follow it)
__device__ __forceinline__ double res_exchange(const ResArgs& A, double part, int t, double* sh, unsigned& budget,
                                              unsigned* xdone) {
    const int tid = threadIdx.x, G = gridDim.x;
    const unsigned tag = A.tag0 + (unsigned)t;
    uint64_t* slot = A.gran + (size_t)(t & 1) * G * 2;
    if (tid == 0) {
        const uint64_t bits = (uint64_t)__double_as_longlong(part);
        __hip_atomic_store(slot + 2 * blockIdx.x, ((uint64_t)tag << 32) | (bits & 0xffffffffull), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(slot + 2 * blockIdx.x + 1, ((uint64_t)tag << 32) | (bits >> 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (A.poll1) {  // ONE wave polls: lane l sums the partials of blocks l, 64 + l, 128 + l, 192 + l.
        // poll1 >= 2: every wave polls the same way, wave w starting w quarter round trips later, so a
        // late granule is seen a quarter of a poll round after it lands instead of half a round on
        // average; the first wave to see all of them publishes the (bit-identical) sum, the others
        // stop at its flag
        const int w = tid >> 6, nw = A.poll1 >= 2 ? kResThreads / 64 : 1;
        if (w < nw) {
            for (int i = 0; i < w; ++i) __builtin_amdgcn_s_sleep(8);
            const int l = tid & 63;
            uint64_t w8[8];
            bool mine = false;  // this wave saw every granule
            for (;;) {
                if (nw > 1 && __hip_atomic_load(xdone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == tag) break;
                bool ok = true;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int bl = 64 * j + l;
                    if (bl < G) {
                        w8[2 * j] = __hip_atomic_load(slot + 2 * bl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        w8[2 * j + 1] = __hip_atomic_load(slot + 2 * bl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = ok && (unsigned)(w8[2 * j] >> 32) == tag && (unsigned)(w8[2 * j + 1] >> 32) == tag;
                    } else {
                        w8[2 * j] = w8[2 * j + 1] = 0;
                    }
                }
                if (__all(ok)) {
                    mine = true;
                    break;
                }
                if (budget == 0 || --budget == 0) {
                    __hip_atomic_store(A.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    mine = true;  // a timed-out grid still drains: publish whatever arrived
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (mine) {
                double p = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    p += __longlong_as_double((long long)(((w8[2 * j + 1] & 0xffffffffull) << 32) | (w8[2 * j] & 0xffffffffull)));
                p = wave_sum(p);
                if (l == 0) {
                    sh[kShB] = p;
                    if (nw > 1) __hip_atomic_store(xdone, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        const double s1 = sh[kShB];
        if (A.mb0 == 0) return s1;
        const unsigned epoch = A.mb0 + (unsigned)t;
        if ((int)blockIdx.x < A.senders) mb_send(s1, epoch);
        __syncthreads();
        return mb_recv(epoch, sh);
    }
    double v = 0.0;
    if (tid < G) {
        const uint64_t* g = slot + 2 * tid;
        uint64_t lo = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t hi = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((unsigned)(lo >> 32) != tag || (unsigned)(hi >> 32) != tag) {
            if (budget == 0 || --budget == 0) {
                __hip_atomic_store(A.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                lo = hi = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
            lo = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            hi = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        v = __longlong_as_double((long long)(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull)));
    }
    __syncthreads();  // thread 0 is done with sh[] of the partial's block_sum
    double s = block_sum<kResThreads>(v, sh);
    if (tid == 0) sh[kShB] = s;
    __syncthreads();
    s = sh[kShB];
    if (A.mb0 == 0) return s;
    const unsigned epoch = A.mb0 + (unsigned)t;  // cross-rank: the peer mailbox, as reduce_input does
    if ((int)blockIdx.x < A.senders) mb_send(s, epoch);
    __syncthreads();
    return mb_recv(epoch, sh);
}

// one pass over this block's chunk: q -= h V_i, partial of <V_{i+1}, q> (NEXT) or <q, q>.  The
// host guarantees every block's chunk covers its RV + rl resident slots (no predicates there).
// The FD Jv of 2D Bratu at the two points (2e, 2e + 1) of one row, exactly as k_st2d<NK_BRATU2D,
// MODE_JFD> evaluates it (w = u + eps v; ((p - 2c) + m) / h^2 in x, then y; + lam exp(c);
// (r - F0) / eps), + the two terms of <V_1, Jv>.  Rows j +- 1 come from memory (ghost planes at the
// slab ends: zero or the neighbour's rows, as in the stencil kernel); x-neighbours outside the row
// are the zero Dirichlet boundary.
__device__ __forceinline__ dx2 res_jv_pair(const ResArgs& A, int64_t e, double& acc) {
    const int64_t p = 2 * e, nx = A.jnx;
    const int64_t i = p % nx;
    const dx2 vc = *reinterpret_cast<const dx2*>(A.jv + p), uc = __builtin_nontemporal_load(reinterpret_cast<const dx2*>(A.ju + p));
    const dx2 vu = *reinterpret_cast<const dx2*>(A.jv + p + nx), uu = *reinterpret_cast<const dx2*>(A.ju + p + nx);
    const dx2 vd = *reinterpret_cast<const dx2*>(A.jv + p - nx), ud = *reinterpret_cast<const dx2*>(A.ju + p - nx);
    const double vl = A.jv[p - 1], ul = A.ju[p - 1], vr = A.jv[p + 2], ur = A.ju[p + 2];
    const dx2 f0 = __builtin_nontemporal_load(reinterpret_cast<const dx2*>(A.jf0 + p));
    const dx2 ax = *reinterpret_cast<const dx2*>(A.jaux + p);
    const double eps = A.jeps;
    const double c0 = uc.x + eps * vc.x, c1 = uc.y + eps * vc.y;
    const double wl = i > 0 ? ul + eps * vl : 0.0;
    const double wr = i + 2 < nx ? ur + eps * vr : 0.0;
    const double u0 = uu.x + eps * vu.x, u1 = uu.y + eps * vu.y;
    const double d0 = ud.x + eps * vd.x, d1 = ud.y + eps * vd.y;
    const double l0 = ((c1 - 2.0 * c0) + wl) / A.jhx2 + ((u0 - 2.0 * c0) + d0) / A.jhy2;
    const double l1 = ((wr - 2.0 * c1) + c0) / A.jhx2 + ((u1 - 2.0 * c1) + d1) / A.jhy2;
    const double r0 = l0 + A.jlam * nk_exp(c0), r1 = l1 + A.jlam * nk_exp(c1);
    const dx2 val{(r0 - f0.x) / eps, (r1 - f0.y) / eps};
    acc = fma(ax.x, val.x, acc);
    acc = fma(ax.y, val.y, acc);
    return val;
}

// V loads of a pass: NTM 0 = V_i non-temporal, V_{i+1} cached (it is the next pass's V_i);
// 1 = both cached; 2 = both non-temporal (kernel-variant bench)
template <int NTM>
__device__ __forceinline__ dx2 ldv(const dx2* p) {
    if constexpr (NTM == 1) return *p;
    else return __builtin_nontemporal_load(p);
}
template <int NTM>
__device__ __forceinline__ dx2 ldw(const dx2* p) {
    if constexpr (NTM == 2) return __builtin_nontemporal_load(p);
    else return *p;
}
// V_{i+1} of resident slot `s`: the kernel-variant build's Infinity-Cache retention probe (NK_RES_NWC = w:
// slots s < w load V_{i+1} with the default policy, the rest non-temporally -- VERDICT r05 item 6); the
// product loads every slot as ldw does
template <int NTM>
__device__ __forceinline__ dx2 ldw_s(const dx2* p, int s, int nwc) {
#ifdef NK_KBENCH
    if (NTM != 2 && s >= nwc) return __builtin_nontemporal_load(p);
#else
    (void)s;
    (void)nwc;
#endif
    return ldw<NTM>(p);
}

// the first register batch of a pass, loaded before the previous pass's hand-off completes (its
// addresses do not depend on h): the load latency hides behind the hand-off
template <int B>
struct ResPre {
    dx2 b[B], c[B];
};
// rev (ALT with PRE, B = 4): the pass starts on the top LDS group, slots RV + rl - 4 .. RV + rl - 1
template <int RV, int B, bool PRE, int NTM = 0>
__device__ __forceinline__ void res_prefetch(const ResArgs& A, ResPre<B>& P, int t, int64_t base, int64_t ss,
                                             bool rev = false) {
    if constexpr (PRE && RV >= B) {
        const int tid = threadIdx.x;
        const int s0 = (B == 4 && rev) ? RV + A.rl - 4 : 0;
        const dx2* vb = reinterpret_cast<const dx2*>(A.V[t]) + base + tid + s0 * ss;
        const dx2* wb = reinterpret_cast<const dx2*>(A.V[t + 1 < A.np ? t + 1 : t]) + base + tid + s0 * ss;
#pragma unroll
        for (int u = 0; u < B; ++u) {
            P.b[u] = ldv<NTM>(vb + u * ss);
            P.c[u] = ldw_s<NTM>(wb + u * ss, s0 + u, A.nwc);
        }
    }
}

// rev (alternate passes, ALT variant): the LDS slots first and in descending order, then the
// register slots -- so the pass starts on the V_i lines the previous pass loaded last as its V_{i+1}
// (the LDS slots, ~5 MB per XCD: still in its L2).  The register slots keep one (ascending) order:
// a second, reversed copy of their unrolled loop costs scratch.
// NTS: the streamed remainder's q and V_{i+1} go non-temporal too (V_i always is), so the Infinity
// Cache keeps only the resident part's V_{i+1} for its re-read as the next pass's V_i
template <int RV, int B, bool PRE, int NTM = 0, bool NTS = false, int LB = 4>
__device__ __forceinline__ double res_pass(const ResArgs& A, ResState<RV>& S, dx2* lq, int t, double mh, int64_t lo,
                                           int64_t hi, ResPre<B>& P, int64_t base, int64_t ss, bool rev = false) {
    const int tid = threadIdx.x;
    const bool next = t + 1 < A.np;  // last pass: <q, q> instead of <V_{i+1}, q>
    const dx2* vb = reinterpret_cast<const dx2*>(A.V[t]) + base + tid;
    const dx2* wb = reinterpret_cast<const dx2*>(A.V[next ? t + 1 : t]) + base + tid;
    double acc = 0.0;
    auto upd = [&](dx2& a, const dx2 b, const dx2 c) {
        a.x = fma(mh, b.x, a.x);
        a.y = fma(mh, b.y, a.y);
        const dx2 p = next ? c : a;
        acc = fma(p.x, a.x, acc);
        acc = fma(p.y, a.y, acc);
    };
    // B slots per batch: 2 x B 16-B loads in flight per lane
    auto regs = [&] {
        constexpr int NB = (RV + B - 1) / B;
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) {
            const int s0 = bi * B;
            dx2 bv[B], cv[B];
            if (PRE && RV >= B && s0 == 0 && !(B == 4 && rev)) {
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    bv[u] = P.b[u];
                    cv[u] = P.c[u];
                }
            } else {
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    if (s0 + u < RV) {
                        bv[u] = ldv<NTM>(vb + (s0 + u) * ss);
                        cv[u] = ldw_s<NTM>(wb + (s0 + u) * ss, s0 + u, A.nwc);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (s0 + u < RV) upd(S.r[s0 + u], bv[u], cv[u]);
            __builtin_amdgcn_sched_barrier(0);  // no hoisting across batches: registers hold q, not loads
        }
    };
    const dx2* vl = vb + RV * ss;
    const dx2* wl = wb + RV * ss;
    const int rl = A.rl;
    // tail group (full residency only; never on a reversed pass): the last tg LDS slots leave the fused
    // loop.  Their update, elementwise and so free of any order, runs first, on the V_i lines this CU
    // loaded last in the previous pass as its V_{i+1} (nothing but the prefetch was loaded since: still
    // in this XCD's L2); their dot runs last, in slot order, so the chain of partial sums is unchanged
    const int tg = rev ? 0 : A.tg;
    const int rf = rl - tg;  // LDS slots of the fused loop
    auto tail_upd = [&](int s, auto nb) {  // slots s .. s+N-1: q -= h V_i, default load policy
        constexpr int N = decltype(nb)::value;
        dx2 bv[N];
#pragma unroll
        for (int u = 0; u < N; ++u) bv[u] = vl[(s + u) * ss];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            dx2 a = lq[(s + u) * kResThreads + tid];
            a.x = fma(mh, bv[u].x, a.x);
            a.y = fma(mh, bv[u].y, a.y);
            lq[(s + u) * kResThreads + tid] = a;
        }
    };
    auto tail_dot = [&](int s, auto nb) {  // slots s .. s+N-1: the partial of <V_{i+1}, q> or <q, q>
        constexpr int N = decltype(nb)::value;
        if (next) {
            dx2 cv[N];
#pragma unroll
            for (int u = 0; u < N; ++u) cv[u] = wl[(s + u) * ss];
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const dx2 a = lq[(s + u) * kResThreads + tid];
                acc = fma(cv[u].x, a.x, acc);
                acc = fma(cv[u].y, a.y, acc);
            }
        } else {
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const dx2 a = lq[(s + u) * kResThreads + tid];
                acc = fma(a.x, a.x, acc);
                acc = fma(a.y, a.y, acc);
            }
        }
    };
    auto tail = [&](auto&& f) {  // batches of 8 slots (8 16-B loads in flight per lane, as a fused batch of 4), then singles
        int s = rf;
        __builtin_amdgcn_sched_barrier(0);  // no fused-phase load hoisted into a tail batch: registers hold q
        for (; s + 8 <= rl; s += 8) {
            f(s, std::integral_constant<int, 8>{});
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; s < rl; ++s) f(s, std::integral_constant<int, 1>{});
        __builtin_amdgcn_sched_barrier(0);
    };
    auto lds = [&] {
        auto one4 = [&](int s, bool down) {  // LDS slots s .. s+3 (down: s+3 .. s)
            dx2 bv[4], cv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bv[u] = ldv<NTM>(vl + (s + u) * ss);
                cv[u] = ldw_s<NTM>(wl + (s + u) * ss, RV + s + u, A.nwc);
            }
#pragma unroll
            for (int u0 = 0; u0 < 4; ++u0) {
                const int u = down ? 3 - u0 : u0;
                dx2 a = lq[(s + u) * kResThreads + tid];
                upd(a, bv[u], cv[u]);
                lq[(s + u) * kResThreads + tid] = a;
            }
        };
        auto one = [&](int s) {
            const dx2 b = ldv<NTM>(vl + s * ss);
            const dx2 cc = ldw_s<NTM>(wl + s * ss, RV + s, A.nwc);
            dx2 a = lq[s * kResThreads + tid];
            upd(a, b, cc);
            lq[s * kResThreads + tid] = a;
        };
        auto oneB = [&](int s) {  // LDS slots s .. s+LB-1, all their loads issued first
            dx2 bv[LB], cv[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                bv[u] = ldv<NTM>(vl + (s + u) * ss);
                cv[u] = ldw_s<NTM>(wl + (s + u) * ss, RV + s + u, A.nwc);
            }
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                dx2 a = lq[(s + u) * kResThreads + tid];
                upd(a, bv[u], cv[u]);
                lq[(s + u) * kResThreads + tid] = a;
            }
        };
        const int r4 = rf / 4 * 4;
        if (!rev && LB != 4) {
            const int rb = rf / LB * LB;
            for (int s = 0; s < rb; s += LB) oneB(s);
            for (int s = rb; s < r4; s += 4) one4(s, false);
            for (int s = r4; s < rf; ++s) one(s);
        } else if (!rev) {
            for (int s = 0; s < r4; s += 4) one4(s, false);
            for (int s = r4; s < rf; ++s) one(s);
        } else if (PRE && B == 4 && RV >= B) {
            // ALT with PRE: groups of 4 from the top (the first one preloaded across the hand-off,
            // the previous pass's last V_{i+1} lines), then the rf % 4 lowest slots
            {
                const int s = rf - 4;
#pragma unroll
                for (int u0 = 0; u0 < 4; ++u0) {
                    const int u = 3 - u0;
                    dx2 a = lq[(s + u) * kResThreads + tid];
                    upd(a, P.b[u], P.c[u]);
                    lq[(s + u) * kResThreads + tid] = a;
                }
            }
            int s = rf - 8;
            for (; s >= 0; s -= 4) one4(s, true);
            for (s += 3; s >= 0; --s) one(s);
        } else {
            for (int s = rf - 1; s >= r4; --s) one(s);
            for (int s = r4 - 4; s >= 0; s -= 4) one4(s, true);
        }
    };
    auto stream = [&] {
        // the streamed remainder: q through memory, as k_mgs_pass
        dx2* q2 = reinterpret_cast<dx2*>(A.q);
        const dx2* v2 = reinterpret_cast<const dx2*>(A.V[t]);
        const dx2* w2 = reinterpret_cast<const dx2*>(A.V[next ? t + 1 : t]);
        auto ld = [](const dx2* p) {
            if constexpr (NTS) return __builtin_nontemporal_load(p);
            else return *p;
        };
        auto st = [](dx2* p, const dx2 v) {
            if constexpr (NTS) __builtin_nontemporal_store(v, p);
            else *p = v;
        };
        int64_t e = lo + (int64_t)(RV + rl) * kResThreads + tid;
        if constexpr (NTS) {  // the first ntc slots: V_{i+1} cached, re-read from the Infinity Cache next pass
            const int64_t hc = std::min<int64_t>(hi, e - tid + (int64_t)A.ntc * kResThreads);
            for (; e + kResThreads < hc; e += 2 * kResThreads) {
                const int64_t e1 = e + kResThreads;
                dx2 a0 = ld(q2 + e), a1 = ld(q2 + e1);
                const dx2 b0 = __builtin_nontemporal_load(v2 + e), b1 = __builtin_nontemporal_load(v2 + e1);
                const dx2 c0 = w2[e], c1 = w2[e1];
                upd(a0, b0, c0);
                upd(a1, b1, c1);
                st(q2 + e, a0);
                st(q2 + e1, a1);
            }
        }
        for (; e + kResThreads < hi; e += 2 * kResThreads) {
            const int64_t e1 = e + kResThreads;
            dx2 a0 = ld(q2 + e), a1 = ld(q2 + e1);
            const dx2 b0 = __builtin_nontemporal_load(v2 + e), b1 = __builtin_nontemporal_load(v2 + e1);
            const dx2 c0 = ld(w2 + e), c1 = ld(w2 + e1);
            upd(a0, b0, c0);
            upd(a1, b1, c1);
            st(q2 + e, a0);
            st(q2 + e1, a1);
        }
        if (e < hi) {
            dx2 a0 = ld(q2 + e);
            const dx2 b0 = __builtin_nontemporal_load(v2 + e);
            const dx2 c0 = ld(w2 + e);
            upd(a0, b0, c0);
            st(q2 + e, a0);
        }
    };
    if (rev) lds();
    tail(tail_upd);
    regs();
    if (!rev) lds();
    tail(tail_dot);
    stream();
    return acc;
}

template <int RV, int B = (RV > 80 ? 6 : RV > 64 ? 4 : 8), bool PRE = false, bool JV = false, bool ALT = false,
          int NTM = 0, bool NTS = false, int LB = 4>
__global__ __launch_bounds__(kResThreads, 1) void k_mgs_res(ResArgs A) {
    extern __shared__ dx2 lq[];  // rl x 256 double2
    __shared__ double sh[kShN];
    __shared__ unsigned xdone;  // tag of the last exchange a polling wave completed (poll1 >= 2)
    const int tid = threadIdx.x, G = gridDim.x;
    if (tid == 0) xdone = 0;  // tags start at 1; the first exchange follows a __syncthreads
    // balanced partition of the ceil(n2 / 256) 256-wide slots: block b owns slots [b S / G, (b+1) S / G)
    const int64_t ns = (A.n2 + kResThreads - 1) / kResThreads;
    const int64_t lo = (int64_t)blockIdx.x * ns / G * kResThreads;
    const int64_t hi = std::min<int64_t>((int64_t)(blockIdx.x + 1) * ns / G * kResThreads, A.n2);
    // slot s of this block: contiguous chunk (base = lo, stride 256) or, with A.strided (every block
    // exactly full), interleaved across the blocks (base = 256 b, stride 256 G) so that every block
    // touches every address region alike
    int64_t base = A.strided ? (int64_t)blockIdx.x * kResThreads : lo;
    int64_t ss = A.strided ? (int64_t)G * kResThreads : kResThreads;
#ifdef NK_KBENCH
    if (A.mirror && (blockIdx.x & 1)) {  // odd blocks walk their chunk from the top: another address phase
        base = hi - kResThreads;
        ss = -(int64_t)kResThreads;
    }
#endif
    ResState<RV> S;
    ResPre<B> P;
    double h;
    unsigned budget = A.spin;
    constexpr int xo = JV ? 1 : 0;  // exchange 0 carries <V_1, J V_k> when the Jv is fused
    if constexpr (JV) {
        double jacc = 0.0;
        // register slots in rounds of kJvStage, each computed by a compact (not unrolled) loop into
        // the LDS and then moved into its registers; the LDS slots last
        constexpr int kJvStage = 16;  // the host guarantees rl >= kJvStage when RV > 0
#pragma unroll
        for (int s0 = 0; s0 < RV; s0 += kJvStage) {
            const int m = RV - s0 < kJvStage ? RV - s0 : kJvStage;
#pragma unroll 4
            for (int u = 0; u < m; ++u) lq[u * kResThreads + tid] = res_jv_pair(A, base + (s0 + u) * ss + tid, jacc);
#pragma unroll
            for (int u = 0; u < kJvStage; ++u)
                if (s0 + u < RV) S.r[s0 + u] = lq[u * kResThreads + tid];
        }
#pragma unroll 4
        for (int s = 0; s < A.rl; ++s) lq[s * kResThreads + tid] = res_jv_pair(A, base + (RV + s) * ss + tid, jacc);
        res_prefetch<RV, B, PRE, NTM>(A, P, 0, base, ss);
        h = res_exchange(A, block_sum<kResThreads>(jacc, sh), 0, sh, budget, &xdone);
    } else {
        const dx2* qb = reinterpret_cast<const dx2*>(A.q) + base + tid;
#pragma unroll
        for (int s = 0; s < RV; ++s) S.r[s] = qb[s * ss];
        for (int s = 0; s < A.rl; ++s) lq[s * kResThreads + tid] = qb[(RV + s) * ss];
        res_prefetch<RV, B, PRE, NTM>(A, P, 0, base, ss);
        h = reduce_input(A.red_in, A.red_len, sh);
    }
    for (int t = 0; t < A.np; ++t) {
        if (blockIdx.x == 0 && tid == 0) {
            A.col[t] = h;
            if (A.colh) A.colh[t] = h;
        }
        const double acc = res_pass<RV, B, PRE, NTM, NTS, LB>(A, S, lq, t, -h, lo, hi, P, base, ss, ALT && (t & 1));
        if (t + 1 < A.np) res_prefetch<RV, B, PRE, NTM>(A, P, t + 1, base, ss, ALT && ((t + 1) & 1));
        const double part = block_sum<kResThreads>(acc, sh);
#ifdef NK_KBENCH
        if (A.tstamp && tid == 0) A.tstamp[((size_t)t * G + blockIdx.x) * 2] = wall_clock64();
        if (!A.noxchg) h = res_exchange(A, part, t + xo, sh, budget, &xdone);
        else __syncthreads();
        if (A.tstamp && tid == 0) A.tstamp[((size_t)t * G + blockIdx.x) * 2 + 1] = wall_clock64();
#else
        h = res_exchange(A, part, t + xo, sh, budget, &xdone);
#endif
    }
    if (blockIdx.x == 0 && tid == 0) {
        const double r = sqrt(h);
        A.col[A.np] = r;
        if (A.colh) A.colh[A.np] = r;
    }
    if (A.vout) {  // the next Arnoldi step's kdivcopy!(V_{k+1}, q, h) done here: q never leaves the chip
        const double hn = sqrt(h);  // == col[np], the h the next Jv would divide by
        dx2* vw = reinterpret_cast<dx2*>(A.vout) + base + tid;
#pragma unroll
        for (int s = 0; s < RV; ++s) vw[s * ss] = dx2{S.r[s].x / hn, S.r[s].y / hn};
        for (int s = 0; s < A.rl; ++s) {
            const dx2 a = lq[s * kResThreads + tid];
            vw[(RV + s) * ss] = dx2{a.x / hn, a.y / hn};
        }
        return;
    }
    dx2* qw = reinterpret_cast<dx2*>(A.q) + base + tid;
#pragma unroll
    for (int s = 0; s < RV; ++s) qw[s * ss] = S.r[s];
    for (int s = 0; s < A.rl; ++s) qw[(RV + s) * ss] = lq[s * kResThreads + tid];
}

// launch one instantiation and name it as rocprofv3 does (the profile entry's kernel: bench.py's PMC lookup)
template <int RV, int B = (RV > 80 ? 6 : RV > 64 ? 4 : 8), bool PRE = false, bool JV = false, bool ALT = false,
          int NTM = 0, bool NTS = false, int LB = 4>
const char* go_res(dim3 g, dim3 b, size_t lds, hipStream_t s, const ResArgs& A) {
    hipLaunchKernelGGL((k_mgs_res<RV, B, PRE, JV, ALT, NTM, NTS, LB>), g, b, lds, s, A);
    static char name[80] = {};
    if (!name[0]) {
        auto tf = [](bool x) { return x ? "true" : "false"; };
        std::snprintf(name, sizeof name, "nk::k_mgs_res<%d, %d, %s, %s, %s, %d, %s, %d>", RV, B, tf(PRE), tf(JV), tf(ALT), NTM,
                      tf(NTS), LB);
    }
    return name;
}

template <int RV, int B = (RV > 80 ? 6 : RV > 64 ? 4 : 8), bool PRE = false, bool JV = false, bool ALT = false,
          int NTM = 0, bool NTS = false, int LB = 4>
bool res_attr(size_t lds) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mgs_res<RV, B, PRE, JV, ALT, NTM, NTS, LB>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}
}  // namespace

// this unit's copy of the mailbox binding (called by mailbox_bind)
hipError_t resident_bind_mb(const MbInfo& m) { return hipMemcpyToSymbol(HIP_SYMBOL(g_mb), &m, sizeof(m)); }

namespace {
// one-time set-up of a context's resident path: the grid, the LDS slots, every instantiation's LDS
// attribute, the granules and the error flag; anything missing turns the resident path off for good
bool res_setup(nk_ctx* c) {
    if (c->res_gran) return true;
    int dev = 0, cus = 0, lds = 0;
    bool ok = hipGetDevice(&dev) == hipSuccess &&
              hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
              hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
              cus >= 1 && cus <= kResThreads;
    if (ok) {
        // ranks sharing this GPU (NK_RES_SHARED test rigs): each sweep grid gets its share of the CUs,
        // so that all the ranks' grids are resident at once
        c->res_blocks = std::max(1, cus / std::max(1, c->res_share));
        const int avail = lds - (int)(sizeof(double) * kShN) - 256;
        c->res_rl = std::max(0, avail / (int)(kResThreads * sizeof(dx2)));
        const size_t lmax = (size_t)c->res_rl * kResThreads * sizeof(dx2);
        ok = res_attr<0>(lmax) && res_attr<16>(lmax) && res_attr<25>(lmax) && res_attr<32>(lmax) && res_attr<48>(lmax) &&
             res_attr<64>(lmax) && res_attr<89, 4, true>(lmax) && res_attr<89, 4, true, false, false, 0, true>(lmax);
#ifdef NK_KBENCH
        ok = ok && res_attr<89>(lmax) && res_attr<89, 4>(lmax) && res_attr<89, 6, false, true>(lmax) &&
             res_attr<0, 8, false, true>(lmax) && res_attr<89, 6, false, false, true>(lmax) &&
             res_attr<89, 6, false, false, false, 1>(lmax) && res_attr<89, 6, false, false, false, 2>(lmax) &&
             res_attr<89, 6, false, false, false, 0, true>(lmax) && res_attr<89, 2, true>(lmax) &&
             res_attr<89, 4, true, false, false, 0, false, 8>(lmax) &&
             res_attr<89, 4, true, false, false, 0, false, 6>(lmax) && res_attr<89, 4, true, false, true>(lmax);
#endif
        int per_cu = 0;  // residency: at least one block of the largest variant per CU
        ok = ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(
                       &per_cu, reinterpret_cast<const void*>(&k_mgs_res<89, 4, true>), kResThreads, lmax) == hipSuccess &&
             per_cu >= 1;
    }
    ok = ok && hipMalloc(&c->res_gran, sizeof(uint64_t) * 4 * kResThreads) == hipSuccess;
    ok = ok && hipMemsetAsync(c->res_gran, 0, sizeof(uint64_t) * 4 * kResThreads, c->stream) == hipSuccess;
    ok = ok && hipHostMalloc(&c->res_err, sizeof(int), hipHostMallocMapped) == hipSuccess;
    if (ok) *c->res_err = 0;
    ok = ok && hipHostGetDevicePointer(reinterpret_cast<void**>(&c->res_err_dev), c->res_err, 0) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        c->res_ok = false;
    }
    return ok;
}

// the plan's knobs: read once per process, NK_RES_MIRROR and the bench hook's tail at every launch
ResKnobs res_knobs() {
    static const ResKnobs once = [] {
        const ResKnobs D;
        ResKnobs K;
        K.rl = NK_TUNE("NK_RES_RL", D.rl);
        K.rv = NK_TUNE("NK_RES_RV", D.rv);
        K.nts = NK_TUNE("NK_RES_NTS", D.nts);
        K.pre = NK_TUNE("NK_RES_PRE", D.pre);
        K.vout = NK_TUNE("NK_RES_VOUT", D.vout);
        K.strided = NK_TUNE("NK_RES_STRIDED", D.strided);
        K.tail = NK_TUNE("NK_RES_TAIL", D.tail);
        K.ntc = NK_TUNE("NK_RES_NTC", D.ntc);
        K.mall_mb = NK_TUNE("NK_RES_MALL_MB", D.mall_mb);
        K.jv = NK_TUNE("NK_RES_JV", D.jv);
        return K;
    }();
    ResKnobs K = once;
    K.mirror = NK_TUNE("NK_RES_MIRROR", K.mirror);
#ifdef NK_KBENCH
    if (g_res_tail_hook >= 0) K.tail = g_res_tail_hook;
#endif
    return K;
}

// launch the instantiation the plan names.  Load policy of the 89-slot variants (kbench: NK_RES_NTS /
// NK_RES_PRE): with a streamed remainder its q and V_{i+1} go non-temporal, so the Infinity Cache keeps
// the resident part's V_{i+1} for the next pass (kbench_res: -2..3 % per pass at half residency, -2..7 %
// at a quarter; config-4 slab bench +2.4 %, heat 8192^2 +3.9 %); batches of 4 with the first one loaded
// across the hand-off (-1.5 % per pass at k = 30, full residency; 4096^2 bench +0.6 %).  Same per-element
// arithmetic and accumulation order in every variant: bit-identical results.
const char* res_dispatch(const ResPlan& P, const ResKnobs& K, [[maybe_unused]] bool jv, dim3 g, dim3 b, size_t lds,
                         hipStream_t s, const ResArgs& A) {
#define NK_GO_RES(...) return go_res<__VA_ARGS__>(g, b, lds, s, A)
    const bool nts = !P.full && K.nts;
#ifdef NK_KBENCH  // the instantiations only the kernel-variant build has
    if (jv && P.rv == 0) NK_GO_RES(0, 8, false, true);
    if (jv) NK_GO_RES(89, 6, false, true);
    if (P.rv == 89) {
        switch (P.xv) {
        case 1: NK_GO_RES(89, 4);
        case 2: NK_GO_RES(89, 6, false, false, true);
        case 3: NK_GO_RES(89, 6, false, false, false, 1);
        case 4: NK_GO_RES(89, 6, false, false, false, 2);
        case 5: NK_GO_RES(89, 6, false, false, false, 0, true);
        case 8: NK_GO_RES(89, 2, true);
        case 9: NK_GO_RES(89, 4, true, false, false, 0, false, 8);
        case 10: NK_GO_RES(89, 4, true, false, false, 0, false, 6);
        case 11: NK_GO_RES(89, 4, true, false, true);
        default: break;
        }
        if (P.xv != 0 && P.xv != 6 && !K.pre) {
            if (nts) NK_GO_RES(89, 6, false, false, false, 0, true);
            NK_GO_RES(89);
        }
    }
#endif
    switch (P.rv) {
    case 0: NK_GO_RES(0);
    case 16: NK_GO_RES(16);
    case 25: NK_GO_RES(25);
    case 48: NK_GO_RES(48);
    case 64: NK_GO_RES(64);
    case 89:
        if (P.xv == 6 || (P.xv != 0 && nts)) NK_GO_RES(89, 4, true, false, false, 0, true);
        NK_GO_RES(89, 4, true);
    default: NK_GO_RES(32);
    }
#undef NK_GO_RES
}
}  // namespace

// Resident sweep: returns NK_OK after enqueueing, or 1 when the resident path does not apply
// (caller falls back to one k_mgs_pass launch per pass).
int launch_mgs_sweep(nk_ctx* c, int64_t n, double* q, const double* const* V, int k, int np, Red in, double* col,
                     double* colh, int rv, double** vout, const ResJv* jin) {
    if (!c->res_ok || (c->comm && !c->mb_on)) return 1;  // RCCL reductions need the host between passes
    if (!res_setup(c)) return 1;
    const ResKnobs K = res_knobs();
    const ResPlan P = res_plan(n, np, c->res_blocks, c->res_rl, rv, vout && *vout, jin ? jin->nx : 0, K);
    if (!P.applies) return 1;
    if (vout && *vout && !P.keep_vout) *vout = nullptr;
#ifdef NK_KBENCH
    g_res_tail_launched = P.tg;
#endif
    ResArgs A{};
    for (int t = 0; t < np; ++t) A.V[t] = V[t % k];
    A.V[np] = V[(np) % k];
    A.q = q;
    A.vout = vout ? *vout : nullptr;
    A.col = col;
    A.colh = colh;
    A.red_in = in.ptr;
    A.red_len = in.len;
    A.gran = c->res_gran;
    A.err = c->res_err_dev;
    A.n2 = n >> 1;
    A.np = np;
    A.rl = P.rl;
    A.tg = P.tg;
    A.strided = P.strided;
    A.mirror = P.mirror;
    A.ntc = P.ntc;
    if (jin) {
        A.jv_on = 1;
        A.ju = jin->u;
        A.jv = jin->v;
        A.jf0 = jin->F0;
        A.jaux = jin->aux;
        A.jeps = jin->eps;
        A.jlam = jin->lam;
        A.jhx2 = jin->hx2;
        A.jhy2 = jin->hy2;
        A.jnx = jin->nx;
    }
    const unsigned nx_ = (unsigned)np + (jin ? 1u : 0u);  // hand-offs in this launch
    if (c->res_tag > 0xfffffff0u - (unsigned)(kResMax + 1)) {  // tag wrap: restart from clean granules
        NK_HIP(c, hipMemsetAsync(c->res_gran, 0, sizeof(uint64_t) * 4 * kResThreads, c->stream));
        c->res_tag = 0;
    }
    A.tag0 = c->res_tag + 1;
    c->res_tag += nx_;
    A.mb0 = 0;
    if (c->mb_on) {  // consecutive mailbox epochs, no 16-bit wrap inside the range
        if (c->mb_epoch + nx_ > 0xffffu) c->mb_epoch = 0;
        A.mb0 = c->mb_epoch + 1;
        c->mb_epoch += nx_;
    }
    A.noxchg = NK_TUNE("NK_RES_NOXCHG", 0);  // kbench timing probe only: the h exchange skipped (wrong results)
    A.poll1 = NK_TUNE("NK_RES_POLL1", 1);
    A.nwc = NK_TUNE("NK_RES_NWC", 1 << 30);
    A.tstamp = c->res_tstamp;
    // cross-rank hand-off: the first `senders` blocks (one per XCD at 8) all send the rank's sum -- the
    // same bits into the same cells -- so the peers see it as soon as the EARLIEST of them has it,
    // not when block 0 happens to finish its local poll
    static const int senders = NK_TUNE("NK_MB_SENDERS", 8);
    A.senders = std::max(1, std::min(senders, c->res_blocks));
    A.spin = 1u << 22;  // polls per thread per launch (~1 s): a grid that is not co-resident fails fast
    const size_t lds = (size_t)A.rl * kResThreads * sizeof(dx2);
    ++c->n_sweep_resident;
    const char* kn = nullptr;
    return launch_dyn(c, jin ? "arnoldi_step" : "mgs_sweep", [&] {
        kn = res_dispatch(P, K, jin != nullptr, dim3(c->res_blocks), dim3(kResThreads), lds, c->stream, A);
        return P.bytes;
    }, P.dram, &kn);
}

}  // namespace nk

#ifdef NK_KBENCH  // kernel-variant bench hooks: lib/libnkhip_kbench.so only
namespace nk {
namespace {
__global__ __launch_bounds__(kBlock) void k_hashfill(int64_t n, double* __restrict__ x, uint64_t seed) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        uint64_t z = (uint64_t)i * 0x9e3779b97f4a7c15ull + seed;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        x[i] = (double)(z >> 11) * 0x1.0p-53 - 0.5;
    }
}
}  // namespace
}  // namespace nk

// The resident MGS sweep (launch_mgs_sweep, register slots rv) against the per-pass chain
// (launch_mgs_pass) on the same q and basis: us_out / us_ref = microseconds per pass of each;
// diff_out = max |q_res - q_chain| / max |q_chain| after the sweep, and the largest relative
// difference of the Hessenberg column in diff_out[1].
// tail >= 0: the sweep's tail-group size instead of NK_RES_TAIL (the host rule still clamps it and
// turns it off without full residency); tail_out: the size the sweep launched with; q_out (n) and
// col_out (k + 1): the sweep's q and Hessenberg column, to compare two schedules bit for bit.
static int mgs_res_bench(nk_ctx* c, int64_t n, int k, int rv, int tail, int reps, double* us_out, double* us_ref,
                         double* diff_out, double* q_out, double* col_out, int* tail_out) {
    using namespace nk;
    if (!c || n < 2 || k < 1 || k > kResMax || reps < 1 || !us_out || !us_ref || !diff_out) return NK_E_ARG;
    // NK_RES_TSTAMP=<file>: also dump the per-pass, per-block wall clocks of the last timed sweep
    const char* tsf = getenv("NK_RES_TSTAMP");
    if (tsf && *tsf && !c->res_tstamp) NK_HIP(c, hipMalloc(&c->res_tstamp, sizeof(uint64_t) * 2 * kResMax * 1024));
    std::vector<double*> V(k + 3, nullptr), Vbase(k + 3, nullptr);
    // the product's vector start offsets (nk_vec_alloc): vector v starts (v mod 8) x
    // NK_ALLOC_STAGGER bytes (128 KB) into its allocation, so the hook times the layout the solver runs on
    const size_t stag = (size_t)std::max(0, NK_TUNE("NK_ALLOC_STAGGER", 131072)) / 256 * 32;  // doubles
    for (size_t v = 0; v < V.size(); ++v) {
        const size_t sh = (v % 8) * stag;
        NK_HIP(c, hipMalloc(&Vbase[v], sizeof(double) * (n + sh)));
        V[v] = Vbase[v] + sh;
        hipLaunchKernelGGL(k_hashfill, dim3(2048), dim3(kBlock), 0, c->stream, n, V[v], (uint64_t)(v + 1) * 7919u);
    }
    double* q0 = V[k];
    double* qa = V[k + 1];
    double* qb = V[k + 2];
    double* col = c->scal + 64;
    double* col2 = c->scal + 64 + 2 * kResMax;
    hipEvent_t e0, e1;
    NK_HIP(c, hipEventCreate(&e0));
    NK_HIP(c, hipEventCreate(&e1));
    double ms_a = 0.0, ms_b = 0.0;
    for (int r = 0; r <= reps; ++r) {
        float ms = 0.f;
        NK_TRY(launch_copy(c, n, qa, q0));
        Red red{};
        NK_TRY(launch_dot(c, n, V[0], qa, &red));
        NK_HIP(c, hipEventRecord(e0, c->stream));
        for (int t = 0; t < k; ++t) {
            Red nxt{};
            NK_TRY(launch_mgs_pass(c, n, qa, V[t], t + 1 < k ? V[t + 1] : nullptr, red, col + t, nullptr, &nxt, 0));
            red = nxt;
        }
        NK_TRY(launch_finalize(c, red, col + k, 1, nullptr));
        NK_HIP(c, hipEventRecord(e1, c->stream));
        NK_HIP(c, hipEventSynchronize(e1));
        NK_HIP(c, hipEventElapsedTime(&ms, e0, e1));
        if (r > 0) ms_a += ms;
        NK_TRY(launch_copy(c, n, qb, q0));
        NK_TRY(launch_dot(c, n, V[0], qb, &red));
        NK_HIP(c, hipEventRecord(e0, c->stream));
        g_res_tail_hook = tail;
        const int rc = launch_mgs_sweep(c, n, qb, V.data(), k, k, red, col2, nullptr, rv, nullptr, nullptr);
        g_res_tail_hook = -1;
        if (rc != NK_OK) return rc == 1 ? fail(c, NK_E_ARG, "resident sweep not applicable") : rc;
        NK_HIP(c, hipEventRecord(e1, c->stream));
        NK_HIP(c, hipEventSynchronize(e1));
        NK_HIP(c, hipEventElapsedTime(&ms, e0, e1));
        if (r > 0) ms_b += ms;
        if (*c->res_err) return fail(c, NK_E_HIP, "resident sweep: granule poll timed out");
    }
    *us_ref = 1e3 * ms_a / ((double)reps * k);
    *us_out = 1e3 * ms_b / ((double)reps * k);
    std::vector<double> a(n), b(n), ca(k + 1), cb(k + 1);
    NK_HIP(c, hipMemcpy(a.data(), qa, sizeof(double) * n, hipMemcpyDeviceToHost));
    NK_HIP(c, hipMemcpy(b.data(), qb, sizeof(double) * n, hipMemcpyDeviceToHost));
    NK_HIP(c, hipMemcpy(ca.data(), col, sizeof(double) * (k + 1), hipMemcpyDeviceToHost));
    NK_HIP(c, hipMemcpy(cb.data(), col2, sizeof(double) * (k + 1), hipMemcpyDeviceToHost));
    double m = 0.0, d = 0.0, dh = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        m = std::max(m, std::fabs(a[i]));
        d = std::max(d, std::fabs(a[i] - b[i]));
    }
    for (int i = 0; i <= k; ++i) dh = std::max(dh, std::fabs(ca[i] - cb[i]) / std::max(1e-300, std::fabs(ca[i])));
    diff_out[0] = m > 0 ? d / m : d;
    diff_out[1] = dh;
    diff_out[2] = (double)c->res_rl;
    if (tail_out) *tail_out = g_res_tail_launched;
    if (q_out) std::copy(b.begin(), b.end(), q_out);
    if (col_out) std::copy(cb.begin(), cb.end(), col_out);
    if (c->res_tstamp && tsf && *tsf) {
        std::vector<uint64_t> ts((size_t)2 * k * c->res_blocks);
        NK_HIP(c, hipMemcpy(ts.data(), c->res_tstamp, sizeof(uint64_t) * ts.size(), hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(tsf, "wb")) {
            std::fwrite(ts.data(), sizeof(uint64_t), ts.size(), f);
            std::fclose(f);
        }
        (void)hipFree(c->res_tstamp);
        c->res_tstamp = nullptr;
    }
    diff_out[3] = (double)c->res_blocks;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    for (auto p : Vbase) (void)hipFree(p);
    return NK_OK;
}

extern "C" int nkb_mgs_res(nk_ctx* c, int64_t n, int k, int rv, int reps, double* us_out, double* us_ref, double* diff_out) {
    return mgs_res_bench(c, n, k, rv, -1, reps, us_out, us_ref, diff_out, nullptr, nullptr, nullptr);
}

extern "C" int nkb_mgs_res_tail(nk_ctx* c, int64_t n, int k, int rv, int tail, int reps, double* us_out, double* us_ref,
                                double* diff_out, double* q_out, double* col_out, int* tail_out) {
    if (!tail_out) return NK_E_ARG;
    return mgs_res_bench(c, n, k, rv, tail, reps, us_out, us_ref, diff_out, q_out, col_out, tail_out);
}

// the tail-group size of this process's last resident sweep launch (a solve's as well as the hook's)
extern "C" int nkb_res_tail_last(void) { return nk::g_res_tail_launched; }
#endif  // NK_KBENCH
