// nk_minres.hip -- the streaming kernels of the device MINRES (nk_krylov.cpp minres()): the
// Lanczos step fused with the preconditioner's diagonal and the next beta^2, the w / x update, and the
// one-block finaliser that leaves beta on the device and alpha's partners in mapped host memory.  fp64,
// 16-B accesses on the NK_CHUNKED order, no atomics on data; every reduction goes through publish /
// reduce_input, so two solves give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nk_device.hpp"

namespace nk {
namespace {

#define NK_CHUNKED2(i) NK_CHUNKED(i, n >> 1)
#define NK_TAIL (((n & 1) != 0) && blockIdx.x == 0 && threadIdx.x == 0)

// One Lanczos step after the Jv launch (which stored v = y / beta and the partials of <v, J v>):
//   alpha = Σ a_in                    (fixed order: the same bits in every block; crosses the mailbox on several ranks)
//   t = (Jv - (beta / oldbeta) r1) - (alpha / beta) r2      stored over r1 (pointwise: the host rotates the pointers)
//   PRE == 1: y = d .* t              (the diagonal M)
//   partials of beta_next^2 = <t, y>  (<t, t> without M) and, with part_y, of ||y||^2 (the FD step's ||v||)
// first: iteration 1 has no r1 term (oldbeta = 0).  part_b == nullptr: M is applied by later launches, which
// also produce <t, y>.  Block 0 mirrors alpha to a_host (mapped host memory).
// 32 B/pt (24 on the first iteration), 48 with the diagonal M.
template <int PRE>
__global__ __launch_bounds__(kBlock) void k_minres_lanczos(int64_t n, const double* __restrict__ jv, double* __restrict__ r1,
                                                          const double* __restrict__ r2, const double* __restrict__ d,
                                                          double* __restrict__ y, const double* __restrict__ beta_p,
                                                          const double* __restrict__ oldbeta_p, int first,
                                                          const double* __restrict__ a_in, int a_len,
                                                          double* __restrict__ a_host, double* __restrict__ part_b,
                                                          int fin_b, double* __restrict__ part_y, int fin_y) {
    __shared__ double sh[kShN];
    __shared__ double shy[kShN];
    const double alpha = reduce_input(a_in, a_len, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a_host = alpha;
    const double beta = *beta_p;
    const double c1 = first ? 0.0 : beta / *oldbeta_p;
    const double c2 = alpha / beta;
    const dx2* j2 = reinterpret_cast<const dx2*>(jv);
    dx2* p2 = reinterpret_cast<dx2*>(r1);
    const dx2* q2 = reinterpret_cast<const dx2*>(r2);
    const dx2* d2 = reinterpret_cast<const dx2*>(d);
    dx2* y2 = reinterpret_cast<dx2*>(y);
    double accb = 0.0, accy = 0.0;
    NK_CHUNKED2(i) {
        dx2 t = j2[i];
        if (!first) {
            const dx2 a = p2[i];
            t.x = fma(-c1, a.x, t.x);
            t.y = fma(-c1, a.y, t.y);
        }
        const dx2 b = q2[i];
        t.x = fma(-c2, b.x, t.x);
        t.y = fma(-c2, b.y, t.y);
        p2[i] = t;
        if constexpr (PRE == 1) {
            const dx2 dd = d2[i];
            dx2 yy;
            yy.x = dd.x * t.x;
            yy.y = dd.y * t.y;
            y2[i] = yy;
            accb = fma(t.x, yy.x, accb);
            accb = fma(t.y, yy.y, accb);
            accy = fma(yy.x, yy.x, accy);
            accy = fma(yy.y, yy.y, accy);
        } else {
            accb = fma(t.x, t.x, accb);
            accb = fma(t.y, t.y, accb);
        }
    }
    if (NK_TAIL) {
        double t = jv[n - 1];
        if (!first) t = fma(-c1, r1[n - 1], t);
        t = fma(-c2, r2[n - 1], t);
        r1[n - 1] = t;
        if constexpr (PRE == 1) {
            const double yy = d[n - 1] * t;
            y[n - 1] = yy;
            accb = fma(t, yy, accb);
            accy = fma(yy, yy, accy);
        } else {
            accb = fma(t, t, accb);
        }
    }
    if (part_b) publish(accb, part_b, fin_b, sh);
    if (part_y) publish(accy, part_y, fin_y, shy);  // (its own wave slots: thread 0 may still be reading sh)
}

// w = ((v - oldeps w1) - delta w2) / gamma, stored over w1 (the host rotates the pointers); x += phi w.  48 B/pt
__global__ __launch_bounds__(kBlock) void k_minres_update(int64_t n, const double* __restrict__ v, double* __restrict__ w1,
                                                         const double* __restrict__ w2, double* __restrict__ x,
                                                         double oldeps, double delta, double gamma, double phi) {
    const dx2* v2 = reinterpret_cast<const dx2*>(v);
    dx2* a2 = reinterpret_cast<dx2*>(w1);
    const dx2* b2 = reinterpret_cast<const dx2*>(w2);
    dx2* x2 = reinterpret_cast<dx2*>(x);
    NK_CHUNKED2(i) {
        const dx2 vv = v2[i], a = a2[i], b = b2[i];
        dx2 xx = x2[i], w;
        w.x = fma(-delta, b.x, fma(-oldeps, a.x, vv.x)) / gamma;
        w.y = fma(-delta, b.y, fma(-oldeps, a.y, vv.y)) / gamma;
        a2[i] = w;
        xx.x = fma(phi, w.x, xx.x);
        xx.y = fma(phi, w.y, xx.y);
        x2[i] = xx;
    }
    if (NK_TAIL) {
        const double w = fma(-delta, w2[n - 1], fma(-oldeps, w1[n - 1], v[n - 1])) / gamma;
        w1[n - 1] = w;
        x[n - 1] = fma(phi, w, x[n - 1]);
    }
}

// beta^2 = Σ b_in (and ||y||^2 = Σ y_in): beta = sqrt(beta^2) stays on the device (the next Jv divides by it, the next
// Lanczos step forms its coefficients from it); host[1] = beta^2 and host[2] = ||y||^2 go to mapped host memory
__global__ __launch_bounds__(kBlock) void k_minres_scalars(const double* __restrict__ b_in, int b_len,
                                                          const double* __restrict__ y_in, int y_len,
                                                          double* __restrict__ beta_dev, double* __restrict__ host) {
    __shared__ double sh[kShN];
    const double b2 = reduce_input(b_in, b_len, sh);
    __syncthreads();
    const double yn2 = y_in ? reduce_input(y_in, y_len, sh) : 0.0;
    if (threadIdx.x == 0) {
        *beta_dev = sqrt(b2);
        host[1] = b2;
        host[2] = yn2;
    }
}

}  // namespace

// this unit's copy of the mailbox binding (mailbox_bind sets every unit's)
hipError_t minres_bind_mb(const MbInfo& m) { return hipMemcpyToSymbol(HIP_SYMBOL(g_mb), &m, sizeof(m)); }

int launch_minres_lanczos(nk_ctx* c, int64_t n, const double* jv, double* r1, const double* r2, const double* d, double* y,
                          const double* beta, const double* oldbeta, int first, Red alpha, double* alpha_host, Red* rb,
                          Red* ry) {
    const int g = red_blocks(n);
    int fin_b = 0, fin_y = 0;
    double* part_b = rb ? red_out(c, g, rb, &fin_b) : nullptr;
    double* part_y = ry ? red_out(c, g, ry, &fin_y) : nullptr;
    const double bytes = (double)n * (d ? (first ? 40.0 : 48.0) : (first ? 24.0 : 32.0));
    return launch(c, d ? "minres_lanczos_diag" : "minres_lanczos", bytes, [&] {
        if (d)
            hipLaunchKernelGGL(k_minres_lanczos<1>, dim3(g), dim3(kBlock), 0, c->stream, n, jv, r1, r2, d, y, beta, oldbeta,
                               first, alpha.ptr, alpha.len, alpha_host, part_b, fin_b, part_y, fin_y);
        else
            hipLaunchKernelGGL(k_minres_lanczos<0>, dim3(g), dim3(kBlock), 0, c->stream, n, jv, r1, r2, d, y, beta, oldbeta,
                               first, alpha.ptr, alpha.len, alpha_host, part_b, fin_b, part_y, fin_y);
    });
}

int launch_minres_update(nk_ctx* c, int64_t n, const double* v, double* w1, const double* w2, double* x, double oldeps,
                         double delta, double gamma, double phi) {
    const int g = wide_blocks(n);
    return launch(c, "minres_update", 48.0 * (double)n, [&] {
        hipLaunchKernelGGL(k_minres_update, dim3(g), dim3(kBlock), 0, c->stream, n, v, w1, w2, x, oldeps, delta, gamma, phi);
    });
}

int launch_minres_scalars(nk_ctx* c, Red rb, const Red* ry, double* beta_dev, double* host) {
    return launch(c, "minres_scalars", 8.0 * ((rb.len > 0 ? rb.len : 1) + (ry && ry->len > 0 ? ry->len : 0)), [&] {
        hipLaunchKernelGGL(k_minres_scalars, dim3(1), dim3(kBlock), 0, c->stream, rb.ptr, rb.len, ry ? ry->ptr : nullptr,
                           ry ? ry->len : 0, beta_dev, host);
    });
}

}  // namespace nk
