// nk_lsq.hpp -- the Krylov drivers' host algebra as pure host code: Krylov.jl's sym_givens, GMRES's
// least-squares state (the Givens rotations, the packed R, z, the back-substitution), its stop rules,
// and MINRES's rotation scalars.  Scalars in, scalars out: nothing here touches a device, so the
// arithmetic is callable -- and tested -- on the CPU (tests/test_lsq.py, bit for bit against
// oracle/ariadne_ref.py and test_hip_minres.py's minres_ref).  nk_krylov.cpp feeds it the Hessenberg
// columns the kernels leave in pinned memory.  Build with -ffp-contract=off (the Makefile does): every
// operation below is one IEEE operation, in Krylov.jl's order.  No HIP header: this file compiles with
// a plain host compiler.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nk {

inline double sgn(double x) { return (double)((x > 0) - (x < 0)); }

// Krylov.jl sym_givens (real case)
inline void sym_givens(double a, double b, double* c, double* s, double* rho) {
    if (b == 0.0) {
        *c = (a == 0.0) ? 1.0 : sgn(a);
        *s = 0.0;
        *rho = std::fabs(a);
    } else if (a == 0.0) {
        *c = 0.0;
        *s = sgn(b);
        *rho = std::fabs(b);
    } else if (std::fabs(b) > std::fabs(a)) {
        const double t = a / b;
        *s = sgn(b) / std::sqrt(1.0 + t * t);
        *c = *s * t;
        *rho = b / *s;
    } else {
        const double t = b / a;
        *c = sgn(a) / std::sqrt(1.0 + t * t);
        *s = *c * t;
        *rho = a / *c;
    }
}

// ---------------------------------------------------------------- GMRES: the stop rules
inline double gmres_btol() { return std::pow(DBL_EPSILON, 0.75); }
inline bool gmres_solved(double rNorm, double eps_) { return (rNorm <= eps_) || (rNorm + 1.0 <= 1.0); }
inline bool gmres_breakdown(double Hbis, double btol) { return Hbis <= btol; }
// step `inner_iter` is the cycle's last whatever its column says (it sets inner_tired): a restarted
// cycle ends at min(memory, inner_itmax), an unrestarted one at inner_itmax
inline bool gmres_last(bool restart, int64_t inner_iter, int mem, int64_t inner_itmax) {
    return restart ? (inner_iter >= std::min<int64_t>(mem, inner_itmax)) : (inner_iter >= inner_itmax);
}

// ---------------------------------------------------------------- GMRES: the least-squares state
// min || beta e_1 - H y || by Givens rotations, one Hessenberg column at a time (same layout as
// Krylov.jl: R column-packed, y left in z by the back-substitution)
struct GmresLsq {
    std::vector<double> cs, sn, z, R;
    int64_t nr = 0;  // entries of R in use: column k starts at nr
    int cap;         // basis vectors the arrays hold: `memory`, doubled when unrestarted GMRES runs past it

    explicit GmresLsq(int mem) : cs(mem), sn(mem), z(mem + 1), R((size_t)mem * (mem + 1) / 2), cap(mem) {}

    void start(double beta) {  // a cycle begins: z = beta e_1
        nr = 0;
        std::fill(cs.begin(), cs.end(), 0.0);
        std::fill(sn.begin(), sn.end(), 0.0);
        std::fill(z.begin(), z.end(), 0.0);
        std::fill(R.begin(), R.end(), 0.0);
        z[0] = beta;
    }

    struct Col {
        double rNorm, Hbis, zeta;
    };
    // Step k's raw column as the kernels leave it: hcol[0 .. k) the first MGS pass, k more entries of the
    // second when reorthogonalising, then h_{k+1,k} = ||q||.  The earlier rotations, the new one, z[k-1].
    Col column(int k, const double* hcol, bool reorth) {
        if (k + 1 > cap) {  // unrestarted GMRES grows beyond `memory`
            const int nc = cap * 2;
            cs.resize(nc, 0.0);
            sn.resize(nc, 0.0);
            z.resize(nc + 1, 0.0);
            R.resize((size_t)nc * (nc + 1) / 2, 0.0);
            cap = nc;
        }
        for (int i = 0; i < k; ++i) R[nr + i] = hcol[i];
        if (reorth)
            for (int i = 0; i < k; ++i) R[nr + i] += hcol[k + i];
        const double Hbis = hcol[reorth ? 2 * k : k];
        for (int i = 1; i <= k - 1; ++i) {
            const double Rtmp = cs[i - 1] * R[nr + i - 1] + sn[i - 1] * R[nr + i];
            R[nr + i] = sn[i - 1] * R[nr + i - 1] - cs[i - 1] * R[nr + i];
            R[nr + i - 1] = Rtmp;
        }
        sym_givens(R[nr + k - 1], Hbis, &cs[k - 1], &sn[k - 1], &R[nr + k - 1]);
        const double zeta = sn[k - 1] * z[k - 1];
        z[k - 1] = cs[k - 1] * z[k - 1];
        nr += k;
        return {std::fabs(zeta), Hbis, zeta};
    }

    void accept(int k, double zeta) { z[k] = zeta; }  // the cycle goes on to step k + 1

    // back substitution R y = z after kk steps (Krylov.jl, y stored in z); returns `inconsistent`
    bool solve(int kk, double btol) {
        bool inconsistent = false;
        for (int i = kk; i >= 1; --i) {
            int64_t pos = nr + i - kk;
            for (int j = kk; j >= i + 1; --j) {
                z[i - 1] = z[i - 1] - R[pos - 1] * z[j - 1];
                pos = pos - j + 1;
            }
            if (std::fabs(R[pos - 1]) <= btol) {
                z[i - 1] = 0.0;
                inconsistent = true;
            } else {
                z[i - 1] = z[i - 1] / R[pos - 1];
            }
        }
        return inconsistent;
    }
    const double* y() const { return z.data(); }
};

// ---------------------------------------------------------------- MINRES: the rotation scalars
// The QR of the Lanczos tridiagonal, one column per step: alpha = <v, J v> and
// beta2 = beta_{k+1}^2 in; the scalars of w = ((v - oldeps w1) - delta w2) / gamma, x += phi w out.
struct MinresRot {
    double oldb = 0.0, beta, dbar = 0.0, eps = 0.0, phibar, cs = -1.0, sn = 0.0;

    explicit MinresRot(double beta1) : beta(beta1), phibar(beta1) {}

    struct Step {
        double oldeps, delta, gamma, phi;
    };
    Step step(double alpha, double beta2) {
        oldb = beta;
        beta = std::sqrt(beta2);
        const double oldeps = eps;
        const double delta = cs * dbar + sn * alpha;
        const double gbar = sn * dbar - cs * alpha;
        eps = sn * beta;
        dbar = -cs * beta;
        const double gamma = std::fmax(std::sqrt(gbar * gbar + beta * beta), DBL_EPSILON);
        cs = gbar / gamma;
        sn = beta / gamma;
        const double phi = cs * phibar;
        phibar = sn * phibar;
        return {oldeps, delta, gamma, phi};
    }
};

}  // namespace nk
