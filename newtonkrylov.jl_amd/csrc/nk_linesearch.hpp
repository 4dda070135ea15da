// nk_linesearch.hpp -- the Newton step's line search as pure host code: Kelley's three-point parabolic
// backtracking on ||F|| (C. T. Kelley, Iterative Methods for Linear and Nonlinear Equations, SIAM 1995, §8.3;
// nsoli's `parab3p`).  Doubles in, doubles out: nothing here touches a device, so the rule is callable -- and
// tested -- on the CPU (tests/test_linesearch_cpu.py, bit for bit against ariadne_hip.Backtracking and the
// test's own restatement).  nk_newton.cpp feeds it the trial norms nk_residual_trial returns.  Build with
// -ffp-contract=off (the Makefile does): every operation below is one IEEE operation, in the order written.
// No HIP header: this file compiles with a plain host compiler.
#pragma once

#include <cmath>

namespace nk {

struct LsOpts {
    double alpha = 1e-4;   // sufficient decrease: ||F(u - lam d)|| < (1 - alpha lam) ||F(u)||
    double sigma0 = 0.1;   // a reduction keeps lam within [sigma0, sigma1] x the current lam
    double sigma1 = 0.5;
    int maxarm = 20;       // reductions per Newton step before the search gives up
};

// 0 < alpha < 1, 0 < sigma0 <= sigma1 < 1, maxarm >= 1 (NaN fails every test)
inline bool ls_opts_ok(const LsOpts& o) {
    return o.alpha > 0.0 && o.alpha < 1.0 && o.sigma0 > 0.0 && o.sigma0 <= o.sigma1 && o.sigma1 < 1.0 && o.maxarm >= 1;
}

// The next lam from the last two: the minimiser of the parabola through (0, ff0), (lc, ffc), (lm, ffm), ff = ||F||^2,
// lc / lm the current / previous lam, clamped to [sigma0 lc, sigma1 lc]; sigma1 lc when a value is not finite or the
// parabola has no minimum (c2 >= 0).
inline double parab3p(const LsOpts& o, double lc, double lm, double ff0, double ffc, double ffm) {
    if (!std::isfinite(ffc) || !std::isfinite(ffm)) return o.sigma1 * lc;
    const double c2 = lm * (ffc - ff0) - lc * (ffm - ff0);
    if (!(c2 < 0.0)) return o.sigma1 * lc;
    const double c1 = lc * lc * (ffm - ff0) - lm * lm * (ffc - ff0);
    double lp = ((-c1) * 0.5) / c2;
    const double lo = o.sigma0 * lc, hi = o.sigma1 * lc;
    if (!(lp >= lo)) lp = lo;  // max(lp, lo)
    if (lp > hi) lp = hi;      // min(.., hi)
    return lp;
}

enum LsVerdict { LS_ACCEPT = 0, LS_RETRY = 1, LS_FAILED = 2 };

// One Newton step's search.  begin(||F(u)||) sets lam = 1; the caller evaluates n_t = ||F(u - lam d)|| and feeds
// it: LS_ACCEPT (take u - lam d), LS_RETRY (lam is the next trial) or LS_FAILED (maxarm reductions were rejected:
// maxarm + 1 trials in all).  A NaN or infinite n_t fails the decrease test and is a rejected trial like any other.
struct LsStep {
    LsOpts o;
    double n_res = 0.0, lam = 1.0, lm = 1.0, lc = 1.0, ff0 = 0.0, ffc = 0.0, ffm = 0.0;
    int k = 0;  // rejected trials that were followed by another
    bool fresh = true;

    void begin(const LsOpts& opts, double n_res_) {
        o = opts;
        n_res = n_res_;
        lam = lm = lc = 1.0;
        k = 0;
        fresh = true;
    }
    LsVerdict feed(double n_t) {
        if (fresh) {
            ff0 = n_res * n_res;
            ffc = ffm = n_t * n_t;
            fresh = false;
        } else {
            ffc = n_t * n_t;
            k += 1;
        }
        if (n_t < (1.0 - o.alpha * lam) * n_res) return LS_ACCEPT;
        if (k == o.maxarm) return LS_FAILED;
        lam = k == 0 ? o.sigma1 * lam : parab3p(o, lc, lm, ff0, ffc, ffm);
        lm = lc;
        lc = lam;
        ffm = ffc;
        return LS_RETRY;
    }
};

}  // namespace nk
