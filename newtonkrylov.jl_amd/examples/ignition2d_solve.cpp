// ignition2d_solve.cpp -- a C++ caller of libnkhip.so through the public C ABI only (include/nkhip.h):
// the solid-fuel-ignition problem u_t = a Δu + λ exp(u) on an NX x NY grid of the unit square, u0 = 0, zero Dirichlet
// ghosts, stepped with the time loop of examples/implicit.jl:54-78 -- one newton_krylov! per step with tol_abs = 6e-6,
// marching on when a step fails, u_n .= u after each step -- over the fused residuals NK_IGNITION2D_EULER / _MIDPOINT /
// _TRAPEZOID.  Below the fold (λ ≈ 6.8 on the unit square) the state relaxes to the steady Bratu solution; above it the
// solution blows up in finite time and the steps stop being solved.
//
//   bin/ignition2d_solve NX [NY] [euler|midpoint|trapezoid] [--lambda L] [--a A] [--dt DT] [--steps K] [--alpha AL] [--mg] [--fd]
//                       [--linesearch]
// --linesearch: backtracking on every Newton step (NK_LINESEARCH_BACKTRACK); each step's line then ends with
// " backtracks B ls_failed F".
// One line per step: step, Newton steps, Krylov steps, ||F||, max u, solved.  The exit status is 0 even when a step
// is not solved (the reference warns and marches on); non-zero only when a library call fails.
// --mg: the geometric multigrid V-cycle as the right preconditioner N, refreshed from J(u) in every Newton step.
// --fd: the finite-difference Jv instead of the exact tangent.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nkhip.h"

#define CHECK(ctx, call)                                                                  \
    do {                                                                                  \
        int rc_ = (call);                                                                 \
        if (rc_ != NK_OK) {                                                               \
            std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, nk_last_error(ctx)); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static bool digits(const char* s) { return s[0] != '\0' && std::strspn(s, "0123456789") == std::strlen(s); }

int main(int argc, char** argv) {
    bool use_mg = false, fd = false, linesearch = false;
    double lambda = 3.51382, a = 1.0, dt = 0.05, alpha = 0.5;
    int steps = 10, nargs = 1;
    for (int i = 1; i < argc; ++i) {  // strip the options, keep the positional arguments
        if (std::strcmp(argv[i], "--mg") == 0) use_mg = true;
        else if (std::strcmp(argv[i], "--fd") == 0) fd = true;
        else if (std::strcmp(argv[i], "--linesearch") == 0) linesearch = true;
        else if (std::strcmp(argv[i], "--lambda") == 0 && i + 1 < argc) lambda = std::atof(argv[++i]);
        else if (std::strcmp(argv[i], "--a") == 0 && i + 1 < argc) a = std::atof(argv[++i]);
        else if (std::strcmp(argv[i], "--dt") == 0 && i + 1 < argc) dt = std::atof(argv[++i]);
        else if (std::strcmp(argv[i], "--alpha") == 0 && i + 1 < argc) alpha = std::atof(argv[++i]);
        else if (std::strcmp(argv[i], "--steps") == 0 && i + 1 < argc) steps = std::atoi(argv[++i]);
        else argv[nargs++] = argv[i];
    }
    argc = nargs;
    if (argc < 2 || !digits(argv[1])) {
        std::fprintf(stderr, "usage: ignition2d_solve NX [NY] [euler|midpoint|trapezoid] [--lambda L] [--a A] [--dt DT] "
                             "[--steps K] [--alpha AL] [--mg] [--fd]\n");
        return 1;
    }
    const int64_t NX = std::atoll(argv[1]);
    const bool has_y = argc > 2 && digits(argv[2]);
    const int64_t NY = has_y ? std::atoll(argv[2]) : NX;
    const char* scheme = argc > (has_y ? 3 : 2) ? argv[has_y ? 3 : 2] : "euler";
    int kind = 0;
    if (std::strcmp(scheme, "euler") == 0) kind = NK_IGNITION2D_EULER;
    else if (std::strcmp(scheme, "midpoint") == 0) kind = NK_IGNITION2D_MIDPOINT;
    else if (std::strcmp(scheme, "trapezoid") == 0) kind = NK_IGNITION2D_TRAPEZOID;
    if (!kind || NX < 1 || NY < 1 || steps < 0 || !(dt > 0.0)) {
        std::fprintf(stderr, "scheme must be euler, midpoint or trapezoid; extents >= 1, steps >= 0, dt > 0\n");
        return 1;
    }
    nk_ctx* ctx = nullptr;
    if (nk_ctx_create(0, &ctx) != NK_OK) {
        std::fprintf(stderr, "no usable GPU\n");
        return 1;
    }
    nk_problem p{};
    p.kind = kind;
    p.bc = NK_BC_ZERO;
    p.nx = NX;
    p.ny = NY;
    p.nz = 1;
    p.hx = 1.0 / (double)(NX + 1);
    p.hy = 1.0 / (double)(NY + 1);
    p.hz = 1.0;
    p.lambda = lambda;
    p.a = a;
    p.dt = dt;
    p.alpha = alpha;
    // grid functions depend on the grid alone: allocated through a kind that carries no u_n (p needs un itself)
    nk_problem grid = p;
    grid.kind = NK_BRATU2D;
    double *u = nullptr, *un = nullptr, *res = nullptr;
    CHECK(ctx, nk_vec_alloc(ctx, &grid, &u));
    CHECK(ctx, nk_vec_alloc(ctx, &grid, &un));
    CHECK(ctx, nk_vec_alloc(ctx, &grid, &res));
    p.un = un;
    const int64_t n = NX * NY;
    std::vector<double> host((size_t)n, 0.0);  // u0 = 0
    CHECK(ctx, nk_memcpy_h2d(ctx, u, host.data(), n));
    CHECK(ctx, nk_memcpy_h2d(ctx, un, host.data(), n));

    nk_newton_opts o;
    CHECK(ctx, nk_newton_defaults(&o));
    o.tol_abs = 6.0e-6;  // implicit.jl:61
    o.krylov.jv_mode = fd ? NK_JV_FD : NK_JV_EXACT;
    if (linesearch) o.linesearch = NK_LINESEARCH_BACKTRACK;
    nk_mg* mg = nullptr;
    nk_precond Nmg{};
    if (use_mg) {
        CHECK(ctx, nk_mg_create(ctx, &p, nullptr, &mg));  // the Newton loop refreshes it from each step's u
        Nmg.kind = NK_PRECOND_MG;
        Nmg.data = mg;
        o.krylov.N = &Nmg;
    }
    int unsolved = 0;
    for (int k = 1; k <= steps; ++k) {
        nk_newton_stats st;
        CHECK(ctx, nk_newton_krylov(ctx, &p, u, res, &o, &st, nullptr, 0, nullptr));
        CHECK(ctx, nk_memcpy_d2h(ctx, host.data(), u, n));
        double umax = -INFINITY;
        for (double v : host) umax = (v > umax || std::isnan(v)) ? v : umax;
        if (!st.solved) {
            ++unsolved;
            std::fprintf(stderr, "non linear solve failed marching on t=%.17g\n", k * dt);
        }
        std::printf("step %d newton %lld krylov %lld n_res %.6e u_max %.6e solved %d", k, (long long)st.outer_iterations,
                    (long long)st.inner_iterations, st.n_res, umax, st.solved ? 1 : 0);
        if (linesearch) std::printf(" backtracks %lld ls_failed %d", (long long)st.n_backtrack, (int)st.ls_failed);
        std::printf("\n");
        CHECK(ctx, nk_memcpy_h2d(ctx, un, host.data(), n));  // u_n .= u
    }
    if (unsolved) std::fprintf(stderr, "%d of %d steps not solved\n", unsolved, steps);
    if (mg) CHECK(ctx, nk_mg_destroy(mg));
    CHECK(ctx, nk_vec_free(ctx, u));
    CHECK(ctx, nk_vec_free(ctx, un));
    CHECK(ctx, nk_vec_free(ctx, res));
    nk_ctx_destroy(ctx);
    return 0;
}
