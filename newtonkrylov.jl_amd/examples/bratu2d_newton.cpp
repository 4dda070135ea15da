// bratu2d_newton.cpp -- a C++ caller of libnkhip.so through the public C ABI only (include/nkhip.h):
// 2D Bratu on an N x N grid, u0 = sin(pi x) sin(pi y), newton_krylov! with GMRES(memory) and the
// Eisenstat-Walker forcing (src/Ariadne.jl:288-372), FD or exact Jv.  Prints one JSON line.
//
//   bin/bratu2d_newton [N=256] [NY] [jv=fd|exact] [memory=30] [restart=1] [--mg] [--mg-semi] [--cg] [--minres]
//                      [--linesearch] [--lambda L] [--amp A] [--no-forcing]
// --linesearch: backtracking on the Newton step (NK_LINESEARCH_BACKTRACK); the JSON line then carries "linesearch",
// "n_backtrack", "ls_failed" and "steps" (the accepted step lengths).  --lambda L: Bratu's λ (default 3.51382);
// --amp A: u0 = A sin sin (default 1); --no-forcing: Krylov's own rtol instead of Eisenstat-Walker -- together a
// start from which the full step overshoots (e.g. 24 20 exact 480 --lambda 1 --amp 5 --no-forcing --linesearch).
// NY (a number right after N): an N x NY grid on the unit square (h_x != h_y); the JSON line then carries "ny".
// --mg (anywhere on the line): the geometric multigrid V-cycle as the right preconditioner N (NK_PRECOND_MG).
// --mg-semi (implies --mg): the hierarchy on the semicoarsened plan (nk_mg_plan_semi / nk_mg_create_levels), for
// N != NY.  The JSON line then carries "coarsening": "semi".
// --cg: Newton-CG (examples/bratu.jl:59-63's algo = :cg) instead of GMRES; with --mg the V-cycle in its SPD form
// (nk_mg_set_spd) is CG's M.  The JSON line then carries "algo": "cg".
// --minres: Newton-MINRES (NK_ALGO_MINRES) instead of GMRES; with --mg the SPD V-cycle is its M, as for --cg.  The JSON
// line then carries "algo": "minres".
#include <chrono>
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

int main(int argc, char** argv) {
    bool use_mg = false, use_cg = false, use_minres = false, semi = false, linesearch = false, no_forcing = false;
    double lambda = 3.51382, amp = 1.0;  // examples/bratu.jl:41-42
    int nargs = 1;
    for (int i = 1; i < argc; ++i) {  // strip --mg / --mg-semi / --cg / --minres, keep the positional arguments
        if (std::strcmp(argv[i], "--mg") == 0) use_mg = true;
        else if (std::strcmp(argv[i], "--mg-semi") == 0) use_mg = semi = true;
        else if (std::strcmp(argv[i], "--cg") == 0) use_cg = true;
        else if (std::strcmp(argv[i], "--minres") == 0) use_minres = true;
        else if (std::strcmp(argv[i], "--linesearch") == 0) linesearch = true;
        else if (std::strcmp(argv[i], "--no-forcing") == 0) no_forcing = true;
        else if (std::strcmp(argv[i], "--lambda") == 0 && i + 1 < argc) lambda = std::atof(argv[++i]);
        else if (std::strcmp(argv[i], "--amp") == 0 && i + 1 < argc) amp = std::atof(argv[++i]);
        else argv[nargs++] = argv[i];
    }
    argc = nargs;
    const int64_t N = argc > 1 ? std::atoll(argv[1]) : 256;
    // a second grid size: a positional argument of digits only right after N (the jv mode is a word)
    const bool has_ny = argc > 2 && argv[2][0] != '\0' && std::strspn(argv[2], "0123456789") == std::strlen(argv[2]);
    const int64_t NY = has_ny ? std::atoll(argv[2]) : N;
    if (has_ny) {
        for (int i = 2; i + 1 < argc; ++i) argv[i] = argv[i + 1];
        --argc;
    }
    const bool fd = argc > 2 ? std::strcmp(argv[2], "exact") != 0 : true;
    const int memory = argc > 3 ? std::atoi(argv[3]) : 30;
    const int restart = argc > 4 ? std::atoi(argv[4]) : 1;
    const double h = 1.0 / (double)(N + 1), hy = 1.0 / (double)(NY + 1);

    nk_ctx* ctx = nullptr;
    if (nk_ctx_create(0, &ctx) != NK_OK) {
        std::fprintf(stderr, "no usable GPU\n");
        return 1;
    }
    nk_problem p{};
    p.kind = NK_BRATU2D;
    p.bc = NK_BC_ZERO;
    p.nx = N;
    p.ny = NY;
    p.nz = 1;
    p.hx = h;
    p.hy = hy;
    p.hz = 1.0;
    p.lambda = lambda;
    double *u = nullptr, *res = nullptr;
    CHECK(ctx, nk_vec_alloc(ctx, &p, &u));
    CHECK(ctx, nk_vec_alloc(ctx, &p, &res));
    std::vector<double> host((size_t)(N * NY));
    for (int64_t j = 0; j < NY; ++j)
        for (int64_t i = 0; i < N; ++i) host[(size_t)(j * N + i)] = amp * (std::sin(M_PI * (i + 1) * h) * std::sin(M_PI * (j + 1) * hy));
    CHECK(ctx, nk_memcpy_h2d(ctx, u, host.data(), N * NY));

    nk_newton_opts o;
    CHECK(ctx, nk_newton_defaults(&o));
    o.memory = memory;
    o.krylov.restart = restart;
    o.krylov.jv_mode = fd ? NK_JV_FD : NK_JV_EXACT;
    if (use_cg && use_minres) {
        std::fprintf(stderr, "--cg and --minres exclude each other\n");
        return 1;
    }
    const bool sym = use_cg || use_minres;  // the short recurrences: M (SPD) instead of N
    if (sym) {
        o.algo = use_cg ? NK_ALGO_CG : NK_ALGO_MINRES;
        o.krylov.restart = 0;  // a GMRES keyword
    }
    nk_mg* mg = nullptr;
    nk_precond Nmg{};
    if (use_mg) {
        if (semi) {  // k = 1 on both axes: the plan follows the spacings
            const int64_t n3[3] = {N, NY, 1};
            const double h3[3] = {h, hy, 1.0};
            int64_t ext[3 * 32];
            int32_t nl = 0;
            if (nk_mg_plan_semi(n3, h3, nullptr, 0.0, 0, ext, 32, &nl) != NK_OK) {
                std::fprintf(stderr, "nk_mg_plan_semi: invalid argument\n");
                return 1;
            }
            CHECK(ctx, nk_mg_create_levels(ctx, &p, nullptr, ext, nl, &mg));
        } else {
            CHECK(ctx, nk_mg_create(ctx, &p, nullptr, &mg));  // the Newton loop refreshes it from each step's u
        }
        Nmg.kind = NK_PRECOND_MG;
        Nmg.data = mg;
        if (sym) {
            CHECK(ctx, nk_mg_set_spd(mg, 1));  // CG's / MINRES's M must be SPD: sigma V, sigma = the sign of J's diagonal
            o.krylov.M = &Nmg;
        } else {
            o.krylov.N = &Nmg;
        }
    }
    double steps[64];
    if (linesearch) {
        o.linesearch = NK_LINESEARCH_BACKTRACK;
        o.ls_hist = steps;
        o.ls_hist_cap = 64;
    }
    if (no_forcing) o.forcing = NK_FORCING_NONE;
    nk_newton_stats st;
    double hist[64];
    int64_t nh = 0;
    const auto t0 = std::chrono::steady_clock::now();
    CHECK(ctx, nk_newton_krylov(ctx, &p, u, res, &o, &st, hist, 64, &nh));
    CHECK(ctx, nk_sync(ctx));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    CHECK(ctx, nk_memcpy_d2h(ctx, host.data(), u, N * NY));
    double umax = 0.0;
    for (double v : host) umax = std::fmax(umax, std::fabs(v));
    char ny_field[48] = "";
    if (has_ny) std::snprintf(ny_field, sizeof ny_field, "\"ny\": %lld, ", (long long)NY);
    std::printf("{\"N\": %lld, %s\"jv\": \"%s\", %s%s%s\"solved\": %s, \"outer\": %lld, \"inner\": %lld, \"n_matvec\": %lld, "
                "\"n_res\": %.17g, \"tol\": %.17g, \"u_max\": %.17g, \"seconds\": %.6f, \"n_res_history\": [",
                (long long)N, ny_field, fd ? "fd" : "exact", use_mg ? "\"mg\": true, " : "",
                semi ? "\"coarsening\": \"semi\", " : "", use_cg ? "\"algo\": \"cg\", " : (use_minres ? "\"algo\": \"minres\", " : ""),
                st.solved ? "true" : "false", (long long)st.outer_iterations,
                (long long)st.inner_iterations, (long long)st.n_matvec, st.n_res, st.tol, umax, secs);
    for (int64_t k = 0; k < nh && k < 64; ++k) std::printf("%s%.17g", k ? ", " : "", hist[k]);
    std::printf("]");
    if (linesearch) {
        std::printf(", \"linesearch\": true, \"n_backtrack\": %lld, \"ls_failed\": %s, \"steps\": [", (long long)st.n_backtrack,
                    st.ls_failed ? "true" : "false");
        for (int64_t k = 0; k < st.outer_iterations && k < 64; ++k) std::printf("%s%.17g", k ? ", " : "", steps[k]);
        std::printf("]");
    }
    std::printf("}\n");
    if (mg) CHECK(ctx, nk_mg_destroy(mg));
    CHECK(ctx, nk_vec_free(ctx, u));
    CHECK(ctx, nk_vec_free(ctx, res));
    nk_ctx_destroy(ctx);
    return 0;
}
