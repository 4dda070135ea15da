// bratu3d_newton.cpp -- a C++ caller of libnkhip.so through the public C ABI only (include/nkhip.h):
// 3D Bratu (NK_BRATU3D) on an NX x NY x NZ grid of the unit cube, u0 = sin(pi x) sin(pi y) sin(pi z),
// newton_krylov! with GMRES(memory) and the Eisenstat-Walker forcing (src/Ariadne.jl:288-372), FD or exact Jv.
// Prints one JSON line, the one bratu2d_newton prints (with "ny" and "nz" when they are given).
//
//   bin/bratu3d_newton [NX=64] [NY NZ] [jv=fd|exact] [memory=30] [restart=1] [--lambda L] [--mg] [--mg-semi] [--cg] [--minres] [--linesearch]
// --linesearch: backtracking on the Newton step (NK_LINESEARCH_BACKTRACK); the JSON line then carries "linesearch",
// "n_backtrack", "ls_failed" and "steps" (the accepted step lengths).
// NY NZ (two numbers right after NX): an NX x NY x NZ grid, h_a = 1 / (n_a + 1); without them NX^3.
// --lambda L: Bratu's λ (default 3.51382, examples/bratu.jl:42; the 3D fold is near 9.9).
// --mg (anywhere on the line): the geometric multigrid V-cycle as the right preconditioner N (NK_PRECOND_MG).
// --mg-semi (implies --mg): the hierarchy on the semicoarsened plan (nk_mg_plan_semi / nk_mg_create_levels), for
// unequal extents.  The JSON line then carries "coarsening": "semi".
// --cg / --minres: Newton-CG / Newton-MINRES instead of GMRES; with --mg the V-cycle in its SPD form
// (nk_mg_set_spd) is their M.  The JSON line then carries "algo".
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

static bool digits(const char* s) { return s[0] != '\0' && std::strspn(s, "0123456789") == std::strlen(s); }

int main(int argc, char** argv) {
    bool use_mg = false, use_cg = false, use_minres = false, semi = false, linesearch = false;
    double lambda = 3.51382;  // examples/bratu.jl:42
    int nargs = 1;
    for (int i = 1; i < argc; ++i) {  // strip the options, keep the positional arguments
        if (std::strcmp(argv[i], "--mg") == 0) use_mg = true;
        else if (std::strcmp(argv[i], "--mg-semi") == 0) use_mg = semi = true;
        else if (std::strcmp(argv[i], "--cg") == 0) use_cg = true;
        else if (std::strcmp(argv[i], "--minres") == 0) use_minres = true;
        else if (std::strcmp(argv[i], "--linesearch") == 0) linesearch = true;
        else if (std::strcmp(argv[i], "--lambda") == 0 && i + 1 < argc) lambda = std::atof(argv[++i]);
        else argv[nargs++] = argv[i];
    }
    argc = nargs;
    if (use_cg && use_minres) {  // (every option is checked before the context exists: nothing to release on these paths)
        std::fprintf(stderr, "--cg and --minres exclude each other\n");
        return 1;
    }
    const int64_t NX = argc > 1 ? std::atoll(argv[1]) : 64;
    // the other two extents: two positional arguments of digits only right after NX (the jv mode is a word)
    const bool has_yz = argc > 3 && digits(argv[2]) && digits(argv[3]);
    const int64_t NY = has_yz ? std::atoll(argv[2]) : NX, NZ = has_yz ? std::atoll(argv[3]) : NX;
    if (has_yz) {
        for (int i = 2; i + 2 < argc; ++i) argv[i] = argv[i + 2];
        argc -= 2;
    }
    if (NX < 1 || NY < 1 || NZ < 1) {
        std::fprintf(stderr, "grid extents must be >= 1\n");
        return 1;
    }
    const bool fd = argc > 2 ? std::strcmp(argv[2], "exact") != 0 : true;
    const int memory = argc > 3 ? std::atoi(argv[3]) : 30;
    const int restart = argc > 4 ? std::atoi(argv[4]) : 1;
    const double hx = 1.0 / (double)(NX + 1), hy = 1.0 / (double)(NY + 1), hz = 1.0 / (double)(NZ + 1);

    // the semicoarsened plan is host code: made (and refused) before anything is allocated
    int64_t ext[3 * 32];
    int32_t nl = 0;
    if (semi) {  // k = 1 on the three axes: the plan follows the spacings
        const int64_t n3[3] = {NX, NY, NZ};
        const double h3[3] = {hx, hy, hz};
        if (nk_mg_plan_semi(n3, h3, nullptr, 0.0, 0, ext, 32, &nl) != NK_OK) {
            std::fprintf(stderr, "nk_mg_plan_semi: invalid argument\n");
            return 1;
        }
    }
    nk_ctx* ctx = nullptr;
    if (nk_ctx_create(0, &ctx) != NK_OK) {
        std::fprintf(stderr, "no usable GPU\n");
        return 1;
    }
    nk_problem p{};
    p.kind = NK_BRATU3D;
    p.bc = NK_BC_ZERO;
    p.nx = NX;
    p.ny = NY;
    p.nz = NZ;
    p.hx = hx;
    p.hy = hy;
    p.hz = hz;
    p.lambda = lambda;
    double *u = nullptr, *res = nullptr;
    CHECK(ctx, nk_vec_alloc(ctx, &p, &u));
    CHECK(ctx, nk_vec_alloc(ctx, &p, &res));
    const int64_t n = NX * NY * NZ;
    std::vector<double> host((size_t)n);
    for (int64_t k = 0; k < NZ; ++k)
        for (int64_t j = 0; j < NY; ++j)
            for (int64_t i = 0; i < NX; ++i)
                host[(size_t)((k * NY + j) * NX + i)] =
                    std::sin(M_PI * (i + 1) * hx) * std::sin(M_PI * (j + 1) * hy) * std::sin(M_PI * (k + 1) * hz);
    CHECK(ctx, nk_memcpy_h2d(ctx, u, host.data(), n));

    nk_newton_opts o;
    CHECK(ctx, nk_newton_defaults(&o));
    o.memory = memory;
    o.krylov.restart = restart;
    o.krylov.jv_mode = fd ? NK_JV_FD : NK_JV_EXACT;
    const bool sym = use_cg || use_minres;  // the short recurrences: M (SPD) instead of N
    if (sym) {
        o.algo = use_cg ? NK_ALGO_CG : NK_ALGO_MINRES;
        o.krylov.restart = 0;  // a GMRES keyword
    }
    nk_mg* mg = nullptr;
    nk_precond Nmg{};
    if (use_mg) {
        if (semi) {
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
    nk_newton_stats st;
    double hist[64];
    int64_t nh = 0;
    const auto t0 = std::chrono::steady_clock::now();
    CHECK(ctx, nk_newton_krylov(ctx, &p, u, res, &o, &st, hist, 64, &nh));
    CHECK(ctx, nk_sync(ctx));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    CHECK(ctx, nk_memcpy_d2h(ctx, host.data(), u, n));
    double umax = 0.0;
    for (double v : host) umax = std::fmax(umax, std::fabs(v));
    char yz_field[96] = "";
    if (has_yz) std::snprintf(yz_field, sizeof yz_field, "\"ny\": %lld, \"nz\": %lld, ", (long long)NY, (long long)NZ);
    std::printf("{\"N\": %lld, %s\"jv\": \"%s\", %s%s%s\"solved\": %s, \"outer\": %lld, \"inner\": %lld, \"n_matvec\": %lld, "
                "\"n_res\": %.17g, \"tol\": %.17g, \"u_max\": %.17g, \"seconds\": %.6f, \"n_res_history\": [",
                (long long)NX, yz_field, fd ? "fd" : "exact", use_mg ? "\"mg\": true, " : "",
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
