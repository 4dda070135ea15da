// nk_krylov.cpp -- device-resident Krylov.jl 0.10 gmres!/fgmres!/cg! for the Jacobian operator, with
// Krylov.jl's right (N) and left (M) preconditioners, and MINRES (minres()) for the symmetric J.
//
// Restates krylov_workspace(algo, KrylovConstructor(res)) + krylov_solve!(workspace, J, b; kwargs)
// as called by Ariadne (src/Ariadne.jl:317-318, :338, :340, :367) -- SURVEY.md Appendix A.
// Krylov.jl itself is third-party and absent from /root/reference; the same restatement lives in
// oracle/nk_oracle.c (oc_gmres / oc_cg) and the tests check this driver against it.
//
// What moves to the device compared with Krylov.jl's generic loop:
//  * the Arnoldi basis V, q (= w), x, and every reduction;
//  * each Arnoldi step is: one fused Jv kernel (also emits the partials of <V_1, q>), k fused
//    MGS passes (q -= h_i V_i and partials of <V_{i+1}, q>; the last pass emits ||q||^2 partials),
//    one 64-thread finaliser, ONE device->host copy of the Hessenberg column and one sync.
//    Krylov.jl's schedule would sync 2k+1 times (every kdot/knorm returns a host scalar).
//  * the per-cycle kfill!(V[i], 0) of Krylov.jl is dropped: every V[i] read in a cycle is
//    overwritten first, so the zeroing is dead work (no observable difference).
// The Givens rotations, the least-squares back-substitution and all stopping tests run on the
// host on the same scalars, in the same order as Krylov.jl: nk_lsq.hpp, which needs no device.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "nk_internal.hpp"
#include "nk_lsq.hpp"

struct nk_workspace {
    nk_ctx* c = nullptr;
    int algo = NK_ALGO_GMRES;
    nk_problem prob{};
    int mem = 20;
    int64_t n = 0;
    double* x = nullptr;
    double* w = nullptr;   // gmres: q (= w) of odd steps / restart residual; cg: Ap
    double* w2 = nullptr;  // gmres: q of even steps (the fused Jv reads q_{k-1} while writing q_k)
    double* xr = nullptr;  // gmres restart: Δx (chunked x update);  cg: r
    double* p = nullptr;   // cg: search direction
    double* mv[4] = {nullptr, nullptr, nullptr, nullptr};  // minres: r2, v, w1, w2 (x = x, w = J v, xr = r1)
    std::vector<double*> V;
    std::vector<double*> Z;  // flexible form: Z_k = N V_k (right preconditioner)
    double* mr = nullptr;    // left preconditioner: r0 = M w (gmres) / z = M r (cg) / y = M r2 (minres)
    double* mw = nullptr;    // left preconditioner: w = A N V_k before q = M w (gmres)
    double* hdev = nullptr;  // device Hessenberg columns: 2 slots of (2*cap + 2) doubles (steps k, k+1 in flight)
    double* ydev = nullptr;  // device y (cap doubles)
    double* bdev = nullptr;  // device divisor of V_1 = r0 / rNorm (fused into step 1)
    bool u_fused = false;    // the last solve applied opts.u_update inside its final x update
    double* hpin = nullptr;  // pinned host mirror of hdev (2 slots), written by the kernels themselves
    double* hpin_dev = nullptr;  // hpin's device address
    double* ypin = nullptr;  // pinned host y
    hipEvent_t col_ready[2] = {nullptr, nullptr};  // Hessenberg column of slot s has landed in hpin
    int cap = 0;             // capacity of hdev / ydev / pinned buffers (in basis vectors)
};

namespace nk {
namespace {

// Grow the Hessenberg/y buffers to hold `need` basis vectors.  Contents are preserved: with the
// one-step-ahead pipeline a column may still be waiting to be read when the basis grows.
int ws_scalars(nk_workspace* ws, int need) {
    if (need <= ws->cap) return NK_OK;
    nk_ctx* c = ws->c;
    int cap = ws->cap ? ws->cap : 64;
    while (cap < need) cap *= 2;
    NK_HIP(c, hipStreamSynchronize(c->stream));
    const size_t ostride = 2 * (size_t)ws->cap + 2, nstride = 2 * (size_t)cap + 2;
    double *hdev = nullptr, *ydev = nullptr, *hpin = nullptr, *ypin = nullptr;
    NK_HIP(c, hipMalloc(&hdev, sizeof(double) * 2 * nstride));
    NK_HIP(c, hipMalloc(&ydev, sizeof(double) * (size_t)cap));
    // fine-grained (coherent) so the kernels' stores are host-visible once the step's event fires
    NK_HIP(c, hipHostMalloc(&hpin, sizeof(double) * 2 * nstride, hipHostMallocMapped | hipHostMallocCoherent));
    NK_HIP(c, hipHostMalloc(&ypin, sizeof(double) * (size_t)cap, hipHostMallocDefault));
    if (ws->cap) {
        for (int slot = 0; slot < 2; ++slot) {
            NK_HIP(c, hipMemcpy(hdev + slot * nstride, ws->hdev + slot * ostride, sizeof(double) * ostride,
                                hipMemcpyDeviceToDevice));
            std::memcpy(hpin + slot * nstride, ws->hpin + slot * ostride, sizeof(double) * ostride);
        }
        (void)hipFree(ws->hdev);
        (void)hipFree(ws->ydev);
        (void)hipHostFree(ws->hpin);
        (void)hipHostFree(ws->ypin);
    }
    ws->hdev = hdev;
    ws->ydev = ydev;
    ws->hpin = hpin;
    ws->ypin = ypin;
    NK_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&ws->hpin_dev), hpin, 0));
    ws->cap = cap;
    return NK_OK;
}

int ws_basis(nk_workspace* ws, int need) {
    while ((int)ws->V.size() < need) {
        double* v = nullptr;
        NK_TRY(nk_vec_alloc(ws->c, &ws->prob, &v));
        ws->V.push_back(v);
    }
    return NK_OK;
}

// a lazily allocated workspace vector (the left preconditioner's buffers)
int ws_vec(nk_workspace* ws, double** v) {
    if (!*v) NK_TRY(nk_vec_alloc(ws->c, &ws->prob, v));
    return NK_OK;
}

int ws_zbasis(nk_workspace* ws, int need) {
    while ((int)ws->Z.size() < need) {
        double* v = nullptr;
        NK_TRY(nk_vec_alloc(ws->c, &ws->prob, &v));
        ws->Z.push_back(v);
    }
    return NK_OK;
}

// NK_MGS_RESIDENT=0 (operational) runs one k_mgs_pass launch per MGS pass instead
// of the resident sweep, which needs every CU of the device at once: for a GPU shared with unrelated
// work.  kbench knobs: NK_MGS_ALT=1 alternates the sweep direction of consecutive MGS passes (see
// k_mgs_pass); NK_RES_JV=1 computes the 2D Bratu FD Jv inside the resident sweep's launch (slower,
// DESIGN.md §4)
const int mgs_alt = NK_TUNE("NK_MGS_ALT", 0);
const int mgs_resident = env_cfg("NK_MGS_RESIDENT", 1);
const int mgs_fused_jv = NK_TUNE("NK_RES_JV", 0);

// the residual history a caller asked for: every value counts, the first `cap` are kept
struct Hist {
    double* v;
    int64_t cap;
    int64_t n;
    void push(double r) {
        if (v && n < cap) v[n] = r;
        ++n;
    }
    void close(int64_t* len) const {
        if (len) *len = n;
    }
};

// a solver's exit.  status: 1 solved, 2 tired, 3 breakdown, 4 zero curvature
int finish(nk_krylov_stats* st, int64_t niter, bool solved, bool inconsistent, bool breakdown, int status) {
    st->niter = niter;
    st->solved = solved;
    st->inconsistent = inconsistent;
    st->breakdown = breakdown;
    st->status = status;
    return NK_OK;
}
// b = 0 (<r, M r> = 0): x = 0 solves it, no iteration
int finish_at_zero(nk_krylov_stats* st) { return finish(st, 0, true, false, false, 1); }

// the preconditioner a solve applies: null for none (Krylov.jl's I)
const nk_precond* active(const nk_precond* P) { return (P && P->kind != NK_PRECOND_NONE) ? P : nullptr; }

// *mg = the hierarchy of a multigrid preconditioner (null: P is none, or of another kind)
int mg_of(nk_ctx* c, const nk_precond* P, nk_mg** mg) {
    *mg = nullptr;
    if (!P || P->kind != NK_PRECOND_MG) return NK_OK;
    if (!P->data) return fail(c, NK_E_ARG, "multigrid preconditioner without its hierarchy (nk_mg_create)");
    *mg = static_cast<nk_mg*>(P->data);
    return NK_OK;
}

struct Op;
int gmres(nk_workspace* ws, const nk_problem* p, Op& A, const double* b, const nk_krylov_opts* o, nk_krylov_stats* st,
          Hist& hist);

struct Op {
    nk_ctx* c;
    const nk_problem* p;
    int mode;  // NK_JV_*
    const double* u;
    const double* F0;
    double unorm;
    int64_t n_matvec = 0;
    bool f0r = false;  // F0 is this library's F(u): the 2D FD stencils recompute it instead of loading it

    // out = J v  (+ epilogue).  vnorm: ||v|| for the FD step (1 for Arnoldi basis vectors).
    // With vdiv/vout the operator is applied to v / *vdiv, which is also stored to vout.
    int apply(double* out, const double* v, double vnorm, int epi, const double* aux, Red* red,
              const double* vdiv = nullptr, double* vout = nullptr) {
        ++n_matvec;
        double eps = 0.0;
        if (mode == NK_JV_FD) {
            if (vnorm == 0.0) {  // J 0 = 0
                NK_TRY(launch_fill(c, ws_n(), out, 0.0));
                if (epi == EPI_RESID) NK_TRY(launch_copy(c, ws_n(), out, aux));
                if (epi != EPI_NONE) {
                    if (epi == EPI_DOT) return launch_dot(c, ws_n(), aux, out, red);
                    return launch_sumsq(c, ws_n(), out, red);
                }
                return NK_OK;
            }
            eps = fd_eps(vnorm);
        }
        StencilIn in{p, mode == NK_JV_FD ? MODE_JFD : MODE_JEXACT, epi, out, u, v, F0, aux, eps, vdiv, vout};
        in.xchg_v = true;  // v's ghost planes: exchanged by the stencil launch itself where it can
        in.f0r = f0r;
        return launch_stencil(c, in, red);
    }
    int64_t ws_n() const { return p->nx * p->ny * p->nz; }
    double fd_eps(double vnorm) const { return std::sqrt(DBL_EPSILON) * std::fmax(1.0, unorm) / vnorm; }
};

// z = N v (right preconditioner); *znorm = ||z|| when the FD operator needs it.
//   DIAG   z = d .* v (Jacobi)
//   USER   the caller's device callback
//   GMRES  sol, _ = gmres(J, v; itmax); copyto!(z, sol) -- the GmresPreconditioner of
//          examples/bratu.jl:139-157: Krylov.jl's gmres defaults (memory 20, no restart,
//          atol = rtol = √eps, x0 = 0) on the same operator, in the preconditioner's own workspace
//   MG     one multigrid V-cycle (nk_mg.hip): kernels on the context's stream only, no host sync
int apply_precond(nk_ctx* c, const nk_problem* p, const nk_precond* N, Op& A, int64_t n, double* z, const double* v,
                  bool need_norm, double* znorm) {
    Red rz{};
    if (N->kind == NK_PRECOND_DIAG) {
        if (!N->diag) return fail(c, NK_E_ARG, "diagonal preconditioner without its diagonal");
        NK_TRY(launch_diag_apply(c, n, z, N->diag, v, need_norm ? &rz : nullptr));
    } else if (N->kind == NK_PRECOND_USER) {
        if (!N->apply) return fail(c, NK_E_ARG, "user preconditioner without its apply callback");
        NK_TRY(halo_exchange(c, p, v));
        int rc = 0;
        NK_TRY(launch(c, "precond_user", 0.0, [&] { rc = N->apply(N->data, c, z, v); }));
        if (rc != 0) return fail(c, NK_E_USER, "user preconditioner callback returned " + std::to_string(rc));
        if (need_norm) NK_TRY(launch_sumsq(c, n, z, &rz));
    } else if (N->kind == NK_PRECOND_ILU0) {
        if (!N->diag) return fail(c, NK_E_ARG, "ILU(0) preconditioner without its factor (nk_ilu0_factor)");
        Geo g;
        NK_TRY(geometry(c, p, &g));
        NK_TRY(launch_ilu0_solve(c, p, g.dim, N->diag, z, v));
        if (need_norm) NK_TRY(launch_sumsq(c, n, z, &rz));
    } else if (N->kind == NK_PRECOND_GMRES) {
        if (!N->inner || N->inner->algo != NK_ALGO_GMRES || N->inner->n != n)
            return fail(c, NK_E_ARG, "GMRES preconditioner needs a GMRES workspace of the problem's size");
        nk_krylov_opts io{};
        io.itmax = N->itmax;
        io.jv_mode = A.mode;
        io.atol = io.rtol = std::sqrt(DBL_EPSILON);
        nk_krylov_stats is{};
        Hist none{nullptr, 0, 0};
        NK_TRY(gmres(N->inner, p, A, v, &io, &is, none));
        NK_TRY(launch_copy(c, n, z, N->inner->x));
        if (need_norm) NK_TRY(launch_sumsq(c, n, z, &rz));
    } else if (N->kind == NK_PRECOND_MG) {
        nk_mg* mg = nullptr;
        NK_TRY(mg_of(c, N, &mg));
        NK_TRY(nk_mg_apply(mg, z, v));
        if (need_norm) NK_TRY(launch_sumsq(c, n, z, &rz));
    } else {
        return fail(c, NK_E_ARG, "unknown preconditioner kind");
    }
    if (need_norm) NK_TRY(host_scalar(c, rz, 1, znorm));
    return NK_OK;
}

// One GMRES solve's Arnoldi process on the device: issues step k (its kernels and the mirror of its
// Hessenberg column into pinned memory) without waiting, and applies the cycle's y to x.
// Step 1 applies J to r0 / rNorm and stores V_1; step k >= 2 applies J to q_{k-1} / h_{k,k-1},
// reading h from the device and storing V_k on the way (fused kdivcopy!).
struct Arnoldi {
    nk_workspace* ws;
    const nk_problem* p;
    Op& A;
    const nk_krylov_opts* o;
    nk_ctx* c;
    const int64_t n;
    double* W[2];  // q_k lives in W[k & 1]
    // right preconditioner, without the one-step-ahead issue (the FD step size needs ||N V_k|| on
    // the host): fgmres! stores Z_k = N V_k and updates x += Z y; gmres! applies N to p = N V_k
    // only for the product and updates x += N (V y) (Krylov.jl 0.10 gmres! / fgmres!)
    const nk_precond* N;
    // left preconditioner M (ldiv = false): r0 = M (b - A x), q = M A (N V_k); beta and the stopping
    // test measure the preconditioned residual (Krylov.jl 0.10 gmres!)
    const nk_precond* M;
    const bool flex, spec;
    const double* v1_src = nullptr;  // r0 of the current cycle; step 1 applies J to r0 / rNorm and stores V_1
    double v1norm = 1.0;             // ||V_1|| = beta / rNorm
    // vready[k]: step k's resident sweep stored V_{k+1} itself, so step k+1's Jv reads it as is
    std::vector<char> vready;

    Arnoldi(nk_workspace* ws_, const nk_problem* p_, Op& A_, const nk_krylov_opts* o_)
        : ws(ws_), p(p_), A(A_), o(o_), c(ws_->c), n(ws_->n), W{ws_->w, ws_->w2}, N(active(o_->N)), M(active(o_->M)),
          flex(N && ws_->algo == NK_ALGO_FGMRES), spec(!N && !M), vready(ws_->mem + 2, 0) {}

    size_t slot(int k) const { return (size_t)(k & 1) * (2 * ws->cap + 2); }
    double* slot_dev(int k) const { return ws->hdev + slot(k); }
    const double* slot_pin(int k) const { return ws->hpin + slot(k); }
    double* slot_pin_dev(int k) const { return ws->hpin_dev + slot(k); }  // the kernels mirror every entry here
    int npasses(int k) const { return o->reorthogonalization ? 2 * k : k; }
    // what step k's Jv divides by and applies J to: h_{k,k-1} and q_{k-1} (step 1: rNorm and r0)
    const double* hprev(int k) const { return k > 1 ? slot_dev(k - 1) + npasses(k - 1) : ws->bdev; }
    const double* qprev(int k) const { return k > 1 ? W[(k - 1) & 1] : v1_src; }

    // (c) kbench only (NK_RES_JV=1): 2D Bratu, FD Jv, V_k stored by the previous resident sweep: Jv + MGS
    // sweep in ONE launch (q = J V_k is computed into the registers that hold it through the sweep).
    // Returns 1 with nothing enqueued where that does not apply.
    int sweep_with_jv(int k) {
        if (!(mgs_fused_jv && spec && k >= 2 && vready[k - 1] && mgs_resident && A.mode == NK_JV_FD &&
              p->kind == NK_BRATU2D))
            return 1;
        NK_TRY(ws_basis(ws, k + 1));
        double* vnext = ws->V[k];
        const ResJv jin{A.u, ws->V[k - 1], A.F0, ws->V[0], A.fd_eps(1.0), p->lambda, p->hx * p->hx, p->hy * p->hy, p->nx};
        NK_TRY(halo_exchange(c, p, ws->V[k - 1]));
        const int rc = launch_mgs_sweep(c, n, W[k & 1], ws->V.data(), k, npasses(k), Red{}, slot_dev(k), slot_pin_dev(k),
                                        -1, &vnext, &jin);
        if (rc != NK_OK) return rc;
        ++A.n_matvec;
        vready[k] = vnext != nullptr;
        NK_HIP(c, hipEventRecord(ws->col_ready[k & 1], c->stream));
        return NK_OK;
    }

    // (a) q = (M) J (N) V_k into W[k & 1], with the partials of <V_1, q> in *red
    int matvec(int k, Red* red) {
        double* q = W[k & 1];
        if (N || M) {  // V_k = q_{k-1} / h (r0 / beta), Z_k = N V_k, q = M J Z_k, <V_1, q>
            NK_TRY(launch_fd_point(c, n, nullptr, nullptr, qprev(k), hprev(k), 0.0, ws->V[k - 1]));
            const double* zk = ws->V[k - 1];
            double znorm = k == 1 ? v1norm : 1.0;
            if (N) {
                NK_TRY(ws_zbasis(ws, flex ? k : 1));  // gmres!: one p = N V_k buffer; fgmres!: Z_k kept
                double* z = ws->Z[flex ? k - 1 : 0];
                NK_TRY(apply_precond(c, p, N, A, n, z, ws->V[k - 1], A.mode == NK_JV_FD, &znorm));
                zk = z;
            }
            if (!M) return A.apply(q, zk, znorm, EPI_DOT, ws->V[0], red);
            NK_TRY(A.apply(ws->mw, zk, znorm, EPI_NONE, nullptr, nullptr));  // w = J Z_k; q = M w
            double unused = 0.0;
            NK_TRY(apply_precond(c, p, M, A, n, q, ws->mw, false, &unused));
            return launch_dot(c, n, ws->V[0], q, red);
        }
        // fused kdivcopy!(V_1, r0, rNorm) + mul! + <V_1, Jv> (the dot partner is V_1 itself).
        // ||V_1|| = beta / rNorm: 1 on the first cycle, |r0| / |zeta| after a restart (the FD step's ||v||)
        if (k == 1) return A.apply(q, v1_src, v1norm, EPI_DOT, nullptr, red, ws->bdev, ws->V[0]);
        // V_k is in place: mul! + <V_1, Jv> only
        if (vready[k - 1]) return A.apply(q, ws->V[k - 1], 1.0, EPI_DOT, ws->V[0], red);
        return A.apply(q, qprev(k), 1.0, EPI_DOT, ws->V[0], red, hprev(k), ws->V[k - 1]);
    }

    // (b) the MGS passes of step k over q, h_{k+1,k} = ||q||, and the column's event: the whole sweep
    // in one launch with q resident on chip, else one launch per pass
    int orthogonalize(int k, Red red) {
        const int np = npasses(k);
        double *q = W[k & 1], *col = slot_dev(k), *colh = slot_pin_dev(k);
        int rc = 1;
        if (mgs_resident) {
            NK_TRY(finish_reduction(c, &red));
            double* vnext = nullptr;
            if (spec) {  // the speculative path's next Jv can take V_{k+1} from the sweep
                NK_TRY(ws_basis(ws, k + 1));
                vnext = ws->V[k];
            }
            rc = launch_mgs_sweep(c, n, q, ws->V.data(), k, np, red, col, colh, -1, &vnext);
            if (rc != NK_OK && rc != 1) return rc;
            if (rc == NK_OK && vnext) vready[k] = 1;
        }
        if (rc == 1) {
            for (int t = 0; t < np; ++t) {
                const double* vi = ws->V[t % k];
                const double* vnext = (t + 1 < np) ? ws->V[(t + 1) % k] : nullptr;
                NK_TRY(finish_reduction(c, &red));
                Red nxt{};
                NK_TRY(launch_mgs_pass(c, n, q, vi, vnext, red, col + t, colh + t, &nxt, mgs_alt ? (t & 1) : 0));
                red = nxt;
            }
            NK_TRY(finish_reduction(c, &red));
            NK_TRY(launch_finalize(c, red, col + np, 1, colh + np));  // h_{k+1,k} = ||q||
        }
        NK_HIP(c, hipEventRecord(ws->col_ready[k & 1], c->stream));  // column complete in pinned memory
        return NK_OK;
    }

    // Issue Arnoldi step k.  It writes only V_k (V_{k+1} too where the sweep stores it), q_k = W[k & 1],
    // slot k & 1 of the column buffers and vready[k]: the speculation below rests on that.
    int issue(int k) {
        NK_TRY(ws_basis(ws, k));
        NK_TRY(ws_scalars(ws, k + 1));
        if ((int)vready.size() < k + 2) vready.resize(k + 2, 0);
        const int rc = sweep_with_jv(k);
        if (rc != 1) return rc;
        Red red{};
        NK_TRY(matvec(k, &red));
        vready[k] = 0;
        return orthogonalize(k, red);
    }

    // Before the host waits for step k's column.  Unpreconditioned, step k is in flight already and
    // step k+1 is issued ahead of the column it depends on (its Jv divides by h_{k+1,k} on the device),
    // unless the cycle certainly ends at k.  If the column then ends the cycle, step k+1 is discarded:
    // it wrote only V_{k+1}, q_{k+1}, slot (k+1) & 1 and vready[k+1], none of which is read when the
    // cycle stops at k (the x update reads V_1 .. V_k and y), and gmres() takes its mul!(J) back out of
    // n_matvec.  Preconditioned (the FD step needs a norm on the host), step k is issued when it is needed.
    int issue_ahead(int k, bool last) {
        if (!spec && k > 1) NK_TRY(issue(k));
        if (spec && !last) NK_TRY(issue(k + 1));
        return NK_OK;
    }

    // a restarted cycle's r0 = (M) (b - A x) in *src, its norm in *beta
    int restart_residual(const double* b, double xnorm, double* beta, const double** src) {
        Red rr{};
        NK_TRY(A.apply(W[0], ws->x, xnorm, EPI_RESID, b, &rr));  // w = b - A x, fused ||w||^2 partials
        NK_TRY(host_scalar(c, rr, 1, beta));
        *src = W[0];
        if (M) {  // r0 = M w, beta = ||r0||
            NK_TRY(apply_precond(c, p, M, A, n, ws->mr, W[0], true, beta));
            *src = ws->mr;
        }
        return NK_OK;
    }

    // The cycle's x update from its kk coefficients y: x = V y (x += from the second restarted cycle on,
    // `accumulate`), Z y for fgmres!, x (+)= N (V y) for gmres! with N.  The final cycle fuses the Newton
    // update u .-= x and leaves ||u|| in st->u_norm; a restarted FD solve that goes on needs ||x|| (*xnorm).
    int update_x(const double* y, int kk, bool accumulate, bool final_cycle, nk_krylov_stats* st, double* xnorm) {
        NK_TRY(ws_scalars(ws, kk + 1));
        for (int i = 0; i < kk; ++i) ws->ypin[i] = y[i];
        NK_HIP(c, hipMemcpyAsync(ws->ydev, ws->ypin, sizeof(double) * kk, hipMemcpyHostToDevice, c->stream));
        const bool need_xnorm = o->restart && A.mode == NK_JV_FD && !final_cycle;
        double* uu = final_cycle ? o->u_update : nullptr;  // fused Newton update u .-= x
        double* x = ws->x;
        Red xr{};
        if (N && !flex) {  // gmres!: xr = V y; p = xr; xr = N p; x += xr (restart) -- x = xr otherwise
            uu = nullptr;  // not fused: nk_krylov_solve applies u .-= x afterwards
            NK_TRY(launch_update_x(c, n, W[0], ws->xr, ws->V.data(), kk, ws->ydev, 0, nullptr, nullptr));
            double dummy = 0.0;
            NK_TRY(apply_precond(c, p, N, A, n, ws->Z[0], W[0], false, &dummy));
            if (accumulate) NK_TRY(launch_axpy(c, n, 1.0, ws->Z[0], x));
            else NK_TRY(launch_copy(c, n, x, ws->Z[0]));
            if (need_xnorm) NK_TRY(launch_sumsq(c, n, x, &xr));
        } else {
            NK_TRY(launch_update_x(c, n, x, ws->xr, N ? ws->Z.data() : ws->V.data(), kk, ws->ydev, accumulate,
                                   (need_xnorm || uu) ? &xr : nullptr, uu));
        }
        if (uu) {
            NK_TRY(host_scalar(c, xr, 1, &st->u_norm));
            ws->u_fused = true;
            return NK_OK;
        }
        if (need_xnorm) return host_scalar(c, xr, 1, xnorm);
        NK_HIP(c, hipStreamSynchronize(c->stream));  // ypin may be rewritten next cycle
        return NK_OK;
    }
};

int gmres(nk_workspace* ws, const nk_problem* p, Op& A, const double* b, const nk_krylov_opts* o, nk_krylov_stats* st,
          Hist& hist) {
    nk_ctx* c = ws->c;
    const int64_t n = ws->n;
    const int mem = ws->mem;
    const bool restart = o->restart != 0, reorth = o->reorthogonalization != 0;
    NK_TRY(ws_basis(ws, mem));
    NK_TRY(ws_scalars(ws, mem + 1));
    Arnoldi S(ws, p, A, o);
    if (S.M) {
        NK_TRY(ws_vec(ws, &ws->mr));
        NK_TRY(ws_vec(ws, &ws->mw));
    }
    // x .= 0 ; r0 = b - A*0 = b.  x is only materialised when no cycle runs: the first cycle's
    // update writes x = Σ y_i V_i directly (bit-identical to 0 + Σ y_i V_i), saving a pass over x.
    double beta = o->b_norm;  // the caller may know ||b|| already (Newton: b = F(u), ||F(u)|| just computed)
    const double* r0 = b;
    if (S.M) {  // r0 = M b, beta = ||M b||
        NK_TRY(apply_precond(c, p, S.M, A, n, ws->mr, b, true, &beta));
        r0 = ws->mr;
    } else if (!(beta > 0.0)) {
        Red rb{};
        NK_TRY(launch_sumsq(c, n, b, &rb));
        NK_TRY(host_scalar(c, rb, 1, &beta));
    }
    double rNorm = beta;
    hist.push(rNorm);
    const double eps_ = o->atol + o->rtol * rNorm;
    if (beta == 0.0) {
        NK_TRY(launch_fill(c, n, ws->x, 0.0));
        return finish_at_zero(st);
    }
    const int64_t itmax = o->itmax == 0 ? 2 * n : o->itmax;
    const double btol = gmres_btol();
    GmresLsq lsq(mem);

    int npass = 0;
    int64_t iter = 0, inner_itmax = itmax;
    bool breakdown = false, inconsistent = false;
    bool solved = rNorm <= eps_;
    bool tired = iter >= itmax;
    double xnorm = 0.0;  // ||x|| for the FD restart residual (from the fused x update)
    while (!(solved || tired || breakdown)) {
        const double* src = r0;
        if (restart && npass >= 1) NK_TRY(S.restart_residual(b, xnorm, &beta, &src));
        Range cycle_range("gmres_cycle");
        lsq.start(beta);
        // kdivcopy!(n, V[1], r0, rNorm) inside step 1's Jv: Krylov.jl divides by rNorm, which is beta on
        // the first pass and, after a restart, the previous cycle's estimate |zeta| (z[1] = beta regardless)
        NK_TRY(launch_fill(c, 1, ws->bdev, rNorm));
        S.v1_src = src;
        S.v1norm = beta / rNorm;
        npass++;
        int64_t inner_iter = 0;
        bool inner_tired = false;
        NK_TRY(S.issue(1));
        while (!(solved || inner_tired || breakdown)) {
            inner_iter++;
            const int k = (int)inner_iter;
            const bool last = gmres_last(restart, inner_iter, mem, inner_itmax);
            NK_TRY(S.issue_ahead(k, last));
            NK_HIP(c, hipEventSynchronize(ws->col_ready[k & 1]));
            NK_TRY(mb_check(c));
            if (c->prof) prof_drain(c, false);
            const GmresLsq::Col h = lsq.column(k, S.slot_pin(k), reorth);
            rNorm = h.rNorm;
            hist.push(rNorm);
            solved = gmres_solved(rNorm, eps_);
            breakdown = gmres_breakdown(h.Hbis, btol);
            inner_tired = last;
            if (!(solved || inner_tired || breakdown)) lsq.accept(k, h.zeta);  // V_{k+1} = q/h was stored by step k+1
            else if (S.spec && !last) A.n_matvec -= 1;  // the speculative step k+1 is discarded: not a mul!(J) of the solve
        }
        const int kk = (int)inner_iter;
        if (lsq.solve(kk, btol)) inconsistent = true;
        iter += inner_iter;
        inner_itmax = itmax - iter;
        tired = iter >= itmax;
        NK_TRY(S.update_x(lsq.y(), kk, restart && npass > 1, solved || tired || breakdown, st, &xnorm));
    }
    if (npass == 0) NK_TRY(launch_fill(c, n, ws->x, 0.0));  // solved (or tired) before the first cycle
    return finish(st, iter, solved, inconsistent, breakdown, solved ? 1 : (tired ? 2 : (breakdown ? 3 : 0)));
}

int cg(nk_workspace* ws, Op& A, const double* b, const nk_krylov_opts* o, nk_krylov_stats* st, Hist& hist) {
    nk_ctx* c = ws->c;
    const int64_t n = ws->n;
    double *x = ws->x, *r = ws->xr, *p = ws->p, *Ap = ws->w;
    // preconditioner M (Krylov.jl cg!: z = M r, gamma = <r, z>, p = z + beta p); M = I: z === r
    const nk_precond* Mp = active(o->M);
    // M = a multigrid hierarchy (in SPD form, nk_krylov_solve checked): the cycle's last launch leaves <r, z> itself
    nk_mg* Mg = nullptr;
    NK_TRY(mg_of(c, Mp, &Mg));
    double* zr = r;
    if (Mp) {
        NK_TRY(ws_vec(ws, &ws->mr));
        zr = ws->mr;
    }
    double unused = 0.0;
    NK_TRY(launch_fill(c, n, x, 0.0));
    NK_TRY(launch_copy(c, n, r, b));
    Red rg{};
    if (Mg) NK_TRY(mg_apply_red(Mg, zr, r, &rg));
    else if (Mp) NK_TRY(apply_precond(c, A.p, Mp, A, n, zr, r, false, &unused));
    NK_TRY(launch_copy(c, n, p, zr));
    if (!Mp) NK_TRY(launch_sumsq(c, n, r, &rg));
    else if (!Mg) NK_TRY(launch_dot(c, n, r, zr, &rg));
    double gamma = 0.0;
    NK_TRY(host_scalar(c, rg, 0, &gamma));
    double rNorm = std::sqrt(gamma);
    hist.push(rNorm);
    if (gamma == 0.0) return finish_at_zero(st);
    int64_t iter = 0, itmax = o->itmax == 0 ? 2 * n : o->itmax;
    double pNorm2 = gamma;
    const double eps_ = o->atol + o->rtol * rNorm;
    bool solved = rNorm <= eps_, tired = iter >= itmax, zero_curvature = false, inconsistent = false;
    while (!(solved || tired || zero_curvature)) {
        double pnorm = 1.0;
        if (A.mode == NK_JV_FD) {
            Red rp{};
            NK_TRY(launch_sumsq(c, n, p, &rp));
            NK_TRY(host_scalar(c, rp, 1, &pnorm));
        }
        Red rpa{};
        NK_TRY(A.apply(Ap, p, pnorm, EPI_DOT, p, &rpa));  // Ap and the partials of <p, Ap>
        double pAp = 0.0;
        NK_TRY(host_scalar(c, rpa, 0, &pAp));
        if (pAp <= DBL_EPSILON * pNorm2) {
            if (std::fabs(pAp) <= DBL_EPSILON * pNorm2) {
                zero_curvature = true;
                inconsistent = true;
            }
        }
        if (zero_curvature) continue;
        const double alpha = gamma / pAp;
        Red rn{};
        NK_TRY(launch_cg_update(c, n, alpha, x, r, p, Ap, &rn));  // x += a p ; r -= a Ap ; <r,r>
        if (Mg) {  // z = M r and <r, z> in the V-cycle's last launch
            rn = Red{};
            NK_TRY(mg_apply_red(Mg, zr, r, &rn));
        } else if (Mp) {  // z = M r ; <r, z> (the update's <r,r> partials are not used)
            rn = Red{};
            NK_TRY(apply_precond(c, A.p, Mp, A, n, zr, r, false, &unused));
            NK_TRY(launch_dot(c, n, r, zr, &rn));
        }
        double gamma_next = 0.0;
        NK_TRY(host_scalar(c, rn, 0, &gamma_next));
        rNorm = std::sqrt(gamma_next);
        hist.push(rNorm);
        const bool mach = (rNorm + 1.0 <= 1.0);
        solved = (rNorm <= eps_) || mach;
        if (!solved) {
            const double beta = gamma_next / gamma;
            pNorm2 = gamma_next + beta * beta * pNorm2;
            gamma = gamma_next;
            NK_TRY(launch_cg_direction(c, n, beta, p, zr));  // p = z + beta p
        }
        iter++;
        tired = iter >= itmax;
    }
    NK_HIP(c, hipStreamSynchronize(c->stream));
    return finish(st, iter, solved, inconsistent, false, solved ? 1 : (tired ? 2 : (zero_curvature ? 4 : 0)));
}

// kbench knob: NK_MINRES_BLAS1=1 assembles the Lanczos step from the BLAS-1 launches (axpy, axpy, sumsq / diagonal
// apply + dot, two host scalars per iteration) instead of k_minres_lanczos (slower)
const int minres_blas1 = NK_TUNE("NK_MINRES_BLAS1", 0);

// MINRES (Paige & Saunders 1975) for the symmetric, possibly indefinite J with an SPD M or none: the recurrence of
// DESIGN.md §11.  Krylov.jl's minres! is not restated line by line (its further stopping tests -- ||A|| ||x||-relative,
// the Acond limit, the windowed forward error -- are absent: parity unpinned).  Per iteration: the Jv launch (applies J
// to y / beta with beta on the device, stores v, emits <v, Jv>), k_minres_lanczos, M where it is not the diagonal,
// k_minres_scalars, ONE host synchronisation (alpha and beta^2 arrive together), then k_minres_update with the
// rotation's scalars by value.
int minres(nk_workspace* ws, Op& A, const double* b, const nk_krylov_opts* o, nk_krylov_stats* st, Hist& hist) {
    nk_ctx* c = ws->c;
    const int64_t n = ws->n;
    double *x = ws->x, *jv = ws->w, *r1 = ws->xr, *r2 = ws->mv[0], *v = ws->mv[1], *w1 = ws->mv[2], *w2 = ws->mv[3];
    const nk_precond* Mp = active(o->M);
    nk_mg* Mg = nullptr;
    NK_TRY(mg_of(c, Mp, &Mg));
    const double* Md = (Mp && Mp->kind == NK_PRECOND_DIAG) ? Mp->diag : nullptr;
    if (Mp && Mp->kind == NK_PRECOND_DIAG && !Md) return fail(c, NK_E_ARG, "diagonal preconditioner without its diagonal");
    if (Mp) NK_TRY(ws_vec(ws, &ws->mr));
    double* y = Mp ? ws->mr : r2;  // without M, y is r2 itself
    const bool need_yn = Mp && A.mode == NK_JV_FD;  // the FD step needs ||v||_2 = ||y||_2 / beta
    NK_TRY(ws_scalars(ws, 1));
    double* sc = ws->hdev;  // beta_k lives in sc[k % 3] (beta_{k-1} and beta_{k+1} beside it)
    volatile double* hp = ws->hpin;  // mapped host scalars: [0] alpha, [1] beta^2, [2] ||y||^2
    double unused = 0.0;
    // y = M r (r in rsrc) with the partials of <r, y> in *rb and, where needed, of ||y||^2 in *ry
    auto precond = [&](const double* rsrc, Red* rb, Red* ry) -> int {
        if (!Mp) return launch_sumsq(c, n, rsrc, rb);
        if (Mg) NK_TRY(mg_apply_red(Mg, y, rsrc, rb));
        else {
            NK_TRY(apply_precond(c, A.p, Mp, A, n, y, rsrc, false, &unused));
            NK_TRY(launch_dot(c, n, rsrc, y, rb));
        }
        if (need_yn) NK_TRY(launch_sumsq(c, n, y, ry));
        return NK_OK;
    };
    // beta_{k} = sqrt(Σ rb) to the device slot, beta^2 and ||y||^2 to the host: the iteration's one synchronisation
    auto scalars = [&](Red rb, Red ry, int64_t k) -> int {
        NK_TRY(finish_reduction(c, &rb));
        if (need_yn) NK_TRY(finish_reduction(c, &ry));
        NK_TRY(launch_minres_scalars(c, rb, need_yn ? &ry : nullptr, sc + k % 3, ws->hpin_dev));
        NK_HIP(c, hipStreamSynchronize(c->stream));
        if (c->prof) prof_drain(c, false);
        return mb_check(c);
    };
    NK_TRY(launch_fill(c, n, x, 0.0));
    NK_TRY(launch_fill(c, n, w1, 0.0));
    NK_TRY(launch_fill(c, n, w2, 0.0));
    NK_TRY(launch_copy(c, n, r1, b));
    NK_TRY(launch_copy(c, n, r2, b));
    Red rb{}, ry{};
    NK_TRY(precond(r2, &rb, &ry));
    NK_TRY(scalars(rb, ry, 1));
    double beta2 = hp[1], ynorm = std::sqrt(hp[2]);
    bool breakdown = beta2 < 0.0;  // <r, M r> < 0: M is not positive definite
    const double beta1 = std::sqrt(beta2);
    hist.push(beta1);
    if (breakdown) return finish(st, 0, false, false, true, 3);
    if (beta2 == 0.0) return finish_at_zero(st);
    int64_t iter = 0, itmax = o->itmax == 0 ? 2 * n : o->itmax;
    MinresRot rot(beta1);  // the rotation's scalars (nk_lsq.hpp)
    const double tol = o->atol + o->rtol * beta1;
    bool solved = rot.phibar <= tol, tired = iter >= itmax;
    while (!(solved || tired || breakdown)) {
        iter++;
        const int first = iter == 1;
        const double* bdev = sc + iter % 3;
        const double* odev = sc + (iter + 2) % 3;
        Red ra{};
        // J (y / beta), v = y / beta stored, partials of <v, J v>
        NK_TRY(A.apply(jv, y, Mp ? ynorm / rot.beta : 1.0, EPI_DOT, nullptr, &ra, bdev, v));
        rb = Red{};
        ry = Red{};
        if (minres_blas1 && (!Mp || Md)) {
            double alpha = 0.0;
            NK_TRY(host_scalar(c, ra, 0, &alpha));
            hp[0] = alpha;
            if (!first) NK_TRY(launch_axpy(c, n, -(rot.beta / rot.oldb), r1, jv));
            NK_TRY(launch_axpy(c, n, -(alpha / rot.beta), r2, jv));
            std::swap(jv, r1);  // t is where r1 is rotated from
            if (Md) {
                NK_TRY(launch_diag_apply(c, n, y, Md, r1, need_yn ? &ry : nullptr));
                NK_TRY(launch_dot(c, n, r1, y, &rb));
            } else {
                NK_TRY(launch_sumsq(c, n, r1, &rb));
            }
        } else {
            NK_TRY(finish_reduction(c, &ra));
            const bool fused = !Mp || Md;  // beta^2 (and ||y||^2) from the Lanczos launch itself
            NK_TRY(launch_minres_lanczos(c, n, jv, r1, r2, Md, Md ? y : nullptr, bdev, odev, first, ra, ws->hpin_dev,
                                         fused ? &rb : nullptr, (fused && need_yn) ? &ry : nullptr));
            if (!fused) NK_TRY(precond(r1, &rb, &ry));
        }
        NK_TRY(scalars(rb, ry, iter + 1));
        const double alpha = hp[0];
        beta2 = hp[1];
        std::swap(r1, r2);  // r1 = r2; r2 = t
        if (!Mp) y = r2;
        if (beta2 < 0.0) {  // x stays the last completed iterate
            breakdown = true;
            iter--;
            break;
        }
        ynorm = std::sqrt(hp[2]);
        const MinresRot::Step s = rot.step(alpha, beta2);
        // w = ((v - oldeps w1) - delta w2) / gamma over w1; x += phi w
        NK_TRY(launch_minres_update(c, n, v, w1, w2, x, s.oldeps, s.delta, s.gamma, s.phi));
        std::swap(w1, w2);  // w1 = w2; w2 = w
        hist.push(rot.phibar);
        solved = rot.phibar <= tol;
        tired = iter >= itmax;
    }
    NK_HIP(c, hipStreamSynchronize(c->stream));
    return finish(st, iter, solved, false, breakdown, solved ? 1 : (breakdown ? 3 : (tired ? 2 : 0)));
}

}  // namespace
}  // namespace nk

using namespace nk;

extern "C" {

int nk_precond_apply(nk_ctx* c, const nk_problem* p, const nk_precond* N, const double* u, const double* F0,
                     int32_t jv_mode, double* z, const double* v) {
    if (!c || !p || !N || !z || !v) return NK_E_ARG;
    Geo g;
    NK_TRY(geometry(c, p, &g));
    if (N->kind == NK_PRECOND_NONE) return launch_copy(c, g.n, z, v);
    if (N->kind == NK_PRECOND_GMRES && (!u || (jv_mode == NK_JV_FD && !F0)))
        return fail(c, NK_E_ARG, "the GMRES preconditioner needs the operator's u (and F0 for FD)");
    Op A{c, p, jv_mode, u, F0, 0.0};
    if (N->kind == NK_PRECOND_GMRES) {
        NK_TRY(halo_exchange(c, p, u));
        NK_TRY(exchange_un(c, p));
        if (jv_mode == NK_JV_FD) {
            Red ru{};
            NK_TRY(launch_sumsq(c, g.n, u, &ru));
            NK_TRY(host_scalar(c, ru, 1, &A.unorm));
        }
    }
    double dummy = 0.0;
    NK_TRY(apply_precond(c, p, N, A, g.n, z, v, false, &dummy));
    int rc = nk_sync(c);
    // a pipelined ILU(0) sweep timed out: once more on the level sweep (one rank only -- with several, the
    // apply recovers by itself, launch_ilu0_solve)
    if (rc != NK_OK && c->ilu_redo && c->nranks == 1) {
        c->ilu_redo = false;
        c->err.clear();
        NK_TRY(apply_precond(c, p, N, A, g.n, z, v, false, &dummy));
        rc = nk_sync(c);
    }
    return rc;
}

int nk_workspace_create(nk_ctx* c, int32_t algo, const nk_problem* p, int32_t memory, nk_workspace** out) {
    if (!c || !p || !out) return NK_E_ARG;
    if (algo != NK_ALGO_GMRES && algo != NK_ALGO_CG && algo != NK_ALGO_FGMRES && algo != NK_ALGO_MINRES)
        return fail(c, NK_E_ARG, "unsupported Krylov algorithm");
    Geo g;
    NK_TRY(geometry(c, p, &g));
    nk_workspace* ws = new nk_workspace();
    ws->c = c;
    ws->algo = algo;
    ws->prob = *p;
    ws->prob.un = p->un ? p->un : reinterpret_cast<const double*>(1);  // geometry only
    ws->mem = memory > 0 ? memory : 20;
    ws->n = g.n;
    int rc = NK_OK;
    if ((rc = nk_vec_alloc(c, &ws->prob, &ws->x)) != NK_OK || (rc = nk_vec_alloc(c, &ws->prob, &ws->w)) != NK_OK ||
        (rc = nk_vec_alloc(c, &ws->prob, &ws->xr)) != NK_OK ||
        (algo != NK_ALGO_CG && algo != NK_ALGO_MINRES && (rc = nk_vec_alloc(c, &ws->prob, &ws->w2)) != NK_OK) ||
        hipMalloc(&ws->bdev, 2 * sizeof(double)) != hipSuccess ||
        hipEventCreateWithFlags(&ws->col_ready[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ws->col_ready[1], hipEventDisableTiming) != hipSuccess) {
        if (rc == NK_OK) rc = fail(c, NK_E_HIP, "hipEventCreate failed");
        nk_workspace_destroy(ws);
        return rc;
    }
    if (algo == NK_ALGO_CG) {
        if ((rc = nk_vec_alloc(c, &ws->prob, &ws->p)) != NK_OK) {
            nk_workspace_destroy(ws);
            return rc;
        }
    } else if (algo == NK_ALGO_MINRES) {  // x, J v, r1 above; r2, v, w1, w2 here; y with the first M (`memory` is ignored)
        for (double*& m : ws->mv)
            if (rc == NK_OK) rc = nk_vec_alloc(c, &ws->prob, &m);
        if (rc != NK_OK || (rc = ws_scalars(ws, 1)) != NK_OK) {
            nk_workspace_destroy(ws);
            return rc;
        }
    } else {
        if ((rc = ws_basis(ws, ws->mem)) != NK_OK || (rc = ws_scalars(ws, ws->mem + 1)) != NK_OK) {
            nk_workspace_destroy(ws);
            return rc;
        }
    }
    *out = ws;
    return NK_OK;
}

int nk_workspace_destroy(nk_workspace* ws) {
    if (!ws) return NK_OK;
    nk_ctx* c = ws->c;
    for (double* v : ws->V) nk_vec_free(c, v);
    for (double* v : ws->Z) nk_vec_free(c, v);
    for (double* v : {ws->x, ws->w, ws->w2, ws->xr, ws->p, ws->mr, ws->mw, ws->mv[0], ws->mv[1], ws->mv[2], ws->mv[3]})
        if (v) nk_vec_free(c, v);
    for (hipEvent_t e : ws->col_ready)
        if (e) (void)hipEventDestroy(e);
    if (ws->hdev) (void)hipFree(ws->hdev);
    if (ws->ydev) (void)hipFree(ws->ydev);
    if (ws->bdev) (void)hipFree(ws->bdev);
    if (ws->hpin) (void)hipHostFree(ws->hpin);
    if (ws->ypin) (void)hipHostFree(ws->ypin);
    delete ws;
    return NK_OK;
}

double* nk_workspace_x(nk_workspace* ws) { return ws ? ws->x : nullptr; }

double* nk_workspace_basis(nk_workspace* ws, int32_t i) {
    return (ws && i >= 0 && i < (int32_t)ws->V.size()) ? ws->V[(size_t)i] : nullptr;
}

int nk_krylov_solve(nk_workspace* ws, const nk_problem* p, const double* u, const double* F0, const double* b,
                    const nk_krylov_opts* o, nk_krylov_stats* st, double* hist, int64_t hist_cap, int64_t* hist_len) {
    if (!ws || !p || !u || !b || !o || !st) return NK_E_ARG;
    nk_ctx* c = ws->c;
    Geo g;
    NK_TRY(geometry(c, p, &g));
    if (g.n != ws->n) return fail(c, NK_E_ARG, "problem size does not match the workspace");
    if (o->jv_mode == NK_JV_FD && !F0) return fail(c, NK_E_ARG, "FD Jv needs F0 = F(u)");
    *st = nk_krylov_stats{};
    Range solve_range(ws->algo == NK_ALGO_CG ? "cg_solve" : (ws->algo == NK_ALGO_MINRES ? "minres_solve" : "gmres_solve"));
    Op A{c, p, o->jv_mode, u, F0, 0.0};
    A.f0r = o->f0_is_residual != 0 && o->jv_mode == NK_JV_FD;
    NK_TRY(halo_exchange(c, p, u));  // u (and u_n) are constant during the solve: one exchange
    NK_TRY(exchange_un(c, p));
    if (o->jv_mode == NK_JV_FD) {
        A.unorm = o->u_norm;  // known from the fused Newton update (nk_axpy_norm), else one pass
        if (!(A.unorm > 0.0)) {
            Red ru{};
            NK_TRY(launch_sumsq(c, ws->n, u, &ru));
            NK_TRY(host_scalar(c, ru, 1, &A.unorm));
        }
    }
    ws->u_fused = false;
    const bool sym = ws->algo == NK_ALGO_CG || ws->algo == NK_ALGO_MINRES;  // the short recurrences: M SPD, no N
    if (sym && active(o->N))
        return fail(c, NK_E_ARG, ws->algo == NK_ALGO_CG ? "the device CG takes no right preconditioner (use GMRES / FGMRES)"
                                                        : "the device MINRES takes no right preconditioner (use GMRES / FGMRES)");
    nk_mg* Mg = nullptr;
    if (sym) NK_TRY(mg_of(c, o->M, &Mg));
    if (Mg && !mg_is_spd(Mg))
        return fail(c, NK_E_ARG, "the multigrid V-cycle as CG's M is not supported in its default form: CG needs an SPD M "
                                 "(nk_mg_set_spd, or use GMRES / FGMRES)");
    auto run = [&] {
        Hist h{hist, hist_cap, 0};
        const int rc = ws->algo == NK_ALGO_CG       ? cg(ws, A, b, o, st, h)
                       : ws->algo == NK_ALGO_MINRES ? minres(ws, A, b, o, st, h)
                                                    : gmres(ws, p, A, b, o, st, h);
        if (rc == NK_OK) h.close(hist_len);
        return rc;
    };
    int rc = run();
    if (rc != NK_OK && c->ilu_redo && !ws->u_fused && c->nranks == 1) {
        // a pipelined ILU(0) sweep timed out (reported at the step's sync, not by a sync per apply):
        // the whole solve once more, every ILU(0) apply now on the level sweep (u is still untouched).
        // One rank only: a redo on one rank would pair its reductions with its peers' later ones, so a
        // distributed solve checks each apply instead (launch_ilu0_solve)
        c->ilu_redo = false;
        c->err.clear();
        (void)hipStreamSynchronize(c->stream);
        *st = nk_krylov_stats{};
        if (hist_len) *hist_len = 0;
        A.n_matvec = 0;
        rc = run();
    }
    c->ilu_redo = false;
    st->n_matvec = A.n_matvec;
    if (rc == NK_OK && o->u_update && !ws->u_fused) {  // not fused (CG, early exits): u .-= x, ||u||
        Red ru{};
        NK_TRY(launch_axpy_sumsq(c, ws->n, -1.0, ws->x, o->u_update, &ru));
        NK_TRY(host_scalar(c, ru, 1, &st->u_norm));
    }
    return rc;
}

}  // extern "C"
