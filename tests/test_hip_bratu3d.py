"""GPU: 3D Bratu (NK_BRATU3D, ah.bratu3d_) -- the k_st3l instantiations of the kind, diag(J) and the preconditioners,
the Newton drivers and the multigrid V-cycle on its grid.

The C oracle has no 3D Bratu; the reference here is the numpy restatement of tests/bratu3d_ref.py (F, the exact
tangent and the FD quotient in the kernels' association, with oracle.exp = the library's correctly rounded exp).
Every pointwise comparison is np.array_equal -- no tolerance; reductions are held to n 2^-53 sum|terms| of
math.fsum; whole solves to a bound that follows from J being symmetric negative definite.  The Jv launches the
solvers fuse with a dot (and with storing V_k) hand their output to the orthogonalisation: those are held to the
Arnoldi relation on the stored basis, with a rounding bound derived in section 2, in both Jv modes.
"""
import ctypes as C
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
import bratu3d_ref as b3
from ariadne_hip import _lib
from oracle import oracle as oc
from test_hip_multigrid import Cycle
from test_hip_multigrid_semi import LevelCycle, plan_semi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -26
# test_hip_schemes.py's 3D edge shapes: a partial x tile, VEC 2 with a two-column last wave, fewer rows than a tile,
# fewer planes than a z-chunk
SHAPES3 = [(12, 12, 12), (33, 17, 9), (130, 5, 4), (3, 3, 3), (65, 7, 5)]
MODE_RES, MODE_JEXACT, MODE_JFD = 0, 1, 2
EPI_NONE, EPI_SUMSQ, EPI_DOT, EPI_RESID, EPI_DOTV, EPI_DOTVS = range(6)


@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def dev(a):
    return ah.DeviceArray.from_numpy(np.ascontiguousarray(a))


def kernel_name(P, mode, epi):
    """the instantiation a launch must have run: k_st3l<KIND, MODE, EPI, VEC, PER, NW, F0R, BLK>"""
    return f"nk::k_st3l<9, {mode}, {epi}, {2 if P.nx % 2 == 0 else 1}, false, 4, false, false>"


class Prof:
    """the profile of the launches inside the block: {name: {launches, kernel, ...}}"""

    def __init__(self, ctx):
        self.ctx, self.read = ctx, {}

    def __enter__(self):
        self.ctx.prof_reset()
        self.ctx.prof_enable(1)
        return self

    def __exit__(self, *exc):
        self.read = self.ctx.prof_read()
        self.ctx.prof_enable(0)
        return False

    def ran(self, name, kernel=None, launches=None):
        assert name in self.read and self.read[name]["launches"] >= 1, (name, sorted(self.read))
        if launches is not None:
            assert self.read[name]["launches"] == launches, (name, self.read[name]["launches"])
        if kernel is not None:
            assert self.read[name]["kernel"] == kernel, (name, self.read[name]["kernel"], kernel)
        return self.read[name]["kernel"]


def field(P, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    return b3.sin_ic(P) + noise * rng.standard_normal(P.shape), rng.standard_normal(P.shape)


def same(a, b):
    """NaN-aware equality (the out-of-range test only)"""
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ----------------------------------------------------------------------------- 1. pointwise, bitwise
def pointwise(ctx, P, u, v, eq=np.array_equal):
    ud, vd = dev(u), dev(v)
    res, out = ud.zero(), ud.zero()
    with Prof(ctx) as pr:
        ah.bratu3d_(res, ud, P.p)
    pr.ran("residual", kernel_name(P, MODE_RES, EPI_NONE), 1)
    F0 = b3.residual(P, u)
    assert eq(res.to_numpy(), F0), "residual"
    with Prof(ctx) as pr:
        ah.mul_(out, ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv="exact"), vd)
    pr.ran("jv_exact", kernel_name(P, MODE_JEXACT, EPI_NONE), 1)
    assert eq(out.to_numpy(), b3.jv_exact(P, u, v)), "exact Jv"
    with Prof(ctx) as pr:
        ah.mul_(out, ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv="fd"), vd, eps=EPS)
    pr.ran("jv_fd", kernel_name(P, MODE_JFD, EPI_NONE), 1)
    assert eq(out.to_numpy(), b3.jv_fd(P, u, v, F0, EPS)), "FD Jv"
    return F0


@pytest.mark.parametrize("shape", SHAPES3, ids=lambda s: "x".join(map(str, s)))
def test_pointwise_bitwise(ctx, shape):
    P = b3.Problem(*shape)
    pointwise(ctx, P, *field(P, 100 + shape[0]))


def test_pointwise_bitwise_three_spacings(ctx):
    P = b3.Problem(33, 17, 9, lam=6.0, h=(0.031, 0.0577, 0.093))
    pointwise(ctx, P, *field(P, 7))


# ----------------------------------------------------------------------------- 2. the fused forms the solvers launch
@pytest.mark.parametrize("shape", SHAPES3, ids=lambda s: "x".join(map(str, s)))
def test_residual_norm_fused(ctx, shape):
    """residual + norm in one launch: the vector bitwise, the sum of squares r within n 2^-53 sum|terms| of fsum.
    The launch hands back RN(sqrt(r)), so the bound is carried through the square root (monotone, one rounding)."""
    P = b3.Problem(*shape)
    u, _ = field(P, 200 + shape[0])
    ud = dev(u)
    res = ud.zero()
    with Prof(ctx) as pr:
        nrm = ah.bratu3d_.residual_norm(res, ud, P.p)
    pr.ran("residual_norm", kernel_name(P, MODE_RES, EPI_SUMSQ), 1)
    F0 = b3.residual(P, u)
    assert np.array_equal(res.to_numpy(), F0)
    S, B = b3.reduction_bound(F0 * F0)
    lo, hi = math.sqrt(S - B) * (1 - 2.0 ** -52), math.sqrt(S + B) * (1 + 2.0 ** -52)
    print(f"{shape}: ||F|| {nrm:.17g}, sqrt(fsum) {math.sqrt(S):.17g}, allowed [{lo:.17g}, {hi:.17g}]")
    assert lo <= nrm <= hi


# The solvers' fused Jv launches hand their output to the orthogonalisation, so the interface shows it only through
# the Arnoldi relation: step k stores V_k (the launch's own input, bit for bit), computes w = J V_k with
# h_1k = <V_1, w> fused, subtracts h_jk V_j for j = 1..k (one pass each) and stores V_{k+1} = q / h_{k+1,k}.  So
#     w = sum_{j <= k+1} h_jk V_j + e,   |e_i| <= (4 k + 1) 2^-53 M_i,   M_i = |w_i| + sum_{j <= k} |h_jk V_j,i|
# (k subtractions of at most two roundings each on operands below M_i, one division).  The test takes w from the
# restatement applied to the stored V_k -- the launch's value bit for bit if the kernel is right -- fits the h_jk by
# least squares in long double (host rounding is then negligible) and asserts
#     ||w - fit||_2 <= ||E||_2              (the fit minimises the 2-norm, so it is below the device's own e)
#     |h_1k - fsum(V_1 w)| <= n 2^-53 sum|V_1 w| + sum_j |G^-1[1, j]| sum_i |V_j,i| E_i
# where the second term is how far the fitted h_1k can lie from the device's (h_fit - h_dev = G^-1 V^T e, G the Gram
# matrix of the stored basis).  FD: the step is eps = sqrt(eps_mach) max(1, ||u||) / ||v|| with ||u|| handed to the solve
# and ||v|| = 1 for basis vectors, so the restatement evaluates the same quotient.
U = 2.0 ** -53


def ld_fit(V, w):
    """least squares of w on the columns V in long double: (h, Ginv, residual vector)"""
    L = np.longdouble
    Vl = [v.reshape(-1).astype(L) for v in V]
    wl = w.reshape(-1).astype(L)
    m = len(Vl)
    A = np.array([[np.dot(Vl[i], Vl[j]) for j in range(m)] + [np.dot(Vl[i], wl)] + [L(i == j) for j in range(m)]
                  for i in range(m)], dtype=L)
    for c in range(m):  # Gauss-Jordan on [G | V^T w | I]; G is within 1e-6 of the identity (asserted by the caller)
        A[c] = A[c] / A[c, c]
        for r in range(m):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    h, Ginv = A[:, m], A[:, m + 1:]
    return h, Ginv, wl - sum(h[j] * Vl[j] for j in range(m))


def check_arnoldi_step(V, k, w, what):
    """step k (1-based) of the relation above on the stored basis V[0..k]; returns the fitted h_1k"""
    n = w.size
    G = np.array([[float(np.dot(a.reshape(-1), b.reshape(-1))) for b in V[:k + 1]] for a in V[:k + 1]])
    assert np.max(np.abs(G - np.eye(k + 1))) <= 1e-6, (what, G)
    h, Ginv, r = ld_fit(V[:k + 1], w)
    M = np.abs(w.reshape(-1)) + sum(abs(float(h[j])) * np.abs(V[j].reshape(-1)) for j in range(k))
    E = (4 * k + 1) * U * M
    rn, En = float(np.sqrt(np.dot(r, r))), float(np.linalg.norm(E))
    S, B = b3.reduction_bound(V[0] * w)
    slack = sum(abs(float(Ginv[0, j])) * math.fsum(np.abs(V[j].reshape(-1)) * E) for j in range(k + 1))
    print(f"{what}: ||w - fit|| {rn:.3e} (allowed {En:.3e}, ||w|| {np.linalg.norm(w):.3e}); h_1{k} {float(h[0]):.17g}, "
          f"fsum {S:.17g}, |diff| {abs(float(h[0]) - S):.3e} (allowed {B:.3e} + {slack:.3e}), n {n}")
    assert rn <= En, what
    assert abs(float(h[0]) - S) <= B + slack, what
    return float(h[0])


def fd_step(unorm, vnorm):
    return math.sqrt(2.0 ** -52) * max(1.0, unorm) / vnorm


@pytest.mark.parametrize("jv", ["exact", "fd"])
@pytest.mark.parametrize("shape", SHAPES3, ids=lambda s: "x".join(map(str, s)))
def test_gmres_fused_jv_forms(ctx, shape, jv):
    """Jv + dot with V_k stored, as GMRES launches it: step 1 (V_1 = b / beta stored, its own dot partner) and steps
    2 and 3 (partner V_1; V_k stored by the launch, or read in place where the sweep stored it).  V_1 is b / beta bit
    for bit; the output vector and the fused reduction of steps 1 and 2 are held to the Arnoldi relation above."""
    P = b3.Problem(*shape)
    u, _ = field(P, 300 + shape[0])
    ud = dev(u)
    res = ud.zero()
    ah.bratu3d_(res, ud, P.p)
    b = res.to_numpy()
    assert np.array_equal(b, b3.residual(P, u))
    unorm = float(np.linalg.norm(u))
    J = ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv=jv)
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=5))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, res, itmax=3, atol=0.0, rtol=0.0, history=True, _u_norm=unorm)
    mode = MODE_JEXACT if jv == "exact" else MODE_JFD
    pr.ran(f"jv_{jv}_dot_v1", kernel_name(P, mode, EPI_DOTVS), 1)
    later = {k: pr.read[k]["kernel"] for k in (f"jv_{jv}_dot_norm", f"jv_{jv}_dot") if k in pr.read}
    assert later, sorted(pr.read)
    for name, kern in later.items():
        assert kern == kernel_name(P, mode, EPI_DOTV if name.endswith("_norm") else EPI_DOT), (name, kern)
    hist = ws.stats.residuals
    V = [ws.basis(i).to_numpy() for i in range(3)]
    np.testing.assert_array_equal(V[0], b / hist[0])
    apply = (lambda v: b3.jv_exact(P, u, v)) if jv == "exact" else (lambda v: b3.jv_fd(P, u, v, b, fd_step(unorm, 1.0)))
    print(f"{shape} {jv}: later steps ran {later}")
    for k in (1, 2):
        check_arnoldi_step(V, k, apply(V[k - 1]), f"{shape} {jv} step {k}")
    ws.free()


@pytest.mark.parametrize("shape", SHAPES3, ids=lambda s: "x".join(map(str, s)))
def test_jacobi_gmres_plain_jv_dot(ctx, shape):
    """Jv + dot with a partner other than its input and nothing stored: right-preconditioned GMRES applies J to
    z_k = d .* V_k (Jacobi) with <V_1, J z_k> fused.  Exact Jv (the FD step of this form takes ||z_k|| from a device
    reduction the host cannot repeat bit for bit; its reduction is test_cg_jv_dot_reduction's).  Steps 1 and 2: the
    output vector and the reduction by the Arnoldi relation, with w = J (d .* V_k) from the restatement."""
    P = b3.Problem(*shape)
    u, _ = field(P, 350 + shape[0])
    ud = dev(u)
    res = ud.zero()
    ah.bratu3d_(res, ud, P.p)
    b = res.to_numpy()
    J = ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv="exact")
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=5))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, res, itmax=3, atol=0.0, rtol=0.0, history=True, N=ah.jacobi(J))
    pr.ran("jv_exact_dot", kernel_name(P, MODE_JEXACT, EPI_DOT))
    assert "jv_exact_dot_v1" not in pr.read and "jv_exact_dot_norm" not in pr.read, sorted(pr.read)
    V = [ws.basis(i).to_numpy() for i in range(3)]
    np.testing.assert_array_equal(V[0], b / ws.stats.residuals[0])
    d = b3.jacobian_diag(P, u, reciprocal=True)
    for k in (1, 2):
        check_arnoldi_step(V, k, b3.jv_exact(P, u, d * V[k - 1]), f"{shape} N=jacobi step {k}")
    ws.free()


@pytest.mark.parametrize("jv", ["exact", "fd"])
@pytest.mark.parametrize("shape", SHAPES3, ids=lambda s: "x".join(map(str, s)))
def test_cg_jv_dot_reduction(ctx, shape, jv):
    """Jv + dot with a partner, nothing stored, both Jv modes: CG's <p, J p>.  After one CG step from x = 0, p = b and
    x = alpha b with alpha = gamma / <p, J p>, gamma = (the first history entry)^2: <p, J p> is observed as gamma / alpha
    to within 8 units of 2^-53 (the square root and the square of gamma, the product alpha b_i, the two quotients) and
    must lie within n 2^-53 sum|terms| of math.fsum over the restatement's terms b_i (J b)_i plus that.  FD: ||p|| is
    the same device reduction as gamma, so the step is eps(||u||, sqrt(gamma)) with ||u|| handed to the solve."""
    P = b3.Problem(*shape)
    u, _ = field(P, 400 + shape[0])
    ud = dev(u)
    res = ud.zero()
    ah.bratu3d_(res, ud, P.p)
    b = res.to_numpy()
    unorm = float(np.linalg.norm(u))
    J = ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv=jv)
    ws = ah.krylov_workspace("cg", ah.KrylovConstructor(res))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, res, itmax=1, atol=0.0, rtol=0.0, history=True, _u_norm=unorm)
    pr.ran(f"jv_{jv}_dot", kernel_name(P, MODE_JEXACT if jv == "exact" else MODE_JFD, EPI_DOT), 1)
    x = ws.x.to_numpy()
    i = np.unravel_index(np.argmax(np.abs(b)), b.shape)
    alpha = x[i] / b[i]
    beta = ws.stats.residuals[0]
    Jb = b3.jv_exact(P, u, b) if jv == "exact" else b3.jv_fd(P, u, b, b, fd_step(unorm, beta))
    S, B = b3.reduction_bound(b * Jb)
    got = beta ** 2 / alpha
    print(f"{shape} {jv}: <p, Jp> observed {got:.17g}, fsum {S:.17g}, |diff| {abs(got - S):.3e} (allowed {B + 8 * U * abs(S):.3e})")
    assert S < 0.0 and abs(got - S) <= B + 8 * U * abs(S)
    ws.free()


# ----------------------------------------------------------------------------- 3. the exp's exact phase
FAM_LO, FAM_N, KMAX = 2 ** 16, 3000, 64


def family(a):
    return np.asarray(a, dtype=np.float64) * 2.0 ** -52 + 2.0 ** -53


class Planted:
    def __init__(self, P, u, plants, patch, a):
        self.P, self.u, self.plants, self.patch, self.a = P, u, plants, patch, a
        for x in (u, plants, patch, a):
            x.flags.writeable = False

    def tangent_zero(self, seed):
        v = np.random.default_rng(seed).standard_normal(self.u.shape)
        v[self.plants] = 0.0
        return v

    def tangent_family(self, seed):
        rng = np.random.default_rng(seed)
        v = rng.standard_normal(self.u.shape)
        v[self.plants] = 0.0
        k = rng.integers(-KMAX, KMAX + 1, self.u.shape)
        v[self.patch] = k[self.patch] * EPS
        return v


@functools.lru_cache(maxsize=None)
def plant3d(nx, ny, nz):
    """The plant map for k_st3l's tiles (one wave per row, 64 VEC columns per wave, 4 rows per tile, z-chunks of 16
    planes) on an ordinary field: (a) the eight corners; (b) plane 2, row 1 at the lane edges -- lane 0 / lane 63 of
    x-tile 0 and lane 0 of x-tile 1 (a partial tile), for VEC 2 both elements of those lanes, one lane with only
    its first and one with only its second element; (c) column 5 of rows 3, 4 and ny - 1 of plane 2 (the last row of a
    tile, the first of the next, the last of a partial tile); (d) column 7 of row 2 in planes 15, 16 and nz - 1 (the
    last plane of a z-chunk, the first of the next, the last of a partial chunk); (e) the patch: rows 3 and 4 of
    plane 8 over the full width (whole rows, either side of a tile boundary), distinct family values."""
    assert ny > 5 and nz > 17 and nx > 64 * (2 if nx % 2 == 0 else 1)
    P = b3.Problem(nx, ny, nz)
    rng = np.random.default_rng(1000 * nx + ny)
    u = b3.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    pool = iter(rng.permutation(np.arange(FAM_LO + KMAX, FAM_LO + FAM_N - KMAX)))
    plants = np.zeros(P.shape, dtype=bool)
    a = np.zeros(P.shape, dtype=np.int64)

    def put(k, j, i):
        assert not plants[k, j, i], (k, j, i)
        a[k, j, i] = next(pool)
        u[k, j, i] = family(a[k, j, i])
        plants[k, j, i] = True

    for j in (3, 4):                                   # (e)
        for i in range(nx):
            put(8, j, i)
    patch = plants.copy()
    for k in (0, nz - 1):                              # (a)
        for j in (0, ny - 1):
            for i in (0, nx - 1):
                put(k, j, i)
    vec = 2 if nx % 2 == 0 else 1
    cols = [0, 1, 126, 127, 128, 129, 20, 41] if vec == 2 else [0, 63, 64, nx - 1]   # (b)
    for i in cols:
        put(2, 1, i)
    for j in (3, 4, ny - 1):                           # (c)
        put(2, j, 5)
    for k in (15, 16, nz - 1):                         # (d)
        put(k, 2, 7)
    assert len(np.unique(u[patch])) == int(patch.sum())
    return Planted(P, u, plants, patch, a)


def check_args(C, x, what):
    """the exp arguments x of one launch: every plant is rare, at most 1/8 of the rest is; returns the number of
    exact-phase evaluations the launch contains"""
    rare = oc.exp_rare(x)
    assert rare[C.plants].all(), f"{what}: a planted argument is not rare"
    assert rare[~C.plants].mean() <= 0.125, what
    n = int(rare.sum())
    assert n >= int(C.plants.sum()) > 0, what
    return n


@pytest.mark.parametrize("shape", [(130, 6, 18), (67, 6, 18)], ids=lambda s: "x".join(map(str, s)))
def test_exact_phase_inside_the_kernels(ctx, shape):
    """MODE_RES, MODE_JEXACT (planted in u) and MODE_JFD (w == u at the plants; w = another family member on the patch)
    on the planted field: bit for bit, each launch with its plants rare"""
    C_ = plant3d(*shape)
    P, u = C_.P, C_.u
    ud = dev(u)
    res, out = ud.zero(), ud.zero()
    cov = {"exp(u)": check_args(C_, u, "exp(u)")}
    ah.bratu3d_(res, ud, P.p)
    F0 = b3.residual(P, u)
    assert np.array_equal(res.to_numpy(), F0), "residual"
    v = np.random.default_rng(11).standard_normal(P.shape)
    v[C_.patch] = 1.0
    ah.mul_(out, ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv="exact"), dev(v))
    assert np.array_equal(out.to_numpy(), b3.jv_exact(P, u, v)), "exact Jv"
    Jfd = ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv="fd")
    for what, v in (("w == u", C_.tangent_zero(12)), ("w = another member", C_.tangent_family(13))):
        w = u + EPS * v
        cov[f"FD {what}"] = check_args(C_, w, f"FD {what}")
        if what == "w == u":
            assert np.array_equal(w[C_.plants], u[C_.plants])
        else:
            assert np.array_equal(w[C_.patch], family(C_.a[C_.patch] + np.rint(v[C_.patch] / EPS).astype(np.int64)))
            assert (w[C_.patch] != u[C_.patch]).mean() > 0.9
        with Prof(ctx) as pr:
            ah.mul_(out, Jfd, dev(v), eps=EPS)
        pr.ran("jv_fd", kernel_name(P, MODE_JFD, EPI_NONE), 1)
        assert np.array_equal(out.to_numpy(), b3.jv_fd(P, u, v, F0, EPS)), f"FD Jv, {what}"
    # the fused residual + norm form on the planted field, and diag(J) (k_jdiag: nk_exp with the global table)
    res2 = ud.zero()
    ah.bratu3d_.residual_norm(res2, ud, P.p)
    assert np.array_equal(res2.to_numpy(), F0)
    assert np.array_equal(ah.jacobian_diag(Jfd).to_numpy(), b3.jacobian_diag(P, u))
    assert all(n > 0 for n in cov.values())
    print(json.dumps(cov))


OOR = {"overflow": 710.0, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "subnormal": -720.0, "zero": -746.0}


def test_out_of_range_arguments(ctx):
    """710 (Inf) at a corner, NaN in lane 63, +-Inf, -720 (a subnormal result) and -746 (0) as isolated points of an
    ordinary field (lam = 0.25): the fast phase clamps x, so these tell "exact phase skipped" from "taken"."""
    P = b3.Problem(130, 6, 18, lam=0.25)
    rng = np.random.default_rng(77)
    u = b3.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    at = {"overflow": (0, 0, 0), "nan": (2, 1, 126), "+inf": (5, 3, 40), "-inf": (9, 4, 77), "subnormal": (15, 2, 30),
          "zero": (16, 5, 129)}
    plants = np.zeros(P.shape, dtype=bool)
    for name, idx in at.items():
        u[idx] = OOR[name]
        plants[idx] = True
    Cp = Planted(P, u, plants, np.zeros(P.shape, dtype=bool), np.zeros(P.shape, dtype=np.int64))
    assert check_args(Cp, u, "out of range") > 0
    with np.errstate(all="ignore"):
        F0 = pointwise(ctx, P, u, Cp.tangent_zero(5), eq=same)
        assert np.isinf(F0[at["overflow"]]) and np.isnan(F0[at["nan"]])
        assert same(ah.jacobian_diag(ah.JacobianOperator(ah.bratu3d_, dev(F0), dev(u), P.p)).to_numpy(), b3.jacobian_diag(P, u))
        e = oc.exp(u)
    assert e[at["zero"]] == 0.0 and 0.0 < e[at["subnormal"]] < 2.3e-308 and np.isinf(e[at["overflow"]])


# ----------------------------------------------------------------------------- 4. diagonal and preconditioners
def operator(P, u, jv="exact"):
    ud = dev(u)
    res = ud.zero()
    ah.bratu3d_(res, ud, P.p)
    return ah.JacobianOperator(ah.bratu3d_, res, ud, P.p, jv=jv)


@pytest.mark.parametrize("shape", SHAPES3, ids=lambda s: "x".join(map(str, s)))
def test_jacobian_diag_bitwise(ctx, shape):
    P = b3.Problem(*shape, lam=6.0)
    u, _ = field(P, 500 + shape[0])
    J = operator(P, u)
    with Prof(ctx) as pr:
        d, dr = ah.jacobian_diag(J).to_numpy(), ah.jacobian_diag(J, reciprocal=True).to_numpy()
    pr.ran("jacobian_diag", None, 2)
    np.testing.assert_array_equal(d, b3.jacobian_diag(P, u))
    np.testing.assert_array_equal(dr, b3.jacobian_diag(P, u, reciprocal=True))


def gmres(J, b, **kw):
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(b, memory=30))
    ah.krylov_solve_(ws, J, b, restart=True, itmax=300, atol=0.0, rtol=1e-8, **kw)
    out = ws.x.to_numpy(), ws.stats
    ws.free()
    return out


@pytest.mark.parametrize("jv", ["exact", "fd"])
def test_jacobi_and_ilu0_preconditioned_gmres(ctx, jv):
    """Jacobi and ILU(0) as N, and the inner-GMRES preconditioner with FGMRES: each solves J x = F(u) -- checked by the
    true residual of the restatement -- and ILU(0) takes fewer steps than no preconditioner"""
    P = b3.Problem(24, 20, 18, lam=6.0)
    u, _ = field(P, 9)
    J = operator(P, u, jv)
    b = J.res.to_numpy()
    # rtol = 1e-8 on the solver's own operator.  Exact Jv: 1e-7, the bar of tests/test_hip_multigrid.py.  FD: the
    # quotient is off by sqrt(eps_mach) = 1.5e-8 relative to the stencil's terms, which exceed J v by up to
    # ||J|| / |lambda_min| = 4 (25^2 + 21^2 + 19^2) / 21 = 270 here: 1e-8 + 270 x 1.5e-8 = 4e-6
    allowed = 1e-7 if jv == "exact" else 4e-6
    steps = {}
    for name, kw in (("none", {}), ("jacobi", {"N": ah.jacobi(J)}), ("ilu0", {"N": ah.ilu0(J)})):
        x, st = gmres(J, J.res, **kw)
        true = np.linalg.norm(b - b3.jv_exact(P, u, x)) / np.linalg.norm(b)
        print(f"{jv} N={name}: niter {st.niter}, true ||r|| / ||b|| {true:.2e}")
        assert st.solved and true <= allowed
        steps[name] = st.niter
    assert steps["ilu0"] < steps["none"]
    ws = ah.krylov_workspace("fgmres", ah.KrylovConstructor(J.res, memory=30))
    ah.krylov_solve_(ws, J, J.res, restart=True, itmax=300, atol=0.0, rtol=1e-8, N=ah.gmres_preconditioner(5)(J))
    true = np.linalg.norm(b - b3.jv_exact(P, u, ws.x.to_numpy())) / np.linalg.norm(b)
    print(f"{jv} N=gmres(5), fgmres: niter {ws.stats.niter}, true ||r|| / ||b|| {true:.2e}")
    assert ws.stats.solved and true <= allowed
    ws.free()


def test_ilu0_factor_bitwise(ctx):
    P = b3.Problem(9, 7, 5, lam=6.0, h=(0.1, 0.125, 0.16))
    u, v = field(P, 3)
    J = operator(P, u)
    N = ah.ilu0(J)
    dref = b3.ilu0_factor(P, u)
    assert np.all(np.isfinite(dref))
    np.testing.assert_array_equal(N.d.to_numpy(), dref)
    # z = (L U)^-1 v against the assembled factors L = I + L_A D~^-1, U = D~ + U_A (a solve: to rounding)
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    A = b3.jacobian(P, u)
    D = sp.diags(dref.reshape(-1))
    L = sp.identity(P.n) + sp.tril(A, -1) @ sp.diags(1.0 / dref.reshape(-1))
    U = D + sp.triu(A, 1)
    zref = spla.spsolve_triangular(U.tocsr(), spla.spsolve_triangular(L.tocsr(), v.reshape(-1), lower=True), lower=False)
    z = N.apply(J, dev(v)).to_numpy().reshape(-1)
    assert np.max(np.abs(z - zref)) <= 1e-12 * np.max(np.abs(zref))


def test_collect_equals_the_assembled_matrix(ctx):
    P = b3.Problem(9, 7, 5, lam=6.0, h=(0.1, 0.125, 0.16))
    u, _ = field(P, 4)
    J = operator(P, u)
    A, ref = ah.collect(J), b3.jacobian(P, u)
    np.testing.assert_array_equal(A.toarray(), ref.toarray())
    assert A.nnz == ref.nnz
    coo = A.tocoo()
    assert set(np.unique(coo.data[coo.row != coo.col])) == {b3.offdiag(P.hx), b3.offdiag(P.hy), b3.offdiag(P.hz)}
    np.testing.assert_array_equal(A.diagonal(), b3.jacobian_diag(P, u).reshape(-1))
    np.testing.assert_array_equal(ah.collect(J.T).toarray(), ref.T.toarray())


@pytest.mark.parametrize("shape", [(33, 17, 9), (130, 5, 4)], ids=lambda s: "x".join(map(str, s)))
def test_batched_and_transposed_mul(ctx, shape):
    """11 columns (two launches) equal the single exact / FD Jv column by column; J^T v = J v"""
    P = b3.Problem(*shape)
    u, _ = field(P, 600 + shape[0])
    rng = np.random.default_rng(5)
    vs = [rng.standard_normal(P.shape) for _ in range(11)]
    F0 = b3.residual(P, u)
    for jv in ("exact", "fd"):
        J = operator(P, u, jv)
        outs = [J.u.zero() for _ in vs]
        with Prof(ctx) as pr:
            ah.mul_(outs, J, [dev(v) for v in vs], eps=EPS)
        pr.ran(f"jv_{jv}_batch", None, 2)
        for o, v in zip(outs, vs):
            ref = b3.jv_exact(P, u, v) if jv == "exact" else b3.jv_fd(P, u, v, F0, EPS)
            np.testing.assert_array_equal(o.to_numpy(), ref)
    J = operator(P, u)
    out = J.u.zero()
    ah.mul_(out, J.T, dev(vs[0]))
    np.testing.assert_array_equal(out.to_numpy(), b3.jv_exact(P, u, vs[0]))
    outs = [J.u.zero() for _ in vs[:3]]
    ah.mul_(outs, J.T, [dev(v) for v in vs[:3]])
    for o, v in zip(outs, vs):
        np.testing.assert_array_equal(o.to_numpy(), b3.jv_exact(P, u, v))


# ----------------------------------------------------------------------------- 5. whole solves
SOLVE_SHAPE, SOLVE_LAM = (24, 20, 18), 6.0


@functools.lru_cache(maxsize=None)
def solve_reference():
    """(P, u0, u* by Newton with sparse LU to 1e-13 ||F(u0)||, the eigenvalue of J(u*) nearest zero)"""
    P = b3.Problem(*SOLVE_SHAPE, lam=SOLVE_LAM)
    u0 = b3.sin_ic(P)
    ustar, steps, hist = b3.newton_lu(P, u0, rtol=1e-13)
    assert hist[-1] <= 1e-13 * hist[0]
    ev = b3.eig_nearest_zero(P, ustar)
    assert -21.35 <= ev <= -21.05
    for x in (u0, ustar):
        x.flags.writeable = False
    return P, u0, ustar, ev


def check_root(P, u, ustar, ev, tol, what):
    """||F(u)|| <= tol by the restatement, and ||u - u*|| <= 2 ||F(u)|| / |lambda_min|: F(u) = J (u - u*) + O(|u - u*|^2)
    with J symmetric negative definite, so |u - u*| <= |F(u)| / |lambda_min| to first order; 2 covers the rest"""
    nF = float(np.linalg.norm(b3.residual(P, u)))
    err = float(np.linalg.norm(u - ustar))
    print(f"{what}: ||F(u)|| {nF:.3e} (tol {tol:.3e}), ||u - u*|| {err:.3e} (allowed {2 * nF / abs(ev):.3e})")
    assert nF <= tol
    assert err <= 2.0 * nF / abs(ev)


@pytest.mark.parametrize("jv", ["fd", "exact"])
def test_newton_drivers_agree_and_reach_the_root(ctx, jv):
    P, u0, ustar, ev = solve_reference()
    tol = 1e-6 * float(np.linalg.norm(b3.residual(P, u0))) + 1e-12
    kw = dict(memory=30, jv=jv, krylov_kwargs={"restart": True})
    u, r = ah.newton_krylov_(ah.bratu3d_, dev(u0), P.p, **kw)
    assert r.solved
    check_root(P, u.to_numpy(), ustar, ev, tol, f"newton_krylov_ {jv}")
    un, rn = ah.newton_krylov_native(ah.bratu3d_, dev(u0), P.p, **kw)
    assert rn.solved
    check_root(P, un.to_numpy(), ustar, ev, tol, f"newton_krylov_native {jv}")
    exe = os.path.join(ROOT, "newtonkrylov.jl_amd", "bin", "bratu3d_newton")
    out = subprocess.run([exe, *map(str, SOLVE_SHAPE), jv, "30", "1", "--lambda", repr(SOLVE_LAM)], capture_output=True, text=True,
                         timeout=120, check=True)
    rb = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"{jv}: python {tuple(r.stats[:2])}, native {tuple(rn.stats[:2])}, binary {(rb['outer'], rb['inner'])}")
    assert rb["solved"] and (rb["N"], rb["ny"], rb["nz"], rb["jv"]) == (*SOLVE_SHAPE, jv)
    assert rb["n_res"] <= rb["tol"] and abs(rb["tol"] - tol) <= 1e-12 * tol
    # the binary prints no solution, so for it the two bounds are checked by proxy: its own ||F(u)|| against its own
    # tol (the same tol as above), and max|u|, the one figure of u it reports, within the bound of max|u*| (the max
    # norm is below the 2-norm); the counts below tie its iteration to the two drivers whose u is checked in full
    assert abs(rb["u_max"] - np.max(np.abs(ustar))) <= 2.0 * rb["n_res"] * (1 + 1e-9) / abs(ev)
    assert tuple(r.stats[:2]) == tuple(rn.stats[:2]) == (rb["outer"], rb["inner"])


# ----------------------------------------------------------------------------- 6. multigrid
MG_CASES = [((12, 12, 12), "full"), ((33, 17, 9), "full"), ((96, 12, 12), "semi")]


@functools.lru_cache(maxsize=None)
def mg_reference(shape, coarsening):
    """(P, u, v, k, s, h, the restatement's V-cycle in float64, its float64-against-long-double sensitivity)"""
    P = b3.Problem(*shape, lam=6.0)
    u, v = field(P, 700 + shape[0])
    k, h = [1.0, 1.0, 1.0], [P.hx, P.hy, P.hz]
    s = P.lam * oc.exp(u)

    def cyc(dt):
        if coarsening == "semi":
            return LevelCycle(plan_semi(shape, h=h), h, k, s, dt=dt)
        return Cycle(shape, h, k, s, dt=dt)

    c64 = cyc(np.float64)
    z64, zl = c64.vcycle(v), cyc(np.longdouble).vcycle(v)
    sens = float(np.max(np.abs(z64 - zl)) / np.max(np.abs(zl)))
    return P, u, v, k, s, h, z64, sens, c64.levels


def mg_tol():
    """16 x the restatement's own float64-against-long-double sensitivity (the largest over the cases here), the
    rule of tests/test_hip_multigrid.py: the device runs the same cycle with fma and another association"""
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    return 16 * max(mg_reference(*c)[7] for c in MG_CASES)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("shape,coarsening", MG_CASES, ids=[f"{'x'.join(map(str, s))}-{c}" for s, c in MG_CASES])
def test_vcycle_on_the_kinds_grid(ctx, shape, coarsening):
    P, u, v, k, s, h, zref, sens, levels = mg_reference(shape, coarsening)
    J = operator(P, u)
    vd = dev(v)
    # the level-0 operator is J's: one level, one sweep from zero, omega = 1 -> z = v ./ diag(J), bitwise
    mg1 = ah.MultigridPreconditioner(J, coarse_sweeps=1, omega=1.0, max_levels=1)
    assert mg1.levels == [tuple(shape)]
    z1 = mg1.apply(J, vd).to_numpy()
    np.testing.assert_array_equal(z1, ah.jacobian_diag(J, reciprocal=True).to_numpy() * v)
    np.testing.assert_array_equal(z1, b3.jacobian_diag(P, u, reciprocal=True) * v)
    mg = ah.MultigridPreconditioner(J, coarsening=coarsening)
    assert mg.levels == [tuple(e) for e in levels]
    if coarsening == "semi":
        assert mg.levels[1] == (48, 12, 12)  # x alone is halved first
    z = mg.apply(J, vd).to_numpy()
    err, tol = rel(z, zref), mg_tol()
    print(f"{shape} {coarsening}: device vs restatement {err:.3e} (allowed {tol:.1e}; this case's sensitivity {sens:.2e})")
    assert err <= tol
    np.testing.assert_array_equal(mg.apply(J, vd).to_numpy(), z)  # two applications: the same bits
    mg.spd = True
    np.testing.assert_array_equal(mg.apply(J, vd).to_numpy(), -z)  # sigma = -1: the default result negated
    # from_coefficients with k = 1 and s = lam exp(u) from the library's exp: the Jacobian's cycle
    sd = J.u.zero()
    ah.exp_(sd, J.u)
    ah.kscal_(len(sd), P.lam, sd)
    np.testing.assert_array_equal(sd.to_numpy(), s)
    mgc = ah.MultigridPreconditioner.from_coefficients(J.u.grid, k, sd, h=h, coarsening=coarsening)
    np.testing.assert_array_equal(mgc.apply(J, vd).to_numpy(), z)


def test_newton_with_multigrid(ctx):
    """40 x 36 x 20, lam = 6: N = multigrid solves with strictly fewer inner iterations than no N; CG and MINRES with
    M = multigrid(spd=True) solve in the same number of Newton steps"""
    P = b3.Problem(40, 36, 20, lam=6.0)
    u0 = b3.sin_ic(P)
    tol = 1e-6 * float(np.linalg.norm(b3.residual(P, u0))) + 1e-12
    kw = dict(memory=30, jv="fd")
    u, r = ah.newton_krylov_(ah.bratu3d_, dev(u0), P.p, N=ah.multigrid, krylov_kwargs={"restart": True}, **kw)
    _, r0 = ah.newton_krylov_(ah.bratu3d_, dev(u0), P.p, krylov_kwargs={"restart": True}, **kw)
    print(f"multigrid outer {r.stats.outer_iterations} inner {r.stats.inner_iterations}; "
          f"plain outer {r0.stats.outer_iterations} inner {r0.stats.inner_iterations}")
    assert r.solved and r0.solved
    assert float(np.linalg.norm(b3.residual(P, u.to_numpy()))) <= tol
    assert r.stats.inner_iterations < r0.stats.inner_iterations
    un, rn = ah.newton_krylov_native(ah.bratu3d_, dev(u0), P.p, N=ah.multigrid, krylov_kwargs={"restart": True}, **kw)
    assert rn.solved and tuple(rn.stats[:2]) == tuple(r.stats[:2])
    for algo in ("cg", "minres"):
        fac = ah.multigrid(spd=True)
        us, rs = ah.newton_krylov_(ah.bratu3d_, dev(u0), P.p, algo=algo, M=fac, **kw)
        fac.free()
        print(f"{algo} + M: outer {rs.stats.outer_iterations} inner {rs.stats.inner_iterations}")
        assert rs.solved and rs.stats.outer_iterations == r.stats.outer_iterations
        assert float(np.linalg.norm(b3.residual(P, us.to_numpy()))) <= tol


# ----------------------------------------------------------------------------- 7. rejections
def test_periodic_and_2d_are_refused(ctx):
    lib = ah.load()
    g = ah.Grid.full(12, 10, 9)
    u = ah.DeviceArray(g, ctx)
    prob = ah.bratu3d_.problem(u, (0.1, 0.1, 0.1, 6.0))
    prob.bc = _lib.NK_BC_PERIODIC
    rc = lib.nk_residual(ctx.handle, C.byref(prob), u.ptr, u.ptr)
    msg = (lib.nk_last_error(ctx.handle) or b"").decode()
    assert rc == _lib.NK_E_ARG and "periodic" in msg, (rc, msg)
    h = C.c_void_p()
    rc = lib.nk_mg_create(ctx.handle, C.byref(prob), None, C.byref(h))
    assert rc == _lib.NK_E_ARG and "periodic" in (lib.nk_last_error(ctx.handle) or b"").decode()
    with pytest.raises(ValueError, match="3D grid"):
        ah.bratu3d_(ah.DeviceArray(ah.Grid.full(12, 10), ctx), ah.DeviceArray(ah.Grid.full(12, 10), ctx), (0.1, 0.1, 0.1, 6.0))
    # a kind beyond the known ones is still unknown
    prob.bc, prob.kind = _lib.NK_BC_ZERO, 10
    rc = lib.nk_residual(ctx.handle, C.byref(prob), u.ptr, u.ptr)
    assert rc == _lib.NK_E_ARG and "unknown problem kind" in (lib.nk_last_error(ctx.handle) or b"").decode()


def test_two_rank_context_is_refused(ctx):
    """on a 2-rank context (z-slabs, then 3D blocks) the kind is NK_E_ARG with a reason naming "one rank\""""
    import test_hip_dist as td

    worker = os.path.join(ROOT, "tests", "bratu3d_rank_worker.py")
    rc, log = td.run_ranks(2, [worker], td.worker_env(2), timeout=120)
    assert rc == 0, log[-3000:]
    lines = [json.loads(line.split("BRATU3D_RANK ", 1)[1]) for line in log.splitlines() if "BRATU3D_RANK " in line]
    assert sorted(r["rank"] for r in lines) == [0, 1], log[-3000:]
    for r in lines:
        assert r["nranks"] == 2
        for form in ("slabs", "blocks"):
            code, msg = r[form]
            assert code == _lib.NK_E_ARG and "one rank" in msg, r
