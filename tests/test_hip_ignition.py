"""GPU: the 2D ignition kinds (NK_IGNITION2D_EULER / _MIDPOINT / _TRAPEZOID, ah.ignition_) -- the k_st2d instantiations
of the kinds, diag(J) and the preconditioners, the Newton drivers, `solve`'s time loop and the multigrid V-cycle.

The reference is the numpy restatement of tests/ignition_ref.py (F, the exact tangent and the FD quotient in the
kernels' association, with oracle.exp = the library's correctly rounded exp).  Every pointwise comparison is
np.array_equal -- no tolerance; reductions are held to n 2^-53 sum|terms| of math.fsum; the fused Jv launches of the
solvers to the Arnoldi relation of tests/test_hip_bratu3d.py; whole solves to the bound that follows from J being
symmetric and definite at the root (the solver's tolerance over the eigenvalue of J nearest zero).
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
import ignition_ref as ig
from ariadne_hip import _lib
from oracle import oracle as oc
from test_hip_bratu3d import Prof, U, check_arnoldi_step, fd_step, same
from test_hip_exp_rare import EPS, plant2d, ziv_fixture
from test_hip_multigrid import Cycle
from test_hip_multigrid_semi import LevelCycle, plan_semi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# test_hip_schemes.SHAPES2: VEC 1 / 2, partial waves, a second x-tile, a last tile of few rows, the minimal grid
SHAPES2 = [(40, 40), (130, 67), (129, 9), (514, 5), (3, 3), (64, 33)]
SCHEMES = [("euler", 0.5), ("midpoint", 0.5), ("midpoint", 0.3), ("trapezoid", 0.5)]
G = {"euler": ah.G_Euler_, "midpoint": ah.G_Midpoint_, "trapezoid": ah.G_Trapezoid_}
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


def device_residual(P):
    """(F, p) of the restatement's problem: the bound residual object and newton_krylov_'s parameter tuple"""
    g = G[P.scheme]
    F = (g(alpha=P.alpha) if P.scheme == "midpoint" else g).bind(ah.ignition_)
    return F, (dev(P.un), P.dt, None, (*P.fp, ah.bc_zero_), 0.0)


def operator(P, u, jv="exact"):
    F, p = device_residual(P)
    ud = dev(u)
    res = ud.zero()
    F(res, ud, p)
    return ah.JacobianOperator(F, res, ud, p, jv=jv)


def kernel_name(P, mode, epi):
    """the instantiation a launch must have run: k_st2d<KIND, MODE, EPI, VEC, PER, F0R> -- never periodic, never F0R"""
    return f"nk::k_st2d<{P.kind}, {mode}, {epi}, {2 if P.nx % 2 == 0 else 1}, false, false>"


def steps_of(shape, which):
    """(a, Δt): the explicit limit of heat_2D.jl:72 with a = 0.01, or one stiff value a Δt / h^2 = 10 with a = 1"""
    hx, hy = 1.0 / (shape[0] + 1), 1.0 / (shape[1] + 1)
    return (0.01, oc.heat_dt_2d(hx, hy, 0.01)) if which == "explicit" else (1.0, 10.0 * min(hx, hy) ** 2)


def problem(shape, scheme, alpha, which, seed, lam=ig.LAM):
    """u_n a random normal field, u = u_n + 0.01 noise, v random"""
    rng = np.random.default_rng(seed)
    un = rng.standard_normal(shape[::-1])
    a, dt = steps_of(shape, which)
    P = ig.Problem(*shape, scheme, lam=lam, a=a, dt=dt, alpha=alpha, un=un)
    return P, un + 0.01 * rng.standard_normal(un.shape), rng.standard_normal(un.shape)


def sid(shape):
    return "x".join(map(str, shape))


# ----------------------------------------------------------------------------- 1. pointwise, bit for bit
def pointwise(ctx, P, u, v, eq=np.array_equal, eps=EPS):
    F, p = device_residual(P)
    ud, vd = dev(u), dev(v)
    res, out = ud.zero(), ud.zero()
    with Prof(ctx) as pr:
        F(res, ud, p)
    pr.ran("residual", kernel_name(P, MODE_RES, EPI_NONE), 1)
    F0 = ig.residual(P, u)
    assert eq(res.to_numpy(), F0), "residual"
    with Prof(ctx) as pr:
        ah.mul_(out, ah.JacobianOperator(F, res, ud, p, jv="exact"), vd)
    pr.ran("jv_exact", kernel_name(P, MODE_JEXACT, EPI_NONE), 1)
    assert eq(out.to_numpy(), ig.jv_exact(P, u, v)), "exact Jv"
    Jfd = ah.JacobianOperator(F, res, ud, p, jv="fd")
    with Prof(ctx) as pr:
        ah.mul_(out, Jfd, vd, eps=eps)
    pr.ran("jv_fd", kernel_name(P, MODE_JFD, EPI_NONE), 1)
    assert eq(out.to_numpy(), ig.jv_fd(P, u, v, F0, eps)), "FD Jv"
    return F0, Jfd, vd, out


@pytest.mark.parametrize("which", ["explicit", "stiff"])
@pytest.mark.parametrize("shape", SHAPES2, ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES, ids=[f"{s}{a if s == 'midpoint' else ''}" for s, a in SCHEMES])
def test_pointwise_bitwise(ctx, scheme, alpha, shape, which):
    P, u, v = problem(shape, scheme, alpha, which, 100 + shape[0])
    F0, Jfd, vd, out = pointwise(ctx, P, u, v)
    # eps <= 0: the library's step rule, sqrt(eps_mach) max(1, ||u||) / ||v|| on its own two norms
    step = fd_step(ah.knorm(P.n, Jfd.u), ah.knorm(P.n, vd))
    ah.mul_(out, Jfd, vd)
    assert np.array_equal(out.to_numpy(), ig.jv_fd(P, u, v, F0, step)), "FD Jv, the library's step"
    ah.mul_(out, Jfd, vd, eps=-1.0)
    assert np.array_equal(out.to_numpy(), ig.jv_fd(P, u, v, F0, step)), "FD Jv, eps < 0"
    # residual + norm in one launch: the vector bitwise, the sum of squares within n 2^-53 sum|terms| of fsum
    F, p = device_residual(P)
    res = Jfd.u.zero()
    with Prof(ctx) as pr:
        nrm = F.residual_norm(res, Jfd.u, p)
    pr.ran("residual_norm", kernel_name(P, MODE_RES, EPI_SUMSQ), 1)
    assert np.array_equal(res.to_numpy(), F0)
    S, B = ig.reduction_bound(F0 * F0)
    lo, hi = math.sqrt(max(S - B, 0.0)) * (1 - 2.0 ** -52), math.sqrt(S + B) * (1 + 2.0 ** -52)
    print(f"{shape} {scheme}: ||F|| {nrm:.17g}, sqrt(fsum) {math.sqrt(S):.17g}, allowed [{lo:.17g}, {hi:.17g}]")
    assert lo <= nrm <= hi


def test_pointwise_bitwise_two_spacings(ctx):
    for scheme, alpha in SCHEMES:
        rng = np.random.default_rng(7)
        un = rng.standard_normal((17, 33))
        P = ig.Problem(33, 17, scheme, lam=6.0, a=0.7, dt=0.003, alpha=alpha, un=un, h=(0.031, 0.0577))
        pointwise(ctx, P, un + 0.01 * rng.standard_normal(un.shape), rng.standard_normal(un.shape))


# ----------------------------------------------------------------------------- 2. the fused forms the solvers launch
FUSED_SHAPES = [(130, 67), (129, 9)]


@pytest.mark.parametrize("jv", ["exact", "fd"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES[:2] + SCHEMES[3:], ids=["euler", "midpoint", "trapezoid"])
def test_gmres_fused_jv_forms(ctx, scheme, alpha, shape, jv):
    """Jv + dot with V_k stored, as GMRES launches it (DOTVS for V_1, then DOTV or DOT), held to the Arnoldi relation
    on the stored basis (tests/test_hip_bratu3d.py, section 2), with w from the restatement applied to the stored V_k"""
    P, u, _ = problem(shape, scheme, alpha, "stiff", 300 + shape[0])
    J = operator(P, u, jv)
    b = J.res.to_numpy()
    assert np.array_equal(b, ig.residual(P, u))
    unorm = float(np.linalg.norm(u))
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=5))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, itmax=3, atol=0.0, rtol=0.0, history=True, _u_norm=unorm)
    mode = MODE_JEXACT if jv == "exact" else MODE_JFD
    pr.ran(f"jv_{jv}_dot_v1", kernel_name(P, mode, EPI_DOTVS), 1)
    later = {k: pr.read[k]["kernel"] for k in (f"jv_{jv}_dot_norm", f"jv_{jv}_dot") if k in pr.read}
    assert later, sorted(pr.read)
    for name, kern in later.items():
        assert kern == kernel_name(P, mode, EPI_DOTV if name.endswith("_norm") else EPI_DOT), (name, kern)
    V = [ws.basis(i).to_numpy() for i in range(3)]
    np.testing.assert_array_equal(V[0], b / ws.stats.residuals[0])
    apply = (lambda v: ig.jv_exact(P, u, v)) if jv == "exact" else (lambda v: ig.jv_fd(P, u, v, b, fd_step(unorm, 1.0)))
    for k in (1, 2):
        check_arnoldi_step(V, k, apply(V[k - 1]), f"{scheme} {shape} {jv} step {k}")
    ws.free()


@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES[:2] + SCHEMES[3:], ids=["euler", "midpoint", "trapezoid"])
def test_jacobi_gmres_plain_jv_dot(ctx, scheme, alpha, shape):
    """Jv + dot with a partner other than its input and nothing stored: GMRES with N = Jacobi applies J to d .* V_k"""
    P, u, _ = problem(shape, scheme, alpha, "stiff", 350 + shape[0])
    J = operator(P, u)
    b = J.res.to_numpy()
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=5))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, itmax=3, atol=0.0, rtol=0.0, history=True, N=ah.jacobi(J))
    pr.ran("jv_exact_dot", kernel_name(P, MODE_JEXACT, EPI_DOT))
    assert "jv_exact_dot_v1" not in pr.read and "jv_exact_dot_norm" not in pr.read, sorted(pr.read)
    V = [ws.basis(i).to_numpy() for i in range(3)]
    np.testing.assert_array_equal(V[0], b / ws.stats.residuals[0])
    d = ig.jacobian_diag(P, u, reciprocal=True)
    for k in (1, 2):
        check_arnoldi_step(V, k, ig.jv_exact(P, u, d * V[k - 1]), f"{scheme} {shape} N=jacobi step {k}")
    ws.free()


@pytest.mark.parametrize("jv", ["exact", "fd"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES[:2] + SCHEMES[3:], ids=["euler", "midpoint", "trapezoid"])
def test_cg_jv_dot_reduction(ctx, scheme, alpha, shape, jv):
    """CG's <p, J p> after one step from x = 0 (p = b, x = alpha b, alpha = gamma / <p, J p>), observed as gamma / alpha
    and held to reduction_bound over the restatement's terms plus the 8 roundings of the observation
    (test_hip_bratu3d.test_cg_jv_dot_reduction)"""
    P, u, _ = problem(shape, scheme, alpha, "stiff", 400 + shape[0])
    J = operator(P, u, jv)
    b = J.res.to_numpy()
    unorm = float(np.linalg.norm(u))
    ws = ah.krylov_workspace("cg", ah.KrylovConstructor(J.res))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, itmax=1, atol=0.0, rtol=0.0, history=True, _u_norm=unorm)
    pr.ran(f"jv_{jv}_dot", kernel_name(P, MODE_JEXACT if jv == "exact" else MODE_JFD, EPI_DOT), 1)
    x = ws.x.to_numpy()
    i = np.unravel_index(np.argmax(np.abs(b)), b.shape)
    alpha_cg = x[i] / b[i]
    beta = ws.stats.residuals[0]
    Jb = ig.jv_exact(P, u, b) if jv == "exact" else ig.jv_fd(P, u, b, b, fd_step(unorm, beta))
    S, B = ig.reduction_bound(b * Jb)
    got = beta ** 2 / alpha_cg
    print(f"{scheme} {shape} {jv}: <p, Jp> observed {got:.17g}, fsum {S:.17g}, |diff| {abs(got - S):.3e} (allowed {B + 8 * U * abs(S):.3e})")
    assert S < 0.0 and abs(got - S) <= B + 8 * U * abs(S)
    ws.free()


@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES[:2] + SCHEMES[3:], ids=["euler", "midpoint", "trapezoid"])
def test_restart_residual_form(ctx, scheme, alpha, shape):
    """w = b - J x with ||w||^2 fused (the RESID epilogue), as a restarted GMRES cycle launches it.  GMRES(2) with
    itmax = 3: cycle 2 starts from w = b - J x_1, stores V = w / beta and ends after one step with x_f = x_1 + y V.  So
        b - J (x_f - y V) - beta V = e,
        |e| <= 12 u |J| (|x_f| + |y V|) + 2 u |beta V|
    (about 8 roundings of the stencil's own arithmetic against the exact product, one of the subtraction, one of the
    division, and |J| times the two roundings of the x update), u = 2^-53.  y and beta are not observable, so they are
    fitted by least squares, whose residual is below the device's own e in the 2-norm."""
    P, u, _ = problem(shape, scheme, alpha, "stiff", 450 + shape[0])
    J = operator(P, u)
    b = J.res.to_numpy()
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=2))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, restart=True, itmax=3, atol=0.0, rtol=0.0, history=True)
    pr.ran("jv_exact_resid", kernel_name(P, MODE_JEXACT, EPI_RESID), 1)
    xf, V = ws.x.to_numpy(), ws.basis(0).to_numpy()
    ws.free()
    L = np.longdouble
    d, cx, cy = ig.jacobian_diag(P, u).astype(L), L(ig.offdiag(P, P.hx)), L(ig.offdiag(P, P.hy))

    def matvec(x, mag=False):  # J x (or |J| |x|) from J's entries, in long double: host rounding is then negligible
        q = np.pad(np.abs(x) if mag else x, 1).astype(L)
        f = abs if mag else (lambda t: t)
        return f(d) * q[1:-1, 1:-1] + f(cx) * (q[1:-1, 2:] + q[1:-1, :-2]) + f(cy) * (q[2:, 1:-1] + q[:-2, 1:-1])

    r0, JV, Vl = (b.astype(L) - matvec(xf)).reshape(-1), matvec(V).reshape(-1), V.astype(L).reshape(-1)
    # the 2 x 2 normal equations of min || r0 + y JV - beta V ||
    g11, g12, g22 = np.dot(JV, JV), -np.dot(JV, Vl), np.dot(Vl, Vl)
    t1, t2 = -np.dot(JV, r0), np.dot(Vl, r0)
    det = g11 * g22 - g12 * g12
    y, beta = (t1 * g22 - t2 * g12) / det, (g11 * t2 - g12 * t1) / det
    r = r0 + y * JV - beta * Vl
    E = 12 * U * matvec(np.abs(xf) + abs(y) * np.abs(V), mag=True).reshape(-1) + 2 * U * abs(beta) * np.abs(Vl)
    rn, En = float(np.sqrt(np.dot(r, r))), float(np.sqrt(np.dot(E, E)))
    print(f"{scheme} {shape}: y {float(y):.6g}, beta {float(beta):.6g}, ||r|| {rn:.3e} (allowed {En:.3e})")
    assert beta > 0.0 and rn <= En


# ----------------------------------------------------------------------------- 3. the exp's exact phase
RARE_SHAPES = [(130, 40), (129, 19), (514, 9)]


def ordinary(C_, seed, keep=None):
    """an ordinary field on the planted grid (no plant of C_ in it); keep: points copied from C_.u"""
    x = np.random.default_rng(seed).standard_normal(C_.u.shape)
    if keep is not None:
        x[keep] = C_.u[keep]
    return x


def check_rare(C_, x, what):
    """every planted argument of the launch is rare, at most 1/8 of the rest; the count of exact-phase evaluations"""
    rare = oc.exp_rare(x)
    assert rare[C_.plants].all(), f"{what}: a planted argument is not rare"
    assert rare[~C_.plants].mean() <= 0.125, what
    assert int(rare.sum()) >= int(C_.plants.sum()) > 0, what
    return int(rare.sum())


@pytest.mark.parametrize("shape", RARE_SHAPES, ids=sid)
@pytest.mark.parametrize("where", ["euler-u", "trapezoid-u", "trapezoid-un", "midpoint-m"])
def test_exact_phase_inside_the_kernels(ctx, where, shape):
    """tests/test_hip_exp_rare.py's plant map (corners, lanes 0 / 63, one or both elements of a VEC 2 lane, the last row
    of a tile and the first of the next, a partial tile, whole rows, the exp_ziv fixture) in every argument the kind
    exponentiates: u (Euler, Trapezoid; FD with v = 0 at the plants), u_n (Trapezoid), m (Midpoint with u_n = u at the
    plants and α = 0.5, so that m is the plant exactly).  Each launch: its planted arguments are rare (oc.exp_rare on
    the host), then np.array_equal to the restatement, un-planted neighbours included."""
    C_ = plant2d(*shape)
    assert oc.exp_rare(ziv_fixture()[:16]).all()
    scheme, arg = where.split("-")
    hx, hy = 1.0 / (shape[0] + 1), 1.0 / (shape[1] + 1)
    a, dt = 1.0, 10.0 * min(hx, hy) ** 2
    if arg == "u":
        u, un = C_.u, ordinary(C_, 21)
    elif arg == "un":
        u, un = ordinary(C_, 22), C_.u
    else:
        u, un = C_.u, ordinary(C_, 23, keep=C_.plants)
    P = ig.Problem(*shape, scheme, lam=ig.LAM, a=a, dt=dt, alpha=0.5, un=un)
    v0 = C_.tangent_zero(12)
    cov = {}
    if arg == "un":  # exp(u_n) is in the residual and the FD operator (evaluated again there); v is free
        cov["exp(u_n)"] = check_rare(C_, un, "exp(u_n)")
        v = np.random.default_rng(13).standard_normal(u.shape)
    else:
        m = ig.mid(P, u)
        assert np.array_equal(m[C_.plants], C_.u[C_.plants])
        cov["exp(m)"] = check_rare(C_, m, "exp(m)")
        w = ig.mid(P, u + EPS * v0)
        assert np.array_equal(w[C_.plants], C_.u[C_.plants])
        cov["FD exp(m(w))"] = check_rare(C_, w, "FD exp(m(w))")
        v = v0
    F0, Jfd, vd, out = pointwise(ctx, P, u, v)
    if arg != "un":  # the exact tangent with v = 1 on the planted rows as well
        v1 = C_.tangent_one(14)
        ah.mul_(out, ah.JacobianOperator(Jfd.f, Jfd.res, Jfd.u, Jfd.p, jv="exact"), dev(v1))
        assert np.array_equal(out.to_numpy(), ig.jv_exact(P, u, v1)), "exact Jv, v = 1 on the patch"
        assert np.array_equal(ah.jacobian_diag(Jfd).to_numpy(), ig.jacobian_diag(P, u))
    print(where, shape, cov)


OOR = {"overflow": 710.0, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "zero": -746.0}


@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_out_of_range_arguments(ctx, scheme):
    """u = 710, NaN, +-Inf and -746 at a few points of an ordinary field, compared NaN-aware"""
    shape = (130, 40)
    rng = np.random.default_rng(77)
    un = rng.standard_normal(shape[::-1])
    u = un + 0.01 * rng.standard_normal(un.shape)
    at = {"overflow": (0, 0), "nan": (3, 126), "+inf": (12, 40), "-inf": (20, 77), "zero": (33, 100)}
    v = rng.standard_normal(un.shape)
    for name, idx in at.items():
        u[idx] = OOR[name]
        v[idx] = 0.0
    a, dt = steps_of(shape, "stiff")
    P = ig.Problem(*shape, scheme, lam=0.25, a=a, dt=dt, alpha=0.5, un=un)
    with np.errstate(all="ignore"):
        F0, Jfd, _vd, _out = pointwise(ctx, P, u, v, eq=same)
        # (G_Midpoint! exponentiates m = (u_n + 710) / 2, which does not overflow; its Inf comes from u = +Inf)
        assert np.isnan(F0[at["nan"]]) and not np.isfinite(F0[at["+inf" if scheme == "midpoint" else "overflow"]])
        assert same(ah.jacobian_diag(Jfd).to_numpy(), ig.jacobian_diag(P, u))


# ----------------------------------------------------------------------------- 5. diagonal, ILU(0), collect, batches
@pytest.mark.parametrize("shape", SHAPES2, ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES, ids=[f"{s}{a if s == 'midpoint' else ''}" for s, a in SCHEMES])
def test_jacobian_diag_bitwise(ctx, scheme, alpha, shape):
    P, u, _ = problem(shape, scheme, alpha, "stiff", 500 + shape[0], lam=6.0)
    J = operator(P, u)
    with Prof(ctx) as pr:
        d, dr = ah.jacobian_diag(J).to_numpy(), ah.jacobian_diag(J, reciprocal=True).to_numpy()
    pr.ran("jacobian_diag", None, 2)
    np.testing.assert_array_equal(d, ig.jacobian_diag(P, u))
    np.testing.assert_array_equal(dr, ig.jacobian_diag(P, u, reciprocal=True))
    e = np.zeros(P.n)
    for i in np.random.default_rng(1).integers(0, P.n, 4):  # the tangent on a unit vector, at its own point
        e[:] = 0.0
        e[i] = 1.0
        assert d.reshape(-1)[i] == ig.jv_exact(P, u, e.reshape(P.shape)).reshape(-1)[i]


def small(scheme, alpha, seed):
    rng = np.random.default_rng(seed)
    un = rng.standard_normal((7, 9))
    P = ig.Problem(9, 7, scheme, lam=6.0, a=1.0, dt=0.02, alpha=alpha, un=un, h=(0.1, 0.125))
    return P, un + 0.01 * rng.standard_normal(un.shape), rng.standard_normal(un.shape)


@pytest.mark.parametrize("scheme,alpha", SCHEMES, ids=[f"{s}{a if s == 'midpoint' else ''}" for s, a in SCHEMES])
def test_ilu0_factor_and_collect(ctx, scheme, alpha):
    P, u, v = small(scheme, alpha, 3)
    J = operator(P, u)
    N = ah.ilu0(J)
    dref = ig.ilu0_factor(P, u)
    assert np.all(np.isfinite(dref))
    np.testing.assert_array_equal(N.d.to_numpy(), dref)
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    ref = ig.jacobian(P, u)
    D = sp.diags(dref.reshape(-1))
    L = sp.identity(P.n) + sp.tril(ref, -1) @ sp.diags(1.0 / dref.reshape(-1))
    Uf = D + sp.triu(ref, 1)
    zref = spla.spsolve_triangular(Uf.tocsr(), spla.spsolve_triangular(L.tocsr(), v.reshape(-1), lower=True), lower=False)
    z = N.apply(J, dev(v)).to_numpy().reshape(-1)
    assert np.max(np.abs(z - zref)) <= 1e-12 * np.max(np.abs(zref))
    A = ah.collect(J)
    np.testing.assert_array_equal(A.toarray(), ref.toarray())
    assert A.nnz == ref.nnz
    coo = A.tocoo()
    assert set(np.unique(coo.data[coo.row != coo.col])) == {ig.offdiag(P, P.hx), ig.offdiag(P, P.hy)}
    np.testing.assert_array_equal(ah.collect(J.T).toarray(), ref.T.toarray())


@pytest.mark.parametrize("shape", [(33, 17), (130, 5)], ids=sid)
@pytest.mark.parametrize("scheme,alpha", SCHEMES, ids=[f"{s}{a if s == 'midpoint' else ''}" for s, a in SCHEMES])
def test_batched_and_transposed_mul(ctx, scheme, alpha, shape):
    """11 columns (two launches) equal the single exact / FD Jv column by column; J^T v = J v"""
    P, u, _ = problem(shape, scheme, alpha, "stiff", 600 + shape[0])
    rng = np.random.default_rng(5)
    vs = [rng.standard_normal(P.shape) for _ in range(11)]
    F0 = ig.residual(P, u)
    for jv in ("exact", "fd"):
        J = operator(P, u, jv)
        outs = [J.u.zero() for _ in vs]
        with Prof(ctx) as pr:
            ah.mul_(outs, J, [dev(v) for v in vs], eps=EPS)
        pr.ran(f"jv_{jv}_batch", None, 2)
        for o, v in zip(outs, vs):
            ref = ig.jv_exact(P, u, v) if jv == "exact" else ig.jv_fd(P, u, v, F0, EPS)
            np.testing.assert_array_equal(o.to_numpy(), ref)
    J = operator(P, u)
    out = J.u.zero()
    ah.mul_(out, J.T, dev(vs[0]))
    np.testing.assert_array_equal(out.to_numpy(), ig.jv_exact(P, u, vs[0]))
    outs = [J.u.zero() for _ in vs[:3]]
    ah.mul_(outs, J.T, [dev(v) for v in vs[:3]])
    for o, v in zip(outs, vs):
        np.testing.assert_array_equal(o.to_numpy(), ig.jv_exact(P, u, v))


# ----------------------------------------------------------------------------- 6. Newton drivers and a time step
def check_root(P, u, ustar, ev, tol, what):
    """||F(u)|| <= tol by the restatement, and ||u - u*|| <= 2 ||F(u)|| / |lambda_min|: F(u) = J (u - u*) + O(|u - u*|^2)
    with J symmetric and definite, so |u - u*| <= |F(u)| / |lambda_min| to first order; 2 covers the rest
    (tests/test_hip_bratu3d.check_root)"""
    nF = float(np.linalg.norm(ig.residual(P, u)))
    err = float(np.linalg.norm(u - ustar))
    print(f"{what}: ||F(u)|| {nF:.3e} (tol {tol:.3e}), ||u - u*|| {err:.3e} (allowed {2 * nF / abs(ev):.3e})")
    assert nF <= tol
    assert err <= 2.0 * nF / abs(ev)


def spd_jacobi(J):
    """the Jacobi M in the form CG takes: J is negative definite, cg! runs on it as on (-J) x = -b, so M = -1 ./ diag(J)"""
    d = ah.jacobian_diag(J, reciprocal=True)
    ah.kscal_(len(d), -1.0, d)
    return ah.DiagonalPreconditioner(d)


def exact_step(P, u0):
    """(u*, the eigenvalue of J(u*) nearest zero) of the step from u0: sparse-LU Newton to 1e-10 ||F(u0)|| (the
    rounding floor of F is near 1e-13 ||F(u0)|| for these steps), five orders below the solver tolerance the bound uses"""
    ustar, _k, ok, hist = ig.newton_lu(P, u0, tol_rel=1e-10, tol_abs=0.0)
    assert ok and hist[-1] <= 1e-10 * hist[0]
    return ustar, ig.eig_nearest_zero(P, ustar)


@functools.lru_cache(maxsize=None)
def step_reference(scheme):
    """(64, 33), a = 1, λ = 6, Δt = 0.05, u_n = the restatement's state after two steps of this scheme from 0"""
    P0 = ig.Problem(64, 33, scheme, lam=6.0, a=1.0, dt=0.05)
    states, _n, solved = ig.time_steps(P0, 2)
    assert all(solved)
    P = P0.with_un(states[-1])
    ustar, ev = exact_step(P, P.un)
    for x in (P.un, ustar):
        x.flags.writeable = False
    return P, ustar, ev


@pytest.mark.parametrize("jv", ["exact", "fd"])
@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_newton_drivers_agree_and_reach_the_root(ctx, scheme, jv):
    """newton_krylov_ (the Python loop) and newton_krylov_native (the C driver nk_newton_krylov) take the same Newton and
    Krylov steps and reach the root of the sparse-LU Newton; GMRES, MINRES, and CG with the Jacobi M"""
    P, ustar, ev = step_reference(scheme)
    F, p = device_residual(P)
    tol = 1e-6 * float(np.linalg.norm(ig.residual(P, P.un))) + ig.TOL_ABS
    for algo, kw in (("gmres", {}), ("minres", {}), ("cg", {"M": spd_jacobi})):
        u, r = ah.newton_krylov_(F, dev(P.un), p, tol_abs=ig.TOL_ABS, jv=jv, algo=algo, **kw)
        assert r.solved, (algo, r)
        check_root(P, u.to_numpy(), ustar, ev, tol, f"{scheme} newton_krylov_ {algo} {jv}")
        if kw:
            continue  # (the C driver takes a multigrid preconditioner only)
        un, rn = ah.newton_krylov_native(F, dev(P.un), p, tol_abs=ig.TOL_ABS, jv=jv, algo=algo)
        assert rn.solved
        check_root(P, un.to_numpy(), ustar, ev, tol, f"{scheme} newton_krylov_native {algo} {jv}")
        print(f"{scheme} {algo} {jv}: python {tuple(r.stats[:2])}, native {tuple(rn.stats[:2])}")
        assert tuple(r.stats[:2]) == tuple(rn.stats[:2])
        assert r.stats.outer_iterations >= 2  # a nonlinear step


# ----------------------------------------------------------------------------- 7. time stepping with solve
N15 = 15


def run_solve(scheme, lam, dt, nsteps, alpha=0.5, **kw):
    """(device states after each step, the per-step results) of ah.solve from u0 = 0 on 15 x 15, a = 1"""
    P = ig.Problem(N15, N15, scheme, lam=lam, a=1.0, dt=dt, alpha=alpha)
    g = G[scheme]
    states, stats = [], []
    un = dev(np.zeros(P.shape))
    ah.solve(g(alpha=alpha) if scheme == "midpoint" else g, ah.ignition_, un, (*P.fp, ah.bc_zero_), dt,
             [i * dt for i in range(nsteps + 1)], callback=lambda u: states.append(u.to_numpy().copy()), stats_out=stats, **kw)
    assert len(states) == len(stats) == nsteps
    np.testing.assert_array_equal(un.to_numpy(), states[-1])
    return P, states, stats


# the linear solves of the sub-critical run: Krylov.jl-tight (the Newton steps are then the exact Newton steps the
# restatement takes), or newton_krylov!'s default Eisenstat-Walker forcing (inexact Newton)
LINEAR = {"exact": dict(krylov_kwargs=dict(rtol=1e-10, atol=0.0, restart=True, itmax=400), memory=40), "forcing": {}}


@pytest.mark.parametrize("linear", sorted(LINEAR))
def test_solve_subcritical_euler_reaches_the_steady_state(ctx, linear):
    """λ = 3.51382, Δt = 0.05: the state relaxes to the steady Bratu solution and a time step needs no Newton step.

    The restatement is an exact Newton (sparse LU), so the +-1 comparison of the first 0-step time step is made on the
    run whose linear solves are exact too ("exact": rtol = 1e-10).  A time step starts from F(u_n) = Δt f(u_n)
    = r + (u_n - u_{n-1}) with r the residual the previous step left: nothing for an exact Newton, up to the tolerance
    6e-6 itself -- the size of the threshold -- for the default inexact Newton.  That run ("forcing") therefore gets
    there later (measured: index 25 against the restatement's 23, with 7, 7, 7, 6, ... Newton steps per time step
    against 2, 2, 2, ...); it is held to reaching a 0-step time step and to the steady-state bounds, which follow from
    the stopping rule alone."""
    P, states, stats = run_solve("euler", ig.LAM, 0.05, 30, **LINEAR[linear])
    newton = [r.stats.outer_iterations for r in stats]
    _s, ref_newton, ref_solved = ig.time_steps(P, 30)
    print(f"{linear}: device Newton steps:", newton, "\nrestatement      :", ref_newton)
    assert all(r.solved for r in stats) and all(ref_solved)
    assert newton[0] > 1 and 0 in newton and 0 in ref_newton
    k = newton.index(0)
    print(f"{linear}: first 0-step time step at index {k}, the restatement's at {ref_newton.index(0)}")
    if linear == "exact":
        assert abs(k - ref_newton.index(0)) <= 1
    # the state there is steady: ah.bratu2d_'s own residual norm <= 6e-6 / (Δt (1 - 1e-6)) ...
    ud = dev(states[k])
    nB = ah.bratu2d_.residual_norm(ud.zero(), ud, (P.hx, P.hy, P.lam))
    print(f"first 0-step time step: index {k}, ||bratu2d F|| = {nB:.3e}")
    assert nB <= ig.TOL_ABS / (0.05 * (1.0 - 1e-6))
    # ... and lies within check_root's bound of the Bratu root: J_B = (J + I) / Δt of the Euler kind, symmetric
    # negative definite below the fold
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    B = oc.bratu2d(N15, N15, lam=ig.LAM)
    JB = lambda w: ((ig.jacobian(P, w) + sp.identity(P.n)) / P.dt).tocsc()  # noqa: E731
    w = states[k].copy()
    for _ in range(20):
        w = w - spla.splu(JB(w)).solve(oc.residual(B, w).reshape(-1)).reshape(P.shape)
    assert np.linalg.norm(oc.residual(B, w)) <= 1e-10
    ev = float(spla.eigsh(JB(w), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    nF = float(np.linalg.norm(oc.residual(B, states[k])))
    err = float(np.linalg.norm(states[k] - w))
    print(f"||Bratu F|| {nF:.3e}, eigenvalue nearest zero {ev:.3f}, ||u - u*|| {err:.3e} (allowed {2 * nF / abs(ev):.3e})")
    assert ev < 0.0 and err <= 2.0 * nF / abs(ev)


@pytest.mark.parametrize("scheme", ["trapezoid", "midpoint"])
def test_solve_five_steps_follow_the_restatement(ctx, scheme):
    """every step is solved and lies within the root bound of the restatement's exact step from the same u_n"""
    P, states, stats = run_solve(scheme, ig.LAM, 0.05, 5)
    un = np.zeros(P.shape)
    for k, (u, r) in enumerate(zip(states, stats)):
        assert r.solved, (k, r)
        Pk = P.with_un(un)
        ustar, ev = exact_step(Pk, un)
        tol = 1e-6 * float(np.linalg.norm(ig.residual(Pk, un))) + ig.TOL_ABS
        check_root(Pk, u, ustar, ev, tol, f"{scheme} step {k + 1}")
        un = u


@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_solve_supercritical_marches_on(ctx, scheme):
    """λ = 10 blows up in finite time: the steps well before the restatement's first failure are solved, a later one is
    reported unsolved, and solve returns (exp overflow is arithmetic: Inf / NaN, no call raises)"""
    P, states, stats = run_solve(scheme, 10.0, 0.02, 25)
    _s, _n, ref_solved = ig.time_steps(P, 25)
    first = ref_solved.index(False)
    solved = [bool(r.solved) for r in stats]
    print(scheme, "device solved:", solved, "restatement's first failure:", first)
    assert all(solved[:first - 1])
    assert not all(solved[first - 1:])


# ----------------------------------------------------------------------------- 8. multigrid
MG_CASES = [((64, 33), "full"), ((96, 12), "semi")]


def mg_coefficients(P, u):
    """k_a = θ a Δt and s = θ Δt λ exp(m) - 1 of J = Σ k_a δ²_a + diag(s) (θ: 1, 1 - α, 1/2)"""
    theta = {"euler": 1.0, "midpoint": 1.0 - P.alpha, "trapezoid": 0.5}[P.scheme]
    return [theta * P.a * P.dt] * 2, theta * P.dt * P.lam * oc.exp(ig.mid(P, u)) - 1.0


@functools.lru_cache(maxsize=None)
def mg_reference(shape, coarsening, scheme):
    P, u, v = problem(shape, scheme, 0.3, "stiff", 700 + shape[0], lam=6.0)
    h = [P.hx, P.hy]
    k, s = mg_coefficients(P, u)

    def cyc(dt):
        if coarsening == "semi":
            return LevelCycle(plan_semi(shape, h=h), h, k, s, dt=dt)
        return Cycle(shape, h, k, s, dt=dt)

    c64 = cyc(np.float64)
    z64, zl = c64.vcycle(v), cyc(np.longdouble).vcycle(v)
    return P, u, v, z64, float(np.max(np.abs(z64 - zl)) / np.max(np.abs(zl))), c64.levels


def mg_tol():
    """16 x the restatement's own float64-against-long-double sensitivity (the largest over the cases here), the rule
    of tests/test_hip_multigrid.py and test_hip_bratu3d.mg_tol"""
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    return 16 * max(mg_reference(*c, s)[4] for c in MG_CASES for s in ig.SCHEMES)


@pytest.mark.parametrize("scheme", ig.SCHEMES)
@pytest.mark.parametrize("shape,coarsening", MG_CASES, ids=[f"{sid(s)}-{c}" for s, c in MG_CASES])
def test_vcycle_on_the_kinds_grid(ctx, shape, coarsening, scheme):
    P, u, v, zref, sens, levels = mg_reference(shape, coarsening, scheme)
    J = operator(P, u)
    vd = dev(v)
    # the level-0 diagonal is nk_jacobian_diag's: one level, one sweep from zero, omega = 1 -> z = v ./ diag(J), bitwise
    mg1 = ah.MultigridPreconditioner(J, coarse_sweeps=1, omega=1.0, max_levels=1)
    np.testing.assert_array_equal(mg1.apply(J, vd).to_numpy(), ig.jacobian_diag(P, u, reciprocal=True) * v)
    mg = ah.MultigridPreconditioner(J, coarsening=coarsening)
    assert mg.levels == [tuple(e) for e in levels]
    z = mg.apply(J, vd).to_numpy()
    err = float(np.max(np.abs(z - zref)) / np.max(np.abs(zref)))
    tol = mg_tol()
    print(f"{scheme} {shape} {coarsening}: device vs restatement {err:.3e} (allowed {tol:.1e}; this case's sensitivity {sens:.2e})")
    assert err <= tol
    mg.spd = True
    np.testing.assert_array_equal(mg.apply(J, vd).to_numpy(), -z)  # J's diagonal is negative: sigma = -1


def test_stiff_step_with_multigrid(ctx):
    """(64, 33), λ = 6, a Δt / h^2 = 800: J's condition number is about 8 a Δt / h^2 while the V-cycle's is O(1), so the
    preconditioned solve is expected to take fewer Krylov steps; both reach the root"""
    dt = 800.0 / 65.0 ** 2
    P = ig.Problem(64, 33, "euler", lam=6.0, a=1.0, dt=dt)
    ustar, ev = exact_step(P, P.un)
    F, p = device_residual(P)
    tol = 1e-6 * float(np.linalg.norm(ig.residual(P, P.un))) + ig.TOL_ABS
    kw = dict(tol_abs=ig.TOL_ABS, memory=30, krylov_kwargs={"restart": True})
    u, r = ah.newton_krylov_(F, dev(P.un), p, N=ah.multigrid, **kw)
    u0, r0 = ah.newton_krylov_(F, dev(P.un), p, **kw)
    print(f"multigrid outer {r.stats.outer_iterations} inner {r.stats.inner_iterations}; "
          f"plain outer {r0.stats.outer_iterations} inner {r0.stats.inner_iterations}")
    assert r.solved and r0.solved
    check_root(P, u.to_numpy(), ustar, ev, tol, "N = multigrid")
    check_root(P, u0.to_numpy(), ustar, ev, tol, "no N")
    assert r.stats.inner_iterations < r0.stats.inner_iterations
    un, rn = ah.newton_krylov_native(F, dev(P.un), p, N=ah.multigrid, **kw)
    assert rn.solved and tuple(rn.stats[:2]) == tuple(r.stats[:2])


# ----------------------------------------------------------------------------- 9. rejections
def test_rejections(ctx):
    lib = ah.load()
    u = ah.DeviceArray(ah.Grid.full(12, 10), ctx)
    un = ah.DeviceArray(ah.Grid.full(12, 10), ctx)
    prob = ah.ignition2d_euler_.problem(u, (un, 0.05, None, (1.0, 0.1, 0.1, 6.0, ah.bc_zero_), 0.0))

    res = u.zero()

    def call():
        rc = lib.nk_residual(ctx.handle, C.byref(prob), res.ptr, u.ptr)
        return rc, (lib.nk_last_error(ctx.handle) or b"").decode()

    assert call()[0] == _lib.NK_OK
    for kind in (20, 21, 22):
        prob.kind, prob.bc = kind, _lib.NK_BC_PERIODIC
        rc, msg = call()
        assert rc == _lib.NK_E_ARG and "periodic" in msg, (kind, rc, msg)
        h = C.c_void_p()
        rc = lib.nk_mg_create(ctx.handle, C.byref(prob), None, C.byref(h))
        assert rc == _lib.NK_E_ARG and "periodic" in (lib.nk_last_error(ctx.handle) or b"").decode()
        prob.bc, prob.nz = _lib.NK_BC_ZERO, 2
        assert call()[0] == _lib.NK_E_ARG
        prob.nz, keep = 1, prob.un
        prob.un = None
        rc, msg = call()
        assert rc == _lib.NK_E_ARG and "u_n" in msg, (rc, msg)
        prob.un = keep
    for kind in (10, 19, 23):  # the numbers around the known kinds are still unknown
        prob.kind = kind
        rc, msg = call()
        assert rc == _lib.NK_E_ARG and "unknown problem kind" in msg, (kind, rc, msg)


# ----------------------------------------------------------------------------- 10. the C binary
def test_c_binary_time_loop(ctx):
    exe = os.path.join(ROOT, "newtonkrylov.jl_amd", "bin", "ignition2d_solve")
    out = subprocess.run([exe, "40", "40", "euler", "--steps", "5", "--mg"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("step ")]
    print(out.stdout)
    assert [int(ln[1]) for ln in lines] == [1, 2, 3, 4, 5]
    assert all(ln[-2:] == ["solved", "1"] for ln in lines)
    assert int(lines[0][3]) >= 2  # a nonlinear step: more than one Newton step
