"""GPU: the fused launches the solvers issue for the ten older kinds (1D and 2D Bratu; heat 2D and 3D under G_Euler!,
G_Midpoint! and G_Trapezoid! with bc_zero! and bc_periodic!) and the per-pass k_mgs_pass chain, at the shapes where
the row march changes behaviour, against references that do not depend on the oracle's device-order emulation.

The solvers never launch the plain stencils the pointwise tests check: they launch Jv with a dot epilogue (with and
without V_k stored: EPI_DOTVS, EPI_DOTV, EPI_DOT), the restart residual (EPI_RESID) and the FD forms that recompute
F(u) (F0R), each a compiled kernel of its own, and then the k_mgs_pass chain.  Here each of them is held to

  * the Arnoldi relation on the stored basis (tests/test_hip_bratu3d.py, section 2: check_arnoldi_step) with
    w = J V_k from the oracle's pointwise restatement in its default mode -- oc.jv_exact / oc.jv_fd, which the
    pointwise kernels equal bit for bit -- applied to the stored V_k;
  * math.fsum bounds on the fused reductions (bratu3d_ref.reduction_bound);
  * a replay of the MGS sweep with the device's own scalars through the fma restatement oc.axpy;

and only then, last, whole solves are compared bit for bit with the oracle's device-order mode at the same shapes,
so that a disagreement there can be assigned to a side.  One form has no reference here that is independent of that
emulation: the FD restart residual (EPI_RESID with MODE_JFD, and its F0R instance).  The relation that holds the exact
one is linear in J, and the FD quotient's truncation error is far above any rounding bound; it runs in the whole
solves only, where its kernel name is asserted whenever a second cycle ran.

Shapes beyond test_hip_schemes.py's: 257 x 9 (VEC 1 with two x-tiles), 128 x 9 (the last column on lane 63 of a
wave: no right neighbour, or the periodic wrap, on the wave's last lane), 129 x 5 x 18 (VEC 1 with three x-tiles, two
y-tiles and two z-chunks), 128 x 6 x 18 (lane 63 with two z-chunks) and 1D grids around the 256-point block.

Every tolerance is a rounding-analysis bound with u = 2^-53, derived where it is used or in the test it is taken from.
tests/test_fused_checks_cpu.py feeds the checkers of this file a numpy stand-in for the device and shows that each
of a list of kernel mistakes is rejected.
"""
import math

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from bratu3d_ref import reduction_bound
from oracle import oracle as oc
from test_hip_bratu3d import Prof, U, check_arnoldi_step, fd_step, ld_fit  # noqa: F401  (ld_fit: check_arnoldi_step's fit)
from test_hip_schemes import SHAPES2, SHAPES3, device_residual

pytestmark = pytest.mark.gpu

MODE_RES, MODE_JEXACT, MODE_JFD = 0, 1, 2
EPI_NONE, EPI_SUMSQ, EPI_DOT, EPI_RESID, EPI_DOTV, EPI_DOTVS = range(6)
L = np.longdouble

SH1 = [(5,), (256,), (257,), (513,)]
SH2 = SHAPES2 + [(257, 9), (128, 9)]
SH3 = SHAPES3 + [(129, 5, 18), (128, 6, 18)]
HEAT = [("euler", 0.5), ("midpoint", 0.3), ("trapezoid", 0.5)]
# the restart-residual form: per dimension the minimal grid, a VEC 2 partial tile, the VEC 1 multi-tile shape and
# the lane-63 shape (1D: below, at and either side of the 256-point block)
RESID_SHAPES = set(SH1) | {(3, 3), (130, 67), (257, 9), (128, 9), (3, 3, 3), (33, 17, 9), (129, 5, 18), (128, 6, 18)}


@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def dev(a):
    return ah.DeviceArray.from_numpy(np.ascontiguousarray(a))


class Case:
    """one kind / boundary / shape: the oracle's problem, the point u of the linearisation, and the test id"""

    def __init__(self, name, shape, P, u):
        self.name, self.shape, self.P, self.u = name, shape, P, u
        self.id = f"{name}-{'x'.join(map(str, shape))}"
        u.flags.writeable = False

    def device(self):
        """(F, p): the device residual object and its parameter tuple"""
        P = self.P
        if P.kind == oc.BRATU1D:
            return ah.bratu_, (P.hx, P.lam)
        if P.kind == oc.BRATU2D:
            return ah.bratu2d_, (P.hx, P.hy, P.lam)
        return device_residual(P)

    def operator(self, jv):
        """J(u) on the device with res = F(u), and b = F(u) on the host (bit for bit the oracle's)"""
        F, p = self.device()
        ud = dev(self.u)
        res = ud.zero()
        F(res, ud, p)
        b = res.to_numpy()
        assert np.array_equal(b, oc.residual(self.P, self.u)), "residual"
        return ah.JacobianOperator(F, res, ud, p, jv=jv), b


def cases():
    """Bratu 1D and 2D: u = sin_ic + 0.05 noise; heat 2D and 3D: u_n random normal, u = u_n + 0.01 noise, as
    test_hip_schemes.cases() builds them"""
    rng = np.random.default_rng(17)
    out = []
    for shape in SH1:
        P = oc.bratu1d(*shape)
        out.append(Case("bratu1d", shape, P, oc.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)))
    for shape in SH2:
        P = oc.bratu2d(*shape)
        out.append(Case("bratu2d", shape, P, oc.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)))
    for scheme, alpha in HEAT:
        for bc in (oc.BC_ZERO, oc.BC_PERIODIC):
            for shape in SH2 + SH3:
                un = rng.standard_normal(shape[::-1])
                mk = oc.heat2d_euler if len(shape) == 2 else oc.heat3d_euler
                P = mk(*shape, un=un, scheme=scheme, bc=bc, alpha=alpha)
                out.append(Case(f"{scheme}-bc{bc}", shape, P, un + 0.01 * rng.standard_normal(un.shape)))
    return out


CASES = cases()
IDS = [c.id for c in CASES]
RESID_CASES = [c for c in CASES if c.shape in RESID_SHAPES]


def kernel_name(P, mode, epi, f0r=False):
    """the instantiation a launch must have run: k_st1d<MODE, EPI>, k_st2d<KIND, MODE, EPI, VEC, PER, F0R> or
    k_st3l<KIND, MODE, EPI, VEC, PER, NW, F0R, BLK> (the product's 4-row tiles, one rank)"""
    tf = {True: "true", False: "false"}
    if P.dim == 1:
        return f"nk::k_st1d<{mode}, {epi}>"
    vec, per = (2 if P.nx % 2 == 0 else 1), tf[P.bc == oc.BC_PERIODIC]
    if P.dim == 2:
        return f"nk::k_st2d<{P.kind}, {mode}, {epi}, {vec}, {per}, {tf[f0r]}>"
    return f"nk::k_st3l<{P.kind}, {mode}, {epi}, {vec}, {per}, 4, {tf[f0r]}, false>"


def f0r_policy(P, launch):
    """st_plan's default policy (csrc/nk_plan.hpp) for an FD launch whose F0 is the library's own F(u): 2D heat
    always; 2D Bratu where the launch also stores V_k; 3D G_Euler! except the V_1 step; never in 1D"""
    if P.dim == 1:
        return False
    stores_v = launch.endswith("_dot_v1") or launch.endswith("_dot_norm")
    if P.dim == 2:
        return P.kind != oc.BRATU2D or stores_v
    return P.kind == oc.HEAT3D_EULER and not launch.endswith("_dot_v1")


# ----------------------------------------------------------------------------- 1. Jv + dot, V_k stored
FORMS = [("exact", False), ("fd", False), ("fd", True)]


@pytest.mark.parametrize("jv,flag", FORMS, ids=["exact", "fd", "fd-f0r"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gmres_fused_jv_forms(ctx, case, jv, flag):
    """Jv + dot with V_k stored, as GMRES launches it: step 1 (EPI_DOTVS: V_1 = b / beta stored, its own dot partner)
    and steps 2 and 3 (EPI_DOTV: partner V_1, V_k = q / h stored by the launch -- at these sizes the resident sweep
    never applies, so no step reads a V_k stored elsewhere).  FD runs with F0 read and with F0 declared to be the
    library's F(u), where the launches the policy picks must be the F0R instances.  V_1 is b / beta bit for bit; the
    output vector and the fused reduction of steps 1 and 2 are held to the Arnoldi relation of
    test_hip_bratu3d.check_arnoldi_step, with w from the oracle's pointwise restatement applied to the stored V_k."""
    P, u = case.P, case.u
    J, b = case.operator(jv)
    unorm = float(np.linalg.norm(u))
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=5))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, itmax=3, atol=0.0, rtol=0.0, history=True, _u_norm=unorm, _f0_is_residual=flag)
    mode = MODE_JEXACT if jv == "exact" else MODE_JFD
    ran = {}
    for launch, epi, count in ((f"jv_{jv}_dot_v1", EPI_DOTVS, 1), (f"jv_{jv}_dot_norm", EPI_DOTV, None)):
        ran[launch] = pr.ran(launch, kernel_name(P, mode, epi, flag and f0r_policy(P, launch)), count)
    assert f"jv_{jv}_dot" not in pr.read, sorted(pr.read)  # no step found its V_k in place
    V = [ws.basis(i).to_numpy() for i in range(3)]
    np.testing.assert_array_equal(V[0], b / ws.stats.residuals[0])
    if jv == "exact":
        apply = lambda v: oc.jv_exact(P, u, v)  # noqa: E731
    else:
        apply = lambda v: oc.jv_fd(P, u, v, b, fd_step(unorm, 1.0))  # noqa: E731
    print(f"{case.id} {jv} f0_is_residual={flag}: ran {ran}")
    for k in (1, 2):
        check_arnoldi_step(V, k, apply(V[k - 1]), f"{case.id} {jv} step {k}")
    ws.free()


# ----------------------------------------------------------------------------- 2. Jv + dot, nothing stored
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jacobi_gmres_plain_jv_dot(ctx, case):
    """EPI_DOT with a partner other than its input and nothing stored: GMRES with N = Jacobi applies J to
    z_k = d .* V_k with <V_1, J z_k> fused.  Exact Jv (the FD step of this form takes ||z_k|| from a device reduction
    the host cannot repeat bit for bit; test_cg_jv_dot_reduction has the FD instance).  Steps 1 and 2: the output
    vector and the reduction by the Arnoldi relation, with w = J (d .* V_k) from the restatement."""
    P, u = case.P, case.u
    J, b = case.operator("exact")
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=5))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, itmax=3, atol=0.0, rtol=0.0, history=True, N=ah.jacobi(J))
    pr.ran("jv_exact_dot", kernel_name(P, MODE_JEXACT, EPI_DOT))
    assert "jv_exact_dot_v1" not in pr.read and "jv_exact_dot_norm" not in pr.read, sorted(pr.read)
    V = [ws.basis(i).to_numpy() for i in range(3)]
    np.testing.assert_array_equal(V[0], b / ws.stats.residuals[0])
    d = oc.jacobian_diag(P, u, reciprocal=True)
    for k in (1, 2):
        check_arnoldi_step(V, k, oc.jv_exact(P, u, d * V[k - 1]), f"{case.id} N=jacobi step {k}")
    ws.free()


# ----------------------------------------------------------------------------- 3. CG's <p, J p>
def check_cg_reduction(b, Jb, x, beta, what):
    """CG's <p, J p> after one step from x = 0 (test_hip_bratu3d.test_cg_jv_dot_reduction): p = b and x = alpha b with
    alpha = gamma / <p, J p>, gamma = beta^2, so <p, J p> is observed as beta^2 / alpha to within 8 units of 2^-53 (the
    square root and the square of gamma, the product alpha b_i, the two quotients) and must lie within
    n 2^-53 sum|terms| of math.fsum over the restatement's terms b_i (J b)_i plus that.  J is negative definite."""
    i = np.unravel_index(np.argmax(np.abs(b)), b.shape)
    alpha = x[i] / b[i]
    S, B = reduction_bound(b * Jb)
    got = beta ** 2 / alpha
    allowed = B + 8 * U * abs(S)
    print(f"{what}: <p, Jp> observed {got:.17g}, fsum {S:.17g}, |diff| {abs(got - S):.3e} (allowed {allowed:.3e}, "
          f"ratio {abs(got - S) / allowed:.3f})")
    assert S < 0.0, what
    assert abs(got - S) <= allowed, what


@pytest.mark.parametrize("jv,flag", FORMS, ids=["exact", "fd", "fd-f0r"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cg_jv_dot_reduction(ctx, case, jv, flag):
    """EPI_DOT with a partner, nothing stored, both Jv modes (FD also with F0 recomputed where the policy picks it):
    one CG step.  FD: ||p|| is the same device reduction as gamma, so the step is eps(||u||, sqrt(gamma)) with ||u||
    handed to the solve."""
    P, u = case.P, case.u
    J, b = case.operator(jv)
    unorm = float(np.linalg.norm(u))
    ws = ah.krylov_workspace("cg", ah.KrylovConstructor(J.res))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, itmax=1, atol=0.0, rtol=0.0, history=True, _u_norm=unorm, _f0_is_residual=flag)
    mode = MODE_JEXACT if jv == "exact" else MODE_JFD
    pr.ran(f"jv_{jv}_dot", kernel_name(P, mode, EPI_DOT, flag and f0r_policy(P, f"jv_{jv}_dot")), 1)
    x, beta = ws.x.to_numpy(), ws.stats.residuals[0]
    ws.free()
    Jb = oc.jv_exact(P, u, b) if jv == "exact" else oc.jv_fd(P, u, b, b, fd_step(unorm, beta))
    check_cg_reduction(b, Jb, x, beta, f"{case.id} {jv} f0_is_residual={flag}")


# ----------------------------------------------------------------------------- 4. the restart residual
def jacobian_entries(P, u):
    """J(u)'s entries from the oracle: (diag, [(numpy axis, off-diagonal)]).  The diagonal is oc.jacobian_diag; the
    off-diagonals are constant per axis, read from the exact tangent of a unit vector at its neighbour (periodic: the
    wrap carries the same entry)."""
    d = oc.jacobian_diag(P, u)
    e = np.zeros(P.shape)
    at = tuple(1 for _ in P.shape)
    e[at] = 1.0
    w = oc.jv_exact(P, u, e)
    offs = []
    for ax in range(P.dim):
        nb = list(at)
        nb[ax] = 2
        offs.append((ax, float(w[tuple(nb)])))
    return d, offs


def stencil_matvec(P, d, offs, x, mag=False):
    """J x (or |J| |x|) from J's entries in long double (host rounding is then negligible): the diagonal plus, per
    axis, the off-diagonal times the two neighbours -- zero ghosts, or the periodic wrap"""
    xa = (np.abs(x) if mag else x).astype(L)
    out = (np.abs(d) if mag else d).astype(L) * xa
    for ax, c in offs:
        if P.bc == oc.BC_PERIODIC:
            nb = np.roll(xa, 1, axis=ax) + np.roll(xa, -1, axis=ax)
        else:
            q = np.pad(xa, [(1, 1) if a == ax else (0, 0) for a in range(xa.ndim)])
            lo = [slice(None)] * xa.ndim
            hi = [slice(None)] * xa.ndim
            lo[ax], hi[ax] = slice(0, -2), slice(2, None)
            nb = q[tuple(lo)] + q[tuple(hi)]
        out = out + L(abs(c) if mag else c) * nb
    return out


def check_restart_residual(P, u, b, xf, V, what):
    """The relation of test_hip_ignition.test_restart_residual_form.  GMRES(2) with itmax = 3: cycle 2 starts from
    w = b - J x_1 (EPI_RESID), stores V = w / rNorm and ends after one step with x_f = x_1 + y V.  So
        b - J (x_f - y V) - beta V = e,
        |e| <= (D + 4) u |J| (|x_f| + |y V|) + 2 u |beta V|,   u = 2^-53
    D roundings of the stencil's own arithmetic against the exact product with J's entries (the deepest path of a
    term through the point formula), one of the subtraction from b, one of the division, and |J| times the two
    roundings of the x update.  2D: D = 8 as that test counts it (e - 2c, + w, / h^2, l_x + l_y, the coefficient a,
    the step, u_n +, - w for the heat schemes; Bratu's path is shorter), D + 4 = 12.  3D: the Laplacian is
    (l_x + l_y) + l_z, one addition more on the path: D = 9, 13.  1D: no sum of axis terms, one fewer: D = 7, 11.
    y and beta are not observable, so they are fitted by least squares in long double, whose residual is below the
    device's own e in the 2-norm."""
    d, offs = jacobian_entries(P, u)
    count = {1: 11, 2: 12, 3: 13}[P.dim]
    r0 = (b.astype(L) - stencil_matvec(P, d, offs, xf)).reshape(-1)
    JV, Vl = stencil_matvec(P, d, offs, V).reshape(-1), V.astype(L).reshape(-1)
    # the 2 x 2 normal equations of min || r0 + y JV - beta V ||
    g11, g12, g22 = np.dot(JV, JV), -np.dot(JV, Vl), np.dot(Vl, Vl)
    t1, t2 = -np.dot(JV, r0), np.dot(Vl, r0)
    det = g11 * g22 - g12 * g12
    y, beta = (t1 * g22 - t2 * g12) / det, (g11 * t2 - g12 * t1) / det
    r = r0 + y * JV - beta * Vl
    E = (count * U * stencil_matvec(P, d, offs, np.abs(xf) + abs(float(y)) * np.abs(V), mag=True).reshape(-1) +
         2 * U * abs(beta) * np.abs(Vl))
    rn, En = float(np.sqrt(np.dot(r, r))), float(np.sqrt(np.dot(E, E)))
    print(f"{what}: y {float(y):.6g}, beta {float(beta):.6g}, ||r|| {rn:.3e} (allowed {En:.3e}, ratio {rn / En:.3f})")
    assert beta > 0.0, what
    assert rn <= En, what


@pytest.mark.parametrize("case", RESID_CASES, ids=[c.id for c in RESID_CASES])
def test_restart_residual_form(ctx, case):
    """w = b - J x with ||w||^2 fused (EPI_RESID), as a restarted GMRES cycle launches it, exact Jv: see
    check_restart_residual"""
    P, u = case.P, case.u
    J, b = case.operator("exact")
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=2))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, restart=True, itmax=3, atol=0.0, rtol=0.0, history=True)
    pr.ran("jv_exact_resid", kernel_name(P, MODE_JEXACT, EPI_RESID), 1)
    xf, V = ws.x.to_numpy(), ws.basis(0).to_numpy()
    ws.free()
    check_restart_residual(P, u, b, xf, V, case.id)


# ----------------------------------------------------------------------------- 5. whole solves, device order
# exact, FD, FD with reorthogonalisation (GMRES only: 1D Bratu runs CG, which has no such keyword)
SOLVES = [pytest.param(c, jv, reorth, id=f"{c.id}-{jv}{'-reorth' if reorth else ''}")
          for c in CASES for jv, reorth in (("exact", False), ("fd", False), ("fd", True)) if not (reorth and c.P.dim == 1)]


@pytest.mark.parametrize("case,jv,reorth", SOLVES)
def test_whole_solve_bitwise_in_device_order(ctx, case, jv, reorth):
    """One restarted solve (GMRES(10), 35 steps, atol = rtol = 0; CG for 1D Bratu) against the oracle in the device's
    reduction order: the residual history and x bit for bit.  The four tests above hold the same launches to
    references that do not depend on that emulation, so a disagreement here at a shape they pass lies in the
    emulation (oracle/nk_oracle.c), one they fail in the kernels."""
    P, u = case.P, case.u
    cg = P.dim == 1
    J, b = case.operator(jv)
    kw = dict(atol=0.0, rtol=0.0, itmax=35)
    if not cg:
        kw.update(restart=True, reorthogonalization=reorth)
    ws = ah.krylov_workspace("cg" if cg else "gmres", ah.KrylovConstructor(J.res, memory=10))
    # FD: F0 is the library's own F(u), declared so -- the launches the policy picks (the FD restart residual among
    # them) then run as their F0R instances, the same bits as with F0 read (tests/test_hip_f0r.py)
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, J.res, history=True, _f0_is_residual=jv == "fd", **kw)
    launch = f"jv_{jv}_resid"
    assert cg or launch in pr.read or ws.stats.niter <= 10, (ws.stats.niter, sorted(pr.read))  # a second cycle ran it
    if launch in pr.read:
        pr.ran(launch, kernel_name(P, MODE_JEXACT if jv == "exact" else MODE_JFD, EPI_RESID, jv == "fd" and f0r_policy(P, launch)))
    x, hist = ws.x.to_numpy(), np.array(ws.stats.residuals)
    path = ctx.path_info()
    ws.free()
    oc.set_devred(True, cus=path["resident_blocks"] or 256)
    try:
        xo, so, ho = oc.krylov_solve(P, u, b, algo="cg" if cg else "gmres", jv=jv, F0=b, memory=10, **kw)
    finally:
        oc.set_devred(False)
    print(f"{case.id} {jv} reorth={reorth}: niter {ws.stats.niter} (oracle {so['niter']}), last ||r|| {hist[-1]:.6e} "
          f"(oracle {ho[-1]:.6e}), max|x - xo| {np.max(np.abs(x - xo)):.3e}")
    assert ws.stats.niter == so["niter"]
    np.testing.assert_array_equal(hist, ho)
    np.testing.assert_array_equal(x, xo)


# ----------------------------------------------------------------------------- 6. the MGS chain as a primitive
MGS_N = [1, 2, 3, 511, 512, 513, 2047, 2048, 2049, 5001, 4198401]


def norm_interval(q):
    """[lo, hi] for RN(sqrt(s)), s any-order sum of q_i^2: reduction_bound carried through the square root (monotone,
    one rounding), as test_hip_bratu3d.test_residual_norm_fused"""
    S, B = reduction_bound(q * q)
    return math.sqrt(max(S - B, 0.0)) * (1 - 2.0 ** -52), math.sqrt(S + B) * (1 + 2.0 ** -52)


def check_mgs_replay(q0, V, h, qf, what):
    """One sweep of the chain, replayed on the host with the device's own scalars: pass i computes h_i = <V_i, q_{i-1}>
    and q_i = fma(-h_i, V_i, q_{i-1}) = oc.axpy(-h_i, V_i, q_{i-1}) (the restatement test_blas1_parity holds to the
    kernels bit for bit).  The final q equals the replay bit for bit; every h_i lies within reduction_bound of fsum
    over the terms V_i q_{i-1} of the replayed q_{i-1}; h_{k+1} = ||q_k|| within norm_interval."""
    k = len(V)
    q = np.array(q0, dtype=np.float64)
    for i in range(k):
        S, B = reduction_bound(V[i] * q)
        print(f"{what}: h_{i + 1} {h[i]:.17g}, fsum {S:.17g}, |diff| {abs(h[i] - S):.3e} (allowed {B:.3e})")
        assert abs(h[i] - S) <= B, (what, i)
        q = oc.axpy(-h[i], V[i], q)
    assert np.array_equal(qf, q), (what, int(np.sum(qf != q)), np.flatnonzero(qf != q)[:4])
    lo, hi = norm_interval(q)
    print(f"{what}: h_{k + 1} {h[k]:.17g}, allowed [{lo:.17g}, {hi:.17g}]")
    assert lo <= h[k] <= hi, what


def check_mgs_reorth(q0, V, h, qf, what):
    """Two sweeps (reorthogonalisation): only H_i = h_i^(1) + h_i^(2) comes back, so nothing can be replayed; the
    reference is the same two sweeps in long double, q_t and h_t for the passes t = 1 .. 2k (v_t = V_((t-1) mod k)+1).

    Bound.  The device's pass t computes hh_t = <v_t, qq_{t-1}> + rho_t with |rho_t| <= B_t, the reduction bound
    n u sum_i |v_t,i qq_{t-1},i|, and qq_t = fma(-hh_t, v_t, qq_{t-1}), one rounding per element: qq_t =
    qq_{t-1} - hh_t v_t + e_t, |e_t,i| <= u |qq_t,i|.  With delta_t = qq_t - q_t:
        hh_t - h_t = <v_t, delta_{t-1}> + rho_t
        delta_t    = (I - v_t v_t^T) delta_{t-1} - rho_t v_t + e_t
    and ||I - v v^T||_2 = 1 for any v with ||v||^2 <= 2 -- unit norm is all the bound needs of V.  So with D_0 = 0
        |hh_t - h_t| <= ||v_t|| D_{t-1} + B_t                              (what the earlier passes hand on + its own)
        D_t = (D_{t-1} + ||v_t|| B_t + u ||q_t||) / (1 - u)  >=  ||delta_t||
    where B_t is evaluated on the reference's q_{t-1}: sum|v qq| <= sum|v q| + ||v|| D_{t-1}.  The returned
    H_i = RN(hh_i + hh_{k+i}) adds u |H_i|:
        |H_i - (h_i + h_{k+i})| <= (||V_i|| D_{i-1} + B_i) + (||V_i|| D_{k+i-1} + B_{k+i}) + u |H_i|
        ||qq_2k - q_2k||_2 <= D_2k
    and h_{k+1} = ||qq_2k|| is held to the device's own final q by norm_interval."""
    k, n = len(V), q0.size
    Vl = [v.astype(L) for v in V]
    vn = [float(np.sqrt(np.dot(v, v))) for v in Vl]
    q = q0.astype(L)
    D, hsum, slack = 0.0, [L(0)] * k, [0.0] * k
    for t in range(2 * k):
        i = t % k
        B = n * U * (float(np.sum(np.abs(Vl[i] * q))) + vn[i] * D)
        ht = np.dot(Vl[i], q)
        hsum[i] = hsum[i] + ht
        slack[i] += vn[i] * D + B
        q = q - ht * Vl[i]
        D = (D + vn[i] * B + U * float(np.sqrt(np.dot(q, q)))) / (1.0 - U)
    for i in range(k):
        allowed = slack[i] + U * abs(h[i])
        diff = abs(float(L(h[i]) - hsum[i]))
        print(f"{what}: H_{i + 1} {h[i]:.17g}, long double {float(hsum[i]):.17g}, |diff| {diff:.3e} (allowed {allowed:.3e})")
        assert diff <= allowed, (what, i)
    dq = qf.astype(L) - q
    dn = float(np.sqrt(np.dot(dq, dq)))
    print(f"{what}: ||q - long double|| {dn:.3e} (allowed {D:.3e}, ||q|| {float(np.sqrt(np.dot(q, q))):.3e})")
    assert dn <= D, what
    lo, hi = norm_interval(qf)
    print(f"{what}: h_{k + 1} {h[k]:.17g}, allowed [{lo:.17g}, {hi:.17g}]")
    assert lo <= h[k] <= hi, what


def mgs_inputs(n, k, reorth):
    """q random with a marked last element (2.0); V_i of unit norm.  Without reorthogonalisation the V_i are random (not
    orthogonal: the replay needs nothing of them), each with a last element of weight 0.4, so that a dropped tail term
    is far outside every bound at any n.  With it they are orthonormal (QR) as far as n allows (n < k: the first n);
    the QR keeps that weight only in V_1 (the later columns' last elements are what the orthogonalisation leaves), so
    there the tail is marked by V_1 and by q."""
    rng = np.random.default_rng(1000 * k + n % 997 + (7 if reorth else 0))
    q = rng.standard_normal(n)
    q[-1] = 2.0
    A = rng.standard_normal((n, k))
    A[-1, :] = 0.4 * np.linalg.norm(A[:-1, :], axis=0) * np.where(rng.random(k) < 0.5, -1.0, 1.0) if n > 1 else 1.0
    if reorth:
        Q, _ = np.linalg.qr(A[:, :min(n, k)])
        A[:, :Q.shape[1]] = Q
    return q, [np.ascontiguousarray(A[:, i] / np.linalg.norm(A[:, i])) for i in range(k)]


@pytest.mark.parametrize("reorth", [False, True], ids=["sweep", "reorth"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", MGS_N)
def test_mgs_chain_replay(ctx, n, k, reorth):
    """nk_mgs_step always runs the k_mgs_pass chain.  n: the odd tail; n < 512, where the unrolled loop never runs;
    2047 / 2048 / 2049, where the reduction grid goes from one block to two; 4198401, odd and above the 2048-block cap,
    where the block-contiguous chunks (1280 double2 each) leave blocks 1640 to 2047 empty.  k = 1: the sweep is the
    HAS_NEXT = false instance alone."""
    q0, V = mgs_inputs(n, k, reorth)
    g = ah.Grid.full(n)
    Vd = [ah.DeviceArray.from_numpy(v, g) for v in V]
    qd = ah.DeviceArray.from_numpy(q0, g)
    with Prof(ctx) as pr:
        h = ah.mgs_step_(Vd, qd, reorthogonalization=reorth)
    np_ = 2 * k if reorth else k  # the chain: np - 1 passes with a next dot (HAS_NEXT), one with the norm
    pr.ran("mgs_pass_last", None, 1)
    if np_ > 1:
        pr.ran("mgs_pass", None, np_ - 1)
    else:
        assert "mgs_pass" not in pr.read, sorted(pr.read)
    (check_mgs_reorth if reorth else check_mgs_replay)(q0, V, h, qd.to_numpy(), f"n {n} k {k}")
