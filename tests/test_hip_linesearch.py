"""GPU: the Newton line search -- nk_residual_trial's fused kernel instances (MODE_TRIAL of k_st1d / k_st2d / k_st3l),
the drivers' backtracking branch (newton_krylov_, newton_krylov_native = nk_newton_krylov, solve), two ranks and the C++
binary.

The kernel's reference is the library itself: F(u + s v) must be, bit for bit, nk_residual_norm on the materialised
w = copy(u); nk_axpy(s, v, w) -- the residual kernels are held to the oracle by the other test files.  The drivers'
reference is a loop written here from those primitives and this file's own parab3p.  Whole solves are held to the
root of a numpy sparse-LU Newton within 2 tol / sigma_min(J(u*)): F(u) = J (u - u*) + O(|u - u*|^2), ||F(u)|| <= tol
at the end, so |u - u*| <= tol / sigma_min to first order; 2 covers the rest (test_hip_ignition.check_root).
"""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
import bratu3d_ref as b3
import ignition_ref as ig
from oracle import oracle as oc
from test_hip_exp_rare import OOR, check_args, plant1d, plant2d, plant_oor, family, same
from test_hip_schemes import SHAPES2, SHAPES3
from test_hip_schemes import device_residual as heat_residual
from test_hip_ignition import device_residual as ignition_residual
from test_hip_ignition import run_solve, spd_jacobi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = [-1.0, -0.5, -0.10476, 0.37, 0.0]
SHAPES1 = [(100,), (5,), (513,)]


@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def dev(a):
    return ah.DeviceArray.from_numpy(np.ascontiguousarray(a))


def sid(shape):
    return "x".join(map(str, shape))


# ----------------------------------------------------------------------------- 1. the kernel, bit for bit
def materialised(F, p, ud, vd, s):
    """(F(w), its norm) with w = copy(u); kaxpy!(s, v, w): the sequence a trial costs without the fused kernel"""
    w = ud.copy()
    ah.kaxpy_(len(w), s, vd, w)
    ref = ud.zero()
    n = F.residual_norm(ref, w, p)
    return ref.to_numpy(), n


def check_trials(F, p, u, v, steps=STEPS, eq=np.array_equal):
    ud, vd = dev(u), dev(v)
    out = ud.zero()
    for s in steps:
        ref, n_ref = materialised(F, p, ud, vd, s)
        out.fill_(7.0)
        n = F.residual_trial(out, ud, vd, s, p)
        assert eq(out.to_numpy(), ref), (s, "residual")
        assert n == n_ref or (math.isnan(n) and math.isnan(n_ref)), (s, n, n_ref)
        out.fill_(7.0)
        assert F.residual_trial(out, ud, vd, s, p, norm=False) is None  # a null n_out
        assert eq(out.to_numpy(), ref), (s, "residual, no norm")
        if s == 0.0:
            r0 = ud.zero()
            n0 = F.residual_norm(r0, ud, p)
            assert eq(out.to_numpy(), r0.to_numpy()) and (n == n0 or (math.isnan(n) and math.isnan(n0)))
    assert np.array_equal(ud.to_numpy(), u, equal_nan=True) and np.array_equal(vd.to_numpy(), v)  # inputs untouched


def stencil_cases():
    out = []
    for shape in SHAPES1:
        out.append(pytest.param("bratu1d", shape, None, None, id=f"bratu1d-{sid(shape)}"))
    for shape in SHAPES2:
        out.append(pytest.param("bratu2d", shape, None, None, id=f"bratu2d-{sid(shape)}"))
        for scheme, alpha in (("euler", 0.5), ("midpoint", 0.3), ("trapezoid", 0.5)):
            out.append(pytest.param("ignition", shape, scheme, alpha, id=f"ignition-{scheme}-{sid(shape)}"))
    for shape in SHAPES3:
        out.append(pytest.param("bratu3d", shape, None, None, id=f"bratu3d-{sid(shape)}"))
    for shape in SHAPES2 + SHAPES3:
        for scheme, alpha in (("euler", 0.5), ("midpoint", 0.3), ("trapezoid", 0.5)):
            for bc in (oc.BC_ZERO, oc.BC_PERIODIC):
                out.append(pytest.param("heat", shape, scheme, (alpha, bc), id=f"heat-{scheme}-bc{bc}-{sid(shape)}"))
    return out


def build_case(kind, shape, scheme, extra, seed):
    """(F, p, u, v): random u and v (Bratu and ignition: u of order one, so that exp stays ordinary)"""
    rng = np.random.default_rng(seed)
    if kind == "bratu1d":
        P = oc.bratu1d(shape[0])
        return ah.bratu_, (P.hx, P.lam), rng.standard_normal(P.shape), rng.standard_normal(P.shape)
    if kind == "bratu2d":
        P = oc.bratu2d(*shape)
        return ah.bratu2d_, (P.hx, P.hy, P.lam), rng.standard_normal(P.shape), rng.standard_normal(P.shape)
    if kind == "bratu3d":
        P = b3.Problem(*shape)
        return ah.bratu3d_, P.p, rng.standard_normal(P.shape), rng.standard_normal(P.shape)
    if kind == "ignition":
        un = rng.standard_normal(shape[::-1])
        h = min(1.0 / (shape[0] + 1), 1.0 / (shape[1] + 1))
        P = ig.Problem(*shape, scheme, lam=6.0, a=1.0, dt=10.0 * h * h, alpha=extra, un=un)
        F, p = ignition_residual(P)
        return F, p, un + 0.01 * rng.standard_normal(un.shape), rng.standard_normal(un.shape)
    alpha, bc = extra
    un = rng.standard_normal(shape[::-1])
    mk = oc.heat2d_euler if len(shape) == 2 else oc.heat3d_euler
    P = mk(*shape, un=un, scheme=scheme, bc=bc, alpha=alpha)
    F, p = heat_residual(P)
    return F, p, un + 0.01 * rng.standard_normal(un.shape), rng.standard_normal(un.shape)


@pytest.mark.parametrize("kind,shape,scheme,extra", stencil_cases())
def test_trial_kernel_bitwise(ctx, kind, shape, scheme, extra):
    F, p, u, v = build_case(kind, shape, scheme, extra, seed=sum(shape) + len(kind))
    check_trials(F, p, u, v)


def test_trial_kernel_runs_the_trial_instance(ctx):
    """the profile names the instantiation: MODE_TRIAL = 3 with the sum-of-squares epilogue / none"""
    from test_hip_exp_rare import Prof

    F, p, u, v = build_case("bratu2d", (130, 67), None, None, 3)
    ud, vd = dev(u), dev(v)
    out = ud.zero()
    with Prof(ctx) as pr:
        F.residual_trial(out, ud, vd, -0.5, p)
    pr.ran("residual_trial_norm", "nk::k_st2d<2, 3, 1, 2, false, false>", 1)
    with Prof(ctx) as pr:
        F.residual_trial(out, ud, vd, -0.5, p, norm=False)
    pr.ran("residual_trial", "nk::k_st2d<2, 3, 0, 2, false, false>", 1)


# ----------------------------------------------------------------------------- 2. the exp's exact phase
def rare_case(which):
    """(F, p, C-like planted field u, plants) with rare exp arguments at the plants"""
    if which == "bratu1d":
        C = plant1d()
        return ah.bratu_, (C.P.hx, C.P.lam), C, C.u
    if which == "bratu2d":
        C = plant2d(130, 40)
        return ah.bratu2d_, (C.P.hx, C.P.hy, C.P.lam), C, C.u
    if which == "ignition":
        C = plant2d(129, 19)
        un = np.random.default_rng(4).standard_normal(C.u.shape)
        h = 1.0 / 130
        P = ig.Problem(129, 19, "euler", lam=6.0, a=1.0, dt=10.0 * h * h, un=un)
        F, p = ignition_residual(P)
        return F, p, C, C.u
    raise AssertionError(which)


@pytest.mark.parametrize("which", ["bratu1d", "bratu2d", "ignition"])
def test_exact_phase_in_the_trial_instances(ctx, which):
    F, p, C, u = rare_case(which)
    v = C.tangent_zero(21)
    for s in (-1.0, -0.10476):
        n_rare = check_args(C, u + s * v, f"{which} trial exp(w)")  # w == u at the plants: v = 0 there
        assert n_rare > 0
    check_trials(F, p, u, v, steps=[-1.0, -0.10476, 0.0])


def test_exact_phase_in_the_trial_instance_3d(ctx):
    """3D Bratu: family values (rounding midpoints of 1 + x, all rare) over two whole planes across a z-chunk
    boundary, at the corners and at the wave's first / last lanes"""
    P = b3.Problem(130, 9, 18)
    rng = np.random.default_rng(9)
    u = b3.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    plants = np.zeros(P.shape, dtype=bool)
    plants[15:17] = True
    for k, j, i in ((0, 0, 0), (17, 8, 129), (3, 4, 0), (3, 4, 127), (3, 4, 128), (3, 5, 1)):
        plants[k, j, i] = True
    a = rng.permutation(np.arange(2 ** 16 + 64, 2 ** 16 + 2900))
    u[plants] = family(np.resize(a, int(plants.sum())))
    assert oc.exp_rare(u)[plants].all()
    v = rng.standard_normal(P.shape)
    v[plants] = 0.0
    check_trials(ah.bratu3d_, P.p, u, v, steps=[-1.0, -0.10476, 0.0])


@pytest.mark.parametrize("which", ["bratu1d", "bratu2d", "bratu3d", "ignition"])
def test_out_of_range_arguments_in_the_trial_instances(ctx, which):
    """710 (overflow), NaN, +-Inf, -746 where v = 0: the non-finite values land where the residual kernel puts them"""
    if which in ("bratu1d", "bratu2d"):
        C, _at = plant_oor(1 if which == "bratu1d" else 2)
        F, p = (ah.bratu_, (C.P.hx, C.P.lam)) if which == "bratu1d" else (ah.bratu2d_, (C.P.hx, C.P.hy, C.P.lam))
        u, v = C.u, C.tangent_zero(5)
    else:
        rng = np.random.default_rng(6)
        if which == "bratu3d":
            P = b3.Problem(33, 17, 9, lam=0.25)
            F, p, u = ah.bratu3d_, P.p, b3.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
        else:
            un = rng.standard_normal((19, 129))
            P = ig.Problem(129, 19, "euler", lam=0.25, a=1.0, dt=1e-3, un=un)
            (F, p), u = ignition_residual(P), un + 0.01 * rng.standard_normal(un.shape)
        v = rng.standard_normal(u.shape)
        flat = u.reshape(-1)
        for i, name in zip(rng.choice(flat.size, 5, replace=False), ("overflow", "nan", "+inf", "-inf", "zero")):
            flat[i] = OOR[name]
            v.reshape(-1)[i] = 0.0
    eq = lambda a, b: bool(np.all(same(a, b)))  # noqa: E731
    check_trials(F, p, u, v, steps=[-1.0, 0.37], eq=eq)
    ud, vd = dev(u), dev(v)
    out = ud.zero()
    F.residual_trial(out, ud, vd, -1.0, p)
    assert not np.isfinite(out.to_numpy()).all()  # the non-finite values did arrive


# ----------------------------------------------------------------------------- 3. a user residual
def test_user_residual_takes_the_materialised_path(ctx):
    from test_hip_user import USER_BRATU

    P = oc.bratu2d(130, 67)
    rng = np.random.default_rng(8)
    u, v = rng.standard_normal(P.shape), rng.standard_normal(P.shape)
    p = (P.hx, P.hy, P.lam)
    check_trials(USER_BRATU, p, u, v)
    # the torch residual restates the built-in one bit for bit (test_hip_user.py): so do the trials
    ud, vd = dev(u), dev(v)
    a, b = ud.zero(), ud.zero()
    na = USER_BRATU.residual_trial(a, ud, vd, -0.5, p)
    nb_ = ah.bratu2d_.residual_trial(b, ud, vd, -0.5, p)
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    assert abs(na - nb_) <= 1e-13 * nb_  # (the user path's norm is a separate pass: another summation order)


# ----------------------------------------------------------------------------- the nonlinear cases
def bratu_jacobian(P, u):
    """J(u) of 1D / 2D Bratu as a scipy CSC matrix (memory order, x fastest)"""
    import scipy.sparse as sp

    def d2(n, h):
        return sp.diags([np.full(n - 1, 1.0), np.full(n, -2.0), np.full(n - 1, 1.0)], [-1, 0, 1]) / (h * h)

    if P.dim == 1:
        L = d2(P.nx, P.hx)
    else:
        L = sp.kron(sp.identity(P.ny), d2(P.nx, P.hx)) + sp.kron(d2(P.ny, P.hy), sp.identity(P.nx))
    return (L + sp.diags(P.lam * np.exp(u.reshape(-1)))).tocsc()


def parab3p(lc, lm, ff0, ffc, ffm, sigma0=0.1, sigma1=0.5):
    """this file's own restatement of the rule"""
    if not (np.isfinite(ffc) and np.isfinite(ffm)):
        return sigma1 * lc
    c2 = lm * (ffc - ff0) - lc * (ffm - ff0)
    if not (c2 < 0):
        return sigma1 * lc
    c1 = lc * lc * (ffm - ff0) - lm * lm * (ffc - ff0)
    lp = ((-c1) * 0.5) / c2
    return min(max(lp, sigma0 * lc), sigma1 * lc)


def backtrack(n_res, trial, alpha=1e-4, maxarm=20):
    """(lam or None, n_t, rejected trials)"""
    lam = lm = lc = 1.0
    k = 0
    n_t = trial(-lam)
    ff0 = n_res * n_res
    ffc = ffm = n_t * n_t
    while not (n_t < (1.0 - alpha * lam) * n_res):
        if k == maxarm:
            return None, n_t, k + 1
        lam = 0.5 * lam if k == 0 else parab3p(lc, lm, ff0, ffc, ffm)
        lm, lc, ffm = lc, lam, ffc
        n_t = trial(-lam)
        ffc = n_t * n_t
        k += 1
    return lam, n_t, k


def numpy_newton(P, u0, linesearch, tol_rel=1e-10, max_niter=60):
    """sparse-LU Newton on oc.residual, full steps or this file's backtracking: (u, steps, lams, solved)"""
    import scipy.sparse.linalg as spla

    u = u0.copy()
    n_res = float(np.linalg.norm(oc.residual(P, u)))
    tol = tol_rel * n_res
    lams = []
    with np.errstate(all="ignore"):
        while n_res > tol and len(lams) <= max_niter:
            d = spla.splu(bratu_jacobian(P, u)).solve(oc.residual(P, u).reshape(-1)).reshape(P.shape)
            if linesearch:
                lam, n_t, _ = backtrack(n_res, lambda s: float(np.linalg.norm(oc.residual(P, u + s * d))))
                if lam is None:
                    return u, len(lams), lams, False
            else:
                lam, n_t = 1.0, float(np.linalg.norm(oc.residual(P, u - d)))
                if not np.isfinite(n_t):
                    return u, len(lams), lams, False
            u = u - lam * d
            lams.append(lam)
            n_res = n_t
    return u, len(lams), lams, bool(n_res <= tol)


def sigma_min(P, ustar):
    """the singular value of the symmetric J(u*) nearest zero"""
    import scipy.sparse.linalg as spla

    return abs(float(spla.eigsh(bratu_jacobian(P, ustar), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]))


class Case:
    """a nonlinear test problem: the residual, its parameters, the start and newton_krylov_'s keywords"""

    def __init__(self, name):
        self.name = name
        if name == "bratu1d":  # case 4: full steps fail from 8 sin
            self.P = oc.bratu1d(100, lam=3.5)
            self.F, self.p = ah.bratu_, (self.P.hx, self.P.lam)
            self.u0 = 8.0 * np.sin(np.pi * np.arange(1, 101) / 101.0)
            self.kw = dict(algo="gmres", memory=100, forcing=None, jv="exact")
        elif name == "bratu2d":  # case 5: the first step is reduced
            self.P = oc.bratu2d(24, 20, lam=1.0)
            self.F, self.p = ah.bratu2d_, (self.P.hx, self.P.hy, self.P.lam)
            self.u0 = 5.0 * oc.sin_ic(self.P)
            self.kw = dict(algo="gmres", memory=480, forcing=None, jv="exact")
        else:  # ignition Euler 40 x 40, lambda = 6, one stiff step (a dt / h^2 = 10), the default forcing
            h = 1.0 / 41
            self.P = ig.Problem(40, 40, "euler", lam=6.0, a=1.0, dt=10.0 * h * h,
                                un=np.random.default_rng(2).standard_normal((40, 40)))
            self.F, self.p = ignition_residual(self.P)
            self.u0 = self.P.un.copy()
            self.kw = dict(algo="gmres", memory=40, jv="exact", tol_abs=ig.TOL_ABS)


def run_driver(case, linesearch, native=False, **over):
    """newton_krylov_ / newton_krylov_native on the case: (u, res, result, the norms the callback saw)"""
    u, norms = dev(case.u0), []
    res = u.zero()
    kw = dict(case.kw, **over)
    if native:
        _, r = ah.newton_krylov_native(case.F, u, case.p, res, linesearch=linesearch, **kw)
    else:
        _, r = ah.newton_krylov_(case.F, u, case.p, res, linesearch=linesearch, callback=lambda _u, _r, n: norms.append(n), **kw)
    return u.to_numpy(), res.to_numpy(), r, norms


def loop_here(case, alpha=1e-4, maxarm=20, max_niter=50, tol_rel=1e-6):
    """The line-search Newton loop from existing primitives only: krylov_solve_ without _u_update, copy + kaxpy_ +
    residual_norm for each trial, this file's backtracking, kaxpy_norm_ on accept."""
    F, p = case.F, case.p
    u = dev(case.u0)
    res, w = u.zero(), u.zero()
    n = len(u)
    n_res = F.residual_norm(res, u, p)
    tol = tol_rel * n_res + case.kw.get("tol_abs", 1e-12)
    forcing = case.kw.get("forcing", ah.EisenstatWalker())
    eta = forcing.initial() if forcing is not None else None
    ws = ah.krylov_workspace(case.kw["algo"], ah.KrylovConstructor(res, memory=case.kw["memory"]))
    J = ah.JacobianOperator(F, res, u, p, jv=case.kw["jv"])
    lams, outer, inner, n_matvec, n_back, u_norm, failed = [], 0, 0, 0, 0, 0.0, False

    def trial(s):
        ah.kcopy_(n, w, u)
        ah.kaxpy_(n, s, ws.x, w)
        return F.residual_norm(res, w, p)

    while n_res > tol and outer <= max_niter:
        kk = {"rtol": eta} if forcing is not None else {}
        ah.krylov_solve_(ws, J, res, _b_norm=n_res, _u_norm=u_norm, _f0_is_residual=True, **kk)
        n_matvec += ws.stats.n_matvec
        inner += ws.stats.niter
        lam, n_t, rej = backtrack(n_res, trial, alpha, maxarm)
        n_back += rej
        if lam is None:
            failed = True
            n_res = F.residual_norm(res, u, p)
            break
        u_norm = ah.kaxpy_norm_(n, -lam, ws.x, u)
        lams.append(lam)
        n_prior, n_res = n_res, n_t
        if forcing is not None:
            eta = forcing(eta, tol, n_res, n_prior)
        outer += 1
    ws.free()
    return dict(u=u.to_numpy(), res=res.to_numpy(), lams=lams, outer=outer, inner=inner, n_matvec=n_matvec, n_back=n_back,
                failed=failed, n_res=n_res, solved=n_res <= tol, tol=tol)


def check_armijo(r, norms, alpha=1e-4):
    assert len(norms) == len(r.steps) + 1 == r.stats.outer_iterations + 1
    for lam, n_old, n_new in zip(r.steps, norms, norms[1:]):
        assert 0.0 < lam <= 1.0 and n_new < (1.0 - alpha * lam) * n_old, (lam, n_old, n_new)


def check_reach(case, u, ustar, what):
    tol = 1e-6 * float(np.linalg.norm(oc.residual(case.P, case.u0))) + 1e-12
    sm = sigma_min(case.P, ustar)
    err = float(np.max(np.abs(u - ustar)))
    nF = float(np.linalg.norm(oc.residual(case.P, u)))
    print(f"{what}: ||F(u)|| {nF:.3e} (tol {tol:.3e}), sigma_min {sm:.4g}, max|u - u*| {err:.3e} (allowed {2 * tol / sm:.3e})")
    assert nF <= tol * (1 + 1e-9)
    assert err <= 2.0 * tol / sm


# ----------------------------------------------------------------------------- 4. full steps fail, backtracking converges
def test_bratu1d_needs_the_line_search(ctx):
    """1D Bratu, N = 100, lambda = 3.5 (just below the fold at 3.5138), u0 = 8 sin: the full step never gets there, the
    backtracking converges in 15 steps with lam = 0.5, 0.105, 0.5 at steps 5-7, like the exact-step numpy run.

    Which root: the equation has two.  The sparse-LU Newton from u0 = 0 finds the one with max u = 1.0856; the
    backtracking iteration from 8 sin -- on the device and in numpy alike -- ends at the other one, max u = 1.296 (the
    figure the feature's description quotes for this run).  u* is therefore the root the numpy exact-step run with the
    same rule reaches from the same start; the root from u0 = 0 is computed and printed, and 0.21 away in max u."""
    case = Case("bratu1d")
    _, _, r0, _ = run_driver(case, None)
    print("full steps:", r0)
    assert not r0.solved
    u, res, r, norms = run_driver(case, ah.Backtracking())
    print("backtracking:", r, "\n||F||:", norms)
    assert r.solved and not r.ls_failed and r.n_backtrack >= 1
    check_armijo(r, norms)
    ustar, kb, lams, okb = numpy_newton(case.P, case.u0, linesearch=True)
    print(f"exact-step numpy run: {kb} steps, lam = {lams}, solved {okb}, max u* = {ustar.max():.4f}; device max u = {u.max():.4f}")
    assert okb and abs(float(ustar.max()) - 1.296) < 1e-2  # (1.2937 at the grid points)
    u_low, _, _, ok = numpy_newton(case.P, np.zeros(case.P.shape), linesearch=False)
    print(f"the root from u0 = 0: max u = {u_low.max():.4f}, max|u - u_low| = {np.max(np.abs(u - u_low)):.3e}")
    assert ok
    check_reach(case, u, ustar, "bratu1d")


# ----------------------------------------------------------------------------- 5. the same in 2D
def test_bratu2d_first_step_is_reduced(ctx):
    case = Case("bratu2d")
    u, res, r, norms = run_driver(case, ah.Backtracking())
    print("backtracking:", r, "\n||F||:", norms)
    assert r.solved and r.steps[0] < 1.0 and r.n_backtrack >= 1
    check_armijo(r, norms)
    ustar, k, lams, ok = numpy_newton(case.P, case.u0, linesearch=True)
    print(f"exact-step numpy run: {k} steps, lam = {lams}, max u* = {ustar.max():.4f}")
    assert ok
    check_reach(case, u, ustar, "bratu2d")


# ----------------------------------------------------------------------------- 6. the drivers against the loop here
@pytest.mark.parametrize("name", ["bratu1d", "bratu2d", "ignition"])
def test_drivers_are_the_loop_written_here(ctx, name):
    case = Case(name)
    ref = loop_here(case)
    print(f"{name}: lam {ref['lams']}, outer {ref['outer']}, inner {ref['inner']}, rejected {ref['n_back']}")
    assert ref["solved"] and not ref["failed"]
    for native in (False, True):
        u, res, r, _ = run_driver(case, ah.Backtracking(), native=native)
        what = "native" if native else "python"
        assert list(r.steps) == ref["lams"], what
        assert (r.stats.outer_iterations, r.stats.inner_iterations, r.n_matvec, r.n_backtrack, r.ls_failed, r.solved) == \
               (ref["outer"], ref["inner"], ref["n_matvec"], ref["n_back"], False, True), what
        assert r.stats.n_res == ref["n_res"], what
        assert np.array_equal(u, ref["u"]) and np.array_equal(res, ref["res"]), what
        ud = dev(u)
        again = ud.zero()
        case.F(again, ud, case.p)
        assert np.array_equal(res, again.to_numpy()), what  # res is F(u)


# ----------------------------------------------------------------------------- 7. no backtrack means today's solve
def easy_runs(algo, **kw):
    P = oc.bratu1d(1000)
    F, p, u0 = ah.bratu_, (P.hx, P.lam), oc.sin_ic(P)
    out = []
    for ls in (None, ah.Backtracking()):
        u = dev(u0)
        res = u.zero()
        _, r = ah.newton_krylov_(F, u, p, res, algo=algo, linesearch=ls, **kw)
        out.append((u.to_numpy(), res.to_numpy(), r))
    return out


@pytest.mark.parametrize("algo", ["cg", "minres"])
def test_unit_steps_are_todays_solve(ctx, algo):
    (u0, r0, a), (u1, r1, b) = easy_runs(algo)
    assert a.solved and b.solved and b.n_backtrack == 0 and b.steps == (1.0,) * b.stats.outer_iterations
    assert np.array_equal(u0, u1) and np.array_equal(r0, r1)
    assert a.stats == b.stats and a.n_matvec == b.n_matvec


def test_unit_steps_gmres_outcome(ctx):
    """GMRES fuses the default update into the solve's last pass (u - x formed from the basis in registers); with a
    line search x is stored and subtracted by kaxpy_norm_: the same value fma(-1, x, u) of the same x, and the same
    partial sums of ||u||.  Measured: bitwise equal, so it is asserted.  Three Newton steps of at most
    150 Arnoldi steps each: a whole GMRES solve of this 1D Laplacian takes about 1000 (12 s for the pair of runs)."""
    kw = dict(max_niter=2, krylov_kwargs=dict(itmax=150))
    (u0, r0, a), (u1, r1, b) = easy_runs("gmres", **kw)
    assert b.stats.outer_iterations == 3 and b.n_backtrack == 0 and b.steps == (1.0, 1.0, 1.0)
    print(f"gmres, all lam = 1: {a} / {b}; max|du| = {np.max(np.abs(u0 - u1)):.3e}")
    assert np.array_equal(u0, u1) and np.array_equal(r0, r1)
    assert a.stats == b.stats and a.n_matvec == b.n_matvec


# ----------------------------------------------------------------------------- 8. the failure path
def test_failure_leaves_the_last_accepted_iterate(ctx):
    case = Case("bratu1d")
    ref = loop_here(case, maxarm=1)
    assert ref["failed"] and not ref["solved"]
    for native in (False, True):
        u, res, r, norms = run_driver(case, ah.Backtracking(maxarm=1), native=native)
        what = "native" if native else "python"
        assert r.ls_failed and not r.solved, what
        assert np.array_equal(u, ref["u"]) and np.array_equal(res, ref["res"]), what
        assert r.stats.outer_iterations == len(r.steps) == ref["outer"] and list(r.steps) == ref["lams"], what
        assert (r.stats.inner_iterations, r.n_matvec, r.n_backtrack) == (ref["inner"], ref["n_matvec"], ref["n_back"]), what
        ud = dev(u)
        again = ud.zero()
        case.F(again, ud, case.p)
        assert np.array_equal(res, again.to_numpy()), what
        if not native:
            assert len(norms) == len(r.steps) + 1  # the callback fired once per accepted step


def test_c_driver_refuses_malformed_options(ctx):
    """nk_newton_krylov's own checks (Backtracking refuses these before the call: the fields are forced here)"""
    case = Case("bratu2d")
    for field, value, msg in (("maxarm", 0, "ls_maxarm"), ("sigma0", 0.6, "ls_sigma0 <= ls_sigma1"), ("sigma1", 1.0, "ls_sigma1 < 1"),
                              ("alpha", 0.0, "ls_alpha"), ("alpha", float("nan"), "ls_alpha")):
        bt = ah.Backtracking()
        object.__setattr__(bt, field, value)
        with pytest.raises(ah.NKError, match=msg):
            run_driver(case, bt, native=True)


# ----------------------------------------------------------------------------- 9. solve with a line search
def test_solve_with_linesearch_below_the_fold(ctx):
    _, s0, st0 = run_solve("euler", ig.LAM, 0.05, 3, algo="cg", M=spd_jacobi)
    _, s1, st1 = run_solve("euler", ig.LAM, 0.05, 3, algo="cg", M=spd_jacobi, linesearch=ah.Backtracking())
    for a, b, x, y in zip(st0, st1, s0, s1):
        assert a.solved and b.solved and b.n_backtrack == 0 and b.steps == (1.0,) * b.stats.outer_iterations
        assert a.stats == b.stats and a.n_matvec == b.n_matvec
        assert np.array_equal(x, y)


# ----------------------------------------------------------------------------- 10. two ranks
def test_two_ranks(ctx, tmp_path):
    from test_hip_dist import run_ranks, worker_env

    out = str(tmp_path / "ls2")
    rc, log = run_ranks(2, [os.path.join(ROOT, "tests", "linesearch_dist_worker.py"), "--out", out], worker_env(2))
    assert rc == 0, log[-3000:]
    meta = json.load(open(out + ".json"))
    u = np.load(out + ".npz")["u"]
    print(meta)
    assert meta["solved"] == [True, True] and meta["steps_equal"] and meta["steps"][0] < 1.0
    case = Case("bratu2d")
    ustar, _, _, ok = numpy_newton(case.P, case.u0, linesearch=True)
    assert ok
    check_reach(case, u, ustar, "two ranks")


# ----------------------------------------------------------------------------- 11. the C++ binary
def test_cpp_binary_linesearch(ctx):
    exe = os.path.join(ROOT, "newtonkrylov.jl_amd", "bin", "bratu2d_newton")
    args = ["24", "20", "exact", "480", "1", "--lambda", "1", "--amp", "5", "--no-forcing", "--linesearch"]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    print(d)
    h = d["n_res_history"]
    assert d["solved"] and d["linesearch"] and not d["ls_failed"] and d["n_backtrack"] >= 1 and d["steps"][0] < 1.0
    assert len(h) == d["outer"] + 1 and all(b < a for a, b in zip(h, h[1:]))
    _, _, r, _ = run_driver(Case("bratu2d"), ah.Backtracking(), native=True)
    assert list(r.steps) == d["steps"] and r.stats.outer_iterations == d["outer"]
