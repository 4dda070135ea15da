"""The multigrid V-cycle (csrc/nk_mg.hip) away from its default options and hierarchy shapes.

test_hip_multigrid.py compares the device cycle with its numpy restatement (`Cycle`) at nu = 2, coarse_sweeps = 8
only: both sweep counts even, every hierarchy at full depth.  This file runs what that leaves out:

* a second derivation of the cycle -- explicit matrices in long double on three tiny grids, the V-cycle as a
  matrix recursion -- against which both the restatement (CPU) and the device (unit vector by unit vector) are held;
* the device against the restatement over odd and even sweep counts, other ω, `max_levels`, the 1024-point
  threshold of the one-launch coarse tail and a hierarchy that the sign check truncates (OPTION_CASES names the
  branch of nk_mg.hip that each case reaches);
* properties that need no reference: z aliasing v, a hierarchy whose operator (and depth) is set again and again,
  determinism and linearity at odd sweep counts;
* GMRES / FGMRES with the V-cycle at non-default options.

Tolerances follow test_hip_multigrid.py's rule: the float64-versus-long-double difference of the reference, measured
on the CPU over exactly the cases used, recorded as a constant (and measured again by a CPU test), times 16 for the
device's fma and its other association of the stencil sums.  No constant comes from device output.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from oracle import oracle as oc

from test_hip_multigrid import (RESIDUALS, Cycle, along, device_operator, gmres_right, host_problem, krylov, plan, reference,
                                rel, truncated_case)

TAIL_POINTS = 1024  # kMgTailPoints of nk_mg.hip: the first tail level G is the first with at most this many points

# float64 versus long double, max-abs over the result relative to its max-abs (the tests named *_is_as_recorded
# measure each again on the CPU and hold it within 1.5 x):
#   DENSE_SENSITIVITY         the dense matrix recursion's M over the 24 dense cases            measured 5.432e-16
#   UNIT_SENSITIVITY          the restatement applied to the unit vectors of those cases        measured 3.181e-16
#   OPTION_SENSITIVITY        the restatement over OPTION_CASES and sign_case() in 2D and 3D    measured 7.330e-16
#   OPTION_SENSITIVITY_1D     ... over the 1D cases (up to 11 levels)                           measured 1.730e-15
DENSE_SENSITIVITY = 5.4e-16
UNIT_SENSITIVITY = 3.2e-16
OPTION_SENSITIVITY = 7.3e-16
OPTION_SENSITIVITY_1D = 1.7e-15


def within(recorded, measured):
    return recorded / 1.5 <= measured <= 1.5 * recorded


# ------------------------------------------------------------------------------------ the dense form (§10's cycle as matrices)
DENSE_GRIDS = [(13,), (9, 7), (6, 5, 4)]
DENSE_S = ["bratu", "heat"]
DENSE_OPTS = [(1, 1), (1, 8), (2, 1), (2, 8)]
DENSE_CASES = [(g, sk, nu, cs) for g in DENSE_GRIDS for sk in DENSE_S for nu, cs in DENSE_OPTS]
DENSE_IDS = [f"{'x'.join(map(str, g))}-{sk}-nu{nu}-cs{cs}" for g, sk, nu, cs in DENSE_CASES]


def dense_coefficients(shape, skind):
    """(h, k, s_0) of a dense case: h = 1 / (n + 1); Bratu-like k = 1 with a positive s that varies along every axis and
    is symmetric along none, heat-like k = 1 (a Δt = 1) with the constant s = -1"""
    h = [1.0 / (n + 1) for n in shape]
    if skind == "heat":
        return h, [1.0] * len(shape), -1.0
    arg, tilt = 1.0, 0.0
    for a, n in enumerate(shape):  # axis a of the grid is numpy axis d - 1 - a
        x = (np.arange(1, n + 1) * h[a]).reshape([-1 if b == len(shape) - 1 - a else 1 for b in range(len(shape))])
        arg, tilt = arg * np.sin(np.pi * x), tilt + 0.3 * (a + 1) * x
    return h, [1.0] * len(shape), 3.5 * np.exp(arg + tilt)


def hat_prolongation(nf, nc, dt):
    """One axis of P from the header's definition: fine point i (1-based) sits at p = i (n_c + 1) / (n_f + 1) in coarse
    index units, and coarse point j carries the hat function max(0, 1 - |p - j|) there (linear interpolation between
    the two coarse neighbours of p; coarse indices 0 and n_c + 1 are the boundary and have no column)."""
    P = np.zeros((nf, nc), dtype=dt)
    for i in range(1, nf + 1):
        p = Fraction(i * (nc + 1), nf + 1)
        for j in range(1, nc + 1):
            w = 1 - abs(p - j)
            if w > 0:
                P[i - 1, j - 1] = dt(w.numerator) / dt(w.denominator)
    return P


def kron_axes(mats):
    """Kronecker product of per-axis matrices given in grid order x, y, z (x fastest: the last factor)"""
    out = mats[0]
    for m in mats[1:]:
        out = np.kron(m, out)
    return out


def second_difference(n, dt):
    return -2 * np.eye(n, dtype=dt) + np.eye(n, k=1, dtype=dt) + np.eye(n, k=-1, dtype=dt)


def dense_vcycle_matrix(shape, h, k, s0, nu, cs, dt, omega=None):
    """M with z = M v for one V-cycle from x = 0, by the matrix recursion, everything in dtype dt"""
    d = len(shape)
    omega = dt(omega) if omega else dt(2 * d) / dt(2 * d + 1)
    levels = plan(shape)
    length = [dt(n + 1) * dt(hh) for n, hh in zip(shape, h)]
    s = (np.asarray(s0, dtype=dt) * np.ones(tuple(reversed(shape)), dtype=dt)).reshape(-1)
    A, P, R = [], [], []
    for l, ext in enumerate(levels):
        if l > 0:
            Pa = [hat_prolongation(nf, nc, dt) for nf, nc in zip(levels[l - 1], ext)]
            Ra = [(p.T / p.T.sum(axis=1)[:, None]) for p in Pa]  # D^-1 P^T, D = the row sums of P^T
            P.append(kron_axes(Pa))
            R.append(kron_axes(Ra))
            s = R[-1] @ s
        Al = np.diag(s)
        for a in range(d):
            hl = dt(h[a]) if l == 0 else length[a] / dt(ext[a] + 1)
            eyes = [np.eye(n, dtype=dt) for n in ext]
            eyes[a] = second_difference(ext[a], dt)
            Al = Al + (dt(k[a]) / (hl * hl)) * kron_axes(eyes)
        A.append(Al)

    def jacobi(l, X, sweeps):
        eye, dinv = np.eye(A[l].shape[0], dtype=dt), 1 / np.diag(A[l])
        for _ in range(sweeps):
            X = X + omega * (dinv[:, None] * (eye - A[l] @ X))
        return X

    def M(l):
        n = A[l].shape[0]
        if l == len(levels) - 1:
            return jacobi(l, np.zeros((n, n), dtype=dt), cs)
        pre = jacobi(l, np.zeros((n, n), dtype=dt), nu)
        return jacobi(l, pre + P[l] @ (M(l + 1) @ (R[l] @ (np.eye(n, dtype=dt) - A[l] @ pre))), nu)

    return M(0)


def on_unit_vectors(shape, apply):
    """the matrix of a linear map on the grid, column by column"""
    n = int(np.prod(shape))
    cols = []
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        cols.append(apply(e.reshape(tuple(reversed(shape)))).reshape(-1).copy())
    return np.stack(cols, axis=1)


_DENSE = {}


def dense_reference(case):
    """(h, k, s_0, M in long double, the float64 restatement on the unit vectors) of a dense case, computed once"""
    if case not in _DENSE:
        shape, skind, nu, cs = case
        h, k, s = dense_coefficients(shape, skind)
        cyc = Cycle(shape, h, k, s, nu=nu, coarse_sweeps=cs)
        assert cyc.levels == plan(shape) and len(cyc.levels) >= 2
        _DENSE[case] = (h, k, s, dense_vcycle_matrix(shape, h, k, s, nu, cs, np.longdouble), on_unit_vectors(shape, cyc.vcycle))
    return _DENSE[case]


# ------------------------------------------------------------------------------------ the option matrix
Case = namedtuple("Case", "kind shape nu cs omega max_levels")
ROWS = [(1, 1), (1, 2), (2, 1), (2, 5), (3, 3), (3, 8)]


def rows(kind, shape, which, max_levels=0, omegas=(None,)):
    return [Case(kind, shape, nu, cs, om, max_levels) for nu, cs in which for om in omegas]


# Which branch of nk_mg.hip a case reaches.  In k_mg_tail, x / residual buffers follow T.nu & 1, the coarse correction
# e of the tail's last level follows kc & 1 = cs & 1 (kc = 2 nu, even, on the levels above it), the result follows
# k0 & 1 (= cs & 1 in a one-level tail, even otherwise).  In nk_mg_apply / mg_sweeps, which of xa / xb holds x and which
# the residual follows nu & 1; with nu = 1 the ascent's only sweep on level 0 is the one that writes z.
OPTION_CASES = (
    # G = 0, the whole cycle in the tail, level 0 exactly kMgTailPoints (32 x 32): every (nu & 1, cs & 1) pair of the
    # multi-level tail, and ω (om1 = 1 - ω = 0 at ω = 1) on the all-odd and the odd / even row
    rows("bratu2d", (32, 32), ROWS)
    + rows("bratu2d", (32, 32), [(1, 1), (3, 8)], omegas=(0.5, 1.0))
    # the same threshold in 3D (an axis of 8 -> 4 -> 2 that stops coarsening before the others) and in 1D (10 levels)
    + rows("heat3d_midpoint", (16, 8, 8), [(1, 2), (3, 3)]) + rows("heat3d_euler", (16, 8, 8), [(2, 5)])
    + rows("bratu1d", (1024,), [(1, 1), (2, 1), (3, 8)])
    # G = 0 just under the threshold, odd extents
    + rows("bratu2d", (33, 31), [(1, 1), (2, 5)])
    # G = 1: level 0 of 1025 / 1088 points on the per-level kernels, then a multi-level tail.  Driver parity nu & 1 with
    # every row; nu = 1: the ascent's single sweep writes z
    + rows("bratu2d", (41, 25), ROWS)
    + rows("bratu2d", (41, 25), [(1, 1), (3, 8)], omegas=(0.5, 1.0))
    + rows("heat2d_trapezoid", (41, 25), [(1, 2), (3, 3)])
    + rows("heat3d_midpoint", (17, 8, 8), [(1, 1), (3, 8)]) + rows("heat3d_euler", (17, 8, 8), [(2, 1), (3, 3)])
    + rows("bratu1d", (1025,), [(1, 1), (2, 5), (3, 8)])
    # G = 1 and the tail's first level has exactly kMgTailPoints points (2049 -> 1024)
    + rows("bratu1d", (2049,), [(1, 2), (3, 3)])
    # T.nlev == 1 behind one per-level level (4032, 1008): k0 = cs, odd and even, under odd and even nu
    + rows("bratu2d", (72, 56), [(2, 1), (1, 2), (3, 3), (3, 8)], max_levels=2)
    # no tail (8580, 2145): l == L - 1 with l > 0 in nk_mg_apply, coarse_sweeps through mg_sweeps, then the ascent from it
    + rows("bratu2d", (130, 66), [(1, 1), (1, 2), (2, 5), (3, 8)], max_levels=2)
    # G = 2 and a one-level tail (8580, 2145, 512)
    + rows("bratu2d", (130, 66), [(1, 1), (1, 2), (2, 1), (3, 8)], max_levels=3)
    # one large level: coarse_sweeps sweeps through mg_sweeps with l == 0, the last of them into z
    + rows("bratu2d", (130, 66), [(3, 3), (3, 8)], max_levels=1)
    # full depth behind two per-level levels (8580, 2145, 512, ...: G = 2, a multi-level tail)
    + rows("bratu2d", (130, 66), [(1, 1), (2, 5)])
)
# the hierarchy that the sign check cuts to L == tail == 2 (130 x 66 -> 65 x 33; the tail is allocated for 32 x 16 and
# below and never launched): the options with which sign_case() is run
SIGN_ROWS = [(2, 8), (1, 1), (3, 3)]


def case_id(c):
    om = "" if c.omega is None else f"-om{c.omega}"
    ml = "" if not c.max_levels else f"-ml{c.max_levels}"
    return f"{c.kind}-{'x'.join(map(str, c.shape))}-nu{c.nu}-cs{c.cs}{om}{ml}"


def options(c):
    return dict(nu=c.nu, coarse_sweeps=c.cs, omega=c.omega, max_levels=c.max_levels)


def option_tol(shape):
    return 16 * (OPTION_SENSITIVITY_1D if len(shape) == 1 else OPTION_SENSITIVITY)


_OPT = {}


def option_reference(c):
    """(the float64 restatement at the case's options, its V-cycle of the case's v), computed once"""
    if c not in _OPT:
        P, u, k, s, h, v, _ = reference(c.kind, c.shape)
        cyc = Cycle(c.shape, h, k, s, **options(c))
        _OPT[c] = (cyc, cyc.vcycle(v))
    return _OPT[c]


def sign_case():
    """(shape, h, k, s, v) of the truncation case: -2 Σ 1/h² = -43300, -11600, -3112 on levels 0 .. 2 of 130 x 66 and
    s between 2156 and 3356 on level 0, so that the diagonal changes sign on level 2"""
    if "sign" not in _OPT:
        shape = (130, 66)
        h = [1.0 / (n + 1) for n in shape]
        x, y = np.arange(1, 131) * h[0], np.arange(1, 67) * h[1]
        s = 2756.0 + 600.0 * np.sin(3 * np.pi * y)[:, None] * np.sin(2 * np.pi * x)[None, :]
        _OPT["sign"] = (shape, h, [1.0, 1.0], s, np.random.default_rng(13).standard_normal(s.shape))
    return _OPT["sign"]


def sign_reference(nu, cs):
    key = ("sign", nu, cs)
    if key not in _OPT:
        shape, h, k, s, v = sign_case()
        cyc = Cycle(shape, h, k, s, nu=nu, coarse_sweeps=cs)
        _OPT[key] = (cyc, cyc.vcycle(v))
    return _OPT[key]


def first_tail_level(levels):
    """G of nk_mg_apply for a hierarchy in use: the first level of at most kMgTailPoints points (len(levels): none)"""
    return next((l for l, ext in enumerate(levels) if np.prod(ext) <= TAIL_POINTS), len(levels))


SOLVER_OPTIONS = [dict(nu=1, coarse_sweeps=3), dict(max_levels=2)]
SOLVER_IDS = ["nu1-cs3", "ml2"]


# ------------------------------------------------------------------------------------ CPU tests
def test_hat_prolongation_is_linear_interpolation():
    """the dense form's P on its own: P applied to coarse samples is numpy's piecewise linear interpolant of them (zero
    on the boundary) at the fine points; an axis that is not coarsened gives the identity"""
    for nf, nc in [(13, 6), (6, 3), (9, 4), (7, 3), (5, 2), (4, 2), (4, 4)]:
        P = hat_prolongation(nf, nc, np.longdouble)
        xc = np.arange(1, nc + 1, dtype=np.longdouble) / (nc + 1)
        xf = np.arange(1, nf + 1, dtype=np.longdouble) / (nf + 1)
        f = lambda x: np.cos(3 * x) + x  # noqa: E731
        want = np.interp(xf.astype(float), np.concatenate([[0.0], xc.astype(float), [1.0]]),
                         np.concatenate([[0.0], f(xc).astype(float), [0.0]]))
        assert np.max(np.abs((P @ f(xc)).astype(float) - want)) <= 4e-16
        assert np.all((P > 0).sum(axis=1) <= 2) and np.all(P.sum(axis=1) <= 1 + 1e-18)
    np.testing.assert_array_equal(hat_prolongation(3, 3, np.float64), np.eye(3))


@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_restatement_matches_dense_form(case):
    h, k, s, M, Z = dense_reference(case)
    err = rel(Z, M)
    print(f"{case}: restatement vs dense long double M {float(err):.3e} (allowed {16 * DENSE_SENSITIVITY:.1e})")
    assert err <= 16 * DENSE_SENSITIVITY


def test_dense_sensitivities_are_as_recorded():
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    dense = unit = 0.0
    for case in DENSE_CASES:
        shape, skind, nu, cs = case
        h, k, s, M, Z = dense_reference(case)
        dense = max(dense, rel(dense_vcycle_matrix(shape, h, k, s, nu, cs, np.float64), M))
        Zl = on_unit_vectors(shape, Cycle(shape, h, k, s, nu=nu, coarse_sweeps=cs, dt=np.longdouble).vcycle)
        unit = max(unit, rel(Z, Zl))
        # in long double the two derivations agree under the same rule, scaled by the ratio of the two epsilons
        assert rel(Zl, M) <= 16 * DENSE_SENSITIVITY * float(np.finfo(np.longdouble).eps) / np.finfo(np.float64).eps
    print(f"dense form float64 vs longdouble: {dense:.3e}; restatement on the unit vectors: {unit:.3e}")
    assert within(DENSE_SENSITIVITY, dense)
    assert within(UNIT_SENSITIVITY, unit)


def test_option_cases_reach_the_hierarchies_they_name():
    """the level point counts and first tail levels that the comments of OPTION_CASES claim"""
    def shape_of(shape, max_levels=0):
        lv = plan(shape, max_levels)
        return [int(np.prod(e)) for e in lv], first_tail_level(lv)

    for shape in [(32, 32), (16, 8, 8), (1024,)]:
        pts, G = shape_of(shape)
        assert pts[0] == TAIL_POINTS and G == 0
    assert shape_of((33, 31))[0][0] == 1023 and shape_of((33, 31))[1] == 0
    for shape, n0 in [((41, 25), 1025), ((17, 8, 8), 1088), ((1025,), 1025)]:
        pts, G = shape_of(shape)
        assert pts[0] == n0 and G == 1
    assert shape_of((2049,))[0][:2] == [2049, 1024] and shape_of((2049,))[1] == 1
    assert shape_of((72, 56), 2) == ([4032, 1008], 1)
    assert shape_of((130, 66), 2) == ([8580, 2145], 2)
    assert shape_of((130, 66), 3) == ([8580, 2145, 512], 2)
    assert shape_of((130, 66), 1) == ([8580], 1)
    assert shape_of((130, 66))[0][:3] == [8580, 2145, 512] and shape_of((130, 66))[1] == 2 and len(plan((130, 66))) > 3
    # every row of the issue's option list, and every ω on (1, 1) and (3, 8), runs on a G = 0 and on a G = 1 shape
    for shape in [(32, 32), (41, 25)]:
        got = {(c.nu, c.cs, c.omega) for c in OPTION_CASES if c.shape == shape and c.kind == "bratu2d"}
        assert got == {(nu, cs, None) for nu, cs in ROWS} | {(nu, cs, om) for nu, cs in [(1, 1), (3, 8)] for om in (0.5, 1.0)}
    assert len(set(OPTION_CASES)) == len(OPTION_CASES)
    for c in OPTION_CASES:
        assert option_reference(c)[0].levels == plan(c.shape, c.max_levels), c  # none of them truncates


def test_sign_case_truncates_after_two_levels():
    shape, h, k, s, v = sign_case()
    cyc = sign_reference(2, 8)[0]
    assert cyc.levels == [(130, 66), (65, 33)] == plan(shape)[:2]
    assert -41144 <= cyc.diag[0].min() and cyc.diag[0].max() <= -39944
    assert -8863 <= cyc.diag[1].min() and cyc.diag[1].max() <= -7673
    # level 2 (32 x 16) is where the diagonal changes sign: R s minus 2 Σ 1/h² there
    s2 = cyc.s[1]
    for a, (nf, nc) in enumerate(zip((65, 33), (32, 16))):
        P = hat_prolongation(nf, nc, np.float64)
        s2 = along(P.T / P.T.sum(axis=1)[:, None], s2, a)
    d2 = s2 - 2 * (33.0 ** 2 + 17.0 ** 2)
    assert d2.min() < 0 < d2.max()
    # L == tail: the tail would start at level 2, which is not in use
    assert first_tail_level(plan(shape)) == 2 == len(cyc.levels)


def test_option_sensitivities_are_as_recorded():
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    worst = {False: 0.0, True: 0.0}  # keyed by "is 1D"
    for c in OPTION_CASES:
        P, u, k, s, h, v, _ = reference(c.kind, c.shape)
        zl = Cycle(c.shape, h, k, s, dt=np.longdouble, **options(c)).vcycle(v)
        worst[len(c.shape) == 1] = max(worst[len(c.shape) == 1], rel(option_reference(c)[1], zl))
    shape, h, k, s, v = sign_case()
    for nu, cs in SIGN_ROWS:
        zl = Cycle(shape, h, k, s, nu=nu, coarse_sweeps=cs, dt=np.longdouble).vcycle(v)
        worst[False] = max(worst[False], rel(sign_reference(nu, cs)[1], zl))
    print(f"restatement float64 vs longdouble over the option cases: {worst[False]:.3e} (2D / 3D), {worst[True]:.3e} (1D)")
    assert within(OPTION_SENSITIVITY, worst[False])
    assert within(OPTION_SENSITIVITY_1D, worst[True])


@pytest.mark.parametrize("opts", SOLVER_OPTIONS, ids=SOLVER_IDS)
def test_restatement_gmres_converges_at_the_solver_options(opts):
    P, u, k, s, h, v, _ = reference("bratu2d", (72, 56))
    b = oc.residual(P, u)
    x, it, ok = gmres_right(lambda q: oc.jv_exact(P, u, q), Cycle((72, 56), h, k, s, **opts).vcycle, b, 1e-8)
    print(f"{opts}: numpy GMRES(30) {it} steps")
    assert ok and it < 60
    assert np.linalg.norm(b - oc.jv_exact(P, u, x)) <= 1e-7 * np.linalg.norm(b)


# ------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def device_s(s):
    return ah.DeviceArray.from_numpy(s) if isinstance(s, np.ndarray) else s


@pytest.mark.gpu
@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_device_matrix_matches_dense_form(ctx, case):
    """the device V-cycle on every unit vector (each a single tail launch) against the long double M: a wrong weight at
    one boundary point shows as one wrong entry"""
    shape, skind, nu, cs = case
    h, k, s, M, _ = dense_reference(case)
    mg = ah.MultigridPreconditioner.from_coefficients(ah.Grid.full(*shape), k, device_s(s), h=h, nu=nu, coarse_sweeps=cs)
    assert mg.levels == plan(shape)
    assert int(np.prod(shape)) <= 120
    zd = ah.DeviceArray(ah.Grid.full(*shape))
    Z = on_unit_vectors(shape, lambda e: mg.vcycle(ah.DeviceArray.from_numpy(e), z=zd).to_numpy())
    err = rel(Z, M.astype(np.float64))
    col = np.max(np.abs(Z - M.astype(np.float64)), axis=0) / float(np.max(np.abs(M)))
    print(f"{case}: device vs dense M {err:.3e} (allowed {16 * UNIT_SENSITIVITY:.1e}), worst column {int(np.argmax(col))}")
    assert err <= 16 * UNIT_SENSITIVITY


@pytest.mark.gpu
@pytest.mark.parametrize("c", OPTION_CASES, ids=[case_id(c) for c in OPTION_CASES])
def test_vcycle_matches_restatement_at_options(ctx, c):
    J, ref = device_operator(c.kind, c.shape)
    cyc, zref = option_reference(c)
    mg = ah.MultigridPreconditioner(J, **options(c))
    assert mg.levels == cyc.levels == plan(c.shape, c.max_levels)
    z = mg.apply(J, ah.DeviceArray.from_numpy(ref[5])).to_numpy()
    err = rel(z, zref)
    print(f"{case_id(c)}: device vs restatement {err:.3e} (allowed {option_tol(c.shape):.1e})")
    assert err <= option_tol(c.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("nu,cs", SIGN_ROWS)
def test_vcycle_on_a_hierarchy_truncated_to_the_per_level_levels(ctx, nu, cs):
    shape, h, k, s, v = sign_case()
    cyc, zref = sign_reference(nu, cs)
    assert cyc.levels == [(130, 66), (65, 33)]
    mg = ah.MultigridPreconditioner.from_coefficients(ah.Grid.full(*shape), k, ah.DeviceArray.from_numpy(s), h=h, nu=nu,
                                                      coarse_sweeps=cs)
    assert mg.levels == cyc.levels == plan(shape)[:2]
    err = rel(mg.vcycle(ah.DeviceArray.from_numpy(v)).to_numpy(), zref)
    print(f"sign truncation nu={nu} cs={cs} {mg.levels}: device vs restatement {err:.3e} (allowed {option_tol(shape):.1e})")
    assert err <= option_tol(shape)


IN_PLACE = [((32, 32), {}), ((32, 32), dict(nu=1, coarse_sweeps=1)),  # G = 0
            ((130, 66), {}), ((130, 66), dict(nu=1)),  # mixed: per-level levels 0 and 1, then the tail
            ((130, 66), dict(max_levels=1, coarse_sweeps=1)), ((130, 66), dict(max_levels=1, coarse_sweeps=3))]
IN_PLACE_IDS = ["x".join(map(str, s)) + "".join(f"-{n}{v}" for n, v in o.items()) for s, o in IN_PLACE]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,opts", IN_PLACE, ids=IN_PLACE_IDS)
def test_vcycle_in_place(ctx, shape, opts):
    """z may alias v: bitwise the out-of-place result"""
    J, ref = device_operator("bratu2d", shape)
    mg = ah.MultigridPreconditioner(J, **opts)
    z = mg.vcycle(ah.DeviceArray.from_numpy(ref[5])).to_numpy()
    assert np.all(np.isfinite(z)) and np.max(np.abs(z)) > 0
    v = ah.DeviceArray.from_numpy(ref[5])
    out = mg.vcycle(v, z=v)
    assert out is v
    np.testing.assert_array_equal(v.to_numpy(), z)


@pytest.mark.gpu
def test_coefficients_set_again_on_a_live_hierarchy(ctx):
    """3 levels (truncated), full depth, 3 levels again on one object: levels and V-cycle bitwise those of a fresh object
    (the levels out of use keep their stale b, s and diagonal)"""
    shape, h, k, s, v, cyc, _ = truncated_case()
    grid = ah.Grid.full(*shape)
    vd = ah.DeviceArray.from_numpy(v)
    live = None
    for step, coeff in enumerate([s, -5.0, s]):
        if live is None:
            live = ah.MultigridPreconditioner.from_coefficients(grid, k, device_s(coeff), h=h)
        else:
            assert live.set_coefficients(k, device_s(coeff)) is live
        fresh = ah.MultigridPreconditioner.from_coefficients(grid, k, device_s(coeff), h=h)
        want = plan(shape)[:3] if step != 1 else plan(shape)
        assert live.levels == fresh.levels == want
        assert live.caller_operator
        np.testing.assert_array_equal(live.vcycle(vd).to_numpy(), fresh.vcycle(vd).to_numpy())
        fresh.free()
    # bad coefficients are refused as at creation
    with pytest.raises(ValueError, match="per axis"):
        live.set_coefficients([1.0], -5.0)


def bratu_operator(P, u0):
    u = ah.DeviceArray.from_numpy(u0)
    res = u.zero()
    p = (P.hx, P.hy, P.lam)
    RESIDUALS["bratu2d"](res, u, p)
    return ah.JacobianOperator(RESIDUALS["bratu2d"], res, u, p)


@pytest.mark.gpu
def test_update_on_a_live_hierarchy(ctx):
    """update(J) for another u, and back: bitwise a fresh object's cycle"""
    shape = (130, 66)
    P, ua, *_, v, _ = reference("bratu2d", shape)
    ub = host_problem("bratu2d", shape, seed=5)[1]
    assert not np.array_equal(ua, ub)
    vd = ah.DeviceArray.from_numpy(v)
    Ja, Jb = bratu_operator(P, ua), bratu_operator(P, ub)
    live = ah.MultigridPreconditioner(Ja)
    za = live.vcycle(vd).to_numpy()
    zs = []
    for J in (Jb, Ja, Jb):
        assert live.update(J) is live
        fresh = ah.MultigridPreconditioner(J)
        assert live.levels == fresh.levels == plan(shape)
        zs.append(live.vcycle(vd).to_numpy())
        np.testing.assert_array_equal(zs[-1], fresh.vcycle(vd).to_numpy())
        fresh.free()
    np.testing.assert_array_equal(zs[1], za)
    assert not np.array_equal(zs[0], za)


LINEAR = [("bratu2d", (41, 25)), ("heat3d_midpoint", (17, 8, 8))]


@pytest.mark.gpu
@pytest.mark.parametrize("nu,cs", [(1, 1), (3, 3)])
@pytest.mark.parametrize("kind,shape", LINEAR, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in LINEAR])
def test_deterministic_and_linear_at_odd_sweeps(ctx, kind, shape, nu, cs):
    J, ref = device_operator(kind, shape)
    rng = np.random.default_rng(3)
    v, w = ref[5], rng.standard_normal(ref[5].shape)
    al, be = 0.7, -1.3
    mg = ah.MultigridPreconditioner(J, nu=nu, coarse_sweeps=cs)
    app = lambda q: mg.apply(J, ah.DeviceArray.from_numpy(q)).to_numpy()  # noqa: E731
    zv, zw = app(v), app(w)
    np.testing.assert_array_equal(zv, app(v))
    np.testing.assert_array_equal(zw, app(w))
    err = rel(app(al * v + be * w), al * zv + be * zw)
    print(f"{kind} {shape} nu={nu} cs={cs}: linearity {err:.3e} (allowed {option_tol(shape):.1e})")
    assert err <= option_tol(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", SOLVER_OPTIONS, ids=SOLVER_IDS)
def test_preconditioned_gmres_at_options(ctx, opts):
    J, ref = device_operator("bratu2d", (72, 56))
    P, u0, k, s, h = ref[:5]
    b = oc.residual(P, u0)
    A = lambda q: oc.jv_exact(P, u0, q)  # noqa: E731
    _, it_ref, ok_ref = gmres_right(A, Cycle((72, 56), h, k, s, **opts).vcycle, b, 1e-8)
    assert ok_ref
    mg = ah.MultigridPreconditioner(J, **opts)
    assert mg.levels == plan((72, 56), opts.get("max_levels", 0))
    for algo in ("gmres", "fgmres"):
        x, st = krylov(J, J.res, algo, N=mg)
        true = np.linalg.norm(b - A(x)) / np.linalg.norm(b)
        print(f"{algo} {opts}: niter {st.niter} (numpy {it_ref}), ||r|| / ||b|| {true:.2e}")
        assert st.solved
        assert abs(st.niter - it_ref) <= 1
        assert true <= 1e-7
