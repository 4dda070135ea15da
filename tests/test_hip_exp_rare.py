"""GPU: the exact phase of the correctly rounded exp (csrc/nk_exp.h) inside every Bratu kernel that calls it.

Every lane runs the exp's branch-free fast phase; the inputs its rounding test does not settle (about 2^-18
of the in-range ones, plus everything non-finite or outside (-708.3, 709.78)) take the exact fixed-point
phase, which reaches the kernels in three device forms (csrc/nk_exp_dev.hpp):

  nk_exp_lane               k_st2d's march: a divergent `noinline` call from the rare lanes, generated per
                            k_st2d<NK_BRATU2D, MODE, EPI, VEC, PER, F0R> instantiation (two call sites with F0R)
  nk_exp_t, LDS table       k_st1d: the wave-serial ballot / readlane loop under `if (i < nx)`
  nk_exp = nk_exp_t, global table   k_jv_batch (exact: once per point; FD: once per point and column),
                            k_jdiag (Jacobi / ILU(0) / multigrid level-0 diagonal), k_exp

Ordinary fields meet that phase at one point in 2^18.  Here the fields carry it where the glue can go wrong:
inputs known to be rare (oracle.exp_rare: nkx_exp_fast's own verdict, from the source the device compiles) are
PLANTED at the corners, the first / last lanes of a wave, both or one element of a VEC 2 lane, the last row
of a tile, the first of the next, a partial tile, a partial wave, and over whole rows across a tile boundary
(every lane of every wave calling, four rows running), and every kernel form is compared with the oracle --
np.array_equal, no tolerance anywhere.  Planted inputs:

  the family   x = a 2^-52 + 2^-53 (~1.46e-11), integer a in [2^16, 2^16 + 3000): 1 + x is a rounding
               midpoint, all 3000 are rare (tests/test_exp.py).  u + 2^-26 (k 2^-26) is the member a + k.
  the fixture  tests/golden/exp_ziv.npz: generic values of [-1, 3] found by scanning (make_exp_ziv.py)
  out of range 710, NaN, +-Inf, -720 (a subnormal result), -746 (0): the fast phase clamps x, so these also
               tell "exact phase skipped" from "exact phase taken" (on the in-range inputs above the fast
               phase's value is already the correctly rounded one: they test that the exact phase runs, returns
               the right bits and disturbs nothing around it)

Each comparison first asserts on the host that every planted argument of that launch is rare and counts the
rare evaluations the launch contains (> 0); at most 1/8 of the rest of the grid is rare, so the un-planted
neighbours are compared too.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from oracle import oracle as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -26            # the explicit FD step: u + EPS (k EPS) = u + k 2^-52, the family member a + k
FAM_LO, FAM_N, KMAX = 2 ** 16, 3000, 64
MODE_RES, MODE_JEXACT, MODE_JFD = 0, 1, 2
EPI_NONE, EPI_SUMSQ, EPI_DOT, EPI_RESID, EPI_DOTV, EPI_DOTVS = range(6)
SHAPES2 = [(130, 40), (129, 19), (514, 9)]   # VEC 2 with a 2-column wave 1 | VEC 1, 3-row last tile | 2 x-tiles


@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def family(a):
    return np.asarray(a, dtype=np.float64) * 2.0 ** -52 + 2.0 ** -53


def same(a, b):
    """NaN-aware equality (the out-of-range tests only)."""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def ziv_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "exp_ziv.npz"))["x"]


class Planted:
    """A Bratu problem, its planted field and where the plants are (host arrays, read-only).
    plants: every planted point; patch: the quiet patch / run of family values (a: their integers);
    inner: the patch points whose whole stencil lies in the patch."""

    def __init__(self, P, u, plants, patch, a, inner):
        self.P, self.u, self.plants, self.patch, self.a, self.inner = P, u, plants, patch, a, inner
        for x in (u, plants, patch, a, inner):
            x.flags.writeable = False

    def tangent_zero(self, seed):
        """v = 0 at every plant (w = u + eps v == u there), random elsewhere."""
        v = np.random.default_rng(seed).standard_normal(self.u.shape)
        v[self.plants] = 0.0
        return v

    def tangent_family(self, seed):
        """v = k 2^-26 on the patch, seeded integers |k| <= 64 (w = the family member a + k: another rare
        input), 0 at the other plants, random elsewhere."""
        rng = np.random.default_rng(seed)
        v = rng.standard_normal(self.u.shape)
        v[self.plants] = 0.0
        k = rng.integers(-KMAX, KMAX + 1, self.u.shape)
        v[self.patch] = k[self.patch] * EPS
        return v

    def tangent_one(self, seed):
        """v = 1 on the patch, random elsewhere (the exact JVP there is lap(1) + lam exp(u))."""
        v = np.random.default_rng(seed).standard_normal(self.u.shape)
        v[self.patch] = 1.0
        return v


def check_args(C, x, what):
    """The exp arguments x of one launch: every plant is rare, at most 1/8 of the rest is; returns the
    number of exact-phase evaluations the launch contains."""
    rare = oc.exp_rare(x)
    assert rare[C.plants].all(), f"{what}: a planted argument is not rare"
    assert rare[~C.plants].mean() <= 0.125, what
    n = int(rare.sum())
    assert n >= int(C.plants.sum()) > 0, what
    return n


def fd_args(C, v, eps=EPS):
    """w = u + eps v as the kernels form it: one multiplication, one addition, nothing fused."""
    return C.u + eps * v


def host_residual2d(P, u, e):
    """bratu2d's residual in numpy with e in place of exp(u) -- the oracle's association order
    (nk_oracle.c lap1 / point_residual)."""
    w = np.pad(u, 1)
    c = w[1:-1, 1:-1]
    with np.errstate(all="ignore"):
        lx = ((w[1:-1, 2:] - 2.0 * c) + w[1:-1, :-2]) / (P.hx * P.hx)
        ly = ((w[2:, 1:-1] - 2.0 * c) + w[:-2, 1:-1]) / (P.hy * P.hy)
        return (lx + ly) + P.lam * e


def host_residual1d(P, u, e):
    w = np.pad(u, 1)
    c = w[1:-1]
    with np.errstate(all="ignore"):
        return ((w[2:] - 2.0 * c) + w[:-2]) / (P.hx * P.hx) + P.lam * e


@functools.lru_cache(maxsize=None)
def plant2d(nx, ny):
    """The 2D plant map on an ordinary field (sin_ic + 0.05 noise), for 8-row tiles and 64 VEC columns per wave:
    (a) the four corners; (b) row 3 at the lane edges -- the columns of lane 0 / lane 63 of wave 0 and lane 0
    of wave 1 (and of the last lane / first lane around an x-tile boundary), for VEC 2 also one lane with
    only its k = 0 and one with only its k = 1 element planted (both planted: one lane calls twice in a row);
    (c) column 5 of rows 7, 8, ny - 1 (the last row of a tile, the first of the next, the last of a partial
    one); (d) the quiet patch: rows 6..9 over the full width, distinct family values; (e) 16 fixture values
    at seeded interior points."""
    P = oc.bratu2d(nx, ny)
    assert 8 < ny <= 64  # 8-row tiles (st_plan's floor, csrc/nk_plan.hpp), at least two of them
    rng = np.random.default_rng(1000 * nx + ny)
    u = oc.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    pool = iter(rng.permutation(np.arange(FAM_LO + KMAX, FAM_LO + FAM_N - KMAX)))
    plants = np.zeros(P.shape, dtype=bool)
    a = np.zeros(P.shape, dtype=np.int64)

    def put(j, i, val=None):
        assert 0 <= j < ny and 0 <= i < nx and not plants[j, i], (j, i)
        if val is None:
            a[j, i] = next(pool)
            val = family(a[j, i])
        u[j, i] = val
        plants[j, i] = True

    rows = list(range(6, min(9, ny - 1) + 1))
    for j in rows:                                  # (d)
        for i in range(nx):
            put(j, i)
    patch = plants.copy()
    inner = np.zeros(P.shape, dtype=bool)
    inner[rows[1]:rows[-1], 1:nx - 1] = True
    for j, i in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)):   # (a)
        if not plants[j, i]:
            put(j, i)
    vec = 2 if nx % 2 == 0 else 1
    cols = [0, 1, 126, 127, 128, 129, 20, 41] if vec == 2 else [0, 63, 64, 127, 128]   # (b); 20: k = 0 only, 41: k = 1 only
    if nx > 256 * vec:  # the last lane of x-tile 0 and the first of x-tile 1
        cols += [256 * vec - 2, 256 * vec - 1, 256 * vec, 256 * vec + 1] if vec == 2 else [256 * vec - 1, 256 * vec]
    for i in cols:
        put(3, i)
    for j in (7, 8, ny - 1):                        # (c)
        if not plants[j, 5]:
            put(j, 5)
    free = [(j, i) for j in range(1, ny - 1) for i in range(1, nx - 1) if not plants[j, i]]
    for (j, i), x in zip(rng.permutation(free)[:16], ziv_fixture()[:16]):   # (e)
        put(j, i, x)
    vals = u[patch]
    assert len(np.unique(vals)) == vals.size
    return Planted(P, u, plants, patch, a, inner)


@functools.lru_cache(maxsize=None)
def plant1d(n=300):
    """The 1D plant map on bratu1d(300) (block 0 full, block 1 with 44 active lanes): i = 0, 63, 64, 255,
    256 and 299 (the last active lane of a partial wave); the run 120..200 of family values (all of wave 2:
    64 iterations of the serial loop); 8 fixture values over the rest."""
    P = oc.bratu1d(n)
    rng = np.random.default_rng(n)
    u = oc.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    pool = iter(rng.permutation(np.arange(FAM_LO + KMAX, FAM_LO + FAM_N - KMAX)))
    plants = np.zeros(n, dtype=bool)
    a = np.zeros(n, dtype=np.int64)
    for i in list(range(120, 201)) + [0, 63, 64, 255, 256, n - 1]:
        a[i] = next(pool)
        u[i] = family(a[i])
        plants[i] = True
    patch = np.zeros(n, dtype=bool)
    patch[120:201] = True
    inner = np.zeros(n, dtype=bool)
    inner[121:200] = True
    free = np.flatnonzero(~plants)
    for i, x in zip(rng.permutation(free)[:8], ziv_fixture()[16:24]):
        u[i] = x
        plants[i] = True
    return Planted(P, u, plants, patch, a, inner)


OOR = {"overflow": 710.0, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "subnormal": -720.0, "zero": -746.0}


@functools.lru_cache(maxsize=None)
def plant_oor(dim):
    """The out-of-range class as isolated points of an ordinary field (lam = 0.25: lam exp stays apart from
    Inf): 710 (Inf) at a corner, NaN in lane 63, +Inf, -Inf, a 3 x 3 block (1D: 3 points) of -720 whose centre
    has Laplacian exactly 0 (its residual is 0.25 exp(-720), a subnormal) and one of -746 (centre residual
    exactly 0).  Returns (Planted, {name: index of the point / the block's centre})."""
    if dim == 2:
        P = oc.bratu2d(130, 40, lam=0.25)
        at = {"overflow": (0, 0), "nan": (3, 126), "+inf": (12, 40), "-inf": (20, 77), "subnormal": (27, 30), "zero": (33, 100)}
    else:
        P = oc.bratu1d(300, lam=0.25)
        at = {"overflow": (0,), "nan": (63,), "+inf": (100,), "-inf": (299,), "subnormal": (151,), "zero": (201,)}
    rng = np.random.default_rng(77 + dim)
    u = oc.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    plants = np.zeros(P.shape, dtype=bool)
    for name, idx in at.items():
        blk = tuple(slice(i - 1, i + 2) for i in idx) if name in ("subnormal", "zero") else idx
        u[blk] = OOR[name]
        plants[blk] = True
    z = np.zeros(P.shape, dtype=bool)
    return Planted(P, u, plants, z.copy(), np.zeros(P.shape, dtype=np.int64), z.copy()), at


# ----------------------------------------------------------------------------- device side
def device_F(P):
    return (ah.bratu_, (P.hx, P.lam)) if P.dim == 1 else (ah.bratu2d_, (P.hx, P.hy, P.lam))


def kernel_name(P, mode, epi, f0r=False):
    """The stencil instantiation a launch must have run: k_st1d<MODE, EPI> / k_st2d<KIND, MODE, EPI, VEC, PER, F0R>."""
    if P.dim == 1:
        return f"nk::k_st1d<{mode}, {epi}>"
    return f"nk::k_st2d<2, {mode}, {epi}, {2 if P.nx % 2 == 0 else 1}, false, {'true' if f0r else 'false'}>"


class Prof:
    """The profile of the launches inside the block: {name: {launches, kernel, ...}}."""

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


def devred(ctx, f, *a, **kw):
    """An oracle call in the device's reduction order (oracle.set_devred, test_hip_devred.py)."""
    oc.set_devred(True, cus=ctx.path_info()["resident_blocks"] or 256)
    try:
        return f(*a, **kw)
    finally:
        oc.set_devred(False)


def pointwise(ctx, C, eq=np.array_equal, norms=True, fd_only=False):
    """Residual (+ norm), exact JVP, the FD product for both tangents and diag(J) on the planted field C
    against the oracle; returns {launch: (rare evaluations, kernel that ran)}."""
    P, u = C.P, C.u
    F, p = device_F(P)
    ud = ah.DeviceArray.from_numpy(u)
    res, out = ud.zero(), ud.zero()
    F0 = oc.residual(P, u)
    cov = {}
    n_u = check_args(C, u, "exp(u)")
    with Prof(ctx) as pr:
        F(res, ud, p)
    assert eq(res.to_numpy(), F0), "residual"
    cov["residual"] = (n_u, pr.ran("residual", kernel_name(P, MODE_RES, EPI_NONE), 1))
    if norms and not fd_only:
        res2 = ud.zero()
        with Prof(ctx) as pr:
            nrm = F.residual_norm(res2, ud, p)
        assert eq(res2.to_numpy(), F0), "residual_norm's residual"
        _, so = devred(ctx, oc.newton_krylov, P, u, tol_abs=1e300, max_niter=0)  # ||F(u)|| alone: no Newton step
        assert so["outer_iterations"] == 0 and nrm == so["n_res_history"][0], (nrm, so["n_res_history"][0])
        cov["residual_norm"] = (n_u, pr.ran("residual_norm", kernel_name(P, MODE_RES, EPI_SUMSQ), 1))
    if not fd_only:
        v = C.tangent_one(11)
        with Prof(ctx) as pr:
            ah.mul_(out, ah.JacobianOperator(F, res, ud, p, jv="exact"), ah.DeviceArray.from_numpy(v))
        assert eq(out.to_numpy(), oc.jv_exact(P, u, v)), "exact JVP"
        cov["jv_exact"] = (n_u, pr.ran("jv_exact", kernel_name(P, MODE_JEXACT, EPI_NONE), 1))
    Jfd = ah.JacobianOperator(F, res, ud, p, jv="fd")
    tangents = [("w == u", C.tangent_zero(12))]
    if C.patch.any():
        tangents.append(("w = another member", C.tangent_family(13)))
    for what, v in tangents:
        w = fd_args(C, v)
        n_w = check_args(C, w, f"FD {what}")
        if what == "w == u":
            assert np.array_equal(w[C.plants], u[C.plants], equal_nan=True)
        else:
            assert np.array_equal(w[C.patch], family(C.a[C.patch] + np.rint(v[C.patch] / EPS).astype(np.int64)))
            assert (w[C.patch] != u[C.patch]).mean() > 0.9
        ref = oc.jv_fd(P, u, v, F0, EPS)
        if what == "w == u" and C.inner.any():
            assert np.all(ref[C.inner] == 0.0)  # the same stencil, the same F: the quotient is exactly 0
        with Prof(ctx) as pr:
            ah.mul_(out, Jfd, ah.DeviceArray.from_numpy(v), eps=EPS)
        assert eq(out.to_numpy(), ref), f"FD product, {what}"
        cov[f"jv_fd [{what}]"] = (n_w, pr.ran("jv_fd", None, 1))
    if not fd_only and norms:
        with Prof(ctx) as pr:
            d = ah.jacobian_diag(Jfd).to_numpy()
            dr = ah.jacobian_diag(Jfd, reciprocal=True).to_numpy()   # as ah.jacobi(J) builds its diagonal
        assert eq(d, oc.jacobian_diag(P, u)) and eq(dr, oc.jacobian_diag(P, u, reciprocal=True)), "diag(J)"
        cov["jacobian_diag"] = (n_u, pr.ran("jacobian_diag", None, 2))
    return cov


# ----------------------------------------------------------------------------- test 1: pointwise kernels
def test_patch_is_sensitive_to_one_ulp_of_exp():
    """Host only: on the quiet patch's interior rows all five stencil points are ~1.5e-11, the Laplacian is
    O(1e-9) and the residual is lam exp(u) to the last bit -- moving exp by one ulp, in either direction,
    changes the residual at >= 3/4 of those points (so a wrong last bit of the exact phase shows)."""
    for nx, ny in SHAPES2:
        C = plant2d(nx, ny)
        e = oc.exp(C.u)
        F0 = oc.residual(C.P, C.u)
        assert np.array_equal(host_residual2d(C.P, C.u, e), F0)  # the numpy restatement is the oracle's, bit for bit
        up = host_residual2d(C.P, C.u, np.nextafter(e, np.inf)) != F0
        dn = host_residual2d(C.P, C.u, np.nextafter(e, -np.inf)) != F0
        n = int(C.inner.sum())
        assert n >= nx - 2
        print(f"{nx}x{ny}: one ulp up moves {int(up[C.inner].sum())}, down {int(dn[C.inner].sum())}, "
              f"both {int((up & dn)[C.inner].sum())} of {n}")
        assert (up & dn)[C.inner].sum() >= 0.75 * n


@pytest.mark.parametrize("nx,ny", SHAPES2)
def test_pointwise_2d(ctx, nx, ny):
    """k_st2d (nk_exp_lane) and k_jdiag (nk_exp) on the planted grid: residual, its norm in the device's
    order, exact JVP, FD products (w == u; w another family member), diag(J) and its reciprocal -- equal to
    the oracle bit for bit, by the intended instantiation, each launch with its plants rare."""
    C = plant2d(nx, ny)
    cov = pointwise(ctx, C)
    vec = 2 if nx % 2 == 0 else 1
    for k in ("jv_fd [w == u]", "jv_fd [w = another member]"):
        assert cov[k][1] == f"nk::k_st2d<2, 2, 0, {vec}, false, false>", cov[k]  # (nk_jv never recomputes F0)
    assert all(n > 0 for n, _ in cov.values())
    print(json.dumps(cov, indent=1))


def test_pointwise_1d(ctx):
    """k_st1d (nk_exp_t, LDS table: the serial loop over a whole wave, a partial wave's last active lane)
    and k_jdiag on bratu1d(300)."""
    C = plant1d()
    cov = pointwise(ctx, C)
    for k in ("jv_fd [w == u]", "jv_fd [w = another member]"):
        assert cov[k][1] == "nk::k_st1d<2, 0>", cov[k]
    assert all(n > 0 for n, _ in cov.values())
    print(json.dumps(cov, indent=1))


# ----------------------------------------------------------------------------- test 2: batched JVPs
def batched(ctx, C, eq=np.array_equal, k=11):
    """k_jv_batch (nk_exp, global table) on the planted field: k = 8 + 3 columns in two launches, exact
    (exp(u) once per point and launch) and FD (exp(u + eps v_b) per point and column: column b moves the
    patch to family members of its own, one column is all zero)."""
    P, u = C.P, C.u
    F, p = device_F(P)
    ud = ah.DeviceArray.from_numpy(u)
    res = ud.zero()
    F(res, ud, p)
    F0 = oc.residual(P, u)
    assert eq(res.to_numpy(), F0)
    cov = {}
    launches, zcol = (k + 7) // 8, min(4, k - 1)  # 8 columns per launch; the all-zero FD column
    for jv in ("exact", "fd"):
        if jv == "exact":
            vs = [C.tangent_one(100 + b) for b in range(k)]
            n = launches * check_args(C, u, "batched exact")  # one evaluation per point in every launch
        else:
            vs = [C.tangent_family(200 + b) if C.patch.any() else C.tangent_zero(200 + b) for b in range(k)]
            vs[zcol] = np.zeros(P.shape)  # (an explicit eps: the kernel computes it, (F(u) - F0) / eps == 0)
            n = sum(check_args(C, fd_args(C, v), f"batched FD column {b}") for b, v in enumerate(vs))
            if C.patch.any():  # every column's patch arguments are its own
                ws = np.array([fd_args(C, v)[C.patch] for v in vs])
                assert all((ws[a] != ws[b]).mean() > 0.9 for a in range(k) for b in range(a))
        J = ah.JacobianOperator(F, res, ud, p, jv=jv)
        outs = [ud.zero() for _ in range(k)]
        with Prof(ctx) as pr:
            ah.mul_(outs, J, [ah.DeviceArray.from_numpy(v) for v in vs], eps=EPS)
        pr.ran(f"jv_{jv}_batch", None, launches)
        for b, (o, v) in enumerate(zip(outs, vs)):
            ref = oc.jv_exact(P, u, v) if jv == "exact" else oc.jv_fd(P, u, v, F0, EPS)
            assert eq(o.to_numpy(), ref), (jv, b)
        if jv == "fd" and eq is np.array_equal:
            assert not outs[zcol].to_numpy().any()
        cov[f"jv_{jv}_batch"] = n
    assert all(n > 0 for n in cov.values())
    return cov


@pytest.mark.parametrize("shape", [(130, 40), (300,)])
def test_batched_jvps(ctx, shape):
    C = plant2d(*shape) if len(shape) == 2 else plant1d(*shape)
    print(batched(ctx, C))


# ----------------------------------------------------------------------------- test 3: fused epilogues, whole solves
SOLVE_KW = dict(restart=True, memory=10, itmax=25, atol=0.0, rtol=0.0)


def gmres_solve(ctx, C, jv, f0r_flag=False, precond=False):
    """One restarted GMRES(10) solve of J(u) x = F(u) on the planted field, 25 steps, against the oracle in
    the device's order: the history and x bit for bit.  Returns (profile, path counters of this solve)."""
    P, u = C.P, C.u
    F, p = device_F(P)
    ud = ah.DeviceArray.from_numpy(u)
    res = ud.zero()
    F(res, ud, p)
    b = res.to_numpy()
    assert np.array_equal(b, oc.residual(P, u))
    kw = dict(SOLVE_KW)
    memory = kw.pop("memory")
    J = ah.JacobianOperator(F, res, ud, p, jv=jv)
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=memory))
    dkw, okw = {}, {}
    if precond:  # Jacobi from k_jdiag on the planted u: the un-fused Jv + dot form (V_k = N V_k is not the stored one)
        dkw["N"] = ah.jacobi(J)
        okw["N"] = ("diag", oc.jacobian_diag(P, u, reciprocal=True))
    before = ctx.path_info()
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, J, res, history=True, _f0_is_residual=f0r_flag, **dkw, **kw)
    after = ctx.path_info()
    x, st = ws.x.to_numpy(), ws.stats
    h = np.array(st.residuals)
    ws.free()
    xo, so, ho = devred(ctx, oc.krylov_solve, P, u, b, jv=jv, F0=b, memory=memory, **okw, **kw)
    assert st.niter == so["niter"] == kw["itmax"] and st.n_matvec == so["n_matvec"]
    np.testing.assert_array_equal(h, ho)
    np.testing.assert_array_equal(x, xo)
    assert np.isfinite(h).all() and np.isfinite(x).all()
    return pr, {k: after[k] - before[k] for k in ("jv_fd_f0r", "jv_fd_f0_read")}


def solves_2d(ctx, nx, ny, forced=False):
    """The solves of test 3 on one shape; `forced`: under NK_F0R=2 (every FD launch recomputes F(u)), the FD
    solves only.  Returns {profile name: (exp(u) rare evaluations per launch, launches, kernel)}."""
    C = plant2d(nx, ny)
    P = C.P
    n_u = check_args(C, C.u, "exp(u)")
    cov = {}

    def note(pr, name, epi, mode, f0r):
        k = pr.ran(name, kernel_name(P, mode, epi, f0r))
        cov[name] = (n_u, pr.read[name]["launches"], k)

    if not forced:
        # exact: every Jv launch evaluates exp(u) at every plant
        pr, _ = gmres_solve(ctx, C, "exact")
        note(pr, "jv_exact_dot_v1", EPI_DOTVS, MODE_JEXACT, False)
        note(pr, "jv_exact_dot_norm", EPI_DOTV, MODE_JEXACT, False)
        note(pr, "jv_exact_resid", EPI_RESID, MODE_JEXACT, False)
        if (nx, ny) == SHAPES2[0]:
            pr, _ = gmres_solve(ctx, C, "exact", precond=True)
            note(pr, "jv_exact_dot", EPI_DOT, MODE_JEXACT, False)
    # FD with F0 = the residual: the V_k-storing launches recompute F(u) -- the second call site evaluates
    # exp(u) at every plant (forced: every FD launch does)
    pr, ran = gmres_solve(ctx, C, "fd", f0r_flag=True)
    assert ran["jv_fd_f0r"] > 0
    note(pr, "jv_fd_dot_v1", EPI_DOTVS, MODE_JFD, True)
    note(pr, "jv_fd_dot_norm", EPI_DOTV, MODE_JFD, True)
    k = pr.ran("jv_fd_resid", kernel_name(P, MODE_JFD, EPI_RESID, forced))
    if forced:
        cov["jv_fd_resid"] = (n_u, pr.read["jv_fd_resid"]["launches"], k)
        assert ran["jv_fd_f0_read"] == 0
    else:
        assert ran["jv_fd_f0r"] == pr.read["jv_fd_dot_v1"]["launches"] + pr.read["jv_fd_dot_norm"]["launches"]
    if (nx, ny) == SHAPES2[0]:
        pr, ran = gmres_solve(ctx, C, "fd", f0r_flag=True, precond=True)
        k = pr.ran("jv_fd_dot", kernel_name(P, MODE_JFD, EPI_DOT, forced))
        if forced:
            cov["jv_fd_dot"] = (n_u, pr.read["jv_fd_dot"]["launches"], k)
            assert ran["jv_fd_f0_read"] == 0 and ran["jv_fd_f0r"] > 0
    assert all(v[0] > 0 and v[1] >= 1 for v in cov.values())
    return cov


@pytest.mark.parametrize("nx,ny", SHAPES2[:2])
def test_fused_epilogues_in_whole_solves_2d(ctx, nx, ny):
    """The epilogue instantiations of k_st2d -- the dot with its partner, the two V_k-storing forms, the
    restart residual -- through restarted GMRES(10) solves on the planted grid: every Jv launch of the exact
    solves, and the F(u)-recomputing launches of the FD solve, evaluate exp(u) at every plant, and the
    history and x equal the device-order oracle's bit for bit."""
    print(json.dumps(solves_2d(ctx, nx, ny), indent=1))


def test_fused_epilogues_in_a_cg_solve_1d(ctx):
    """k_st1d's Jv + <p, J p> (exact: exp(u) at every plant in every launch) through 40 CG steps on the
    planted bratu1d(300), bit for bit against the oracle in the device's order."""
    C = plant1d()
    P, u = C.P, C.u
    n_u = check_args(C, u, "exp(u)")
    F, p = device_F(P)
    ud = ah.DeviceArray.from_numpy(u)
    res = ud.zero()
    F(res, ud, p)
    b = res.to_numpy()
    assert np.array_equal(b, oc.residual(P, u))
    ws = ah.krylov_workspace("cg", ah.KrylovConstructor(res))
    with Prof(ctx) as pr:
        ah.krylov_solve_(ws, ah.JacobianOperator(F, res, ud, p, jv="exact"), res, history=True, itmax=40, atol=0.0, rtol=0.0)
    x, st = ws.x.to_numpy(), ws.stats
    ws.free()
    xo, so, ho = devred(ctx, oc.krylov_solve, P, u, b, algo="cg", itmax=40, atol=0.0, rtol=0.0)
    assert st.niter == so["niter"] == 40
    np.testing.assert_array_equal(np.array(st.residuals), ho)
    np.testing.assert_array_equal(x, xo)
    k = pr.ran("jv_exact_dot", kernel_name(P, MODE_JEXACT, EPI_DOT))
    assert pr.read["jv_exact_dot"]["launches"] >= 40 and n_u > 0
    print({"jv_exact_dot": (n_u, pr.read["jv_exact_dot"]["launches"], k)})


# ----------------------------------------------------------------------------- test 4: the out-of-range class
def oor_mismatches(ctx, dim):
    """The residual on the out-of-range field against the oracle: the indices that differ (NaN-aware)."""
    C, _ = plant_oor(dim)
    F, p = device_F(C.P)
    ud = ah.DeviceArray.from_numpy(C.u)
    res = ud.zero()
    F(res, ud, p)
    bad = ~same(res.to_numpy(), oc.residual(C.P, C.u))
    return [tuple(int(t) for t in idx) for idx in np.argwhere(bad)]


@pytest.mark.parametrize("dim", [2, 1])
def test_out_of_range_inputs(ctx, dim):
    """Inf, NaN, overflow, underflow and a subnormal result inside the stencils (k_st2d / k_st1d) and
    k_jv_batch: residual, exact JVP and the FD product (v = 0 at the plants) equal the oracle's, NaN-aware.
    The fast phase clamps these inputs, so a skipped exact phase cannot pass (test 6 shows it fail)."""
    C, at = plant_oor(dim)
    P, u = C.P, C.u
    F0 = oc.residual(P, u)
    # what the plants must give, from the oracle alone
    assert F0[at["subnormal"]] == 0.25 * oc.exp(np.array([-720.0]))[0] and 0.0 < F0[at["subnormal"]] < 2.2250738585072014e-308
    assert F0[at["zero"]] == 0.0 and np.isnan(F0[at["nan"]]) and np.isnan(F0[at["+inf"]]) and F0[at["-inf"]] == np.inf
    assert oc.exp(np.array([710.0]))[0] == np.inf
    assert oor_mismatches(ctx, dim) == []
    cov = pointwise(ctx, C, eq=lambda a, b: bool(same(a, b).all()), norms=False)
    assert all(n >= int(C.plants.sum()) for n, _ in cov.values())
    print(json.dumps(cov, indent=1))
    print(batched(ctx, C, eq=lambda a, b: bool(same(a, b).all()), k=3))


# ----------------------------------------------------------------------------- tests 5 and 6: the kernel-variant library
def child(code, **env):
    """A fresh python child on the kernel-variant library (lib/libnkhip_kbench.so: its knobs are read once
    per process); returns the JSON of its last output line."""
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=dict(os.environ, NK_KBENCH_LIB="1", **env),
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


CHILD_HEAD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import _nkpath
import ariadne_hip as ah
import test_hip_exp_rare as t
ctx = ah.Context(0); ah.set_default_context(ctx)
"""

F0R_CHILD = CHILD_HEAD + r"""
cov = t.pointwise(ctx, t.plant2d(130, 40), fd_only=True)
print(json.dumps(dict(pointwise=cov, solves=t.solves_2d(ctx, 130, 40, forced=True))))
"""

FASTONLY_CHILD = CHILD_HEAD + r"""
print(json.dumps({str(dim): t.oor_mismatches(ctx, dim) for dim in (2, 1)}))
"""


def test_f0_recomputing_call_site_when_forced():
    """NK_F0R=2 (kernel-variant library): every FD launch of a solve -- the plain Jv + dot and the restart
    residual too -- recomputes F(u), so their second exp call site evaluates exp(u) at every plant; the FD
    parts of the pointwise and whole-solve tests on 130 x 40 hold there bit for bit (asserted in the child).
    (The pointwise FD product, nk_jv, never recomputes F0: it runs k_st2d<2, 2, 0, VEC, false, false>.)"""
    r = child(F0R_CHILD, NK_F0R="2")
    s = r["solves"]
    for name, epi in (("jv_fd_dot", 2), ("jv_fd_resid", 3), ("jv_fd_dot_norm", 4), ("jv_fd_dot_v1", 5)):
        n, launches, kernel = s[name]
        assert n > 0 and launches >= 1 and kernel == f"nk::k_st2d<2, 2, {epi}, 2, false, true>", (name, s[name])
    assert all(n > 0 for n, _ in r["pointwise"].values())
    print(json.dumps(r, indent=1))


def test_a_skipped_exact_phase_is_noticed():
    """NK_EXP_FASTONLY=1 (the kernel-variant library's diagnosis knob: the stencils return the fast phase's
    value and ignore its rounding test): the out-of-range residual comparison then fails at exactly the
    points where the clamped fast value changes the residual -- predicted on the host from the oracle's fast
    value -- which are plants, and include 710, +Inf and the centres of the -720 and -746 blocks.
    (test_out_of_range_inputs holds the same comparison clean on the product library.)"""
    got = child(FASTONLY_CHILD, NK_EXP_FASTONLY="1")
    for dim, host in ((2, host_residual2d), (1, host_residual1d)):
        C, at = plant_oor(dim)
        F0 = oc.residual(C.P, C.u)
        assert same(host(C.P, C.u, oc.exp(C.u)), F0).all()  # the numpy restatement is the oracle's
        want = ~same(host(C.P, C.u, oc.exp_fast(C.u)), F0)
        assert not want[~C.plants].any()
        for name in ("overflow", "+inf", "subnormal", "zero"):
            assert want[at[name]], name
        # (NaN and -Inf cannot show in the residual: the point's own Laplacian term is already NaN / +Inf)
        assert not want[at["nan"]] and not want[at["-inf"]]
        mism = np.zeros(C.P.shape, dtype=bool)
        for idx in got[str(dim)]:
            mism[tuple(idx)] = True
        assert np.array_equal(mism, want), (np.argwhere(mism).tolist(), np.argwhere(want).tolist())
        print(dim, "mismatches under NK_EXP_FASTONLY=1:", np.argwhere(mism).tolist())
