"""Semicoarsening for the geometric multigrid preconditioner (coarsening="semi": nk_mg_plan_semi,
nk_mg_create_levels, nk_mg_level_extents and the transfer kernels per set of coarsened axes).

The restatement is test_hip_multigrid.py's `Cycle` on a caller-given level list (`LevelCycle`); the plan has its own
restatement here (`plan_semi`).  CPU tests: the plan, why the feature exists (GMRES step counts of the restatement
with both plans), symmetry and definiteness of the semicoarsened cycle, the restatement's rounding sensitivity, the
header / ctypes / shim agreement on the three new names.  GPU tests: the V-cycle against the restatement where
semicoarsened levels run per-level kernels and where they run inside the one-launch tail, on every axis;
nk_mg_create_levels against nk_mg_create; from_coefficients with an anisotropic k; GMRES, Newton (both drivers and
the C++ example) and CG with the semicoarsened hierarchy.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from ariadne_hip import _lib
from oracle import oracle as oc
from test_hip_multigrid import (Cycle, ROOT, along, device_operator, gmres_right, host_problem, krylov, plan, rel,
                                transfers)

# The restatement's own rounding sensitivity on the semicoarsened plans: max over SEMI_CASES and the anisotropic-k
# case of max|float64 - longdouble| / max|longdouble| of one V-cycle, measured by
# test_restatement_sensitivity_is_as_recorded below (CPU): 4.108e-16.  The device evaluates the same cycle with fma and another
# association of the stencil sums: 16 x the value is allowed, the margin test_hip_multigrid.py uses.
# The long case (an x axis of 70000 points, 16 levels) gets its own value, as the long 1D case of test_hip_multigrid.py
# does: measured 1.113e-15.
SEMI_SENSITIVITY = 4.1e-16
SEMI_SENSITIVITY_LONG = 1.1e-15
SEMI_TOL = 16 * SEMI_SENSITIVITY


# ------------------------------------------------------------------------------------ the restatement
def plan_semi(shape, h=None, k=None, tau=0.5, max_levels=0):
    """the rule of the issue, in double precision and in its order"""
    d = len(shape)
    h = [1.0 / (n + 1) for n in shape] if h is None else h
    k = [1.0] * d if k is None else k
    length = [float(n + 1) * float(hh) for n, hh in zip(shape, h)]
    lv = [tuple(shape)]
    while any(n > 3 for n in lv[-1]) and (max_levels == 0 or len(lv) < max_levels):
        n = lv[-1]
        c = [0.0] * d
        for a in range(d):
            if n[a] > 3:
                q = float(n[a] + 1) / length[a]
                c[a] = abs(float(k[a])) * (q * q)
        bar = tau * max(c)
        lv.append(tuple(n[a] // 2 if n[a] > 3 and c[a] >= bar else n[a] for a in range(d)))
    return lv


class LevelCycle(Cycle):
    """Cycle on a given level list (Cycle.__init__ with `levels` in place of plan(shape, max_levels))"""

    def __init__(self, levels, h, k, s0, nu=2, coarse_sweeps=8, omega=None, dt=np.float64):
        shape = levels[0]
        d = len(shape)
        self.dt, self.nu, self.cs = dt, nu, coarse_sweeps
        self.omega = dt(omega) if omega else dt(2 * d) / dt(2 * d + 1)
        self.levels = [tuple(e) for e in levels]
        length = [dt(n + 1) * dt(hh) for n, hh in zip(shape, h)]
        self.c, self.s, self.diag, self.P, self.R = [], [], [], [], []
        s = np.asarray(s0, dtype=dt) * np.ones(tuple(reversed(shape)), dtype=dt)
        for l, ext in enumerate(self.levels):
            if l > 0:
                Ps, Rs = zip(*[transfers(nf, nc, dt) for nf, nc in zip(self.levels[l - 1], ext)])
                for a in range(d):
                    s = along(Rs[a], s, a)
            hl = [dt(h[a]) if l == 0 else length[a] / dt(ext[a] + 1) for a in range(d)]
            c = [dt(k[a]) / (hl[a] * hl[a]) for a in range(d)]
            diag = s - 2 * sum(c)
            if not (np.all(diag > 0) or np.all(diag < 0)):  # truncate before this level
                self.levels = self.levels[:l]
                break
            if l > 0:
                self.P.append(Ps)
                self.R.append(Rs)
            self.c.append(c)
            self.s.append(s)
            self.diag.append(diag)


# The GPU cases: semicoarsened levels in per-level kernels and inside the tail (the first level of at most 1024
# points), on each axis.  96 x 12: 1152 -> (48, 12) in the tail.  160 x 20: two x-only transfers before the tail.
# 64 x 8: the whole cycle in the tail.  32 x 32 x 4: x and y, z kept.  48 x 6 x 6: x only.  6 x 40 x 10: y only
# (2400 -> 1200 per level), then y and z in the tail.  (Each case of at most 10^4 points; LONG_SEMI below is the one
# larger case, for the index width.)
SEMI_CASES = [("bratu2d", (96, 12)), ("bratu2d", (12, 96)), ("bratu2d", (130, 66)), ("bratu2d", (160, 20)),
              ("bratu2d", (64, 8)), ("heat2d_trapezoid", (96, 12)), ("heat3d_euler", (32, 32, 4)),
              ("heat3d_midpoint", (48, 6, 6)), ("heat3d_euler", (6, 40, 10))]
# an x axis whose transfer index products pass 2^31 on a semicoarsened level: (70000 + 4) (35000 + 2) > 2^31, so the first
# x-only transfer runs the 64-bit instantiation of the per-mask kernels (every other case runs the 32-bit one)
LONG_SEMI = ("bratu2d", (70000, 4))
SEMI_CASES.append(LONG_SEMI)
SEMI_IDS = [f"{k}-{'x'.join(map(str, s))}" for k, s in SEMI_CASES]


def semi_tol(kind, shape):
    return 16 * SEMI_SENSITIVITY_LONG if (kind, shape) == LONG_SEMI else SEMI_TOL
ANISO = ((48, 48), [64.0, 1.0], -1.0)  # from_coefficients: shape, k, s (h = 1 / (n + 1))

_REF = {}


def semi_reference(kind, shape):
    """(P, u, k, s, h, v, levels, the float64 restatement's V-cycle of v) of one case, computed once"""
    key = (kind, shape)
    if key not in _REF:
        P, u, k, s, h = host_problem(kind, shape)
        v = np.random.default_rng(11).standard_normal(P.shape)
        lv = plan_semi(shape, h, k)
        _REF[key] = (P, u, k, s, h, v, lv, LevelCycle(lv, h, k, s).vcycle(v))
    return _REF[key]


def aniso_reference():
    if "aniso" not in _REF:
        shape, k, s = ANISO
        h = [1.0 / (n + 1) for n in shape]
        v = np.random.default_rng(13).standard_normal(tuple(reversed(shape)))
        lv = plan_semi(shape, h, k)
        _REF["aniso"] = (shape, h, k, s, v, lv, LevelCycle(lv, h, k, s).vcycle(v))
    return _REF["aniso"]


# ------------------------------------------------------------------------------------ CPU tests
def c_plan_semi(shape, h=None, k=None, tau=0.0, max_levels=0):
    """nk_mg_plan_semi itself: (return code, levels)"""
    d = len(shape)
    n = (C.c_int64 * 3)(*(list(shape) + [1, 1])[:3])
    hh = (C.c_double * 3)(*(list(h if h is not None else [1.0 / (m + 1) for m in shape]) + [1.0, 1.0])[:3])
    kk = None if k is None else (C.c_double * 3)(*(list(k) + [1.0, 1.0])[:3])
    ext, nl = (C.c_int64 * (3 * 64))(), C.c_int32(0)
    rc = ah.load().nk_mg_plan_semi(n, hh, kk, tau, max_levels, ext, 64, C.byref(nl))
    return rc, [tuple(int(ext[3 * l + a]) for a in range(d)) for l in range(nl.value if rc == 0 else 0)]


PLAN_EXPECTED = {
    (96, 12): [(96, 12), (48, 12), (24, 12), (12, 12), (6, 6), (3, 3)],
    (130, 66): [(130, 66), (65, 66), (32, 33), (16, 16), (8, 8), (4, 4), (2, 2)],
    (6, 40, 10): [(6, 40, 10), (6, 20, 10), (6, 10, 10), (6, 5, 5), (3, 2, 2)],
}
PLAN_SAME_AS_FULL = [(4096, 4096), (72, 56), (100,), (5,), (4, 4), (3, 3)]
PLAN_ALL = list(PLAN_EXPECTED) + [(16384, 2048)] + PLAN_SAME_AS_FULL


@pytest.mark.parametrize("shape", PLAN_ALL, ids=str)
def test_semi_plan_matches_restatement(shape):
    want = plan_semi(shape)
    assert ah.multigrid_plan(shape, coarsening="semi") == want
    assert c_plan_semi(shape) == (0, want)  # threshold 0: the default 0.5
    assert c_plan_semi(shape, tau=0.5) == (0, want)
    if shape in PLAN_EXPECTED:
        assert want == PLAN_EXPECTED[shape]
    if shape == (16384, 2048):
        assert len(want) == 14 and want[-1] == (2, 2)
        assert want[:5] == [(16384, 2048), (8192, 2048), (4096, 2048), (2048, 2048), (1024, 1024)]
    if shape in PLAN_SAME_AS_FULL:
        assert want == plan(shape) == ah.multigrid_plan(shape)
    # max_levels cuts the list; a tiny threshold lets every axis qualify: nk_mg_plan's levels
    assert ah.multigrid_plan(shape, 3, coarsening="semi") == want[:3] == plan_semi(shape, max_levels=3)
    assert ah.multigrid_plan(shape, coarsening="semi", threshold=1e-300) == plan(shape)
    assert c_plan_semi(shape, tau=1e-300) == (0, plan(shape))
    # every level coarsens at least one axis by n // 2, and keeps the others
    for f, c in zip(want, want[1:]):
        assert f != c and all(nc == nf or (nf > 3 and nc == nf // 2) for nf, nc in zip(f, c))


def test_semi_plan_follows_the_coefficients_and_the_threshold():
    got = ah.multigrid_plan((64, 64), coarsening="semi", k=(64.0, 1.0))
    assert got == plan_semi((64, 64), k=[64.0, 1.0])
    assert got[:4] == [(64, 64), (32, 64), (16, 64), (8, 64)] and got[4] == (4, 32)  # x only until c_x = c_y
    assert ah.multigrid_plan((64, 64), coarsening="semi", k=(-64.0, 1.0)) == got  # |k|
    assert c_plan_semi((64, 64), k=[64.0, 1.0]) == (0, got)
    # a ratio of 4 between the couplings (130 x 66): coarsened together from a threshold of 1/4 on
    assert ah.multigrid_plan((130, 66), coarsening="semi", threshold=0.25) == plan_semi((130, 66), tau=0.25) == plan((130, 66))
    assert ah.multigrid_plan((130, 66), coarsening="semi", threshold=1.0) == plan_semi((130, 66), tau=1.0)
    # other spacings than 1 / (n + 1): a square grid on a 4 : 1 rectangle
    h = [4.0 / 65, 1.0 / 65]
    assert ah.multigrid_plan((64, 64), coarsening="semi", h=h) == plan_semi((64, 64), h=h)
    assert plan_semi((64, 64), h=h)[1] == (64, 32)


def test_semi_plan_rejects_bad_arguments():
    E = _lib.NK_E_ARG
    assert c_plan_semi((96, 12), tau=1.5)[0] == E
    assert c_plan_semi((96, 12), tau=-0.1)[0] == E
    assert c_plan_semi((96, 12), tau=math.nan)[0] == E
    assert c_plan_semi((96, 12), k=[0.0, 1.0])[0] == E
    assert c_plan_semi((96, 12), k=[1.0, math.nan])[0] == E
    assert c_plan_semi((96, 12), k=[math.inf, 1.0])[0] == E
    assert c_plan_semi((96, 12), h=[0.0, 0.1])[0] == E
    assert c_plan_semi((0, 12))[0] == E
    assert c_plan_semi((96, 12), max_levels=-1)[0] == E
    nl = C.c_int32(0)
    n, h = (C.c_int64 * 3)(9, 1, 1), (C.c_double * 3)(0.1, 1.0, 1.0)
    assert ah.load().nk_mg_plan_semi(n, h, None, 0.0, 0, None, 0, C.byref(nl)) == 0 and nl.value == 3  # a null k: ones
    assert ah.load().nk_mg_plan_semi(n, None, None, 0.0, 0, None, 0, C.byref(nl)) == E
    # the unused axes of a 1D grid are not read: a zero k there is no error
    assert c_plan_semi((9,), k=[1.0, 0.0, 0.0]) == (0, [(9,), (4,), (2,)])


def test_python_rejects_bad_coarsening_without_a_device():
    with pytest.raises(ValueError, match="coarsening"):
        ah.multigrid_plan((96, 12), coarsening="line")
    with pytest.raises(ValueError, match="threshold"):
        ah.multigrid_plan((96, 12), coarsening="semi", threshold=0.0)
    with pytest.raises(ValueError, match="threshold"):
        ah.multigrid_plan((96, 12), coarsening="semi", threshold=1.5)
    with pytest.raises(ValueError, match="coarsening"):
        ah.multigrid(coarsening="zebra")
    with pytest.raises(ValueError, match="threshold"):
        ah.multigrid(coarsening="semi", threshold=-1.0)
    with pytest.raises(ValueError, match="coarsening"):
        ah.MultigridPreconditioner.from_coefficients(ah.Grid.full(16, 12), [1.0, 1.0], -1.0, coarsening="both",
                                                     ctx=object())
    fac = ah.multigrid(spd=True, coarsening="semi", threshold=0.25)
    assert fac.opts == {"spd": True, "coarsening": "semi", "threshold": 0.25}


def gmres_steps(kind, shape, levels):
    P, u, k, s, h = host_problem(kind, shape)
    b = oc.residual(P, u)
    _, it, ok = gmres_right(lambda q: oc.jv_exact(P, u, q), LevelCycle(levels, h, k, s).vcycle, b, 1e-8)
    return it, ok


@pytest.mark.parametrize("kind,shape,semi_max,full_min", [("bratu2d", (96, 12), 10, 20), ("heat3d_euler", (32, 32, 4), 10, 18)],
                         ids=["bratu2d-96x12", "heat3d_euler-32x32x4"])
def test_restatement_gmres_counts_with_both_plans(kind, shape, semi_max, full_min):
    """why the feature exists: GMRES(30) to rtol 1e-8 with the restatement as N.  Measured: 96 x 12 semi 7, full 29;
    32 x 32 x 4 semi 7, full 26"""
    it_semi, ok_semi = gmres_steps(kind, shape, plan_semi(shape))
    it_full, ok_full = gmres_steps(kind, shape, plan(shape))
    print(f"{kind} {shape}: GMRES steps semi {it_semi}, full {it_full}")
    assert ok_semi and it_semi <= semi_max
    assert ok_full and it_full >= full_min


@pytest.mark.parametrize("kind,shape", [("bratu2d", (24, 4)), ("heat2d_euler", (5, 33)), ("heat3d_euler", (12, 4, 3))],
                         ids=["bratu2d-24x4", "heat2d_euler-5x33", "heat3d_euler-12x4x3"])
def test_semicoarsened_cycle_is_symmetric_and_definite(kind, shape):
    P, u, k, s, h = host_problem(kind, shape)
    lv = plan_semi(shape, h, k)
    assert lv != plan(shape)
    cyc = LevelCycle(lv, h, k, s)
    n = int(np.prod(shape))
    V = np.empty((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        V[:, j] = cyc.vcycle(e.reshape(P.shape)).reshape(-1)
    asym = float(np.max(np.abs(V - V.T)) / np.max(np.abs(V)))
    lam = np.linalg.eigvalsh(-(V + V.T) / 2)
    print(f"{kind} {shape}: max|V - V^T| / max|V| {asym:.2e}, lambda_min / lambda_max of -V {lam[0] / lam[-1]:.2e}")
    assert asym <= 1e-14
    assert lam[0] > 0.0


def test_restatement_sensitivity_is_as_recorded():
    def sens(lv, h, k, s, v, z64):
        zl = LevelCycle(lv, h, k, s, dt=np.longdouble).vcycle(v)
        return float(np.max(np.abs(z64 - zl)) / np.max(np.abs(zl)))

    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    worst = 0.0
    for kind, shape in SEMI_CASES:
        if (kind, shape) != LONG_SEMI:
            P, u, k, s, h, v, lv, z64 = semi_reference(kind, shape)
            worst = max(worst, sens(lv, h, k, s, v, z64))
    shape, h, k, s, v, lv, z64 = aniso_reference()
    worst = max(worst, sens(lv, h, k, s, v, z64))
    P, u, k, s, h, v, lv, z64 = semi_reference(*LONG_SEMI)
    assert len(lv) == 16 and lv[1] == (35000, 4) and lv[-2:] == [(4, 4), (2, 2)]
    long = sens(lv, h, k, s, v, z64)
    print(f"semicoarsened restatement float64 vs longdouble: {worst:.3e}, long case {long:.3e}")
    assert SEMI_SENSITIVITY / 1.5 <= worst <= 1.5 * SEMI_SENSITIVITY
    assert SEMI_SENSITIVITY_LONG / 1.5 <= long <= 1.5 * SEMI_SENSITIVITY_LONG


NEW_NAMES = ["nk_mg_plan_semi", "nk_mg_create_levels", "nk_mg_level_extents"]


def test_header_ctypes_and_shim_agree_on_the_new_names():
    hdr = open(_lib.HEADER).read()
    shim = open(os.path.join(ROOT, "newtonkrylov.jl_amd", "julia", "AriadneHIP.jl")).read()
    lib = ah.load()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "ptr"
        return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "double": "f64"}[decl.replace("const", "").split()[0]]

    def ct_class(t):
        return {C.c_int: "i32", C.c_int32: "i32", C.c_int64: "i64", C.c_double: "f64"}.get(t, "ptr")

    def jl_class(t):
        t = t.strip()
        return "ptr" if t.startswith(("Ptr", "Ref")) or t == "VP" else {"Cint": "i32", "Int32": "i32", "Int64": "i64",
                                                                       "Float64": "f64"}[t]

    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    expected = {"nk_mg_plan_semi": ["ptr", "ptr", "ptr", "f64", "i32", "ptr", "i32", "ptr"],
                "nk_mg_create_levels": ["ptr", "ptr", "ptr", "ptr", "i32", "ptr"],
                "nk_mg_level_extents": ["ptr", "ptr", "i32", "ptr"]}
    for n in NEW_NAMES:
        assert re.search(rf"^int {n}\(", hdr, re.M), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
        assert f"ccall((:{n}, libnkhip)" in shim, n
        args = re.search(rf"\bint {n}\(([^;]*?)\);", flat, re.S).group(1)
        want = [c_class(a.strip()) for a in args.split(",")]
        assert want == expected[n], n
        assert [ct_class(t) for t in _lib.SIGNATURES[n][1]] == want, n
        call = shim[shim.index(f"ccall((:{n}, libnkhip)"):]
        jl = re.match(r"ccall\(\(:\w+, libnkhip\), Cint,\s*\((.*?)\),\s", call, re.S).group(1)
        depth, cur, got = 0, "", []
        for ch in jl + ",":
            depth += ch == "{"
            depth -= ch == "}"
            if ch == "," and depth == 0:
                if cur.strip():
                    got.append(jl_class(cur))
                cur = ""
            else:
                cur += ch
        assert got == want, (n, got, want)
    assert re.search(r"function hip_multigrid\(J::Ariadne\.JacobianOperator; spd = false, coarsening = :full, threshold = 0\.5\)", shim)
    # nk_mg_opts is as it was
    assert C.sizeof(_lib.nk_mg_opts) == 24 and [f for f, _ in _lib.nk_mg_opts._fields_] == ["nu", "coarse_sweeps", "omega", "max_levels"]


# ------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", SEMI_CASES, ids=SEMI_IDS)
def test_semi_vcycle_matches_restatement(ctx, kind, shape):
    J, _ = device_operator(kind, shape)
    P, u, k, s, h, v, lv, zref = semi_reference(kind, shape)
    mg = ah.MultigridPreconditioner(J, coarsening="semi")
    assert mg.levels == lv == ah.multigrid_plan(shape, coarsening="semi", h=h)
    vd = ah.DeviceArray.from_numpy(v)
    z = mg.vcycle(vd).to_numpy()
    err = rel(z, zref)
    print(f"{kind} {shape} {lv[:6]}: device vs restatement {err:.3e} (allowed {semi_tol(kind, shape):.1e})")
    assert err <= semi_tol(kind, shape)
    # two applications give the same bits, through nk_precond_apply too; in place (z == v) as well
    np.testing.assert_array_equal(mg.vcycle(vd).to_numpy(), z)
    np.testing.assert_array_equal(mg.apply(J, vd).to_numpy(), z)
    w = ah.DeviceArray.from_numpy(v)
    assert mg.vcycle(w, z=w) is w
    np.testing.assert_array_equal(w.to_numpy(), z)


def create_levels(ctx, prob, levels, opts=None):
    """nk_mg_create_levels itself: (return code, message, handle)"""
    lib = ah.load()
    h = C.c_void_p()
    flat = [n for e in levels for n in (list(e) + [1, 1])[:3]]
    ext = (C.c_int64 * max(1, len(flat)))(*flat)
    rc = lib.nk_mg_create_levels(ctx.handle, C.byref(prob), C.byref(opts) if opts is not None else None, ext, len(levels), C.byref(h))
    return rc, (lib.nk_last_error(ctx.handle) or b"").decode(), h


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [("bratu2d", (72, 56)), ("bratu2d", (40, 6)), ("heat3d_euler", (17, 13, 9))],
                         ids=["bratu2d-72x56", "bratu2d-40x6", "heat3d_euler-17x13x9"])
def test_create_levels_on_the_full_plan_is_nk_mg_create(ctx, kind, shape):
    lib = ah.load()
    J, ref = device_operator(kind, shape)
    v = ah.DeviceArray.from_numpy(ref[5])
    z0 = ah.MultigridPreconditioner(J).vcycle(v).to_numpy()
    prob = J.problem()
    opts = _lib.nk_mg_opts(0, 0, 0.0, 2)  # max_levels is ignored: the list is the plan
    rc, msg, h = create_levels(ctx, prob, ah.multigrid_plan(shape), opts)
    assert rc == 0, msg
    try:
        assert lib.nk_mg_set_jacobian(h, C.byref(prob), J.u.ptr) == 0
        ext, nl, n1 = (C.c_int64 * (3 * 64))(), C.c_int32(0), C.c_int32(0)
        assert lib.nk_mg_level_extents(h, ext, 64, C.byref(nl)) == 0 and lib.nk_mg_levels(h, C.byref(n1)) == 0
        assert nl.value == n1.value == len(plan(shape))
        assert [tuple(ext[3 * l + a] for a in range(len(shape))) for l in range(nl.value)] == plan(shape)
        assert lib.nk_mg_level_extents(h, ext, 2, C.byref(nl)) == 0 and nl.value == len(plan(shape))  # cap < count
        z = v.zero()
        assert lib.nk_mg_apply(h, z.ptr, v.ptr) == 0
        ctx.sync()
        np.testing.assert_array_equal(z.to_numpy(), z0)
    finally:
        assert lib.nk_mg_destroy(h) == 0


@pytest.mark.gpu
def test_create_levels_rejections(ctx):
    g = ah.Grid.full(96, 12)
    prob = g.geometry_problem()
    prob.hx, prob.hy = 1.0 / 97, 1.0 / 13
    good = plan_semi((96, 12))
    rc, msg, h = create_levels(ctx, prob, good)
    assert rc == 0, msg
    assert ah.load().nk_mg_destroy(h) == 0
    E = _lib.NK_E_ARG
    rc, msg, _ = create_levels(ctx, prob, [(48, 12), (24, 12)])
    assert rc == E and "level 0" in msg
    rc, msg, _ = create_levels(ctx, prob, [(96, 12), (48, 5)])  # 12 -> 5
    assert rc == E and "neither kept nor" in msg
    rc, msg, _ = create_levels(ctx, prob, [(96, 12), (48, 12), (48, 12)])
    assert rc == E and "coarsens no axis" in msg
    rc, msg, _ = create_levels(ctx, prob, [(96, 12), (192, 12)])  # refined
    assert rc == E and "neither kept nor" in msg
    rc, msg, _ = create_levels(ctx, prob, [])
    assert rc == E and "levels" in msg
    rc, msg, _ = create_levels(ctx, prob, [(96, 12)] * 33)
    assert rc == E and "levels" in msg
    # an axis of at most 3 points is not coarsened
    g3 = ah.Grid.full(96, 3)
    p3 = g3.geometry_problem()
    p3.hx, p3.hy = 1.0 / 97, 0.25
    rc, msg, _ = create_levels(ctx, p3, [(96, 3), (48, 1)])
    assert rc == E and "neither kept nor" in msg
    prob.bc = _lib.NK_BC_PERIODIC
    rc, msg, _ = create_levels(ctx, prob, good)
    assert rc == E and "periodic" in msg
    prob.bc, prob.kind = _lib.NK_BC_ZERO, _lib.NK_USER2D
    rc, msg, _ = create_levels(ctx, prob, good)
    assert rc == E and "user residual" in msg


@pytest.mark.gpu
def test_from_coefficients_with_an_anisotropic_k(ctx):
    shape, h, k, s, v, lv, zref = aniso_reference()
    assert lv[:4] == [(48, 48), (24, 48), (12, 48), (6, 48)]
    grid = ah.Grid.full(*shape)
    mg = ah.MultigridPreconditioner.from_coefficients(grid, k, s, coarsening="semi")
    assert mg.levels == lv
    vd = ah.DeviceArray.from_numpy(v)
    err = rel(mg.vcycle(vd).to_numpy(), zref)
    print(f"k = {k} on {shape} {lv}: device vs restatement {err:.3e} (allowed {SEMI_TOL:.1e})")
    assert err <= SEMI_TOL
    # other coefficients on the live hierarchy: the plan stays
    mg.set_coefficients([1.0, 1.0], -1.0)
    assert mg.levels == lv
    err = rel(mg.vcycle(vd).to_numpy(), LevelCycle(lv, h, [1.0, 1.0], -1.0).vcycle(v))
    assert err <= SEMI_TOL
    # the default plan of the same operator is the full one
    assert ah.MultigridPreconditioner.from_coefficients(grid, k, s).levels == plan(shape)


@pytest.mark.gpu
def test_gmres_with_the_semicoarsened_cycle(ctx):
    shape = (96, 12)
    J, _ = device_operator("bratu2d", shape)
    P, u0, k, s, h, v, lv, _ = semi_reference("bratu2d", shape)
    b = oc.residual(P, u0)
    A = lambda q: oc.jv_exact(P, u0, q)  # noqa: E731
    _, it_ref, ok_ref = gmres_right(A, LevelCycle(lv, h, k, s).vcycle, b, 1e-8)
    assert ok_ref
    x, st = krylov(J, J.res, "gmres", N=ah.multigrid(coarsening="semi"))
    _, st_full = krylov(J, J.res, "gmres", N=ah.multigrid())
    print(f"GMRES(30) on bratu2d {shape}: semi {st.niter} (numpy {it_ref}), full {st_full.niter}")
    assert st.solved and abs(st.niter - it_ref) <= 1
    assert np.linalg.norm(b - A(x)) <= 1e-7 * np.linalg.norm(b)
    assert st_full.niter >= 2 * st.niter


@pytest.mark.gpu
def test_newton_with_the_semicoarsened_factory(ctx):
    P = oc.bratu2d(160, 20)
    u0 = oc.sin_ic(P)
    p = (P.hx, P.hy, P.lam)
    fac = ah.multigrid(coarsening="semi")
    u, r = ah.newton_krylov_(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, N=fac, memory=20)
    assert r.solved and fac.mg.levels == plan_semi((160, 20))
    un, rn = ah.newton_krylov_native(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, N=ah.multigrid(coarsening="semi"), memory=20)
    assert rn.solved and rn.stats[:2] == r.stats[:2]
    uf, rf = ah.newton_krylov_(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, N=ah.multigrid, memory=20)
    assert rf.solved
    print(f"Newton 160 x 20: semi outer {r.stats.outer_iterations} inner {r.stats.inner_iterations}; "
          f"full outer {rf.stats.outer_iterations} inner {rf.stats.inner_iterations}")
    # Both solves stop at ||F(u)|| <= tol, and F(u_a) - F(u_b) = J (u_a - u_b) with J = Δ_h + λ e^u between the two.
    # -Δ_h >= 2 π² - O(h²) > 19 on the unit square and λ e^u < 3.52 e^0.5 < 6 (u_max of this problem is below 0.5), so
    # ||J^-1|| <= 1 / 13 < 1: the solutions differ by less than the sum of the two residual norms
    bound = r.stats.n_res + rf.stats.n_res
    assert float(np.max(u.to_numpy())) < 0.5
    for other in (un, uf):
        assert np.linalg.norm(u.to_numpy() - other.to_numpy()) <= bound
    np.testing.assert_array_equal(un.to_numpy(), u.to_numpy())
    # the C++ caller on the same grid
    exe = os.path.join(ROOT, "newtonkrylov.jl_amd", "bin", "bratu2d_newton")
    out = subprocess.run([exe, "160", "20", "exact", "20", "0", "--mg-semi"], capture_output=True, text=True, timeout=120, check=True)
    j = json.loads(out.stdout.strip().splitlines()[-1])
    assert j["mg"] and j["coarsening"] == "semi" and j["ny"] == 20 and j["solved"]
    assert (j["outer"], j["inner"]) == tuple(r.stats[:2])


@pytest.mark.gpu
def test_spd_form_of_the_semicoarsened_cycle(ctx):
    shape = (96, 12)
    J, _ = device_operator("bratu2d", shape)
    P, u0, k, s, h, v, lv, _ = semi_reference("bratu2d", shape)
    vd = ah.DeviceArray.from_numpy(v)
    z = ah.MultigridPreconditioner(J, coarsening="semi").vcycle(vd).to_numpy()
    mg = ah.MultigridPreconditioner(J, spd=True, coarsening="semi")
    assert mg.spd and mg.levels == lv
    zs = mg.vcycle(vd).to_numpy()
    np.testing.assert_array_equal(zs, -z)
    zd, vz = mg.vcycle_dot(vd)
    np.testing.assert_array_equal(zd.to_numpy(), zs)
    # <v, z> in another summation order than numpy's: n eps Σ|v_i z_i| bounds both (Higham, Accuracy and Stability, §3.1)
    n = v.size
    exact = math.fsum((v * zs).reshape(-1))
    assert abs(vz - exact) <= n * np.finfo(float).eps * float(np.sum(np.abs(v * zs)))
    assert vz > 0.0
    # CG on -J x = -F with M: no more steps than with the fully coarsened M
    counts = {}
    for name, fac in (("semi", ah.multigrid(spd=True, coarsening="semi")), ("full", ah.multigrid(spd=True))):
        ws = ah.krylov_workspace("cg", ah.KrylovConstructor(J.res))
        ah.krylov_solve_(ws, J, J.res, itmax=200, atol=0.0, rtol=1e-8, M=fac(J))
        counts[name] = (ws.stats.niter, ws.stats.solved)
        ws.free()
        fac.free()
    print(f"CG on bratu2d {shape}: {counts}")
    assert counts["semi"][1] and counts["full"][1]
    assert counts["semi"][0] <= counts["full"][0]
