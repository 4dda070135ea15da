"""3D Bratu (NK_BRATU3D, ah.bratu3d_) without a GPU: the ABI names, the Python residual object, the stencil plan
of a 3D non-heat shape, and the numpy restatement the GPU tests compare against (tests/bratu3d_ref.py) -- its
Newton iteration with a sparse LU and the eigenvalue of J nearest zero, against the numbers recorded when the
kind was defined.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
import bratu3d_ref as b3
from ariadne_hip import _lib
from oracle import oracle as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "newtonkrylov.jl_amd", "csrc")
SHIM = os.path.join(ROOT, "newtonkrylov.jl_amd", "julia", "AriadneHIP.jl")


def test_header_ctypes_and_shim_agree_on_the_kind():
    hdr = open(_lib.HEADER).read()
    m = re.search(r"^#define NK_BRATU3D (\d+)\b", hdr, re.M)
    assert m and int(m.group(1)) == 9 == _lib.NK_BRATU3D
    jl = open(SHIM).read()
    assert re.search(r"^const NK_BRATU3D = Int32\(9\)$", jl, re.M)
    # no other kind has the number
    kinds = re.findall(r"^#define (NK_(?:BRATU|HEAT|USER)\w+) (\d+)\b", hdr, re.M)
    assert [k for k, v in kinds if int(v) == 9] == ["NK_BRATU3D"]
    # the shim's problem() method and residual constant
    assert re.search(r"^problem\(F::HipResidual\{:bratu3d\}, u::HipVector, \(dx, dy, dz, λ\)\) = "
                     r"NkProblem\(NK_BRATU3D, 0, u\.grid\.\.\., dx, dy, dz, λ, 0, 0, C_NULL, C_NULL, F\.α\)$", jl, re.M)
    assert re.search(r"^const bratu3d! = HipResidual\{:bratu3d\}\(\)", jl, re.M)


class FakeArray:
    def __init__(self, *dims):
        self.grid = ah.Grid.full(*dims)


def test_bratu3d_builds_the_problem():
    assert ah.bratu3d_.kind == 9 and "bratu3d_" in ah.__all__ and repr(ah.bratu3d_) == "bratu3d!"
    p = ah.bratu3d_.problem(FakeArray(12, 10, 9), (0.1, 0.2, 0.3, 6.0))
    assert (p.kind, p.bc, p.nx, p.ny, p.nz) == (_lib.NK_BRATU3D, _lib.NK_BC_ZERO, 12, 10, 9)
    assert (p.hx, p.hy, p.hz) == (0.1, 0.2, 0.3)
    assert (p.lam, p.a, p.dt) == (6.0, 0.0, 0.0)
    assert not p.un and not p.user


@pytest.mark.parametrize("dims", [(12,), (12, 10)])
def test_bratu3d_needs_a_3d_grid(dims):
    with pytest.raises(ValueError, match="3D grid"):
        ah.bratu3d_.problem(FakeArray(*dims), (0.1, 0.1, 0.1, 1.0))
    for f, p in ((ah.bratu_, (0.1, 1.0)), (ah.bratu2d_, (0.1, 0.1, 1.0))):  # and its siblings refuse a 3D grid
        with pytest.raises(ValueError):
            f.problem(FakeArray(12, 10, 9), p)


# ----------------------------------------------------------------------------- the stencil plan
PLAN_SRC = r"""
#include <cstdio>
#include "nk_plan.hpp"
int main() {
    long long nx, ny, nz, mode, heat, vstore, vdot;
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld", &nx, &ny, &nz, &mode, &heat, &vstore, &vdot) == 7) {
        nk::StShape S{};
        S.dim = 3; S.nx = nx; S.ny = ny; S.nz = nz; S.mode = (int)mode; S.heat = heat != 0; S.scheme = 0;
        S.vstore = vstore != 0; S.vdot = vdot != 0;
        S.f0r = true;  // the caller's F0 is the library's F(u): the Newton loop's launches
        const nk::StPlan P = nk::st_plan(S, nk::StKnobs{});
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", P.f0r, P.vec, P.tiles_x, P.tiles_y, P.rows, P.grid, P.lds3, P.nw,
                    P.zalt, P.ym, P.group, P.nparts);
    }
    return 0;
}
"""
PLAN_SHAPES = [(12, 12, 12), (33, 17, 9), (130, 5, 4), (3, 3, 3), (65, 7, 5), (24, 20, 18), (40, 36, 20), (96, 12, 12),
               (256, 256, 256), (512, 512, 512)]


def test_3d_non_heat_shape_plans_no_f0r_and_the_heat_tiles():
    """k_st3l's F0R form is instantiated for G_Euler! only, so a 3D Bratu launch must never plan it -- whatever the
    mode and the fused form, with the caller's F0 known to be F(u) -- while G_Euler!'s Jv + dot does (the rule is
    live); every tile field is the heat shape's."""
    forms = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 0, 1), (2, 1, 1), (2, 1, 0)]  # (mode, vstore, vdot)
    lines = [f"{nx} {ny} {nz} {m} {heat} {vs} {vd}" for nx, ny, nz in PLAN_SHAPES for m, vs, vd in forms for heat in (0, 1)]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "plan3.cpp"), os.path.join(d, "plan3")
        with open(src, "w") as f:
            f.write(PLAN_SRC)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src], check=True)
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = [tuple(int(v) for v in o.split()) for o in p.stdout.splitlines()]
    assert len(out) == len(lines)
    ans = dict(zip(lines, out))
    heat_f0r = 0
    for nx, ny, nz in PLAN_SHAPES:
        for m, vs, vd in forms:
            bratu, heat = ans[f"{nx} {ny} {nz} {m} 0 {vs} {vd}"], ans[f"{nx} {ny} {nz} {m} 1 {vs} {vd}"]
            assert bratu[0] == 0, (nx, ny, nz, m, vs, vd)
            assert bratu[1:] == heat[1:], (nx, ny, nz, m, vs, vd)
            assert bratu[6:10] == (1, 4, 0, 0)  # k_st3l, 4-row tiles, plane-major upward marches, no y-march
            assert bratu[1] == (2 if nx % 2 == 0 else 1) and bratu[2] == -(-nx // (64 * bratu[1])) and bratu[3] == -(-ny // 4)
            assert bratu[4] == min(nz, max(16, -(-nz * bratu[2] * bratu[3] // 8192)))
            heat_f0r += heat[0]
    assert heat_f0r > 0


# ----------------------------------------------------------------------------- the restatement
def test_exp_rare_family():
    """all 3000 members a 2^-52 + 2^-53 are inputs the exp's fast phase does not settle"""
    assert oc.exp_rare(np.arange(2 ** 16, 2 ** 16 + 3000) * 2.0 ** -52 + 2.0 ** -53).all()


def test_restatement_is_consistent():
    """the tangent is the derivative of the residual, the diagonal and the assembled matrix are the tangent's"""
    P = b3.Problem(7, 6, 5, lam=6.0, h=(0.11, 0.13, 0.17))
    rng = np.random.default_rng(1)
    u, v = b3.sin_ic(P) + 0.1 * rng.standard_normal(P.shape), rng.standard_normal(P.shape)
    F0 = b3.residual(P, u)
    jv = b3.jv_exact(P, u, v)
    assert np.max(np.abs(b3.jv_fd(P, u, v, F0, 2.0 ** -26) - jv)) <= 1e-5 * np.max(np.abs(jv))
    A = b3.jacobian(P, u)
    assert np.max(np.abs(A @ v.reshape(-1) - jv.reshape(-1))) <= 1e-12 * np.max(np.abs(jv))
    assert abs(A - A.T).max() == 0.0
    np.testing.assert_array_equal(A.diagonal(), b3.jacobian_diag(P, u).reshape(-1))
    e = np.zeros(P.n)
    for i in (0, 17, P.n - 1):  # a column of the assembled matrix is the exact tangent of a unit vector, bit for bit
        e[:] = 0.0
        e[i] = 1.0
        np.testing.assert_array_equal(A[:, i].toarray().reshape(-1), b3.jv_exact(P, u, e.reshape(P.shape)).reshape(-1))
    # a 2D-like slab: with one plane the z term is ((0 - 2u) + 0) / hz^2 on top of the 2D oracle's residual
    Q = b3.Problem(9, 8, 1, lam=2.0)
    w = rng.standard_normal(Q.shape)
    P2 = oc.bratu2d(9, 8, lam=2.0)
    with np.errstate(all="ignore"):
        lz = ((0.0 - 2.0 * w[0]) + 0.0) / (Q.hz * Q.hz)
    lap2 = oc.residual(P2, w[0]) - P2.lam * oc.exp(w[0])
    assert np.max(np.abs(b3.lap(Q, w)[0] - (lap2 + lz))) <= 1e-12 * np.max(np.abs(lz))


@pytest.mark.parametrize("lam,eig_lo,eig_hi", [(3.51382, -25.55, -25.25), (6.0, -21.35, -21.05), (9.5, -8.45, -8.35)])
def test_newton_with_sparse_lu_converges(lam, eig_lo, eig_hi):
    """12 x 10 x 9 from the sine: 4 Newton steps to 1e-10 ||F(u0)||, J symmetric negative definite at the root with
    the recorded eigenvalue nearest zero: -25.3 ... -25.5, -21.1 ... -21.3 and -8.4 over the grids 12 x 10 x 9 to 40^3,
    figures rounded to one decimal, hence the 0.05 either side (9.5 is just under the 3D fold near 9.9)"""
    P = b3.Problem(12, 10, 9, lam=lam)
    u, steps, hist = b3.newton_lu(P, b3.sin_ic(P))
    print(f"lam {lam}: {steps} steps, ||F|| {hist}")
    assert steps == 4 and hist[-1] <= 1e-10 * hist[0]
    ev = b3.eig_nearest_zero(P, u)
    print(f"lam {lam}: eigenvalue nearest 0 {ev:.4f}")
    assert eig_lo <= ev <= eig_hi
    import scipy.sparse.linalg as spla

    top = float(spla.eigsh(b3.jacobian(P, u), k=1, which="LA", return_eigenvectors=False)[0])
    assert top < 0.0 and abs(top - ev) <= 1e-6 * abs(ev)  # negative definite: the largest eigenvalue is that one
