"""The 2D ignition kinds (NK_IGNITION2D_*, ah.ignition_) without a GPU: the Python residual objects the implicit
schemes bind, the problem struct they fill, and the numpy restatement the GPU tests compare against
(tests/ignition_ref.py) -- against what is already pinned (the oracle's heat and Bratu restatements) and against the
physics of u_t = a Δu + λ exp(u): relaxation to the steady Bratu solution below the fold, blow-up above it.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
import ignition_ref as ig
from ariadne_hip import _lib
from oracle import oracle as oc

SCHEMES = {"euler": ah.G_Euler_, "midpoint": ah.G_Midpoint_, "trapezoid": ah.G_Trapezoid_}


class FakeArray(ah.DeviceArray):
    """a DeviceArray the residual objects accept for u and u_n, with no device behind it"""

    def __init__(self, *dims, ptr=0x1000):
        self.grid = ah.Grid.full(*dims)
        self.ptr = ptr


# ----------------------------------------------------------------------------- 1-3: the Python layer
@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_schemes_bind_ignition(scheme):
    F = SCHEMES[scheme].bind(ah.ignition_)
    assert isinstance(F, ah.DeviceResidual) and F.kind == ig.KINDS[scheme]
    assert F.kind == getattr(_lib, f"NK_IGNITION2D_{scheme.upper()}")
    assert F.kind == getattr(ah, f"ignition2d_{scheme}_").kind and F.alpha == 0.5
    assert f"ignition2d_{scheme}_" in ah.__all__ and "ignition_" in ah.__all__


def test_midpoint_carries_alpha_and_others_refuse_it():
    F = ah.G_Midpoint_(alpha=0.3).bind(ah.ignition_)
    assert F.kind == 21 and F.alpha == 0.3
    assert ah.ignition2d_midpoint_.with_alpha(0.3).alpha == 0.3
    with pytest.raises(ValueError):
        ah.ignition2d_euler_.with_alpha(0.3)
    with pytest.raises(NotImplementedError):  # any other f still has no fused residual
        ah.G_Euler_.bind(lambda du, u, p, t: None)


def test_header_and_ctypes_agree_on_the_kinds():
    hdr = open(_lib.HEADER).read()
    got = dict(re.findall(r"^#define (NK_IGNITION2D_\w+) (\d+)\b", hdr, re.M))
    assert got == {"NK_IGNITION2D_EULER": "20", "NK_IGNITION2D_MIDPOINT": "21", "NK_IGNITION2D_TRAPEZOID": "22"}
    kinds = re.findall(r"^#define (NK_(?:BRATU|HEAT|USER|IGNITION)\w+) (\d+)\b", hdr, re.M)
    assert len({v for _, v in kinds}) == len(kinds)  # no number is used twice


@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_problem_fills_the_struct(scheme):
    F = SCHEMES[scheme](alpha=0.3).bind(ah.ignition_) if scheme == "midpoint" else SCHEMES[scheme].bind(ah.ignition_)
    u, un = FakeArray(12, 10), FakeArray(12, 10, ptr=0x2000)
    p = F.problem(u, (un, 0.05, None, (1.5, 0.1, 0.2, 6.0, ah.bc_zero_), 0.0))
    assert (p.kind, p.bc, p.nx, p.ny, p.nz) == (ig.KINDS[scheme], _lib.NK_BC_ZERO, 12, 10, 1)
    assert (p.hx, p.hy) == (0.1, 0.2)
    assert (p.lam, p.a, p.dt) == (6.0, 1.5, 0.05)
    assert p.alpha == (0.3 if scheme == "midpoint" else 0.5)
    assert p.un == 0x2000 and not p.user


def test_problem_refuses_3d_and_other_boundaries():
    un2, un3 = FakeArray(12, 10), FakeArray(12, 10, 9)
    with pytest.raises(ValueError, match="2D grid"):
        ah.ignition2d_euler_.problem(FakeArray(12, 10, 9), (un3, 0.05, None, (1.0, 0.1, 0.1, 6.0, ah.bc_zero_), 0.0))
    for bc in (ah.bc_periodic_, None):
        with pytest.raises(NotImplementedError):
            ah.ignition2d_euler_.problem(FakeArray(12, 10), (un2, 0.05, None, (1.0, 0.1, 0.1, 6.0, bc), 0.0))
    with pytest.raises(ValueError, match="u_n"):  # u_n on another grid
        ah.ignition2d_euler_.problem(FakeArray(12, 10), (FakeArray(12, 9), 0.05, None, (1.0, 0.1, 0.1, 6.0, ah.bc_zero_), 0.0))


# ----------------------------------------------------------------------------- 4: the restatement against what is pinned
def _fields(shape, seed=3):
    rng = np.random.default_rng(seed)
    un = rng.standard_normal(shape)
    return un, un + 0.01 * rng.standard_normal(shape), rng.standard_normal(shape)


@pytest.mark.parametrize("scheme", ig.SCHEMES)
@pytest.mark.parametrize("alpha", [0.5, 0.3])
def test_lambda_zero_is_the_heat_restatement(scheme, alpha):
    """λ (exp ...) = 0 adds +0 to a L(w): residual and tangent are the oracle's heat kind's, bit for bit"""
    nx, ny = 13, 9
    un, u, v = _fields((ny, nx))
    P = ig.Problem(nx, ny, scheme, lam=0.0, a=0.7, dt=0.013, alpha=alpha, un=un)
    H = oc.heat2d_euler(nx, ny, a=0.7, dt=0.013, un=un, scheme=scheme, alpha=alpha)
    np.testing.assert_array_equal(ig.residual(P, u), oc.residual(H, u))
    np.testing.assert_array_equal(ig.jv_exact(P, u, v), oc.jv_exact(H, u, v))
    np.testing.assert_array_equal(ig.jacobian_diag(P, u), oc.jacobian_diag(H, u))


def test_euler_with_a_one_is_bratu_under_the_scheme():
    """a = 1: 1 L(u) = L(u), so F = (u_n + Δt (Bratu 2D residual of u)) - u with the oracle's Bratu residual"""
    nx, ny = 13, 9
    un, u, _v = _fields((ny, nx))
    P = ig.Problem(nx, ny, "euler", lam=6.0, a=1.0, dt=0.05, un=un)
    B = oc.bratu2d(nx, ny, lam=6.0)
    np.testing.assert_array_equal(ig.residual(P, u), (un + 0.05 * oc.residual(B, u)) - u)


@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_tangent_matches_its_own_fd_and_matrix(scheme):
    nx, ny = 11, 7
    un, u, v = _fields((ny, nx))
    P = ig.Problem(nx, ny, scheme, lam=6.0, a=1.0, dt=0.05, alpha=0.3, un=un, h=(0.11, 0.13))
    jv = ig.jv_exact(P, u, v)
    fd = ig.jv_fd(P, u, v, ig.residual(P, u), 2.0 ** -26)
    # the FD's accuracy: truncation eps |F''| |v|^2 / 2 plus rounding 2^-53 |F| / eps, both far below 1e-5 |Jv| here
    assert np.max(np.abs(fd - jv)) <= 1e-5 * np.max(np.abs(jv))
    A = ig.jacobian(P, u)
    assert abs(A - A.T).max() == 0.0
    np.testing.assert_array_equal(A.diagonal(), ig.jacobian_diag(P, u).reshape(-1))
    assert np.max(np.abs(A @ v.reshape(-1) - jv.reshape(-1))) <= 1e-12 * np.max(np.abs(jv))
    e = np.zeros(P.n)
    for i in (0, 17, P.n - 1):  # a column of the assembled matrix is the exact tangent of a unit vector, bit for bit
        e[:] = 0.0
        e[i] = 1.0
        np.testing.assert_array_equal(A[:, i].toarray().reshape(-1), ig.jv_exact(P, u, e.reshape(P.shape)).reshape(-1))


# ----------------------------------------------------------------------------- 5: the physics
N, DT_SUB, DT_SUP, LAM_SUP = 15, 0.05, 0.02, 10.0


@pytest.fixture(scope="module")
def subcritical():
    P = ig.Problem(N, N, "euler", lam=ig.LAM, a=1.0, dt=DT_SUB)
    return P, ig.time_steps(P, 40)


def test_subcritical_euler_is_nonlinear_then_steady(subcritical):
    P, (states, newton, solved) = subcritical
    print("Newton steps per time step:", newton)
    assert newton[0] > 1 and all(solved)  # a nonlinear step: Newton does not finish in one
    assert 0 in newton
    k = newton.index(0)
    B = oc.bratu2d(N, N, lam=ig.LAM)
    # the step's initial residual is Δt f(u_n) <= tol = 1e-6 ||F|| + 6e-6, i.e. ||Bratu F(u)|| <= 6e-6 / (Δt (1 - 1e-6))
    nf = float(np.linalg.norm(oc.residual(B, states[k])))
    print(f"first 0-step time step: index {k}, ||Bratu F|| = {nf:.3e}")
    assert nf <= ig.TOL_ABS / (DT_SUB * (1.0 - 1e-6))


@pytest.mark.parametrize("scheme", ig.SCHEMES)
def test_supercritical_blows_up(scheme):
    P = ig.Problem(N, N, scheme, lam=LAM_SUP, a=1.0, dt=DT_SUP)
    _states, newton, solved = ig.time_steps(P, 25)
    print(scheme, "Newton steps:", newton, "first unsolved:", solved.index(False) if False in solved else None)
    assert False in solved


# ----------------------------------------------------------------------------- the launch plan's trait
def test_plan_header_has_no_f0r_for_the_kinds():
    """csrc/nk_kind.hpp's kind_of(k).f0r (host code; the launcher's question before it plans): false for 20 .. 22 -- no
    F0R instantiation exists, the launcher clears the request and the FD launch reads F0 -- and true for every other
    built-in stencil kind"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = ["-I", os.path.join(root, "newtonkrylov.jl_amd", "csrc"), "-I", os.path.join(root, "include")]
    src = ('#include <cstdio>\n#include "nk_kind.hpp"\n'
           'int main() { for (int k : nk::kStencilKinds) std::printf("%d:%d ", k, nk::kind_of(k).f0r ? 1 : 0); }\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as fh:
            fh.write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *inc, "-o", os.path.join(d, "t"), os.path.join(d, "t.cpp")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout
    assert out.split() == [f"{k}:1" for k in range(1, 10)] + ["20:0", "21:0", "22:0"]
