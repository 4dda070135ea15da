"""The numpy restatement of 3D Bratu (NK_BRATU3D) the bratu3d tests share -- not a test module.

Grid nx x ny x nz, x fastest (arrays have shape (nz, ny, nx)), zero Dirichlet ghosts, p = (hx, hy, hz, lam).
With l_a(w) = ((w+ - 2 w) + w-) / (h_a h_a):

    F(u)      = ((l_x(u) + l_y(u)) + l_z(u)) + lam exp(u)
    J(u) v    = ((l_x(v) + l_y(v)) + l_z(v)) + lam (exp(u) v)          (the exact tangent)
    FD        = (F(u + eps v) - F0) / eps, w = u + eps v formed with one multiplication and one addition

in exactly this association, nothing fused, with exp = oracle.exp (the library's correctly rounded nk_exp): the
device kernels compute the same doubles, so every pointwise comparison against it is np.array_equal.
"""
import math

import numpy as np

import _nkpath  # noqa: F401
from oracle import oracle as oc

LAM = 3.51382


class Problem:
    def __init__(self, nx, ny, nz, lam=LAM, h=None):
        self.nx, self.ny, self.nz, self.lam = nx, ny, nz, float(lam)
        self.hx, self.hy, self.hz = h if h is not None else (1.0 / (nx + 1), 1.0 / (ny + 1), 1.0 / (nz + 1))
        self.shape = (nz, ny, nx)
        self.n = nx * ny * nz

    @property
    def p(self):
        return (self.hx, self.hy, self.hz, self.lam)


def sin_ic(P):
    x = np.sin(np.pi * np.arange(1, P.nx + 1) * P.hx)
    y = np.sin(np.pi * np.arange(1, P.ny + 1) * P.hy)
    z = np.sin(np.pi * np.arange(1, P.nz + 1) * P.hz)
    return np.ascontiguousarray(z[:, None, None] * y[None, :, None] * x[None, None, :])


def lap(P, w):
    """((l_x + l_y) + l_z) of w with zero ghosts"""
    q = np.pad(w, 1)
    c = q[1:-1, 1:-1, 1:-1]
    with np.errstate(all="ignore"):
        lx = ((q[1:-1, 1:-1, 2:] - 2.0 * c) + q[1:-1, 1:-1, :-2]) / (P.hx * P.hx)
        ly = ((q[1:-1, 2:, 1:-1] - 2.0 * c) + q[1:-1, :-2, 1:-1]) / (P.hy * P.hy)
        lz = ((q[2:, 1:-1, 1:-1] - 2.0 * c) + q[:-2, 1:-1, 1:-1]) / (P.hz * P.hz)
        return (lx + ly) + lz


def residual(P, u, e=None):
    """F(u); e: a stand-in for exp(u) (the one-ulp sensitivity checks)"""
    with np.errstate(all="ignore"):
        return lap(P, u) + P.lam * (oc.exp(u) if e is None else e)


def jv_exact(P, u, v):
    with np.errstate(all="ignore"):
        return lap(P, v) + P.lam * (oc.exp(u) * v)


def jv_fd(P, u, v, F0, eps):
    with np.errstate(all="ignore"):
        return (residual(P, u + eps * v) - F0) / eps


def jacobian_diag(P, u, reciprocal=False):
    """the exact tangent of the unit vector at its own point: ((0 - 2 1) + 0) / h_a^2 summed (x + y) + z, + lam (exp(u) 1)"""
    dx = ((0.0 - 2.0 * 1.0) + 0.0) / (P.hx * P.hx)
    dy = ((0.0 - 2.0 * 1.0) + 0.0) / (P.hy * P.hy)
    dz = ((0.0 - 2.0 * 1.0) + 0.0) / (P.hz * P.hz)
    with np.errstate(all="ignore"):
        d = ((dx + dy) + dz) + P.lam * (oc.exp(u) * 1.0)
        return 1.0 / d if reciprocal else d


def offdiag(h):
    """J's entry towards a neighbour along an axis of spacing h: ((1 - 2 0) + 0) / h^2 (the other terms add +0)"""
    return ((1.0 - 2.0 * 0.0) + 0.0) / (h * h)


def jacobian(P, u):
    """J(u) as a scipy CSC matrix, rows / columns in memory order (x fastest): the entries of the restatement"""
    import scipy.sparse as sp

    def d2(n, c):
        return sp.diags([np.full(n - 1, c), np.full(n - 1, c)], [-1, 1], shape=(n, n)) if n > 1 else sp.csr_matrix((1, 1))

    ix, iy, iz = sp.identity(P.nx), sp.identity(P.ny), sp.identity(P.nz)
    off = (sp.kron(iz, sp.kron(iy, d2(P.nx, offdiag(P.hx)))) + sp.kron(iz, sp.kron(d2(P.ny, offdiag(P.hy)), ix)) +
           sp.kron(d2(P.nz, offdiag(P.hz)), sp.kron(iy, ix)))
    return (off + sp.diags(jacobian_diag(P, u).reshape(-1))).tocsc()


def newton_lu(P, u0, rtol=1e-10, max_steps=20):
    """exact Newton with a sparse LU of J: (u, steps, ||F|| history); stops at ||F|| <= rtol ||F(u0)||"""
    import scipy.sparse.linalg as spla

    u = u0.copy()
    hist = [float(np.linalg.norm(residual(P, u)))]
    steps = 0
    while hist[-1] > rtol * hist[0] and steps < max_steps:
        d = spla.splu(jacobian(P, u)).solve(residual(P, u).reshape(-1))
        u = u - d.reshape(P.shape)
        hist.append(float(np.linalg.norm(residual(P, u))))
        steps += 1
    return u, steps, hist


def eig_nearest_zero(P, u):
    """the eigenvalue of the symmetric J(u) nearest 0 (shift-invert Lanczos about 0)"""
    import scipy.sparse.linalg as spla

    return float(spla.eigsh(jacobian(P, u), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])


def ilu0_factor(P, u):
    """the ILU(0) pivots of J(u) in natural order, the recurrence documented at csrc/nk_precond.hip:
    D~_i = ((a_ii - (c_z / D~_b) c_z) - (c_y / D~_s) c_y) - (c_x / D~_w) c_x, lower neighbours below, south, west"""
    a = jacobian_diag(P, u)
    cx, cy, cz = offdiag(P.hx), offdiag(P.hy), offdiag(P.hz)
    d = np.zeros(P.shape)
    for k in range(P.nz):
        for j in range(P.ny):
            for i in range(P.nx):
                t = a[k, j, i]
                if k > 0:
                    t = t - (cz / d[k - 1, j, i]) * cz
                if j > 0:
                    t = t - (cy / d[k, j - 1, i]) * cy
                if i > 0:
                    t = t - (cx / d[k, j, i - 1]) * cx
                d[k, j, i] = t
    return d


def reduction_bound(terms):
    """(fsum, bound): a sum of n doubles in any order, fused or not, lies within n 2^-53 sum|terms| of the exact
    sum (first-order error of recursive summation; tests/test_hip_multigrid_cg.py uses the same bound for <v, z>)"""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    return math.fsum(t), t.size * 2.0 ** -53 * math.fsum(np.abs(t))
