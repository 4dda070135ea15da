"""The numpy restatement of the 2D ignition kinds (NK_IGNITION2D_EULER / _MIDPOINT / _TRAPEZOID) the ignition tests
share -- not a test module.

u_t = a Δu + λ exp(u) under the implicit schemes of examples/implicit.jl.  Grid nx x ny, x fastest (arrays have shape
(ny, nx)), zero Dirichlet ghosts.  With l_a(w) = ((w+ - 2 w) + w-) / (h_a h_a), L(w) = l_x(w) + l_y(w) and
f(w) = a L(w) + λ exp(w):

    Euler      F(u) = (u_n + Δt f(u)) - u                       J v = Δt (a L(v) + λ (exp(u) v)) - v
    Midpoint   F(u) = (u_n + Δt f(m)) - u, m = α u_n + (1-α) u   J v = Δt (a L(c) + λ (exp(m) c)) - v, c = (1-α) v
    Trapezoid  F(u) = (u_n + (Δt/2) (f(u_n) + f(u))) - u         J v = (Δt/2) (a L(v) + λ (exp(u) v)) - v
    FD         (F(u + eps v) - F0) / eps, w = u + eps v formed with one multiplication and one addition

in exactly this association, nothing fused, with exp = oracle.exp (the library's correctly rounded nk_exp): the device
kernels compute the same doubles, so every pointwise comparison against it is np.array_equal.
"""
import math

import numpy as np

import _nkpath  # noqa: F401
from oracle import oracle as oc

SCHEMES = ("euler", "midpoint", "trapezoid")
KINDS = {"euler": 20, "midpoint": 21, "trapezoid": 22}
LAM = 3.51382  # below the fold of the unit square (about 6.8)
TOL_ABS = 6.0e-6  # implicit.jl:61


class Problem:
    def __init__(self, nx, ny, scheme="euler", lam=LAM, a=1.0, dt=0.05, alpha=0.5, un=None, h=None):
        assert scheme in SCHEMES
        self.nx, self.ny, self.scheme = nx, ny, scheme
        self.lam, self.a, self.dt, self.alpha = float(lam), float(a), float(dt), float(alpha)
        self.hx, self.hy = h if h is not None else (1.0 / (nx + 1), 1.0 / (ny + 1))
        self.shape = (ny, nx)
        self.n = nx * ny
        self.un = np.zeros(self.shape) if un is None else np.ascontiguousarray(un, dtype=np.float64)

    @property
    def kind(self):
        return KINDS[self.scheme]

    @property
    def fp(self):
        """the tuple p of f: (a, Δx, Δy, λ) -- the boundary marker is appended by the caller"""
        return (self.a, self.hx, self.hy, self.lam)

    @property
    def tdt(self):
        """the scheme's step factor as the kernels form it: Δt, or Δt / 2 for Trapezoid"""
        return self.dt / 2.0 if self.scheme == "trapezoid" else self.dt

    def with_un(self, un):
        return Problem(self.nx, self.ny, self.scheme, self.lam, self.a, self.dt, self.alpha, un, (self.hx, self.hy))


def lap(P, w):
    """L(w) = l_x(w) + l_y(w) with zero ghosts"""
    q = np.pad(w, 1)
    c = q[1:-1, 1:-1]
    with np.errstate(all="ignore"):
        lx = ((q[1:-1, 2:] - 2.0 * c) + q[1:-1, :-2]) / (P.hx * P.hx)
        ly = ((q[2:, 1:-1] - 2.0 * c) + q[:-2, 1:-1]) / (P.hy * P.hy)
        return lx + ly


def f(P, w):
    with np.errstate(all="ignore"):
        return P.a * lap(P, w) + P.lam * oc.exp(w)


def mid(P, u):
    """the argument the scheme's exp (and Laplacian) takes: G_Midpoint!'s α u_n + (1 - α) u, else u"""
    if P.scheme != "midpoint":
        return u
    with np.errstate(all="ignore"):
        return P.alpha * P.un + (1.0 - P.alpha) * u


def residual(P, u):
    with np.errstate(all="ignore"):
        if P.scheme == "trapezoid":
            return (P.un + (P.dt / 2.0) * (f(P, P.un) + f(P, u))) - u
        return (P.un + P.dt * f(P, mid(P, u))) - u


def jv_exact(P, u, v):
    with np.errstate(all="ignore"):
        c = (1.0 - P.alpha) * v if P.scheme == "midpoint" else v
        return P.tdt * (P.a * lap(P, c) + P.lam * (oc.exp(mid(P, u)) * c)) - v


def jv_fd(P, u, v, F0, eps):
    with np.errstate(all="ignore"):
        return (residual(P, u + eps * v) - F0) / eps


def fd_eps(u, v):
    """the library's step rule for eps <= 0 (the oracle's oc_fd_eps on the two norms)"""
    return oc.fd_eps(oc.norm(u), oc.norm(v))


def jacobian_diag(P, u, reciprocal=False):
    """the exact tangent of the unit vector at its own point: the field's centre c = 1 ((1 - α) 1 for Midpoint), every
    neighbour 0, the "- v" term 1"""
    c = (1.0 - P.alpha) * 1.0 if P.scheme == "midpoint" else 1.0
    lsum = ((0.0 - 2.0 * c) + 0.0) / (P.hx * P.hx) + ((0.0 - 2.0 * c) + 0.0) / (P.hy * P.hy)
    with np.errstate(all="ignore"):
        d = P.tdt * (P.a * lsum + P.lam * (oc.exp(mid(P, u)) * c)) - 1.0
        return 1.0 / d if reciprocal else d


def offdiag(P, h):
    """J's entry towards a neighbour along an axis of spacing h: the heat kind's value, the exp term adding +0"""
    fv = (1.0 - P.alpha) * 1.0 if P.scheme == "midpoint" else 1.0
    lsum = ((fv - 2.0 * 0.0) + 0.0) / (h * h)
    return P.tdt * (P.a * lsum) - 0.0


def jacobian(P, u):
    """J(u) as a scipy CSC matrix, rows / columns in memory order (x fastest): the entries of the restatement"""
    import scipy.sparse as sp

    def d2(n, c):
        return sp.diags([np.full(n - 1, c), np.full(n - 1, c)], [-1, 1], shape=(n, n)) if n > 1 else sp.csr_matrix((1, 1))

    ix, iy = sp.identity(P.nx), sp.identity(P.ny)
    off = sp.kron(iy, d2(P.nx, offdiag(P, P.hx))) + sp.kron(d2(P.ny, offdiag(P, P.hy)), ix)
    return (off + sp.diags(jacobian_diag(P, u).reshape(-1))).tocsc()


def ilu0_factor(P, u):
    """the ILU(0) pivots of J(u) in natural order: bratu3d_ref.ilu0_factor's recurrence in 2D,
    D~_i = (a_ii - (c_y / D~_s) c_y) - (c_x / D~_w) c_x"""
    a = jacobian_diag(P, u)
    cx, cy = offdiag(P, P.hx), offdiag(P, P.hy)
    d = np.zeros(P.shape)
    for j in range(P.ny):
        for i in range(P.nx):
            t = a[j, i]
            if j > 0:
                t = t - (cy / d[j - 1, i]) * cy
            if i > 0:
                t = t - (cx / d[j, i - 1]) * cx
            d[j, i] = t
    return d


def newton_lu(P, u0, tol_rel=1e-6, tol_abs=TOL_ABS, max_niter=50):
    """exact Newton with a sparse LU of J under newton_krylov!'s stopping rule (tol = tol_rel ||F(u0)|| + tol_abs, the
    loop runs while ||F|| > tol and steps <= max_niter): (u, steps, solved, ||F|| history).  A non-finite ||F|| ends the
    loop unsolved, as the comparison does in the library."""
    import scipy.sparse.linalg as spla

    u = u0.copy()
    hist = [float(np.linalg.norm(residual(P, u)))]
    tol = tol_rel * hist[0] + tol_abs
    steps = 0
    while hist[-1] > tol and steps <= max_niter:
        try:
            with np.errstate(all="ignore"):
                d = spla.splu(jacobian(P, u)).solve(residual(P, u).reshape(-1))
        except (RuntimeError, ValueError):  # a singular or non-finite J: the step is not solved
            hist.append(float("nan"))
            break
        u = u - d.reshape(P.shape)
        hist.append(float(np.linalg.norm(residual(P, u))))
        steps += 1
    return u, steps, bool(hist[-1] <= tol), hist


def time_steps(P, nsteps, u0=None):
    """the time loop of implicit.jl:54-78 with newton_lu, marching on: (states after each step, Newton steps per step,
    solved per step)"""
    un = P.un.copy() if u0 is None else u0.copy()
    states, newton, solved = [], [], []
    for _ in range(nsteps):
        u, k, ok, _h = newton_lu(P.with_un(un), un)
        states.append(u)
        newton.append(k)
        solved.append(ok)
        un = u.copy()
    return states, newton, solved


def eig_nearest_zero(P, u):
    """the eigenvalue of the symmetric J(u) nearest 0 (shift-invert Lanczos about 0)"""
    import scipy.sparse.linalg as spla

    return float(spla.eigsh(jacobian(P, u), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])


def reduction_bound(terms):
    """(fsum, bound): a sum of n doubles in any order, fused or not, lies within n 2^-53 sum|terms| of the exact
    sum (first-order error of recursive summation; bratu3d_ref.reduction_bound)"""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    return math.fsum(t), t.size * 2.0 ** -53 * math.fsum(np.abs(t))
