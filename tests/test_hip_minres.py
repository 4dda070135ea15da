"""MINRES (algo = :minres) for the symmetric stencil Jacobians.

The file carries the Paige-Saunders recurrence the device runs as a numpy restatement, evaluated in float64 and in
np.longdouble.  The float64-against-long-double difference of the restatement on a case is that case's sensitivity;
the sensitivities are recorded below, and the device's iterates are held within 16 x of them (the multigrid tests'
convention: the margin covers the device's other summation trees).

CPU tests: the constant in header / ctypes / shim, the rejections, the restatement against scipy's minres at fixed k
and the recorded sensitivities.  GPU tests: fixed k against the restatement and scipy, MINRES against the device's own
unrestarted GMRES, convergence counts, the FD operator, M = -1 ./ diag(J) and its breakdown with the wrong sign,
M = multigrid(spd=True), reductions across blocks, determinism, Newton-MINRES in the three drivers and in solve(),
and two ranks over both mailboxes.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import _nkpath  # noqa: F401
import ariadne_hip as ah
from ariadne_hip import _lib
from oracle import oracle as oc

from test_hip_multigrid import ROOT, Cycle, device_operator, host_problem

LAM = 3.51382
# (shape (nx, ny), λ, u): A and B definite at sin_ic; C indefinite (61 positive eigenvalues), diag(J) <= -1144
CASES = {"A": ((24, 20), LAM, "sin"), "B": ((37, 23), LAM, "sin"), "C": ((24, 20), 600.0, "uniform"),
         "1D7": ((7,), LAM, "sin")}  # (and 1D with N = 7: less than one wave; at sin_ic its Krylov space has 4 dimensions)
BIG = (300, 257)  # n = 77100: the reduction grid has 38 blocks (one per 2048 points) and a ragged last chunk

# Sensitivities: max|x64 - xld| / max|xld| (and the same for the history) of the restatement, float64 against long
# double, at the fixed k of the tests (test_sensitivities_are_as_recorded measures them again and holds them within
# 1.5 x).  Keys: (case, M, k); M "" = none, "jac" = -1 ./ diag(J).
SENS_X = {("A", "", 10): 1.7e-15, ("A", "", 40): 2.7e-15, ("B", "", 10): 1.1e-15, ("B", "", 40): 5.5e-15,
          ("C", "", 10): 5.1e-16, ("C", "", 40): 1.6e-14, ("A", "jac", 40): 2.2e-15, ("C", "jac", 40): 5.7e-15,
          ("A", "", 20): 2.6e-15, ("1D7", "", 4): 1.2e-14}
SENS_H = {("A", "", 10): 5.3e-16, ("A", "", 40): 5.7e-16, ("B", "", 10): 8.2e-16, ("B", "", 40): 1.4e-15,
          ("C", "", 10): 1.4e-16, ("C", "", 40): 1.4e-16, ("A", "jac", 40): 1.6e-16, ("C", "jac", 40): 1.5e-16,
          ("A", "", 20): 5.7e-16, ("1D7", "", 4): 1.1e-15}
SENS_BIG = (3.7e-15, 1.2e-16)  # 300 x 257 at k = 10: x, history
# numpy MINRES against numpy unrestarted GMRES on A at k = 40: max|x_m - x_g| / max|x| and the same for the history
MINRES_VS_GMRES_X = 2.8e-15
MINRES_VS_GMRES_H = 6.6e-16
# ||x_fd - x_exact|| / ||x|| of the restatement pair (library's eps rule) at rtol = 1e-6, cases A and B
FD_VS_EXACT = {"A": 3.1e-8, "B": 1.5e-8}
# restatement counts: rtol = 1e-6 on A, B (exact and FD Jv alike); M = -1 ./ diag(J) on A at rtol = 1e-8; M = -V (the
# SPD V-cycle) on Bratu 72 x 56 at rtol = 1e-8 (CG with the same M: 7).  The indefinite case C takes the restatement
# 409 iterations to 0.98 rtol of true residual; its count moves with the summation order and is not asserted
COUNTS = {"A": 43, "B": 61}
COUNT_JAC_A = 51
COUNT_JAC_A_FD = 52  # the same with the FD operator: at rtol = 1e-8 the difference quotient's error costs one step
COUNT_MG = 8
MAXIT = "maximum number of iterations exceeded"
GOOD = "solution good enough given atol and rtol"


# ------------------------------------------------------------------------------------ the restatement
def minres_ref(A, b, M=None, itmax=0, atol=0.0, rtol=0.0, dt=np.float64, trace=None):
    """The recurrence of DESIGN.md §11 in dtype dt.  A: a matrix or a callable on flat vectors; M: a callable (SPD) or
    None.  Returns (x, history, niter, status) with status 1 solved, 2 itmax, 3 breakdown.  `trace` (a list) receives
    every completed step's rotation scalars (alpha, g = <r2, y>, oldeps, delta, gamma, phi)."""
    mul = A if callable(A) else (lambda q: A @ q)
    b = np.asarray(b, dtype=dt).reshape(-1)
    n = b.size
    sqrt = np.sqrt
    x, r1 = np.zeros(n, dtype=dt), b.copy()
    y = r1 if M is None else np.asarray(M(r1), dtype=dt)
    g = r1 @ y
    if g < 0:
        return x, [float("nan")], 0, 3
    beta1 = sqrt(g)
    hist = [beta1]
    if beta1 == 0:
        return x, hist, 0, 1
    zero, eps = dt(0), dt(np.finfo(np.float64).eps)
    oldb, beta, dbar, epsl, phibar, cs, sn = zero, beta1, zero, zero, beta1, dt(-1), zero
    w, w2, r2 = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt), r1
    tol = dt(atol) + dt(rtol) * beta1
    itmax = itmax or 2 * n
    it, status = 0, 0
    while not (phibar <= tol or it >= itmax):
        it += 1
        v = y / beta
        jv = np.asarray(mul(v), dtype=dt)
        alpha = v @ jv
        t = jv - (beta / oldb) * r1 if it >= 2 else jv
        t = t - (alpha / beta) * r2
        r1, r2 = r2, t
        y = r2 if M is None else np.asarray(M(r2), dtype=dt)
        g = r2 @ y
        if g < 0:
            it -= 1
            status = 3
            break
        oldb, beta = beta, sqrt(g)
        oldeps = epsl
        delta = cs * dbar + sn * alpha
        gbar = sn * dbar - cs * alpha
        epsl = sn * beta
        dbar = -cs * beta
        gamma = max(sqrt(gbar * gbar + beta * beta), eps)
        cs, sn = gbar / gamma, beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        if trace is not None:
            trace.append((alpha, g, oldeps, delta, gamma, phi))
        w1, w2 = w2, w
        w = ((v - oldeps * w1) - delta * w2) / gamma
        x = x + phi * w
        hist.append(phibar)
    if status == 0:
        status = 1 if phibar <= tol else 2
    return x, hist, it, status


def gmres_ref(A, b, k):
    """k steps of unrestarted GMRES (x0 = 0, MGS, Givens): (x, the residual estimates)"""
    b = b.reshape(-1)
    beta = np.linalg.norm(b)
    V, H, g = [b / beta], np.zeros((k + 1, k)), np.zeros(k + 1)
    g[0] = beta
    cs, sn, hist = np.zeros(k), np.zeros(k), [beta]
    for j in range(k):
        w = A @ V[j]
        for i in range(j + 1):
            H[i, j] = V[i] @ w
            w = w - H[i, j] * V[i]
        H[j + 1, j] = np.linalg.norm(w)
        V.append(w / H[j + 1, j])
        for i in range(j):
            H[i, j], H[i + 1, j] = cs[i] * H[i, j] + sn[i] * H[i + 1, j], -sn[i] * H[i, j] + cs[i] * H[i + 1, j]
        rho = np.hypot(H[j, j], H[j + 1, j])
        cs[j], sn[j] = H[j, j] / rho, H[j + 1, j] / rho
        H[j, j], H[j + 1, j] = rho, 0.0
        g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
        hist.append(abs(g[j + 1]))
    yk = np.linalg.solve(np.triu(H[:k, :k]), g[:k])
    return sum(yk[i] * V[i] for i in range(k)), hist


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


_HOST = {}


def host_case(name):
    """(oracle problem, u, b = F(u), dense J from the oracle's exact Jv on the unit vectors), once"""
    if name not in _HOST:
        shape, lam, ukind = CASES[name]
        P = oc.bratu2d(*shape, lam=lam) if len(shape) == 2 else oc.bratu1d(*shape, lam=lam)
        u = oc.sin_ic(P) if ukind == "sin" else 0.5 * np.random.default_rng(0).uniform(size=P.shape)
        n = P.n
        J = np.empty((n, n))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            J[:, j] = oc.jv_exact(P, u, e.reshape(P.shape)).reshape(-1)
            e[j] = 0.0
        _HOST[name] = (P, u, oc.residual(P, u), J)
    return _HOST[name]


def stencil_coefficients(P, u):
    """the five coefficient arrays (centre, E, N, S, W) of the 2D Jacobian from five coloured probes of the oracle's
    exact Jv: with the colour (i + 2 j) mod 5 the five points of every row's stencil have five different colours"""
    ny, nx = P.shape
    colour = (np.arange(nx)[None, :] + 2 * np.arange(ny)[:, None]) % 5
    outs = [oc.jv_exact(P, u, (colour == c).astype(np.float64)) for c in range(5)]
    return [np.choose((colour + off) % 5, outs) for off in range(5)]  # off 0 centre, 1 E, 2 N, 3 S, 4 W


def stencil_mul(coef, v):
    """J v from the coefficient arrays, in v's dtype (v flat)"""
    c = [a.astype(v.dtype) for a in coef]
    q = v.reshape(coef[0].shape)
    out = c[0] * q
    out[:, :-1] += c[1][:, :-1] * q[:, 1:]
    out[:-1, :] += c[2][:-1, :] * q[1:, :]
    out[1:, :] += c[3][1:, :] * q[:-1, :]
    out[:, 1:] += c[4][:, 1:] * q[:, :-1]
    return out.reshape(-1)


def big_host():
    if "BIG" not in _HOST:
        P = oc.bratu2d(*BIG)
        u = oc.sin_ic(P)
        _HOST["BIG"] = (P, u, oc.residual(P, u), stencil_coefficients(P, u))
    return _HOST["BIG"]


def jac_M(J, sign=-1.0, dt=np.float64):
    d = (dt(sign) / np.diag(J).astype(dt))
    return lambda r: d * r


_RUNS = {}


def ref_run(name, M, k, dt=np.float64, A=None, b=None):
    """the restatement at fixed k on a host case (cached per dtype)"""
    key = (name, M, k, dt)
    if key not in _RUNS:
        _, _, bb, J = host_case(name)
        Jd = (J if A is None else A).astype(dt)
        _RUNS[key] = minres_ref(Jd, bb if b is None else b, jac_M(Jd, dt=dt) if M == "jac" else None, itmax=k, dt=dt)
    return _RUNS[key]


def sensitivity(name, M, k):
    x64, h64, _, _ = ref_run(name, M, k)
    xld, hld, _, _ = ref_run(name, M, k, np.longdouble)
    return relmax(x64, xld), relmax(h64, hld)


def fd_operator(P, u, F0):
    return lambda v: oc.jv_fd(P, u, np.asarray(v, dtype=np.float64).reshape(P.shape), F0).reshape(-1)


# ------------------------------------------------------------------------------------ CPU tests
def test_constant_agrees_in_header_ctypes_and_shim():
    hdr = open(_lib.HEADER).read()
    shim = open(os.path.join(ROOT, "newtonkrylov.jl_amd", "julia", "AriadneHIP.jl")).read()
    val = int(re.search(r"^#define NK_ALGO_MINRES (\d+)", hdr, re.M).group(1))
    assert val == _lib.NK_ALGO_MINRES == 3
    names = re.search(r"^const (NK_ALGO_GMRES.*?) = (.*)$", shim, re.M)
    consts = dict(zip([s.strip() for s in names.group(1).split(",")], re.findall(r"Int32\((\d+)\)", names.group(2))))
    assert int(consts["NK_ALGO_MINRES"]) == val
    assert re.search(r"method === :minres \? NK_ALGO_MINRES", shim)
    from ariadne_hip import krylov
    assert krylov._ALGOS["minres"] == val


def test_rejections_need_no_device():
    ws = types.SimpleNamespace(algo="minres")
    mg = ah.MultigridPreconditioner.__new__(ah.MultigridPreconditioner)  # default form
    with pytest.raises(NotImplementedError, match="spd=True"):
        ah.krylov_solve_(ws, None, None, M=mg)
    jac = ah.DiagonalPreconditioner.__new__(ah.DiagonalPreconditioner)
    with pytest.raises(TypeError, match="M"):
        ah.krylov_solve_(ws, None, None, N=jac)
    for kw in (dict(restart=True), dict(reorthogonalization=True)):
        with pytest.raises(TypeError, match="GMRES keywords"):
            ah.krylov_solve_(ws, None, None, **kw)
    g2 = ah.Grid.full(16, 12)
    arr = lambda: ah.DeviceArray(g2, types.SimpleNamespace(nranks=1, handle=None), _ptr=8)  # noqa: E731
    with pytest.raises(NotImplementedError, match="spd=True"):
        ah.newton_krylov_native(ah.bratu2d_, arr(), (0.1, 0.1, 3.5), res=arr(), algo="minres", M=mg)
    with pytest.raises(TypeError, match="M"):
        ah.newton_krylov_native(ah.bratu2d_, arr(), (0.1, 0.1, 3.5), res=arr(), algo="minres", N=mg)
    with pytest.raises(TypeError, match="GMRES keywords"):
        ah.newton_krylov_native(ah.bratu2d_, arr(), (0.1, 0.1, 3.5), res=arr(), algo="minres",
                                krylov_kwargs=dict(restart=True))
    kc = ah.KrylovConstructor.__new__(ah.KrylovConstructor)
    with pytest.raises(NotImplementedError, match=":minres"):
        ah.krylov.KrylovWorkspace("qmr", kc)
    with pytest.raises(NotImplementedError):
        ah.krylov.KrylovWorkspace("bicgstab", kc)


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("k", [10, 40])
def test_restatement_matches_scipy(name, k):
    _, _, b, J = host_case(name)
    x, hist, it, status = ref_run(name, "", k)
    xs, _ = spla.minres(J, b.reshape(-1), maxiter=k, rtol=1e-300)
    err = relmax(x, xs)
    print(f"{name} k={k}: restatement vs scipy {err:.2e} (allowed {16 * SENS_X[name, '', k]:.2e})")
    assert it == k and status == 2 and len(hist) == k + 1
    assert err <= 16 * SENS_X[name, "", k]


def test_case_c_is_indefinite_with_a_negative_diagonal():
    _, _, _, J = host_case("C")
    assert np.max(np.abs(J - J.T)) == 0.0
    w = np.linalg.eigvalsh(J)
    assert int(np.sum(w > 0)) == 61 and np.max(np.diag(J)) <= -1144.0  # so -1 ./ diag(J) is SPD
    _, _, _, JA = host_case("A")
    assert np.linalg.eigvalsh(JA)[-1] < 0.0


def test_sensitivities_are_as_recorded():
    for (name, M, k), want in SENS_X.items():
        sx, sh = sensitivity(name, M, k)
        print(f"sensitivity {name} M={M or 'none'} k={k}: x {sx:.3e} (recorded {want:.3e}), history {sh:.3e} "
              f"(recorded {SENS_H[name, M, k]:.3e})")
        assert want / 1.5 <= sx <= 1.5 * want and SENS_H[name, M, k] / 1.5 <= sh <= 1.5 * SENS_H[name, M, k]
    _, _, b, coef = big_host()
    x64, h64, _, _ = minres_ref(lambda q: stencil_mul(coef, q), b, itmax=10)
    xld, hld, _, _ = minres_ref(lambda q: stencil_mul(coef, q), b, itmax=10, dt=np.longdouble)
    sx, sh = relmax(x64, xld), relmax(h64, hld)
    print(f"sensitivity 300 x 257 k=10: x {sx:.3e}, history {sh:.3e} (recorded {SENS_BIG})")
    assert SENS_BIG[0] / 1.5 <= sx <= 1.5 * SENS_BIG[0] and SENS_BIG[1] / 1.5 <= sh <= 1.5 * SENS_BIG[1]
    _, _, b, J = host_case("A")
    xm, hm, _, _ = ref_run("A", "", 40)
    xg, hg = gmres_ref(J, b, 40)
    dx, dh = relmax(xm, xg), relmax(hm, hg)
    print(f"numpy MINRES vs numpy GMRES on A, k = 40: x {dx:.3e}, history {dh:.3e}")
    assert MINRES_VS_GMRES_X / 1.5 <= dx <= 1.5 * MINRES_VS_GMRES_X
    assert MINRES_VS_GMRES_H / 1.5 <= dh <= 1.5 * MINRES_VS_GMRES_H


def test_restatement_counts():
    for name in ("A", "B"):
        P, u, b, J = host_case(name)
        x, _, it, status = minres_ref(J, b, rtol=1e-6)
        xf, _, itf, stf = minres_ref(fd_operator(P, u, b), b, rtol=1e-6)
        d = float(np.linalg.norm(xf - x) / np.linalg.norm(x))
        print(f"{name}: exact {it}, FD {itf}, ||x_fd - x|| / ||x|| {d:.3e}")
        assert status == stf == 1 and it == itf == COUNTS[name]
        assert FD_VS_EXACT[name] / 1.5 <= d <= 1.5 * FD_VS_EXACT[name]
    _, _, b, J = host_case("A")
    assert minres_ref(J, b, jac_M(J), rtol=1e-8)[2:] == (COUNT_JAC_A, 1)
    P, u, _, _ = host_case("A")
    assert minres_ref(fd_operator(P, u, b), b, jac_M(J), rtol=1e-8)[2:] == (COUNT_JAC_A_FD, 1)
    _, _, b, J = host_case("C")
    x, hist, it, status = minres_ref(J, b, rtol=1e-6)
    true = np.linalg.norm(b.reshape(-1) - J @ x) / np.linalg.norm(b)
    print(f"C: {it} iterations, true residual {true / 1e-6:.2f} rtol")
    assert status == 1 and true <= 2e-6 and all(h1 <= h0 for h0, h1 in zip(hist, hist[1:]))
    assert minres_ref(J, b, jac_M(J, sign=1.0), itmax=5)[2:] == (0, 3)


_MG = {}


def mg_case(shape=(72, 56)):
    """Bratu 72 x 56 of the CG tests: (J as a callable, b, the restatement with M = -V: x, history, count, status)"""
    if shape not in _MG:
        P, u, k, s, h = host_problem("bratu2d", shape)
        A = lambda q: oc.jv_exact(P, u, q.reshape(P.shape)).reshape(-1)  # noqa: E731
        b = oc.residual(P, u)
        cyc = Cycle(shape, h, k, s)
        M = lambda r: -cyc.vcycle(r.reshape(P.shape)).reshape(-1)  # noqa: E731
        _MG[shape] = (A, b, minres_ref(A, b, M, rtol=1e-8))
    return _MG[shape]


def test_restatement_with_the_spd_cycle():
    A, b, (x, hist, it, status) = mg_case()
    print(f"Bratu 72 x 56, M = -V: MINRES {it} iterations (CG: 7)")
    assert status == 1 and it == COUNT_MG and abs(it - 7) <= 2
    assert np.linalg.norm(b.reshape(-1) - A(x)) <= 1e-7 * np.linalg.norm(b)


# ------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


_DEV = {}


def dev_case(name, jv="exact"):
    """the case on the device: (J, collect(J) as a dense matrix, b = F(u) as the device computed it)"""
    key = (name, jv)
    if key not in _DEV:
        (nx, ny), lam, _ = CASES[name]
        P, u0, _, _ = host_case(name)
        u = ah.DeviceArray.from_numpy(u0)
        res = u.zero()
        p = (P.hx, P.hy, lam)
        ah.bratu2d_(res, u, p)
        J = ah.JacobianOperator(ah.bratu2d_, res, u, p, jv=jv)
        _DEV[key] = (J, ah.collect(J).toarray(), res.to_numpy())
    return _DEV[key]


def solve(J, b, **kw):
    ws = ah.krylov_workspace("minres", ah.KrylovConstructor(b))
    ah.krylov_solve_(ws, J, b, history=True, **{"atol": 0.0, "rtol": 0.0, **kw})
    out = (ws.x.to_numpy(), ws.stats)
    ws.free()
    return out


def check_fixed(tag, x, st, ref, k, sx, sh):
    xr, hr, _, _ = ref
    ex, eh = relmax(x.reshape(-1), xr), relmax(st.residuals, hr)
    print(f"{tag} k={k}: x {ex:.2e} (allowed {16 * sx:.2e}), history {eh:.2e} (allowed {16 * sh:.2e})")
    assert st.status == MAXIT and not st.solved and st.niter == k and st.n_matvec == k
    assert len(st.residuals) == k + 1
    assert ex <= 16 * sx and eh <= 16 * sh


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("k", [10, 40])
def test_fixed_k_matches_restatement_and_scipy(ctx, name, k):
    J, Jm, b = dev_case(name)
    x, st = solve(J, J.res, itmax=k)
    ref = minres_ref(Jm, b, itmax=k)
    check_fixed(name, x, st, ref, k, SENS_X[name, "", k], SENS_H[name, "", k])
    xs, _ = spla.minres(Jm, b.reshape(-1), maxiter=k, rtol=1e-300)
    es = relmax(x.reshape(-1), xs)
    print(f"  vs scipy {es:.2e}")
    assert es <= 16 * SENS_X[name, "", k]


@pytest.mark.gpu
def test_minres_is_unrestarted_gmres(ctx):
    J, _, _ = dev_case("A")
    x, st = solve(J, J.res, itmax=40)
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(J.res, memory=40))
    ah.krylov_solve_(ws, J, J.res, atol=0.0, rtol=0.0, itmax=40, history=True)
    xg, hg = ws.x.to_numpy(), ws.stats.residuals
    ws.free()
    ex, eh = relmax(x, xg), relmax(st.residuals, hg)
    print(f"device MINRES vs device GMRES(40), k = 40: x {ex:.2e} (allowed {16 * MINRES_VS_GMRES_X:.2e}), history "
          f"{eh:.2e} (allowed {16 * MINRES_VS_GMRES_H:.2e})")
    assert len(hg) == 41
    assert ex <= 16 * MINRES_VS_GMRES_X and eh <= 16 * MINRES_VS_GMRES_H


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_convergence_counts(ctx, name):
    J, Jm, b = dev_case(name)
    x, st = solve(J, J.res, rtol=1e-6)
    true = np.linalg.norm(b.reshape(-1) - Jm @ x.reshape(-1)) / np.linalg.norm(b)
    print(f"{name}: niter {st.niter} (restatement {COUNTS[name]}), true residual {true:.2e}")
    assert st.solved and st.status == GOOD and st.niter == st.n_matvec == COUNTS[name]
    assert true <= 2e-6


@pytest.mark.gpu
def test_convergence_on_the_indefinite_case(ctx):
    J, Jm, b = dev_case("C")
    x, st = solve(J, J.res, rtol=1e-6)
    true = np.linalg.norm(b.reshape(-1) - Jm @ x.reshape(-1)) / np.linalg.norm(b)
    print(f"C: niter {st.niter} (restatement 409), true residual {true / 1e-6:.2f} rtol")
    assert st.solved and len(st.residuals) == st.niter + 1
    assert all(h1 <= h0 for h0, h1 in zip(st.residuals, st.residuals[1:]))
    assert true <= 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_fd_operator(ctx, name):
    J, _, _ = dev_case(name)
    Jf, _, _ = dev_case(name, jv="fd")
    x, st = solve(J, J.res, rtol=1e-6)
    xf, stf = solve(Jf, Jf.res, rtol=1e-6)
    d = float(np.linalg.norm(xf - x) / np.linalg.norm(x))
    print(f"{name}: exact {st.niter}, FD {stf.niter}, ||x_fd - x|| / ||x|| {d:.3e} (allowed {16 * FD_VS_EXACT[name]:.3e})")
    assert stf.solved and stf.niter == st.niter == COUNTS[name]
    assert d <= 16 * FD_VS_EXACT[name]


@pytest.mark.gpu
def test_jacobi_m_and_breakdown(ctx):
    for name in ("A", "C"):
        J, Jm, b = dev_case(name)
        M = ah.DiagonalPreconditioner(ah.DeviceArray.from_numpy((-1.0 / np.diag(Jm)).reshape(b.shape)))
        x, st = solve(J, J.res, itmax=40, M=M)
        check_fixed(f"{name} M=-1/diag", x, st, minres_ref(Jm, b, jac_M(Jm), itmax=40), 40, SENS_X[name, "jac", 40],
                    SENS_H[name, "jac", 40])
    J, Jm, b = dev_case("A")
    M = ah.DiagonalPreconditioner(ah.DeviceArray.from_numpy((-1.0 / np.diag(Jm)).reshape(b.shape)))
    _, st = solve(J, J.res, rtol=1e-8, M=M)
    assert st.solved and st.niter == COUNT_JAC_A
    Jf, _, _ = dev_case("A", jv="fd")  # the FD step needs ||v||_2 = ||y||_2 / beta: the fused ||y||^2
    _, stf = solve(Jf, Jf.res, rtol=1e-8, M=M)
    assert stf.solved and stf.niter == COUNT_JAC_A_FD
    Mp = ah.DiagonalPreconditioner(ah.DeviceArray.from_numpy((1.0 / np.diag(Jm)).reshape(b.shape)))
    x, st = solve(J, J.res, rtol=1e-8, M=Mp)
    assert st.status == "breakdown" and st.niter == 0 and not st.solved
    assert not np.any(x)


@pytest.mark.gpu
@pytest.mark.parametrize("jv", ["exact", "fd"])
def test_multigrid_m(ctx, jv):
    A, b, (xr, _, it_ref, _) = mg_case()
    J, _ = device_operator("bratu2d", (72, 56), jv=jv)
    mg = ah.MultigridPreconditioner(J, spd=True)
    x, st = solve(J, J.res, rtol=1e-8, M=mg)
    true = np.linalg.norm(b.reshape(-1) - A(x.reshape(-1))) / np.linalg.norm(b)
    print(f"72 x 56 jv={jv}: niter {st.niter} (restatement {it_ref}), true residual {true:.2e}")
    assert st.solved and st.niter == it_ref == COUNT_MG
    assert true <= 1e-7
    assert st.residuals[0] == math.sqrt(mg.vcycle_dot(J.res)[1])
    # a hierarchy in its default form is refused: in Python, and by the library
    mg.spd = False
    with pytest.raises(NotImplementedError, match="spd=True"):
        solve(J, J.res, M=mg)
    ws = ah.krylov_workspace("minres", ah.KrylovConstructor(J.res))
    lib, pj = ah.load(), J.problem()
    pc = C.cast(C.pointer(mg.as_c()), C.c_void_p)
    st_c, hl = _lib.nk_krylov_stats(), C.c_int64(0)
    F0 = J.res.ptr if jv == "fd" else None
    o = _lib.nk_krylov_opts(0, 0, 100, J.jv_mode, 0.0, 1e-8, 0.0, 0.0, None, None, pc, 0)
    rc = lib.nk_krylov_solve(ws.handle, C.byref(pj), J.u.ptr, F0, J.res.ptr, C.byref(o), C.byref(st_c), None, 0, C.byref(hl))
    assert rc == _lib.NK_E_ARG and "nk_mg_set_spd" in lib.nk_last_error(ctx.handle).decode()
    mg.spd = True
    o = _lib.nk_krylov_opts(0, 0, 100, J.jv_mode, 0.0, 1e-8, 0.0, 0.0, None, pc, None, 0)  # as N
    rc = lib.nk_krylov_solve(ws.handle, C.byref(pj), J.u.ptr, F0, J.res.ptr, C.byref(o), C.byref(st_c), None, 0, C.byref(hl))
    assert rc == _lib.NK_E_ARG and "right preconditioner" in lib.nk_last_error(ctx.handle).decode()
    ws.free()


@pytest.mark.gpu
def test_semicoarsened_multigrid_m(ctx):
    from test_hip_multigrid_semi import LevelCycle, plan_semi

    shape = (96, 12)
    P, u, k, s, h = host_problem("bratu2d", shape)
    cyc = LevelCycle(plan_semi(shape, h, k), h, k, s)
    A = lambda q: oc.jv_exact(P, u, q.reshape(P.shape)).reshape(-1)  # noqa: E731
    b = oc.residual(P, u)
    _, _, it_ref, status = minres_ref(A, b, lambda r: -cyc.vcycle(r.reshape(P.shape)).reshape(-1), rtol=1e-8)
    J, _ = device_operator("bratu2d", shape)
    x, st = solve(J, J.res, rtol=1e-8, M=ah.MultigridPreconditioner(J, spd=True, coarsening="semi"))
    true = np.linalg.norm(b.reshape(-1) - A(x.reshape(-1))) / np.linalg.norm(b)
    print(f"96 x 12 semi: niter {st.niter} (restatement {it_ref}), true residual {true:.2e}")
    assert status == 1 and st.solved and st.niter == it_ref and true <= 1e-7


_BIG = {}


def big_case():
    """300 x 257 on the device; collect(J) stays sparse"""
    if not _BIG:
        P = oc.bratu2d(*BIG)
        u0 = oc.sin_ic(P)
        u = ah.DeviceArray.from_numpy(u0)
        res = u.zero()
        p = (P.hx, P.hy, LAM)
        ah.bratu2d_(res, u, p)
        J = ah.JacobianOperator(ah.bratu2d_, res, u, p)
        _BIG["c"] = (J, ah.collect(J).tocsr(), res.to_numpy())
    return _BIG["c"]


@pytest.mark.gpu
def test_reductions_across_blocks(ctx):
    J, Jm, b = big_case()
    assert b.size == 77100 and b.size % 2048 != 0 and b.size > 2048
    x, st = solve(J, J.res, itmax=10)
    check_fixed("300 x 257", x, st, minres_ref(lambda q: Jm @ q, b, itmax=10), 10, *SENS_BIG)


@pytest.mark.gpu
def test_less_than_one_wave_and_zero_rhs(ctx):
    P = oc.bratu1d(7)
    u0 = oc.sin_ic(P)
    u = ah.DeviceArray.from_numpy(u0)
    res = u.zero()
    p = (P.hx, P.lam)
    ah.bratu_(res, u, p)
    J = ah.JacobianOperator(ah.bratu_, res, u, p)
    Jm, b = ah.collect(J).toarray(), res.to_numpy()
    x, st = solve(J, J.res, itmax=4)
    check_fixed("1D N=7", x, st, minres_ref(Jm, b, itmax=4), 4, SENS_X["1D7", "", 4], SENS_H["1D7", "", 4])
    true = np.linalg.norm(b - Jm @ x) / np.linalg.norm(b)
    assert true <= 1e-12  # u and b are symmetric about the midpoint: 4 steps span the solution
    x, st = solve(J, u.zero(), rtol=1e-8)
    assert st.niter == 0 and st.solved and st.residuals == [0.0] and not np.any(x)


@pytest.mark.gpu
def test_two_solves_give_identical_bits(ctx):
    J, Jm, b = dev_case("A")
    M = ah.DiagonalPreconditioner(ah.DeviceArray.from_numpy((-1.0 / np.diag(Jm)).reshape(b.shape)))
    for kw in ({}, {"M": M}):
        (x1, s1), (x2, s2) = solve(J, J.res, itmax=40, **kw), solve(J, J.res, itmax=40, **kw)
        np.testing.assert_array_equal(x1, x2)
        assert s1.residuals == s2.residuals


@pytest.mark.gpu
def test_newton_minres_1d_reaches_cgs_root(ctx):
    P = oc.bratu1d(1000)
    u0 = oc.sin_ic(P)
    p = (P.hx, P.lam)
    um, rm = ah.newton_krylov_(ah.bratu_, ah.DeviceArray.from_numpy(u0), p, algo="minres")
    uc, rc = ah.newton_krylov_(ah.bratu_, ah.DeviceArray.from_numpy(u0), p, algo="cg")
    print(f"1D 1000: MINRES {tuple(rm.stats[:2])} ||F|| {rm.stats.n_res:.2e} solved {rm.solved}; CG {tuple(rc.stats[:2])} "
          f"||F|| {rc.stats.n_res:.2e} solved {rc.solved}")
    assert rm.solved and rc.solved
    tol = 1e-6 * np.linalg.norm(oc.residual(P, u0)) + 1e-12
    assert rm.stats.n_res <= tol
    # "within the Newton tolerance": F(u_m) - F(u_c) = J (u_m - u_c) to first order, so ||u_m - u_c||_2 <= (||F(u_m)|| +
    # ||F(u_c)||) / min|λ(J)|; λ sits at the fold, where J is nearly singular (min|λ| = 0.023), and the factor 2 covers
    # the second-order term
    from scipy.linalg import eigvalsh_tridiagonal

    w = eigvalsh_tridiagonal(-2.0 / P.hx ** 2 + P.lam * np.exp(uc.to_numpy()), np.full(999, 1.0 / P.hx ** 2))
    bound = 2.0 * (rm.stats.n_res + rc.stats.n_res) / float(np.min(np.abs(w)))
    d = float(np.linalg.norm(um.to_numpy() - uc.to_numpy()))
    print(f"  ||u_minres - u_cg||_2 {d:.2e} (allowed {bound:.2e}, min|λ(J)| {np.min(np.abs(w)):.3e})")
    assert d <= bound


@pytest.mark.gpu
def test_newton_minres_drivers_agree(ctx):
    P = oc.bratu2d(64)
    u0 = oc.sin_ic(P)
    p = (P.hx, P.hy, P.lam)
    u, r = ah.newton_krylov_(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, algo="minres")
    un, rn = ah.newton_krylov_native(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, algo="minres")
    assert r.solved and rn.solved and tuple(rn.stats[:2]) == tuple(r.stats[:2])
    np.testing.assert_array_equal(un.to_numpy(), u.to_numpy())
    exe = os.path.join(ROOT, "newtonkrylov.jl_amd", "bin", "bratu2d_newton")
    out = subprocess.run([exe, "64", "exact", "20", "0", "--minres"], capture_output=True, text=True, timeout=120, check=True)
    rj = json.loads(out.stdout.strip().splitlines()[-1])
    assert rj["algo"] == "minres" and rj["solved"] and (rj["outer"], rj["inner"]) == tuple(r.stats[:2])
    # with the SPD hierarchy as M, refreshed every Newton step
    um, rmg = ah.newton_krylov_(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, algo="minres", M=ah.multigrid(spd=True))
    fac = ah.multigrid(spd=True)
    _, rmn = ah.newton_krylov_native(ah.bratu2d_, ah.DeviceArray.from_numpy(u0), p, algo="minres", M=fac)
    fac.free()
    out = subprocess.run([exe, "64", "exact", "20", "0", "--minres", "--mg"], capture_output=True, text=True, timeout=120,
                         check=True)
    rj = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"2D 64: plain {tuple(r.stats[:2])}, M = multigrid {tuple(rmg.stats[:2])}")
    assert rmg.solved and rmn.solved and tuple(rmn.stats[:2]) == tuple(rmg.stats[:2]) == (rj["outer"], rj["inner"])
    assert rmg.stats.inner_iterations < r.stats.inner_iterations
    np.testing.assert_allclose(um.to_numpy(), u.to_numpy(), rtol=0, atol=1e-5 * np.abs(u.to_numpy()).max())


@pytest.mark.gpu
def test_newton_minres_root_is_the_golden_root(ctx, golden_dir):
    """scipy's sparse-direct Newton root of 2D Bratu 64^2, as test_hip.py's golden test compares it (tol_rel = 1e-10,
    1e-8 of max|u*|)"""
    g = np.load(os.path.join(golden_dir, "bratu2d_64.npz"))
    P = oc.bratu2d(64)
    u, r = ah.newton_krylov_(ah.bratu2d_, ah.DeviceArray.from_numpy(g["u0"]), (P.hx, P.hy, P.lam), algo="minres",
                             tol_rel=1e-10)
    err = float(np.max(np.abs(u.to_numpy() - g["ustar"])) / np.max(np.abs(g["ustar"])))
    print(f"Newton-MINRES 64^2: outer {r.stats.outer_iterations} inner {r.stats.inner_iterations}, max|u - u*| / max|u*| {err:.2e}")
    assert r.solved and err <= 1e-8


@pytest.mark.gpu
def test_implicit_euler_step_periodic_odd_widths(ctx):
    nx, ny = 33, 27
    hx, hy, a = 1.0 / nx, 1.0 / ny, 0.01
    dt = 20.0 * hx * hx * hy * hy / (2.0 * a * (hx * hx + hy * hy))
    un0 = np.random.default_rng(8).standard_normal((ny, nx))
    sp = (a, hx, hy, ah.bc_periodic_)
    outs = {}
    for algo in ("gmres", "minres"):
        st = []
        un = ah.solve(ah.G_Euler_, ah.diffusion_, ah.DeviceArray.from_numpy(un0), sp, dt, [0.0, dt], algo=algo, stats_out=st)
        assert st[0].solved
        outs[algo] = (un.to_numpy(), st[0])
    d = float(np.max(np.abs(outs["minres"][0] - outs["gmres"][0])))
    print(f"implicit Euler {nx} x {ny} periodic: max|u_minres - u_gmres| {d:.2e}; inner gmres "
          f"{outs['gmres'][1].stats.inner_iterations} minres {outs['minres'][1].stats.inner_iterations}")
    assert d <= 6.0e-6  # the Newton tolerance of solve() (tol_abs = 6e-6 on ||F||; J = -I + dt a Δ: ||J^-1|| <= 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mailbox", ["device", "host"])
def test_two_ranks(ctx, tmp_path, mailbox):
    from test_hip_dist import run_ranks, worker_env

    out = str(tmp_path / "minres2")
    env = worker_env(2, **({"NK_DIST_MAILBOX": "host"} if mailbox == "host" else {}))
    rc, log = run_ranks(2, [os.path.join(ROOT, "tests", "minres_dist_worker.py"), "--out", out, "--itmax", "20"], env)
    assert rc == 0, log[-3000:]
    meta = json.load(open(out + ".json"))
    d = np.load(out + ".npz")
    assert meta["path"]["mailbox"] and meta["path"]["mailbox_host"] == (mailbox == "host")
    assert meta["niter"] == [20, 20] and meta["histories_equal"]
    J, _, _ = dev_case("A")
    x, st = solve(J, J.res, itmax=20)
    ex, eh = relmax(d["x"], x), relmax(d["h"], st.residuals)
    print(f"two ranks ({mailbox} mailbox) vs one, k = 20: x {ex:.2e} (allowed {16 * SENS_X['A', '', 20]:.2e}), history "
          f"{eh:.2e} (allowed {16 * SENS_H['A', '', 20]:.2e})")
    assert ex <= 16 * SENS_X["A", "", 20] and eh <= 16 * SENS_H["A", "", 20]
