"""CPU: the checkers of tests/test_hip_fused_edges.py, fed a numpy stand-in for the device.

A check that would accept a wrong kernel is worth nothing.  The stand-in does what the device does in float64 with
another summation order (products rounded, 256-element blocks summed pairwise, the block sums added in order -- neither
the kernels' fma chains nor math.fsum) and the fma update oc.axpy; it can be told to make one of the mistakes a kernel
could make:

  tail_dot   the last element of an odd-n vector left out of a dot
  block      one block's partial sum dropped
  tail_q     the tail element of q not updated by a pass
  stale      h_i taken against q_{i-2} instead of q_{i-1}
  wrap       w = J v with the last column's right neighbour taken as zero under bc_periodic!
  edge       w = J v with one x-tile's first column taking its left neighbour from the row before

The honest stand-in passes every checker -- the MGS replay, the reorthogonalised sweep's bound, check_arnoldi_step as
test_hip_fused_edges.py uses it, the CG and the restart-residual bounds -- and every mistake is rejected, at the small
end of that file's shapes.
"""
import math

import numpy as np
import pytest

import _nkpath  # noqa: F401
import test_hip_fused_edges as fe
from oracle import oracle as oc
from test_hip_bratu3d import check_arnoldi_step

BY_ID = {c.id: c for c in fe.CASES}
MGS_N = [n for n in fe.MGS_N if n <= 5001]


def need(ok, why):
    """a precondition of the stand-in itself: never an AssertionError, which the rejection tests wait for"""
    if not ok:
        raise ValueError(why)


def dot(x, y, mut=None, block=256):
    t = (np.asarray(x) * np.asarray(y)).reshape(-1)
    if mut == "tail_dot":
        need(t.size % 2 == 1, "tail_dot needs an odd n")
        t = t[:-1]
    parts = [float(np.sum(t[i:i + block])) for i in range(0, t.size, block)] or [0.0]
    if mut == "block":
        need(len(parts) >= 2, "block needs two blocks or more")
        parts[(len(parts) - 1) // 2] = 0.0
    s = 0.0
    for p in parts:
        s += p
    return s


def standin_mgs(q0, V, reorth, mut=None):
    """(h, q): nk_mgs_step's chain -- h_i = <V_i, q>, q = fma(-h_i, V_i, q), then ||q||; two sweeps with the h_i added"""
    k = len(V)
    q, prev = q0.copy(), None
    h = np.zeros(k + 1)
    for t in range(2 * k if reorth else k):
        i = t % k
        ht = dot(V[i], prev if (mut == "stale" and prev is not None) else q, mut)
        prev = q
        q = oc.axpy(-ht, V[i], q)
        if mut == "tail_q":
            q[-1] = prev[-1]
        h[i] += ht
    h[k] = math.sqrt(dot(q, q, mut))
    return h, q


def applies(mut, n, k, reorth):
    if mut == "tail_dot":
        return n % 2 == 1
    if mut == "block":
        return n > 256  # two blocks or more
    if mut == "stale":
        # against an orthonormal basis <V_i, q_{i-2}> = <V_i, q_{i-1}> in exact arithmetic (classical Gram-Schmidt):
        # only the replay on a basis that is not orthogonal tells the two apart
        return k > 1 and not reorth
    return True


@pytest.mark.parametrize("reorth", [False, True], ids=["sweep", "reorth"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", MGS_N)
def test_mgs_checkers(n, k, reorth):
    """the honest chain in another summation order stays inside the replay's and the two-sweep bound; each mistake
    leaves them"""
    q0, V = fe.mgs_inputs(n, k, reorth)
    check = fe.check_mgs_reorth if reorth else fe.check_mgs_replay
    h, q = standin_mgs(q0, V, reorth)
    check(q0, V, h, q, f"honest n {n} k {k}")
    for mut in ("tail_dot", "block", "tail_q", "stale"):
        if not applies(mut, n, k, reorth):
            continue
        h, q = standin_mgs(q0, V, reorth, mut)  # (outside the block: only the checker may raise in it)
        with pytest.raises(AssertionError):
            check(q0, V, h, q, f"{mut} n {n} k {k}")


def test_stale_pass_is_seen_at_every_size_with_three_vectors():
    """the mistake the reorthogonalised form cannot see is rejected by the replay wherever it can occur"""
    for n in MGS_N:
        q0, V = fe.mgs_inputs(n, 3, False)
        h, q = standin_mgs(q0, V, False, "stale")
        with pytest.raises(AssertionError):
            fe.check_mgs_replay(q0, V, h, q, f"stale n {n}")


# ----------------------------------------------------------------------------- the stencil launches
def x_offdiag(P, u):
    return dict(fe.jacobian_entries(P, u)[1])[P.dim - 1]


def spoil(P, u, w, v, mut):
    """w = J v with one of the two stencil mistakes (the x axis is numpy's last)"""
    w = w.copy()
    cx = x_offdiag(P, u)
    if mut == "wrap":
        need(P.bc == oc.BC_PERIODIC, "wrap needs bc_periodic!")
        w[..., -1] -= cx * v[..., 0]
    elif mut == "edge":
        c0 = {2: 256, 3: 64}[P.dim]  # the first column of the second VEC 1 tile
        need(P.nx % 2 == 1 and P.nx > c0, "edge needs a second VEC 1 tile")
        rows = v.reshape(-1, P.nx)
        out = w.reshape(-1, P.nx)
        out[1:, c0] += cx * (rows[:-1, c0 - 1] - rows[1:, c0 - 1])
    return w


def standin_arnoldi(P, u, b, d=None, mut=None, jv=None):
    """V_1 .. V_3 of two Arnoldi steps with exact Jv (on d .* V_k for a Jacobi N; jv: another operator): modified
    Gram-Schmidt in float64, the fused <V_1, w> with the dot mistakes, w with the stencil mistakes"""
    jv = jv or (lambda z: oc.jv_exact(P, u, z))
    V = [b / math.sqrt(dot(b, b))]
    for k in (1, 2):
        z = V[k - 1] if d is None else d * V[k - 1]
        q = spoil(P, u, jv(z), z, mut)
        for j in range(k):
            h = dot(V[j], q, mut if j == 0 else None)
            q = oc.axpy(-h, V[j], q).reshape(P.shape)
        V.append(q / math.sqrt(dot(q, q)))
    return V


ARNOLDI = [("bratu1d-257", ("tail_dot", "block")), ("bratu2d-3x3", ("tail_dot",)),
           ("bratu2d-257x9", ("tail_dot", "block", "edge")), ("euler-bc1-128x9", ("block", "wrap")),
           ("midpoint-bc1-3x3", ("tail_dot", "wrap")), ("trapezoid-bc1-257x9", ("tail_dot", "wrap", "edge")),
           ("euler-bc0-129x5x18", ("block", "edge")), ("euler-bc0-65x7x5", ("tail_dot", "block", "edge")),
           ("trapezoid-bc1-128x6x18", ("block", "wrap")),
           ("midpoint-bc1-3x3x3", ("tail_dot", "wrap"))]


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("cid,muts", ARNOLDI, ids=[a[0] for a in ARNOLDI])
def test_arnoldi_checker(cid, muts, jacobi):
    """check_arnoldi_step on steps 1 and 2 as test_gmres_fused_jv_forms and test_jacobi_gmres_plain_jv_dot call it"""
    c = BY_ID[cid]
    P, u = c.P, c.u
    b = oc.residual(P, u)
    d = oc.jacobian_diag(P, u, reciprocal=True) if jacobi else None

    def check(V, what):
        for k in (1, 2):
            z = V[k - 1] if d is None else d * V[k - 1]
            check_arnoldi_step(V, k, oc.jv_exact(P, u, z), f"{cid} {what} step {k}")

    check(standin_arnoldi(P, u, b, d), "honest")
    for mut in muts:
        V = standin_arnoldi(P, u, b, d, mut)
        with pytest.raises(AssertionError):
            check(V, mut)


@pytest.mark.parametrize("cid,muts", ARNOLDI, ids=[a[0] for a in ARNOLDI])
def test_cg_checker(cid, muts):
    """check_cg_reduction on one CG step from x = 0: alpha = gamma / <p, J p>, x = alpha b"""
    c = BY_ID[cid]
    P, u = c.P, c.u
    b = oc.residual(P, u)
    Jb = oc.jv_exact(P, u, b)
    beta = math.sqrt(dot(b, b))

    def step(mut=None):
        alpha = beta * beta / dot(b, spoil(P, u, Jb, b, mut), mut)
        return alpha * b

    fe.check_cg_reduction(b, Jb, step(), beta, f"{cid} honest")
    for mut in muts:
        x = step(mut)
        with pytest.raises(AssertionError):
            fe.check_cg_reduction(b, Jb, x, beta, f"{cid} {mut}")


RESID = [a for a in ARNOLDI if BY_ID[a[0]] in fe.RESID_CASES]


@pytest.mark.parametrize("cid,muts", RESID, ids=[a[0] for a in RESID])
def test_restart_residual_checker(cid, muts):
    """check_restart_residual on a second cycle of one step: w = b - J x_1, V = w / rNorm, x_f = x_1 + y V, with the
    stencil mistakes in w (the dot mistakes change only its norm, which the relation does not observe)"""
    c = BY_ID[cid]
    P, u = c.P, c.u
    b = oc.residual(P, u)
    V3 = standin_arnoldi(P, u, b)
    x1 = 0.3 * V3[0] - 0.2 * V3[1]  # any x_1 serves: the relation holds for every first cycle

    def cycle(mut=None):
        w = b - spoil(P, u, oc.jv_exact(P, u, x1), x1, mut)
        V = w / (0.9 * math.sqrt(dot(w, w)))  # rNorm is the previous cycle's estimate, not ||w||
        JV = oc.jv_exact(P, u, V)
        y = dot(JV, w) / dot(JV, JV)
        return x1 + y * V, V

    fe.check_restart_residual(P, u, b, *cycle(), f"{cid} honest")
    for mut in muts:
        if mut in ("wrap", "edge"):
            xf, V = cycle(mut)
            with pytest.raises(AssertionError):
                fe.check_restart_residual(P, u, b, xf, V, f"{cid} {mut}")


def test_the_cases_are_the_issue_s():
    """102 kind / boundary / shape combinations, in both Jv modes (204), every one with a two-step Arnoldi basis the
    helper accepts: the Gram matrix of the stand-in's basis within 1e-12 of the identity (check_arnoldi_step requires
    1e-6).  FD: the solver's step for a unit vector, fd_step(||u||, 1)."""
    assert len(fe.CASES) == 102 and len(set(fe.IDS)) == 102
    per_dim = {dim: {c.shape for c in fe.RESID_CASES if c.P.dim == dim} for dim in (1, 2, 3)}
    assert all(len(s) >= 4 for s in per_dim.values())
    worst = 0.0
    for c in fe.CASES:
        P, u = c.P, c.u
        b = oc.residual(P, u)
        eps = fe.fd_step(float(np.linalg.norm(u)), 1.0)
        for jv in (None, lambda z: oc.jv_fd(P, u, z, b, eps)):
            V = standin_arnoldi(P, u, b, jv=jv)
            G = np.array([[float(np.dot(a.reshape(-1), b_.reshape(-1))) for b_ in V] for a in V])
            worst = max(worst, float(np.max(np.abs(G - np.eye(3)))))
    print(f"max |G - I| over the cases: {worst:.3e}")
    assert worst <= 1e-12
