"""GPU tests of the ILU(0) sweeps (csrc/nk_precond.hip) where their strip, chunk and level logic changes.

k_ilu0_pipe: one wave per strip of 64 rows, lanes skewed by one column, loads in chunks of 16 columns, strips
handing over through progress counters, in 3D up to three awaited strips (s - 1, sb, sb2), a grid-stride loop
when there are more strips than CUs.  k_ilu0_factor / k_ilu0_solve: one work-group of 1024 threads striding
over each anti-diagonal level.  Every result is the oracle's sequential loop (oc.ilu0_factor / oc.ilu0_solve,
pinned against a textbook IKJ ILU(0) in test_oracle.py) bit for bit -- no tolerance -- and every case checks from
the launch counts which kernels ran, so that it cannot pass on the other path.
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
PIPE = {"ilu0_factor": 1, "ilu0_forward": 1, "ilu0_backward": 1, "ilu0_factor_levels": 0, "ilu0_solve_levels": 0}
LEVELS = {"ilu0_factor": 0, "ilu0_forward": 0, "ilu0_backward": 0, "ilu0_factor_levels": 1, "ilu0_solve_levels": 1}


@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def cu_count():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count  # the attribute ilu_pipe_setup reads


def problem(spec, rng, dt=None):
    """spec = ("bratu1d", nx) | ("bratu2d", nx, ny) | ("heat2d" | "heat3d", nx, ny[, nz], scheme) -> the oracle's
    problem and u0 (the sine / u_n plus seeded noise); midpoint runs with alpha = 0.3, dt = None is the
    examples' stability-limit step."""
    kind, *dims = spec
    if kind.startswith("bratu"):
        P = oc.bratu1d(*dims) if kind == "bratu1d" else oc.bratu2d(*dims)
        return P, oc.sin_ic(P) + 0.05 * rng.standard_normal(P.shape)
    *dims, scheme = dims
    make = oc.heat2d_euler if kind == "heat2d" else oc.heat3d_euler
    P = make(*dims, un=rng.standard_normal(tuple(reversed(dims))), scheme=scheme, alpha=0.3, dt=dt)
    return P, P.un + 0.05 * rng.standard_normal(P.shape)


def device_operator(c, P, u0):
    """The JacobianOperator of P at u0 on context c (and F(u0), computed by the device residual)."""
    if P.kind == oc.BRATU1D:
        F, p = ah.bratu_, (P.hx, P.lam)
    elif P.kind == oc.BRATU2D:
        F, p = ah.bratu2d_, (P.hx, P.hy, P.lam)
    else:
        scheme = {v: k for k, v in oc.HEAT_KINDS.items()}[P.kind][0]
        F = getattr(ah, f"heat{P.dim}d_{scheme}_")
        F = F.with_alpha(P.alpha) if scheme == "midpoint" else F
        h = (P.hx, P.hy) if P.dim == 2 else (P.hx, P.hy, P.hz)
        p = (ah.DeviceArray.from_numpy(P.un, ctx=c), P.dt, None, (P.a, *h, ah.bc_zero_), 0.0)
    u = ah.DeviceArray.from_numpy(u0, ctx=c)
    res = u.zero()
    F(res, u, p)
    return ah.JacobianOperator(F, res, u, p), res


def ilu_launches(c):
    prof = c.prof_read()
    return {k: prof.get(k, {}).get("launches", 0) for k in PIPE}


def factor_and_apply(c, P, u0, v):
    """N = ilu0(J), z = N v on context c -> (pivots, z, launches per ILU(0) kernel class)."""
    J, _ = device_operator(c, P, u0)
    c.prof_reset()
    c.prof_enable(1 << 20)
    try:
        N = ah.ilu0(J)
        z = N.apply(J, ah.DeviceArray.from_numpy(v, ctx=c))
        return N.d.to_numpy(), z.to_numpy(), ilu_launches(c)
    finally:
        c.prof_enable(0)


def check_sweeps(c, spec, expected, seed=31):
    rng = np.random.default_rng(seed)
    P, u0 = problem(spec, rng)
    v = rng.standard_normal(P.shape)
    d, z, ran = factor_and_apply(c, P, u0, v)
    assert ran == expected
    dref = oc.ilu0_factor(P, u0)
    assert np.all(np.isfinite(dref))
    np.testing.assert_array_equal(d, dref)
    np.testing.assert_array_equal(z, oc.ilu0_solve(P, dref, v))


# ----------------------------------------------------------------------------- 1. pipelined, 1D and 2D
@pytest.mark.parametrize("spec", [
    ("bratu1d", 1), ("bratu1d", 15), ("bratu1d", 16), ("bratu1d", 17),  # one lane, around the 16-column chunk
    ("bratu2d", 1, 200),   # rows of one column: every strip but the first waits on `done` clamped from below
    ("bratu2d", 2, 65),    # 64 + 1 rows: the second strip has one lane
    ("bratu2d", 15, 129),  # nx < chunk, two strips + one row
    ("bratu2d", 16, 64),   # nx = chunk, exactly one strip
    ("bratu2d", 17, 63),   # nx = chunk + 1, one row short of a strip
    ("bratu2d", 33, 128),  # nx < the lane skew, exactly two strips
    ("bratu2d", 300, 1),   # one row
    ("bratu2d", 1, 1),     # one point
    ("heat2d", 33, 70, "midpoint"),  # the (1 - alpha) off-diagonal on the pipelined path
], ids=lambda s: "-".join(map(str, s)))
def test_ilu0_pipelined_chunk_and_strip_edges(ctx, spec):
    """Rows shorter than one chunk (nx < 16: need = nx at every step) or than the lane skew (nx < 64 with
    several strips: `done` clamped, steps = nx + last), the chunk edges nx = 15, 16, 17 and R = 63, 64, 65,
    128, 129 rows."""
    check_sweeps(ctx, spec, PIPE)


# ----------------------------------------------------------------------------- 2. pipelined, 3D
@pytest.mark.parametrize("spec", [
    ("heat3d", 5, 129, 3, "midpoint"),    # sb, sb2 and s - 1 all distinct: the third wait
    ("heat3d", 17, 200, 2, "trapezoid"),
    ("heat3d", 16, 128, 3, "euler"),      # sb == sb2 == s - 2
    ("heat3d", 3, 127, 2, "euler"),       # sb2 == s - 1, nx < 16
], ids=lambda s: "-".join(map(str, s)))
def test_ilu0_pipelined_3d_below_strips(ctx, spec):
    """3D with ny >= 64: the plane below a strip's rows lies in the strips sb .. sb2, which are neither each
    other nor the predecessor once ny >= 129."""
    check_sweeps(ctx, spec, PIPE)


# ----------------------------------------------------------------------------- 3. more strips than CUs
@functools.lru_cache(maxsize=None)
def many_strips_2d(cus):
    """bratu2d(16, R) with cus + 4 strips, and the oracle's pivots and solve: computed once, read-only."""
    R = 64 * (cus + 3) + 5
    rng = np.random.default_rng(41)
    P, u0 = problem(("bratu2d", 16, R), rng)
    v = rng.standard_normal(P.shape)
    d = oc.ilu0_factor(P, u0)
    z = oc.ilu0_solve(P, d, v)
    for a in (u0, v, d, z):
        a.setflags(write=False)
    return P, u0, v, d, z


def test_ilu0_pipelined_grid_stride_2d(ctx):
    """More strips (cus + 4) than CUs: the launch has cus waves and the first four take a second strip
    (s += gridDim.x), the last of them a partial one."""
    cus = cu_count()
    P, u0, v, dref, zref = many_strips_2d(cus)
    assert P.ny > 64 * cus  # more strips than the launch has waves, whatever the part's CU count
    assert np.all(np.isfinite(dref))
    d, z, ran = factor_and_apply(ctx, P, u0, v)
    assert ran == PIPE
    np.testing.assert_array_equal(d, dref)
    np.testing.assert_array_equal(z, zref)


def test_ilu0_pipelined_grid_stride_3d(ctx):
    """The same in 3D: ny = 64, one strip per plane, cus + 4 planes -- the second strip of a wave waits on the
    plane below, which another wave's first strip wrote."""
    cus = cu_count()
    ny, nz = 64, cus + 4
    assert ny * nz > 64 * cus
    check_sweeps(ctx, ("heat3d", 8, ny, nz, "euler"), PIPE)


# ----------------------------------------------------------------------------- 4. level sweeps
@pytest.mark.parametrize("spec", [
    ("heat3d", 5, 40, 40, "midpoint"),    # levels of up to 1600 points: the q += blockDim.x stride
    ("heat3d", 40, 63, 30, "trapezoid"),  # ny one below the pipelined threshold
    ("heat3d", 1, 1, 5, "euler"),
], ids=lambda s: "-".join(map(str, s)))
def test_ilu0_level_sweeps(ctx, spec):
    """3D with ny < 64: one work-group sweeps the anti-diagonal levels, more than 1024 points on a level."""
    check_sweeps(ctx, spec, LEVELS)


# ----------------------------------------------------------------------------- 5. counter buffer reuse
def test_ilu0_progress_counters_reused():
    """A fresh context: the many-strip case (ilu_prog grows), one strip (the counters beyond it keep the
    first case's final values), and the many-strip case again (every launch must clear the counters it polls)."""
    c = ah.Context(0)
    try:
        P, u0, v, dref, zref = many_strips_2d(cu_count())
        for big in (True, False, True):
            if big:
                d, z, ran = factor_and_apply(c, P, u0, v)
                assert ran == PIPE
                np.testing.assert_array_equal(d, dref)
                np.testing.assert_array_equal(z, zref)
            else:
                check_sweeps(c, ("bratu2d", 17, 63), PIPE)
        c.sync()
    finally:
        c.close()


# ----------------------------------------------------------------------------- 6. inside a solve, 3D
@pytest.mark.parametrize("side", ["N", "M"])
def test_ilu0_preconditioned_gmres_heat3d(ctx, side):
    """ILU(0) as N (ldiv = true) and as M of restarted GMRES(10) on a 3D problem (G_Trapezoid!, 24 x 64 x 6, the
    pipelined sweeps): 20 steps against the oracle's preconditioned GMRES -- equal counts, history to 1e-9, x
    to 1e-9 of its norm, and bit for bit in the device's reduction order.

    dt = 10, about 1000 explicit steps: with the examples' stability-limit dt, J = I - (dt / 2) a lap has its
    spectrum in [1, 2], the preconditioned residual is at rounding level (1e-16 ||b||) after 7 steps, and the rest
    of a 20-step history is noise that no bar independent of the reduction order can compare -- the oracle's own
    histories in plain and in device order then differ by factors of up to 17.  At dt = 10 the residual falls by
    1e-5 to 1e-6 in 20 steps and the oracle's two orders agree to 4e-11 (history) and 3e-15 (x)."""
    rng = np.random.default_rng(51)
    P, u0 = problem(("heat3d", 24, 64, 6, "trapezoid"), rng, dt=10.0)
    J, res = device_operator(ctx, P, u0)
    kw = dict(restart=True, itmax=20, atol=0.0, rtol=0.0)
    ctx.prof_reset()
    ctx.prof_enable(1 << 20)
    try:
        N = ah.ilu0(J)
        ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=10))
        if side == "N":
            ah.krylov_solve_(ws, J, res, N=N, ldiv=True, history=True, **kw)
        else:
            ah.krylov_solve_(ws, J, res, M=N, history=True, **kw)
        ran = ilu_launches(ctx)
    finally:
        ctx.prof_enable(0)
    x, st, h = ws.x.to_numpy(), ws.stats, np.array(ws.stats.residuals)
    ws.free()
    assert ran["ilu0_factor"] == 1 and ran["ilu0_forward"] == ran["ilu0_backward"] >= 20
    assert ran["ilu0_factor_levels"] == ran["ilu0_solve_levels"] == 0
    d = oc.ilu0_factor(P, u0)
    np.testing.assert_array_equal(N.d.to_numpy(), d)
    F0 = res.to_numpy()
    okw = dict(memory=10, **{side: ("ilu0", d)}, **kw)
    xo, so, ho = oc.krylov_solve(P, u0, F0, **okw)
    assert st.niter == so["niter"] == 20 and st.n_matvec == so["n_matvec"]
    np.testing.assert_allclose(h, ho, rtol=1e-9)
    assert np.linalg.norm(x - xo) <= 1e-9 * np.linalg.norm(xo)
    oc.set_devred(True, cus=ctx.path_info()["resident_blocks"] or 256)
    try:
        xr, _, hr = oc.krylov_solve(P, u0, F0, **okw)
    finally:
        oc.set_devred(False)
    np.testing.assert_array_equal(h, hr)
    np.testing.assert_array_equal(x, xr)


# ----------------------------------------------------------------------------- 7. single-rank recovery
def test_ilu0_timeout_recovers_on_one_rank(ctx, tmp_path):
    """One rank's recovery from a pipelined solve sweep that timed out: nk_precond_apply redoes the apply, and
    nk_krylov_solve the whole solve, on the level sweep (the ilu_redo branches; the two-rank test of
    test_hip_dist.py takes the rank-local redo inside launch_ilu0_solve instead).  tests/ilu_timeout_worker.py
    runs bratu2d(20, 1100) -- 18 strips, levels of 1100 points -- with NK_ILU_SPIN_LIMIT=1: (a) factor, apply,
    factor, apply in one context, (b) ILU(0)-preconditioned GMRES(10), 12 steps, in a fresh one.  Pivots and
    both z bit for bit the oracle's, history and x bit for bit this process's pipelined solve, each context
    reported its timeout, and the contexts stayed on the level sweep afterwards.

    Not covered, being out of reach of NK_ILU_SPIN_LIMIT (it shortens the solve sweeps' poll budget only, and
    a solve that fused the Newton update is not redone): the refactor branch of nk_ilu0_factor (a factor sweep
    that timed out) and a timeout after a fused Newton update."""
    rng = np.random.default_rng(61)
    P, u0 = problem(("bratu2d", 20, 1100), rng)
    v = rng.standard_normal(P.shape)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, u0=u0, v=v, lam=P.lam)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ilu_timeout_worker.py"), inp, out],
                       env=dict(os.environ, NK_ILU_SPIN_LIMIT="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stderr.count("pipelined ILU(0) sweep timed out") == 2, r.stderr[-3000:]  # once per context
    w = np.load(out)
    # (a): the first factor pipelined, its apply timed out and was redone; then the level sweep only
    first, a, b = ({k: json.loads(str(w[name])).get(k, 0) for k in PIPE} for name in ("prof_first", "prof_a", "prof_b"))
    assert first == dict(PIPE, ilu0_solve_levels=1)
    assert a == dict(PIPE, ilu0_factor_levels=1, ilu0_solve_levels=2)
    d = oc.ilu0_factor(P, u0)
    z = oc.ilu0_solve(P, d, v)
    np.testing.assert_array_equal(w["d"], d)
    np.testing.assert_array_equal(w["d2"], d)
    np.testing.assert_array_equal(w["z1"], z)
    np.testing.assert_array_equal(w["z2"], z)
    # (b): one pipelined apply, then the solve again with every apply on the level sweep
    assert b["ilu0_factor"] == 1 and b["ilu0_forward"] == 1 and b["ilu0_factor_levels"] == 0
    assert b["ilu0_solve_levels"] >= 12
    J, res = device_operator(ctx, P, u0)
    ctx.prof_reset()
    ctx.prof_enable(1 << 20)
    try:
        N = ah.ilu0(J)
        ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=10))
        ah.krylov_solve_(ws, J, res, N=N, ldiv=True, history=True, restart=True, atol=0.0, rtol=0.0, itmax=12)
        ran = ilu_launches(ctx)
    finally:
        ctx.prof_enable(0)
    assert ran["ilu0_forward"] >= 12 and ran["ilu0_solve_levels"] == 0  # this process: pipelined throughout
    assert int(w["niter"]) == ws.stats.niter == 12 and int(w["n_matvec"]) == ws.stats.n_matvec
    np.testing.assert_array_equal(w["h"], np.array(ws.stats.residuals))
    np.testing.assert_array_equal(w["x"], ws.x.to_numpy())
    ws.free()
