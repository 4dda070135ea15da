"""Every register-slot variant of the resident MGS sweep (k_mgs_res in csrc/nk_resident.hip; the selection rule is
res_plan in csrc/nk_plan.hpp).

The host picks the register slots rv from {89, 64, 48, 32, 25, 16, 0} by the vector length alone, and each value is
an instantiation of its own with its own unrolled register loops.  test_hip_resident.py and test_hip.py reach rv = 0,
16 (streamed remainder only) and 89; the shapes here reach 16 at full residency (V_{k+1} or q stored straight from
the registers), 25, 32, 48 and 64 -- each at full residency, unpreconditioned (the sweep stores V_{k+1}) and with a
Jacobi N (it writes q back), and with a streamed remainder whose last slot is partial and whose blocks are uneven --
one selection threshold (the last slot count of 25 against the first of 32), and the pass-count edge: a sweep of
exactly kResMax = 64 passes and a cycle that crosses it and falls back to the per-pass chain.

`sweep_plan` restates the host's selection rule (tests/test_plan.py holds it against res_plan itself); a CPU test holds
every case against the variant and geometry it names, so the cases stay honest if a shape is edited.  Each GPU case then asserts that the variant ran (the profile's
kernel name), the history and x bit for bit against the oracle in device order, against the plain-order oracle to
test_resident_sweep_matches_oracle's tolerances, the true residual of the device's x (host Jv) against the estimate
and the orthonormality of the last cycle's basis (test_full_size_cycle_properties's tolerances).
"""
from collections import namedtuple

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from oracle import oracle as oc

K_RES_MAX = 64  # kResMax of nk_plan.hpp: passes per resident launch
RV_SET = (89, 64, 48, 32, 25, 16, 0)  # kRv: the instantiated register-slot counts
SLOT = 256  # kResThreads: double2 elements per slot


def whole_slots(n, G=256):
    """Slots that every block's chunk holds in full (the last block's last slot may be partial)."""
    n2 = n // 2
    ns = -(-n2 // SLOT)
    return ns // G - (n2 % SLOT != 0)


def sweep_plan(n, G=256, rl=39):
    """res_plan's selection for a vector of n doubles on G blocks with rl LDS slots available:
    (rv, rl, full, partial_last_slot, ragged_blocks); None where no block holds a whole slot."""
    n2 = n // 2
    ns = -(-n2 // SLOT)
    whole = whole_slots(n, G)
    if whole < 1:
        return None
    rl = min(whole, rl)  # LDS first
    rv = next(r for r in RV_SET if r <= whole - rl)  # registers hold what the LDS cannot
    full = n2 % SLOT == 0 and -(-ns // G) <= rv + rl
    return rv, rl, full, n2 % SLOT != 0, ns % G != 0


def sweep_applies(n, np_, G=256, rl=39):
    """Does a sweep of np_ passes over n doubles run resident?  2 to kResMax passes (a one-pass sweep only adds q's
    load and store), an even n, a whole slot in every block, and a tenth of a block's chunk or more resident."""
    plan = sweep_plan(n, G, rl)
    if not 2 <= np_ <= K_RES_MAX or n % 2 or plan is None:
        return False
    return (plan[0] + plan[1]) / max(1, -(-(n // 2) // SLOT) // G) >= 0.1


def sweep_steps(itmax, memory, reorth):
    """Arnoldi steps of a restarted solve whose sweep is one resident launch: 2 to kResMax passes."""
    steps = [k for c in range(0, itmax, memory) for k in range(1, min(memory, itmax - c) + 1)]
    return sum(1 for k in steps if 2 <= (2 * k if reorth else k) <= K_RES_MAX)


# whole = whole slots per block, streamed = whole streamed slots per block at the least (256 blocks, 39 LDS slots)
Case = namedtuple("Case", "nx ny whole rv full streamed precond reorth")
FULL_SHAPES = [(2048, 3520, 55, 16), (2048, 4096, 64, 25), (2048, 4544, 71, 32), (2048, 5568, 87, 48),
               (2048, 6592, 103, 64)]
STREAMED_SHAPES = [(2050, 4093, 63, 16, 8), (2050, 4445, 68, 25, 4), (2050, 5179, 80, 32, 9), (2050, 6139, 95, 48, 8),
                   (2050, 7737, 120, 64, 17)]
FULL_CASES = [Case(nx, ny, whole, rv, True, 0, precond, False) for nx, ny, whole, rv in FULL_SHAPES
              for precond in (False, True)]
STREAMED_CASES = [Case(nx, ny, whole, rv, False, st, False, False) for nx, ny, whole, rv, st in STREAMED_SHAPES]
STREAMED_CASES.insert(2, Case(2050, 4445, 68, 25, False, 4, False, True))  # rv = 25: a 1-slot last register batch
THRESHOLD_BELOW = Case(2048, 4480, 70, 25, False, 6, False, False)  # the last slot count of 25 ...
THRESHOLD_ABOVE = FULL_CASES[4]  # ... and the first of 32 (2048 x 4544, whole 71)
CASES = FULL_CASES + STREAMED_CASES  # test_variant_matches_oracle's; the threshold pair has a test of its own
EDGE_SHAPE = (1024, 1024)  # rv = 0, all of q in the LDS
SUITE_SHAPES = [((1000, 1000), 0), ((1024, 1024), 0), ((2560, 2560), 0), ((2900, 2901), 16), ((4096, 4096), 89)]


def case_id(c):
    return (f"{c.nx}x{c.ny}-rv{c.rv}-{'full' if c.full else 'streamed'}-{'jacobi' if c.precond else 'plain'}"
            f"{'-reorth' if c.reorth else ''}")


def table_holds(G=256):
    """Every case reaches the variant and geometry it names on G blocks; the first one that does not, else None."""
    for c in CASES + [THRESHOLD_BELOW]:
        plan = sweep_plan(c.nx * c.ny, G)
        if plan is None or plan[0] != c.rv or plan[2] != c.full or whole_slots(c.nx * c.ny, G) != c.whole:
            return c, plan
        rv, rl, full, partial, ragged = plan
        if whole_slots(c.nx * c.ny, G) - (rv + rl) < c.streamed:
            return c, plan
        if full and (partial or ragged or c.whole != rv + rl):
            return c, plan
    for c in STREAMED_CASES:
        if not (sweep_plan(c.nx * c.ny, G)[3] and sweep_plan(c.nx * c.ny, G)[4]):
            return c, sweep_plan(c.nx * c.ny, G)
    return None


def test_cases_reach_the_variants_they_name():
    """On 256 blocks with 39 LDS slots: every row of the case tables selects the rv and the geometry it names, the
    existing suite's shapes select 0, 0, 0, 16, 89, and 16, 25, 32, 48 and 64 each run full, full under a
    preconditioner and streamed."""
    assert table_holds(256) is None, table_holds(256)
    for shape, rv in SUITE_SHAPES:
        assert sweep_plan(shape[0] * shape[1])[0] == rv, shape
    assert sweep_plan(2900 * 2901)[2] is False and sweep_plan(4096 * 4096)[2] is True
    # the slab the code comment names as the reason for 25: 4096^2 on two GPUs
    assert sweep_plan(4096 * 2048) == (25, 39, True, False, False)
    for rv in (16, 25, 32, 48, 64):
        got = {(c.full, c.precond) for c in CASES if c.rv == rv}
        assert got >= {(True, False), (True, True), (False, False)}, rv
    assert any(c.reorth for c in STREAMED_CASES)
    # the threshold pair: neighbouring slot counts, different variants, only the upper one full
    lo, hi = THRESHOLD_BELOW, THRESHOLD_ABOVE
    assert (lo.whole + 1, lo.rv, lo.full) == (hi.whole, 25, False) and (hi.rv, hi.full) == (32, True)
    assert sweep_plan(lo.nx * lo.ny)[3:] == (False, False)  # streamed, yet no partial slot and even blocks
    assert len(set(CASES)) == len(CASES) == 16 and THRESHOLD_BELOW not in CASES
    # the pass-count edge: all of q in the LDS, and the step counts its two solves assert
    assert sweep_plan(EDGE_SHAPE[0] * EDGE_SHAPE[1]) == (0, 8, True, False, False)
    assert sweep_steps(12, 8, False) == 10 and sweep_steps(12, 8, True) == 12
    assert sweep_steps(32, 32, True) == 32 and sweep_steps(34, 34, True) == 32


# ----------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


Run = namedtuple("Run", "x stats prof gram sweeps_resident mgs_passes")


def device_solve(ctx, P, u, b, *, memory, itmax, reorth=False, precond=False):
    """Restarted GMRES on the device under the profiling bracket of test_hip_resident.py's solve: x, the stats, the
    mgs_sweep profile entry, the Gram matrix of the last cycle's basis, and what the solve added to path_info()'s
    sweeps_resident / mgs_passes."""
    ctx.prof_reset()
    ctx.prof_enable(1 << 20)  # count launches (time almost none)
    before = ctx.path_info()
    g = ah.Grid.full(P.nx, P.ny)
    ud = ah.DeviceArray.from_numpy(u, g, ctx)
    bd = ah.DeviceArray.from_numpy(b, g, ctx)
    res = ud.zero()
    p = (P.hx, P.hy, P.lam)
    ah.bratu2d_(res, ud, p)
    J = ah.JacobianOperator(ah.bratu2d_, res, ud, p, jv="exact")
    ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=memory))
    ah.krylov_solve_(ws, J, bd, N=ah.jacobi(J) if precond else None, history=True, restart=True,
                     reorthogonalization=reorth, atol=0.0, rtol=0.0, itmax=itmax)
    prof = ctx.prof_read().get("mgs_sweep", {})
    ctx.prof_enable(0)
    after = ctx.path_info()
    x = ws.x.to_numpy()
    nlast = itmax - memory * ((itmax - 1) // memory)  # Arnoldi steps of the last cycle
    V = np.stack([ws.basis(i).to_numpy().ravel() for i in range(nlast)])
    stats = ws.stats
    ws.free()
    return Run(x, stats, prof, V @ V.T, after["sweeps_resident"] - before["sweeps_resident"],
               after["mgs_passes"] - before["mgs_passes"])


def check(ctx, G, P, u, b, *, rv, memory, itmax, reorth=False, precond=False, label=""):
    """One solve and the five assertions of this file, in order; returns the Run."""
    run = device_solve(ctx, P, u, b, memory=memory, itmax=itmax, reorth=reorth, precond=precond)
    x, st = run.x, run.stats
    kw = dict(jv="exact", memory=memory, restart=True, reorthogonalization=reorth, atol=0.0, rtol=0.0, itmax=itmax)
    if precond:
        kw["N"] = ("diag", oc.jacobian_diag(P, u, reciprocal=True))
    print(f"\n{label}: mgs_sweep x {run.prof.get('launches', 0)} = {run.prof.get('kernel', '')!r}, "
          f"sweeps_resident +{run.sweeps_resident}, mgs_passes +{run.mgs_passes}")
    # 1. the variant ran, for every step of two passes or more (a one-pass step takes the chain by design)
    assert run.prof.get("kernel", "").startswith(f"nk::k_mgs_res<{rv},"), run.prof
    assert run.prof["launches"] >= sweep_steps(itmax, memory, reorth) > 0
    # 2. bit for bit in the sweep's own order: a dropped, duplicated or misplaced slot changes the bits
    oc.set_devred(True, cus=G)
    try:
        xr, _, hr = oc.krylov_solve(P, u, b, **kw)
    finally:
        oc.set_devred(False)
    np.testing.assert_array_equal(np.array(st.residuals), hr)
    np.testing.assert_array_equal(x, xr)
    # 3. the plain-order oracle: the same MGS arithmetic per element, only the order of the partial sums differs
    xo, sto, ho = oc.krylov_solve(P, u, b, **kw)
    assert st.niter == sto["niter"] == itmax and st.n_matvec == sto["n_matvec"]
    print(f"  history vs plain order {np.max(np.abs(np.array(st.residuals) / ho - 1.0)):.2e}, "
          f"x {np.max(np.abs(x - xo)) / np.max(np.abs(xo)):.2e}")
    np.testing.assert_allclose(np.array(st.residuals), ho, rtol=1e-9, atol=0)
    assert np.max(np.abs(x - xo)) <= 1e-9 * np.max(np.abs(xo))
    # 4. the true residual of the device's x, by the host's Jv: no reduction mirror, no device Jv
    est = st.residuals[-1]
    true = float(np.linalg.norm(b - oc.jv_exact(P, u, x)))
    print(f"  | ||b - J x|| - estimate | / estimate {abs(true - est) / est:.2e}")
    assert abs(true - est) <= 1e-12 * est
    # 5. the last cycle's basis is orthonormal
    print(f"  max |G - I| over {len(run.gram)} vectors {np.max(np.abs(run.gram - np.eye(len(run.gram)))):.2e}")
    assert np.max(np.abs(run.gram - np.eye(len(run.gram)))) <= 1e-12
    return run


def problem(nx, ny):
    P = oc.bratu2d(nx, ny)
    u = oc.sin_ic(P)
    return P, u, oc.residual(P, u)


@pytest.fixture(scope="module")
def edge(ctx):
    """The 1024^2 problem after a first resident sweep on it, and the blocks of the sweep's grid (path_info()'s
    resident_blocks is 0 until a sweep ran).  On 256 blocks every case's plan holds: none may skip."""
    P, u, b = problem(*EDGE_SHAPE)
    run = device_solve(ctx, P, u, b, memory=8, itmax=3)
    assert run.sweeps_resident >= 2, "the resident MGS sweep did not run"
    G = ctx.path_info()["resident_blocks"]
    assert G > 0
    if G == 256:
        assert table_holds(G) is None, table_holds(G)
    return G, P, u, b


def plan_or_skip(c, G):
    plan = sweep_plan(c.nx * c.ny, G)
    if plan is None or plan[0] != c.rv or plan[2] != c.full:
        pytest.skip(f"{G} blocks: {c.nx} x {c.ny} plans (rv, rl, full, partial, ragged) = {plan}, not rv = {c.rv}, "
                    f"full = {c.full}")
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_variant_matches_oracle(ctx, edge, case):
    """2D Bratu, exact Jv, 12 restarted GMRES(8) steps (the residual barely moves: no step reaches the rounding
    floor): the variant the case names ran, and the five assertions of `check`."""
    G = edge[0]
    plan_or_skip(case, G)
    P, u, b = problem(case.nx, case.ny)
    check(ctx, G, P, u, b, rv=case.rv, memory=8, itmax=12, reorth=case.reorth, precond=case.precond,
          label=case_id(case))


@pytest.mark.gpu
def test_selection_threshold(ctx, edge):
    """One slot more per block and the next variant runs: 2048 x 4480 (70 slots, rv = 25 + 6 streamed) against
    2048 x 4544 (71 slots, rv = 32, full; its results are test_variant_matches_oracle's).  The lower shape streams
    six slots per block with no partial slot and even blocks: the five assertions of `check` there as well."""
    G = edge[0]
    lo, hi = THRESHOLD_BELOW, THRESHOLD_ABOVE
    plan_or_skip(lo, G)
    plan_or_skip(hi, G)
    P, u, b = problem(hi.nx, hi.ny)
    run = device_solve(ctx, P, u, b, memory=8, itmax=12)
    print(f"\n{case_id(hi)}: {run.prof.get('kernel', '')!r}")
    assert run.prof.get("kernel", "").startswith(f"nk::k_mgs_res<{hi.rv},"), run.prof
    assert run.prof["launches"] >= sweep_steps(12, 8, False)
    P, u, b = problem(lo.nx, lo.ny)
    check(ctx, G, P, u, b, rv=lo.rv, memory=8, itmax=12, label=case_id(lo))


@pytest.mark.gpu
def test_sweep_of_exactly_kresmax_passes(ctx, edge):
    """GMRES(32) with reorthogonalisation, 32 steps: step 32 is a sweep of 64 = kResMax passes (ResArgs::V's last
    entry, the tag range); every step is resident, none takes the per-pass chain."""
    G, P, u, b = edge
    run = check(ctx, G, P, u, b, rv=0, memory=32, itmax=32, reorth=True, label="1024x1024-kresmax")
    assert run.sweeps_resident >= 32 and run.mgs_passes == 0


@pytest.mark.gpu
def test_cycle_across_kresmax_passes(ctx, edge):
    """GMRES(34) with reorthogonalisation, 34 steps: steps 33 and 34 have 66 and 68 passes and take the per-pass
    chain in mid-cycle; still bit for bit with the oracle in device order, which has the same rule."""
    G, P, u, b = edge
    run = check(ctx, G, P, u, b, rv=0, memory=34, itmax=34, reorth=True, label="1024x1024-across-kresmax")
    assert run.sweeps_resident >= 32 and run.mgs_passes > 0
