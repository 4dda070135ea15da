"""The multigrid V-cycle on periodic grids, on the device (periodic=True; csrc/nk_mg.hip's PER instantiations and the
k_mg_restrict_p / k_mg_prolong_p transfers; DESIGN.md §10 "Periodic grids").

The references, cases and recorded sensitivities are tests/test_mg_periodic_cpu.py's: the numpy restatement `PerCycle`
and the dense long-double matrix recursion.  Tolerance: the recorded float64-versus-long-double sensitivity of the
reference x 16, as in the other multigrid files; no constant comes from device output.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from ariadne_hip import _lib
from oracle import oracle as oc

from test_hip_multigrid import ALPHA, gmres_right, krylov, rel
from test_mg_periodic_cpu import (CYCLE_CASES, DENSE_CASES, DENSE_IDS, PER_CYCLE_SENSITIVITY, PER_DENSE_SENSITIVITY, SOLVER_2D,
                                  SOLVER_3D, PerCycle, case_id, coefficient_case, dense_reference, jv_per, options, per_problem,
                                  per_reference, plan_per, restated_solve)

DENSE_TOL = 16 * PER_DENSE_SENSITIVITY
TOL = 16 * PER_CYCLE_SENSITIVITY

RESIDUALS = {"heat2d_euler": ah.heat2d_euler_, "heat2d_midpoint": ah.heat2d_midpoint_.with_alpha(ALPHA),
             "heat2d_trapezoid": ah.heat2d_trapezoid_, "heat3d_euler": ah.heat3d_euler_,
             "heat3d_midpoint": ah.heat3d_midpoint_.with_alpha(ALPHA), "heat3d_trapezoid": ah.heat3d_trapezoid_}


@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


def device_operator(kind, P, u0, jv="exact"):
    """the periodic heat problem on the device: its JacobianOperator at u0 (res = F(u0))"""
    u = ah.DeviceArray.from_numpy(u0)
    res = u.zero()
    un = ah.DeviceArray.from_numpy(P.un)
    sp = (P.a, P.hx, P.hy, ah.bc_periodic_) if P.dim == 2 else (P.a, P.hx, P.hy, P.hz, ah.bc_periodic_)
    p = (un, P.dt, u.zero(), sp, 0.0)
    f = RESIDUALS[kind]
    f(res, u, p)
    return ah.JacobianOperator(f, res, u, p, jv=jv)


def case_operator(c):
    ref = per_reference(c)
    return device_operator(c.kind, ref[0], ref[1]), ref


def dev(a):
    return ah.DeviceArray.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------ the cycle
@pytest.mark.gpu
@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_device_matrix_matches_dense_form(ctx, case):
    """unit vector by unit vector against the long-double matrix recursion; these grids are in the tail (its PER form),
    and the SPD form and vcycle_dot run its OUT = 1 / 2 closing forms on the same columns"""
    shape, skind, nu, cs = case
    h, k, s, V, _ = dense_reference(case)
    grid = ah.Grid.full(*shape)
    sd = dev(s) if skind == "var" else s
    mg = ah.MultigridPreconditioner.from_coefficients(grid, k, sd, h=h, nu=nu, coarse_sweeps=cs, periodic=True)
    assert mg.levels == plan_per(shape)
    n = int(np.prod(shape))
    z = ah.DeviceArray(grid, ctx)
    cols, cols_spd, cols_dot = [], [], []
    for j in range(n):
        unit = np.zeros(n)
        unit[j] = 1.0
        ej = dev(unit.reshape(tuple(reversed(shape))))
        mg.spd = False
        cols.append(mg.vcycle(ej, z=z).to_numpy().reshape(-1).copy())
        if j % 7 == 0:
            mg.spd = True
            cols_spd.append((j, mg.vcycle(ej, z=z).to_numpy().reshape(-1).copy()))
            zd, vz = mg.vcycle_dot(ej, z=z)
            cols_dot.append((j, zd.to_numpy().reshape(-1).copy(), vz))
    M = np.stack(cols, axis=1)
    err = rel(M, V)
    print(f"{case}: device matrix vs dense long double V {float(err):.3e} (allowed {DENSE_TOL:.1e})")
    assert err <= DENSE_TOL
    for (j, zs), (_, zdot, vz) in zip(cols_spd, cols_dot):
        np.testing.assert_array_equal(zs, -M[:, j])  # the diagonal is negative: sigma = -1
        np.testing.assert_array_equal(zdot, zs)
        assert vz == zs[j]  # <e_j, z>: one non-zero product


@pytest.mark.gpu
@pytest.mark.parametrize("case", CYCLE_CASES, ids=[case_id(c) for c in CYCLE_CASES])
def test_vcycle_matches_restatement(ctx, case):
    J, ref = case_operator(case)
    v, cyc, zref = ref[5], ref[6], ref[7]
    mg = ah.MultigridPreconditioner(J, periodic=True, **options(case))
    assert mg.levels == cyc.levels == plan_per(case.shape, case.max_levels)
    z = mg.apply(J, dev(v)).to_numpy()
    err = rel(z, zref)
    print(f"{case_id(case)} {mg.levels}: device vs restatement {err:.3e} (allowed {TOL:.1e})")
    assert err <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", CYCLE_CASES[:5], ids=[case_id(c) for c in CYCLE_CASES[:5]])
def test_level0_operator_is_the_jacobian(ctx, case):
    """one level, ω = 1.  One sweep from zero: z1 = v ./ diag(A_0), bitwise jacobian_diag's.  Two sweeps:
    z2 = (v - off(z1)) ./ diag with off = A_0 - diag, so diag .* (z2 - z1) is the residual v - A_0 z1 of the known
    x = z1, held against the periodic Jacobian's own product (mul_)"""
    J, ref = case_operator(case)
    P, u0, v = ref[0], ref[1], ref[5]
    mg = ah.MultigridPreconditioner(J, coarse_sweeps=1, omega=1.0, max_levels=1, periodic=True)
    assert mg.levels == [tuple(case.shape)]
    idg = ah.jacobian_diag(J, reciprocal=True).to_numpy()
    z1 = mg.apply(J, dev(v)).to_numpy()
    np.testing.assert_array_equal(z1, idg * v)
    np.testing.assert_array_equal(z1, oc.jacobian_diag(P, u0, reciprocal=True) * v)
    # the residual of a known x = z1: the second sweep is z2 = 0 z1 + 1 (idg (v - off(z1))), so
    # v - A_0 z1 = v - off(z1) - diag z1 = diag (z2 - z1)
    mg2 = ah.MultigridPreconditioner(J, coarse_sweeps=2, omega=1.0, max_levels=1, periodic=True)
    z2 = mg2.apply(J, dev(v)).to_numpy()
    dg = ah.jacobian_diag(J).to_numpy()
    out = J.u.zero()
    ah.mul_(out, J, dev(z1))
    want = v - out.to_numpy()
    got = dg * (z2 - z1)
    scale = np.max(np.abs(dg)) * np.max(np.abs(z1))  # the size of the terms that cancel in v - A z1
    assert np.max(np.abs(got - want)) <= 16 * np.finfo(np.float64).eps * scale


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CYCLE_CASES[0], CYCLE_CASES[1], CYCLE_CASES[4], CYCLE_CASES[5], CYCLE_CASES[8]],
                         ids=[case_id(c) for c in (CYCLE_CASES[0], CYCLE_CASES[1], CYCLE_CASES[4], CYCLE_CASES[5], CYCLE_CASES[8])])
def test_deterministic_linear_and_in_place(ctx, case):
    J, ref = case_operator(case)
    rng = np.random.default_rng(3)
    v, w = ref[5], rng.standard_normal(ref[5].shape)
    al, be = 0.7, -1.3
    mg = ah.MultigridPreconditioner(J, periodic=True, **options(case))
    app = lambda q: mg.apply(J, dev(q)).to_numpy()  # noqa: E731
    zv, zw = app(v), app(w)
    np.testing.assert_array_equal(zv, app(v))
    np.testing.assert_array_equal(zw, app(w))
    assert rel(app(al * v + be * w), al * zv + be * zw) <= TOL
    x = dev(v)
    mg.vcycle(x, z=x)
    np.testing.assert_array_equal(x.to_numpy(), zv)


@pytest.mark.gpu
def test_from_coefficients_and_set_coefficients(ctx):
    shape, h, k, s, v, cyc, zref = coefficient_case()
    grid = ah.Grid.full(*shape)
    mg = ah.MultigridPreconditioner.from_coefficients(grid, k, dev(s), periodic=True)  # the default spacings 1 / n
    assert mg.levels == cyc.levels == plan_per(shape)
    z = mg.vcycle(dev(v)).to_numpy()
    err = rel(z, zref)
    print(f"from_coefficients {shape}: device vs restatement {err:.3e} (allowed {TOL:.1e})")
    assert err <= TOL
    # other coefficients on the live hierarchy, then these again: a fresh hierarchy's bits
    mg.set_coefficients([0.3, 0.2], -2.0)
    fresh = ah.MultigridPreconditioner.from_coefficients(grid, [0.3, 0.2], -2.0, periodic=True)
    np.testing.assert_array_equal(mg.vcycle(dev(v)).to_numpy(), fresh.vcycle(dev(v)).to_numpy())
    assert rel(mg.vcycle(dev(v)).to_numpy(), PerCycle(shape, h, [0.3, 0.2], -2.0).vcycle(v)) <= TOL
    mg.set_coefficients(k, dev(s))
    np.testing.assert_array_equal(mg.vcycle(dev(v)).to_numpy(), z)
    # update(J) on a live hierarchy against a fresh one (J of the carrier kind, heat2d_euler_, on the same spacings)
    P, u0, _, _, hJ = per_problem("heat2d_euler", shape)
    J = device_operator("heat2d_euler", P, u0)
    live = ah.MultigridPreconditioner.from_coefficients(grid, k, dev(s), h=hJ, periodic=True)
    live.update(J)
    np.testing.assert_array_equal(live.vcycle(dev(v)).to_numpy(), ah.MultigridPreconditioner(J, periodic=True).vcycle(dev(v)).to_numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CYCLE_CASES[0], CYCLE_CASES[3], CYCLE_CASES[5], CYCLE_CASES[7], CYCLE_CASES[8]],
                         ids=[case_id(c) for c in (CYCLE_CASES[0], CYCLE_CASES[3], CYCLE_CASES[5], CYCLE_CASES[7], CYCLE_CASES[8])])
def test_spd_form_and_vcycle_dot(ctx, case):
    J, ref = case_operator(case)
    v = ref[5]
    mg = ah.MultigridPreconditioner(J, periodic=True, **options(case))
    z = mg.vcycle(dev(v)).to_numpy()
    mg.spd = True
    zs = mg.vcycle(dev(v)).to_numpy()
    np.testing.assert_array_equal(zs, -z)  # sigma = -1: J is negative definite
    zd, vz = mg.vcycle_dot(dev(v))
    np.testing.assert_array_equal(zd.to_numpy(), zs)
    prod = (v * zs).reshape(-1)
    exact, bound = math.fsum(prod), prod.size * 2.0 ** -53 * math.fsum(np.abs(prod))
    print(f"{case_id(case)}: <v, z> {vz:.17g}, fsum {exact:.17g}, |diff| {abs(vz - exact):.3e} (allowed {bound:.3e})")
    assert abs(vz - exact) <= bound and vz > 0.0
    mg.spd = False
    zd0, vz0 = mg.vcycle_dot(dev(v))
    np.testing.assert_array_equal(zd0.to_numpy(), z)
    assert abs(vz0 + exact) <= bound


# ------------------------------------------------------------------------------------ solvers
@pytest.mark.gpu
def test_preconditioned_gmres_on_periodic_heat(ctx):
    kind, shape = SOLVER_2D
    P, u0, k, b, xref, it_ref, ok_ref, it0_ref, _, cyc = restated_solve(SOLVER_2D)
    assert ok_ref
    J = device_operator(kind, P, u0)
    A = lambda q: jv_per(P, k, q)  # noqa: E731
    # the unpreconditioned device solve: GMRES(30) does not get there within krylov()'s itmax of 60 (the restatement
    # neither, within 200), so the solution to compare with is unpreconditioned CG's (J is symmetric)
    _, st30 = krylov(J, J.res, "gmres")
    assert not st30.solved and st30.niter == 60
    ws = ah.krylov_workspace("cg", ah.KrylovConstructor(J.res))
    ah.krylov_solve_(ws, J, J.res, itmax=5000, atol=0.0, rtol=1e-8)
    x0, st0 = ws.x.to_numpy(), ws.stats
    ws.free()
    assert st0.solved and np.linalg.norm(b - A(x0)) <= 1e-7 * np.linalg.norm(b)
    mg = ah.MultigridPreconditioner(J, periodic=True)
    for algo in ("gmres", "fgmres"):
        x, st = krylov(J, J.res, algo, N=mg)
        print(f"{algo} N: niter {st.niter} (numpy {it_ref}); unpreconditioned CG {st0.niter} (numpy GMRES(30) at itmax 200: {it0_ref})")
        assert st.solved and abs(st.niter - it_ref) <= 1
        assert np.linalg.norm(b - A(x)) <= 1e-7 * np.linalg.norm(b)
        # x - x0 = J^-1 (r0 - r) and ||J^-1|| = 1 (the smallest eigenvalue in size is -1, the constant mode's), so
        # ||x - x0|| <= ||r|| + ||r0||, with the true residuals of the two device solutions
        r, r0 = np.linalg.norm(b - A(x)), np.linalg.norm(b - A(x0))
        print(f"  ||x - x0|| {np.linalg.norm(x - x0):.3e} (allowed ||r|| + ||r0|| = {r + r0:.3e}; ||b|| {np.linalg.norm(b):.3e})")
        assert np.linalg.norm(x - x0) <= r + r0
        assert 4 * st.niter <= st0.niter
    Mh = cyc.vcycle
    _, it_left, ok_left = gmres_right(lambda q: Mh(A(q)), lambda q: q, Mh(b), 1e-8)
    assert ok_left
    x, st = krylov(J, J.res, "gmres", M=mg)
    pre = np.linalg.norm(Mh(b - A(x))) / np.linalg.norm(Mh(b))
    print(f"left M: niter {st.niter} (numpy {it_left}), ||M r|| / ||M b|| {pre:.2e}")
    assert st.solved and abs(st.niter - it_left) <= 1 and pre <= 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["cg", "minres"])
def test_spd_form_in_cg_and_minres(ctx, algo):
    kind, shape = SOLVER_3D
    P, u0, k, b, xref, it_ref, ok_ref, _, _, _ = restated_solve(SOLVER_3D)
    J = device_operator(kind, P, u0)
    A = lambda q: jv_per(P, k, q)  # noqa: E731

    def run(**kw):
        ws = ah.krylov_workspace(algo, ah.KrylovConstructor(J.res))
        ah.krylov_solve_(ws, J, J.res, atol=0.0, rtol=1e-8, itmax=400, **kw)
        out = (ws.x.to_numpy(), ws.stats)
        ws.free()
        return out

    x, st = run(M=ah.multigrid(spd=True, periodic=True))
    x0, st0 = run()
    true = np.linalg.norm(b - A(x)) / np.linalg.norm(b)
    print(f"{algo} with M: niter {st.niter}, without {st0.niter}; restated GMRES {it_ref}; ||b - J x|| / ||b|| {true:.2e}")
    assert st.solved and st0.solved and st.niter < st0.niter
    assert true <= 1e-6  # (the stopping test is on the M-norm of the residual)
    assert np.linalg.norm(x - x0) <= 2e-6 * np.linalg.norm(b)
    with pytest.raises(NotImplementedError, match=algo):
        run(M=ah.multigrid(periodic=True))  # the default form stays refused


@pytest.mark.gpu
def test_newton_drivers_on_a_stiff_midpoint_step(ctx):
    P, u0, k, s, h = per_problem("heat2d_midpoint", (96, 48))
    f = RESIDUALS["heat2d_midpoint"]
    sp = (P.a, P.hx, P.hy, ah.bc_periodic_)

    def p_of():
        return (dev(P.un), P.dt, dev(np.zeros(P.shape)), sp, 0.0)

    fac = ah.multigrid(periodic=True)
    u, r = ah.newton_krylov_(f, dev(P.un), p_of(), N=fac, memory=30)
    u_plain, r0 = ah.newton_krylov_(f, dev(P.un), p_of(), memory=30)
    print(f"Newton midpoint 96x48: with N outer {r.stats.outer_iterations} inner {r.stats.inner_iterations}; "
          f"plain outer {r0.stats.outer_iterations} inner {r0.stats.inner_iterations}")
    assert r.solved and fac.mg is not None and fac.mg.periodic
    assert r.stats.inner_iterations < r0.stats.inner_iterations
    un, rn = ah.newton_krylov_native(f, dev(P.un), p_of(), N=ah.multigrid(periodic=True), memory=30)
    assert rn.solved and rn.stats[:2] == r.stats[:2]
    np.testing.assert_allclose(un.to_numpy(), u.to_numpy(), rtol=0, atol=1e-9 * np.abs(u.to_numpy()).max())
    fac.free()


@pytest.mark.gpu
def test_solve_over_three_steps(ctx):
    P, u0, k, s, h = per_problem("heat2d_trapezoid", (96, 48))
    sp = (P.a, P.hx, P.hy, ah.bc_periodic_)
    ts = [0.0, P.dt, 2 * P.dt, 3 * P.dt]
    with_mg, plain = [], []
    ua = ah.solve(ah.G_Trapezoid_, ah.diffusion_, dev(P.un), sp, P.dt, ts, N=ah.multigrid(periodic=True), stats_out=with_mg,
                  memory=30)
    ub = ah.solve(ah.G_Trapezoid_, ah.diffusion_, dev(P.un), sp, P.dt, ts, stats_out=plain, memory=30,
                  krylov_kwargs=dict(itmax=400, restart=True))
    inner = [r.stats.inner_iterations for r in with_mg], [r.stats.inner_iterations for r in plain]
    print(f"solve, 3 trapezoid steps: inner with N {inner[0]}, without {inner[1]}")
    assert len(with_mg) == 3 and all(r.solved for r in with_mg) and all(r.solved for r in plain)
    assert sum(inner[0]) < sum(inner[1])
    # The problem is linear: a step that stops at the residual F is J^-1 F away from the exact step, and ||J^-1|| = 1 (the
    # constant mode has the eigenvalue -1, every other one is larger in size); the trapezoid step map does not amplify
    # (||(I - k L)^-1 (I + k L)|| <= 1).  So the two runs differ by at most the sum of their final residual norms.
    bound = sum(r.stats.n_res for r in with_mg) + sum(r.stats.n_res for r in plain)
    diff = float(np.linalg.norm(ua.to_numpy() - ub.to_numpy()))
    print(f"  ||u_N - u_plain|| {diff:.3e} (allowed: the sum of the six final ||F|| {bound:.3e})")
    assert diff <= bound


# ------------------------------------------------------------------------------------ the C ABI
@pytest.mark.gpu
def test_c_abi(ctx):
    lib = ah.load()
    h = C.c_void_p()

    def err():
        return (lib.nk_last_error(ctx.handle) or b"").decode()

    heat = _lib.nk_problem(_lib.NK_HEAT2D_TRAPEZOID, _lib.NK_BC_PERIODIC, 96, 48, 1, 1.0 / 96, 1.0 / 48, 1.0, 0.0, 0.01, 0.1, 8)
    assert lib.nk_mg_create(ctx.handle, C.byref(heat), None, C.byref(h)) == 0, err()
    ext, n = (C.c_int64 * (3 * 64))(), C.c_int32(0)
    assert lib.nk_mg_level_extents(h, ext, 64, C.byref(n)) == 0
    assert [(int(ext[3 * l]), int(ext[3 * l + 1])) for l in range(n.value)] == plan_per((96, 48))
    assert all(int(ext[3 * l + 2]) == 1 for l in range(n.value))
    v = ah.DeviceArray(ah.Grid.full(96, 48), ctx)
    assert lib.nk_mg_apply(h, v.ptr, v.ptr) == _lib.NK_E_STATE  # no operator yet
    # the "same geometry" check takes the hierarchy's own bc, and only that
    heat0 = _lib.nk_problem(_lib.NK_HEAT2D_TRAPEZOID, _lib.NK_BC_ZERO, 96, 48, 1, 1.0 / 96, 1.0 / 48, 1.0, 0.0, 0.01, 0.1, 8)
    assert lib.nk_mg_set_jacobian(h, C.byref(heat0), v.ptr) == _lib.NK_E_ARG and "does not match" in err()
    assert lib.nk_mg_set_jacobian(h, C.byref(heat), v.ptr) == 0, err()
    assert lib.nk_mg_destroy(h) == 0
    lv = (C.c_int64 * 6)(96, 48, 1, 48, 24, 1)
    rc = lib.nk_mg_create_levels(ctx.handle, C.byref(heat), None, lv, 2, C.byref(h))
    assert rc == _lib.NK_E_ARG and "periodic" in err()
    bratu = _lib.nk_problem(_lib.NK_BRATU2D, _lib.NK_BC_PERIODIC, 96, 48, 1, 1.0 / 96, 1.0 / 48, 1.0, 3.5, 0.0, 0.0, 1)
    rc = lib.nk_mg_create(ctx.handle, C.byref(bratu), None, C.byref(h))
    assert rc == _lib.NK_E_ARG and "periodic" in err()
    ign = _lib.nk_problem(_lib.NK_IGNITION2D_EULER, _lib.NK_BC_PERIODIC, 96, 48, 1, 1.0 / 96, 1.0 / 48, 1.0, 1.0, 0.01, 0.1, 8)
    rc = lib.nk_mg_create(ctx.handle, C.byref(ign), None, C.byref(h))
    assert rc == _lib.NK_E_ARG and "periodic" in err()
