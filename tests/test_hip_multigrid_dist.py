"""The multigrid V-cycle on slab-distributed grids (distributed=True; nk_mg_create on a distributed context,
nk_mg_plan_slabs; DESIGN.md §10 "Slab-distributed hierarchy").

By definition the distributed cycle is the one-rank cycle of the global grid with max_levels = L_d, the number of
levels the local slab extent can be halved through -- so the GPU tests hold the gathered result of the ranks
(tests/mg_dist_worker.py, the mailbox transport, ranks sharing device 0 where the box has one GPU) to the one-rank
device cycle of this process BIT FOR BIT, and to the numpy restatement of tests/test_hip_multigrid.py within 16 x its own
float64-vs-longdouble sensitivity.  CPU tests: the plan against a restatement of the rule, the one-ghost-plane ownership
property the slab kernels rely on, acceptance and refusals of distributed=True on device-less operators, the names.
"""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from ariadne_hip import _lib
from oracle import oracle as oc

import test_hip_multigrid as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mg_dist_worker.py")
RTOL = 1e-8

# name -> (kind, global shape (x fastest, slab axis last), ranks): the smallest shapes at which the slab logic can go
# wrong -- two ranks, an odd rank count with a middle rank, one row per rank on the coarsest level, z-slabs down to one plane
CASES = {"bratu-2": ("bratu2d", (24, 24), 2), "bratu-3": ("bratu2d", (40, 36), 3), "bratu-8": ("bratu2d", (48, 64), 8),
         "heat3d-2": ("heat3d_midpoint", (20, 24, 16), 2), "newton-4": ("bratu2d", (64, 96), 4)}
LEVELS = {"bratu-2": 3, "bratu-3": 3, "bratu-8": 4, "heat3d-2": 4, "newton-4": 4}
VCYCLE_CASES = ["bratu-2", "bratu-3", "bratu-8", "heat3d-2"]

# max over VCYCLE_CASES and the truncation case of max|float64 - longdouble| / max|longdouble| of one V-cycle of the
# restatement with max_levels = L_d (measured on the CPU: 2.03e-16, 2.22e-16, 3.40e-16, 1.70e-16; truncation 2.89e-16;
# test_restatement_sensitivity_of_the_cut_cycles_is_as_recorded measures it again).  The project's rule
# (test_hip_multigrid.py): the device may differ from the restatement by 16 x that.
SENSITIVITY = 3.4e-16
TOL = 16 * SENSITIVITY


def slab_levels(local, nranks, max_levels=0):
    """the rule: the one-rank plan of the global grid, cut after L_d levels (level l + 1 exists only while the local
    slab extent m_l is even), in local extents"""
    glob = tuple(local[:-1]) + (nranks * local[-1],)
    ld, m = 1, local[-1]
    while m % 2 == 0:
        ld, m = ld + 1, m // 2
    if max_levels:
        ld = min(ld, max_levels)
    lv = tm.plan(glob, ld)
    assert len(lv) == ld and all(e[-1] % nranks == 0 for e in lv)
    return [tuple(e[:-1]) + (e[-1] // nranks,) for e in lv]


def case_vectors(P, u0):
    """(v, a second v, another u) of a case, seeded: the same in the workers and in the pytest process"""
    v = np.random.default_rng(11).standard_normal(P.shape)  # = test_hip_multigrid.reference's v
    v2 = np.random.default_rng(13).standard_normal(P.shape)
    u2 = u0 + 0.1 * np.random.default_rng(21).standard_normal(P.shape)
    return v, v2, u2


def truncation_problem():
    """(shape, h, k, s, v): on the fourth level (9 x 8) of 72 x 64 only global row 6 (0-based) has positive diagonal
    entries -- in rank 1's slab of two; rank 0's rows are all negative there.  The restatement keeps 3 of the 6 levels."""
    shape = (72, 64)
    h = [1.0 / (n + 1) for n in shape]
    x, y = np.arange(1, 73) * h[0], np.arange(1, 65) * h[1]
    s = 150.0 + 300.0 * np.exp(-((y - 0.75) / 0.12) ** 2)[:, None] * np.exp(-((x - 0.5) / 0.2) ** 2)[None, :]
    return shape, h, [1.0, 1.0], s, np.random.default_rng(12).standard_normal(s.shape)


def heat_start(P):
    return oc.sin_ic(P) + 0.05 * np.random.default_rng(5).standard_normal(P.shape)


# ------------------------------------------------------------------------------------ CPU tests
def plan_slabs(local, nranks, max_levels=0):
    """nk_mg_plan_slabs itself: (return code, levels)"""
    n = (C.c_int64 * 3)(*(list(local) + [1, 1])[:3])
    ext, nl = (C.c_int64 * (3 * 64))(), C.c_int32(0)
    rc = ah.load().nk_mg_plan_slabs(n, nranks, max_levels, ext, 64, C.byref(nl))
    return rc, [tuple(int(ext[3 * l + a]) for a in range(len(local))) for l in range(nl.value)] if rc == 0 else None


def test_plan_slabs_matches_the_rule():
    rc, lv = plan_slabs((48, 8), 8)
    assert rc == 0 and lv == [(48, 8), (24, 4), (12, 2), (6, 1)] == slab_levels((48, 8), 8)
    rc, lv = plan_slabs((40, 12), 3)
    assert rc == 0 and lv == [(40, 12), (20, 6), (10, 3)] == slab_levels((40, 12), 3)
    rc, lv = plan_slabs((20, 24, 8), 2)
    assert rc == 0 and lv == slab_levels((20, 24, 8), 2) and len(lv) == 4
    assert [e[:2] + (2 * e[2],) for e in lv] == tm.plan((20, 24, 16))  # here the cut plan is the full one-rank plan
    for name in CASES:
        kind, shape, R = CASES[name]
        local = shape[:-1] + (shape[-1] // R,)
        assert plan_slabs(local, R) == (0, slab_levels(local, R)) and len(slab_levels(local, R)) == LEVELS[name]
        assert ah.multigrid_plan(local, nranks=R) == slab_levels(local, R)
    # other shapes: large local extents, axes that stop at 3 points, max_levels
    for local, R in [((4096, 512), 8), ((130, 40), 5), ((7, 64), 2), ((3, 3, 32), 4), ((17, 13, 6), 3)]:
        for ml in (0, 1, 2, 3, 9):
            assert plan_slabs(local, R, ml) == (0, slab_levels(local, R, ml)), (local, R, ml)
            assert ah.multigrid_plan(local, ml, nranks=R) == slab_levels(local, R, ml)
    assert len(slab_levels((4096, 512), 8)) == 10
    assert plan_slabs((48, 8), 8, 2) == (0, [(48, 8), (24, 4)])
    # refusals: an odd local slab extent, a 1D grid, fewer than 2 ranks, bad arguments
    E = _lib.NK_E_ARG
    assert plan_slabs((48, 7), 8)[0] == E and plan_slabs((20, 24, 9), 2)[0] == E
    assert plan_slabs((48,), 2)[0] == E and plan_slabs((48, 8), 1)[0] == E and plan_slabs((48, 8), 0)[0] == E
    assert plan_slabs((48, 8), 2, -1)[0] == E and plan_slabs((0, 8), 2)[0] == E
    with pytest.raises(NotImplementedError, match="odd number of planes"):
        ah.multigrid_plan((48, 7), nranks=8)
    with pytest.raises(NotImplementedError, match="semi"):
        ah.multigrid_plan((48, 8), nranks=8, coarsening="semi")


def test_one_ghost_plane_is_enough_for_equal_slabs():
    """Rank r owns fine rows r m_f + 1 .. (r + 1) m_f and coarse rows r m_c + 1 .. (r + 1) m_c (1-based, global,
    m_c = m_f / 2).  With the transfer stencils of the GLOBAL extents (the kernels' integer formulas: mg_rax_t,
    mg_pax_t), every fine row a coarse row of rank r gathers lies in r m_f .. (r + 1) m_f + 1 and every coarse row a
    fine row interpolates from in r m_c .. (r + 1) m_c + 1: exhaustively for 2 <= ranks <= 16 and even m_f <= 64."""
    for R in range(2, 17):
        for mf in range(2, 65, 2):
            mc, nf, nc = mf // 2, R * mf, R * (mf // 2)
            F, Cc = nf + 1, nc + 1
            J = np.arange(1, nc + 1)
            lo = np.maximum(((J - 1) * F) // Cc + 1, 1)  # mg_rax_t
            hi = np.minimum(np.minimum(((J + 1) * F - 1) // Cc, nf), lo + 3)
            r = (J - 1) // mc
            assert np.all(lo >= r * mf) and np.all(hi <= (r + 1) * mf + 1), (R, mf)
            assert np.all(lo <= hi)
            I = np.arange(1, nf + 1)
            j = (I * Cc) // F  # mg_pax_t: coarse rows j and j + 1 (1-based; 0 and n_c + 1 are the boundary)
            r = (I - 1) // mf
            assert np.all(j >= r * mc) and np.all(j + 1 <= (r + 1) * mc + 1), (R, mf)


def test_restatement_sensitivity_of_the_cut_cycles_is_as_recorded():
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    worst = 0.0
    for name in VCYCLE_CASES:
        kind, shape, R = CASES[name]
        P, u0, k, s, h = tm.host_problem(kind, shape)
        v = case_vectors(P, u0)[0]
        z64, zl = (tm.Cycle(shape, h, k, s, max_levels=LEVELS[name], dt=dt).vcycle(v) for dt in (np.float64, np.longdouble))
        worst = max(worst, float(np.max(np.abs(z64 - zl)) / np.max(np.abs(zl))))
    shape, h, k, s, v = truncation_problem()
    cyc = tm.Cycle(shape, h, k, s, max_levels=6)
    assert cyc.levels == tm.plan(shape)[:3] and len(slab_levels((72, 32), 2)) == 6  # 3 of 6 levels
    zl = tm.Cycle(shape, h, k, s, max_levels=6, dt=np.longdouble).vcycle(v)
    worst = max(worst, float(np.max(np.abs(cyc.vcycle(v) - zl)) / np.max(np.abs(zl))))
    print(f"restatement float64 vs longdouble on the cut cycles: {worst:.3e}")
    assert SENSITIVITY / 1.5 <= worst <= 1.5 * SENSITIVITY
    # the finding behind the truncation case: on the fourth level only global row 6 (0-based; rank 1 owns rows 4 .. 7)
    # has positive diagonal entries, so rank 0 alone would keep the level
    full = tm.Cycle(shape, h, k, s, max_levels=3)
    s3 = full.s[2]
    for a in range(2):
        s3 = tm.along(tm.transfers(full.levels[2][a], full.levels[2][a] // 2, np.float64)[1], s3, a)
    d3 = s3 - 2 * sum(1.0 / (1.0 / (n + 1)) ** 2 for n in (9, 8))
    assert s3.shape == (8, 9) and sorted(set(np.nonzero(d3 > 0)[0])) == [6] and np.all(d3[:4] < 0) and np.any(d3[4:] < 0)


def test_distributed_flag_acceptance_and_refusals_need_no_device():
    bratu_p = lambda u: (0.1, 0.1, 3.5)  # noqa: E731
    heat_p = lambda bc: (lambda u: (u, 0.1, u, (0.01, 0.1, 0.1, bc), 0.0))  # noqa: E731
    fake, MG = tm.fake_operator, ah.MultigridPreconditioner
    ctx2 = types.SimpleNamespace(nranks=2, handle=None)
    # the default still refuses, and says how to ask for it
    for args in ((ah.bratu2d_, ah.Grid.full(16, 12), bratu_p, 2), (ah.bratu2d_, ah.slab((16, 24), 0, 2), bratu_p, 1)):
        with pytest.raises(NotImplementedError, match="one rank.*distributed=True"):
            MG(fake(args[0], args[1], args[2], nranks=args[3]))
    with pytest.raises(NotImplementedError, match="one rank.*distributed=True"):
        MG.from_coefficients(ah.slab((16, 24), 1, 2), [1.0, 1.0], -1.0, ctx=ctx2)
    # acceptance: everything checked on the host passes, and construction goes on to the library (the fake context
    # has no handle: not a NotImplementedError)
    from ariadne_hip.precond import _mg_problem, _mg_slab_check
    prob = _mg_problem(fake(ah.bratu2d_, ah.slab((16, 24), 1, 2), bratu_p, nranks=2), True)
    assert (prob.kind, prob.nx, prob.ny) == (_lib.NK_BRATU2D, 16, 12)
    _mg_slab_check(types.SimpleNamespace(nranks=4, handle=None), ah.slab((8, 6, 16), 3, 4))
    _mg_problem(fake(ah.heat2d_midpoint_, ah.slab((16, 24), 0, 2), heat_p(ah.bc_zero_), nranks=2), True)
    # refusals, each naming its reason
    with pytest.raises(NotImplementedError, match="several ranks"):
        MG(fake(ah.bratu2d_, ah.Grid.full(16, 12), bratu_p), distributed=True)
    with pytest.raises(NotImplementedError, match="uneven slabs"):
        MG(fake(ah.bratu2d_, ah.slab((16, 25), 0, 2), bratu_p, nranks=2), distributed=True)
    with pytest.raises(NotImplementedError, match="uneven slabs"):  # a slab of another rank count than the context's
        MG(fake(ah.bratu2d_, ah.slab((16, 24), 0, 4), bratu_p, nranks=2), distributed=True)
    with pytest.raises(NotImplementedError, match="uneven slabs"):  # the whole grid on every rank
        MG(fake(ah.bratu2d_, ah.Grid.full(16, 12), bratu_p, nranks=2), distributed=True)
    with pytest.raises(NotImplementedError, match="odd number of planes"):
        MG(fake(ah.bratu2d_, ah.slab((16, 22), 0, 2), bratu_p, nranks=2), distributed=True)
    with pytest.raises(NotImplementedError, match="3D blocks"):
        MG.from_coefficients(ah.block((8, 8, 8), 1, (2, 1, 1)), [1.0] * 3, -1.0, ctx=ctx2, distributed=True)
    with pytest.raises(NotImplementedError, match="3D blocks"):
        MG.from_coefficients(ah.slab((8, 8, 8), 1, 2), [1.0] * 3, -1.0, distributed=True,
                             ctx=types.SimpleNamespace(nranks=2, handle=None, pgrid=(2, 1, 1)))
    with pytest.raises(NotImplementedError, match="semi"):
        MG(fake(ah.bratu2d_, ah.slab((16, 24), 0, 2), bratu_p, nranks=2), distributed=True, coarsening="semi")
    with pytest.raises(NotImplementedError, match="semi"):
        MG.from_coefficients(ah.slab((16, 24), 1, 2), [1.0, 1.0], -1.0, ctx=ctx2, distributed=True, coarsening="semi")
    with pytest.raises(NotImplementedError, match="periodic"):
        MG(fake(ah.heat2d_euler_, ah.slab((16, 24), 0, 2), heat_p(ah.bc_periodic_), nranks=2), distributed=True)
    with pytest.raises(NotImplementedError, match="1D"):
        MG(fake(ah.bratu_, ah.slab((24,), 0, 2), lambda u: (0.1, 3.5), nranks=2), distributed=True)
    with pytest.raises(NotImplementedError, match="several ranks"):
        MG.from_coefficients(ah.Grid.full(16, 12), [1.0, 1.0], -1.0, ctx=types.SimpleNamespace(nranks=1, handle=None),
                             distributed=True)
    # the factory refuses alike, when it is called with the operator
    with pytest.raises(NotImplementedError, match="uneven slabs"):
        ah.multigrid(distributed=True)(fake(ah.bratu2d_, ah.slab((16, 25), 0, 2), bratu_p, nranks=2))
    with pytest.raises(NotImplementedError, match="one rank"):
        ah.multigrid()(fake(ah.bratu2d_, ah.slab((16, 24), 0, 2), bratu_p, nranks=2))


def test_header_ctypes_and_shim_agree_on_plan_slabs():
    hdr = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "newtonkrylov.jl_amd", "julia", "AriadneHIP.jl")).read()
    n = "nk_mg_plan_slabs"
    args = re.search(rf"\bint {n}\(([^;]*?)\);", hdr, re.S).group(1)
    names = [a.strip() for a in args.split(",")]
    assert [a.split()[-1] for a in names] == ["n_local[3]", "nranks", "max_levels", "extents", "cap", "nlevels"]
    want = ["ptr", "i32", "i32", "ptr", "i32", "ptr"]
    c_class = lambda d: "ptr" if "*" in d or "[" in d else {"int32_t": "i32", "int64_t": "i64", "double": "f64"}[d.split()[0]]  # noqa: E731
    assert [c_class(a) for a in names] == want
    ct = {C.c_int: "i32", C.c_int32: "i32", C.c_int64: "i64", C.c_double: "f64"}
    assert n in _lib.SIGNATURES and hasattr(ah.load(), n)
    assert _lib.SIGNATURES[n][0] is C.c_int and [ct.get(t, "ptr") for t in _lib.SIGNATURES[n][1]] == want
    call = shim[shim.index(f"ccall((:{n}, libnkhip)"):]
    jl = re.match(r"ccall\(\(:\w+, libnkhip\), Cint,\s*\((.*?)\),\s", call, re.S).group(1)
    jl = re.sub(r"\{[^{}]*\{[^{}]*\}[^{}]*\}|\{[^{}]*\}", "", jl)  # drop the type parameters
    got = ["ptr" if t.strip() in ("Ref", "Ptr", "VP") else {"Cint": "i32", "Int32": "i32", "Int64": "i64", "Float64": "f64"}[t.strip()]
           for t in jl.split(",") if t.strip()]
    assert got == want


# ------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    c = ah.Context(0)
    ah.set_default_context(c)
    yield c
    c.sync()


_RUNS = {}


def ranks_run(name, tmp_path_factory):
    """the worker run of a case (once per session): (arrays, per-rank scalars, meta)"""
    if name not in _RUNS:
        import test_hip_dist as thd

        world = CASES[name][2]
        out = str(tmp_path_factory.mktemp("mgd_" + name) / "r")
        rc, log = thd.run_ranks(world, [WORKER, "--out", out, "--case", name], thd.worker_env(world), timeout=180)
        assert rc == 0, log[-4000:]
        meta = json.load(open(out + ".json"))
        assert meta["world"] == world and len(meta["ranks"]) == world
        _RUNS[name] = (dict(np.load(out + ".npz")), meta["ranks"], meta)
    return _RUNS[name]


def one_rank(name):
    """the global case on this process's context, as test_hip_multigrid.device_operator builds it"""
    kind, shape, R = CASES[name]
    J, ref = tm.device_operator(kind, shape)
    return J, ref, case_vectors(ref[0], ref[1])


def local_levels(name):
    kind, shape, R = CASES[name]
    return [list(e) for e in slab_levels(shape[:-1] + (shape[-1] // R,), R)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", VCYCLE_CASES)
def test_vcycle_is_the_one_rank_cycle_bit_for_bit(ctx, tmp_path_factory, name):
    arr, ranks, _ = ranks_run(name, tmp_path_factory)
    kind, shape, R = CASES[name]
    Ld = LEVELS[name]
    J, ref, (v, v2, u2) = one_rank(name)
    P, u0, k, s, h = ref[:5]
    for r in ranks:
        assert r["levels"] == r["levels_spd"] == r["levels_updated"] == local_levels(name)
    mg = ah.MultigridPreconditioner(J, max_levels=Ld)
    assert len(mg.levels) == Ld
    vd = ah.DeviceArray.from_numpy(v)
    z1 = mg.apply(J, vd).to_numpy()
    np.testing.assert_array_equal(arr["z"], z1)
    np.testing.assert_array_equal(arr["z_again"], arr["z"])
    np.testing.assert_array_equal(arr["z_dot"], arr["z"])
    mg.spd = True
    zs, vzs = mg.vcycle_dot(vd)
    np.testing.assert_array_equal(arr["z_spd"], zs.to_numpy())
    np.testing.assert_array_equal(arr["z_spd_dot"], arr["z_spd"])
    np.testing.assert_array_equal(arr["z_spd"], -arr["z"])  # the built-in Jacobians are negative definite: sigma = -1
    mg.spd = False
    # <v, z>: the same bits on every rank; against the one-rank value only the order of the sum differs
    for key, want in (("vz", -vzs), ("vz_spd", vzs)):
        assert len({r[key] for r in ranks}) == 1
        # (two orders of a sum of n terms: each is within n u Σ|v_i z_i| of the exact sum, u = eps / 2)
        assert abs(ranks[0][key] - want) <= v.size * np.finfo(float).eps * float(np.abs(v).ravel() @ np.abs(z1).ravel())
    zref = tm.Cycle(shape, h, k, s, max_levels=Ld).vcycle(v)
    err = tm.rel(arr["z"], zref)
    print(f"{name}: {R} ranks vs restatement {err:.3e} (allowed {TOL:.2e}); one rank vs restatement {tm.rel(z1, zref):.3e}")
    assert err <= TOL
    # the level-0 operator after update(J) at another u, on a second v
    res2 = J.u.zero()
    u2d = ah.DeviceArray.from_numpy(u2)
    J.f(res2, u2d, J.p)
    J2 = ah.JacobianOperator(J.f, res2, u2d, J.p)
    mg.update(J2)
    assert len(mg.levels) == Ld
    np.testing.assert_array_equal(arr["z_updated"], mg.apply(J2, ah.DeviceArray.from_numpy(v2)).to_numpy())
    if kind.startswith("bratu"):
        assert not np.array_equal(arr["z_updated"], mg.update(J).apply(J, ah.DeviceArray.from_numpy(v2)).to_numpy())


@pytest.mark.gpu
def test_setup_truncates_on_every_rank_alike(ctx, tmp_path_factory):
    arr, ranks, _ = ranks_run("bratu-2", tmp_path_factory)
    shape, h, k, s, v = truncation_problem()
    want = [list(e) for e in slab_levels((72, 32), 2)[:3]]
    assert [r["trunc_levels"] for r in ranks] == [want, want]
    mg = ah.MultigridPreconditioner.from_coefficients(ah.Grid.full(*shape), k, ah.DeviceArray.from_numpy(s), h=h, max_levels=6)
    assert mg.levels == tm.plan(shape)[:3]
    np.testing.assert_array_equal(arr["trunc_z"], mg.vcycle(ah.DeviceArray.from_numpy(v)).to_numpy())
    err = tm.rel(arr["trunc_z"], tm.Cycle(shape, h, k, s, max_levels=6).vcycle(v))
    print(f"truncated on 2 ranks vs restatement {err:.3e} (allowed {TOL:.2e})")
    assert err <= TOL


def one_rank_solve(J, algo, **kw):
    ws = ah.krylov_workspace(algo, ah.KrylovConstructor(J.res, memory=30))
    opts = dict(restart=True, itmax=60) if algo == "gmres" else {}
    ah.krylov_solve_(ws, J, J.res, atol=0.0, rtol=RTOL, **opts, **kw)
    st = ws.stats
    ws.free()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", VCYCLE_CASES)
def test_preconditioned_solves_on_slabs(ctx, tmp_path_factory, name):
    arr, ranks, _ = ranks_run(name, tmp_path_factory)
    kind, shape, R = CASES[name]
    J, ref, _ = one_rank(name)
    P, u0 = ref[0], ref[1]
    b = arr["b"]
    algos = [("gmres", "N", {})] + ([("cg", "M", {"spd": True}), ("minres", "M", {"spd": True})] if name == "bratu-2" else [])
    for algo, side, opt in algos:
        st1 = one_rank_solve(J, algo, **{side: ah.MultigridPreconditioner(J, max_levels=LEVELS[name], **opt)})
        assert st1.solved
        runs = [r[algo] for r in ranks]
        assert all(q["solved"] for q in runs) and all(q["h"] == runs[0]["h"] and q["niter"] == runs[0]["niter"] for q in runs)
        x = arr["x_" + algo]
        true = np.linalg.norm(b - oc.jv_exact(P, u0, x)) / np.linalg.norm(b)
        print(f"{name} {algo}: {R} ranks niter {runs[0]['niter']} (one rank {st1.niter}), ||b - J x|| / ||b|| {true:.3e} "
              f"(allowed {1.01 * RTOL:.3e})")
        assert runs[0]["niter"] <= st1.niter + 1
        assert true <= 1.01 * RTOL


@pytest.mark.gpu
def test_newton_and_an_implicit_step_on_slabs(ctx, tmp_path_factory):
    arr, ranks, _ = ranks_run("newton-4", tmp_path_factory)
    kind, shape, R = CASES["newton-4"]
    P = oc.bratu2d(*shape)
    p = (P.hx, P.hy, P.lam)
    u1, r1 = ah.newton_krylov_(ah.bratu2d_, ah.DeviceArray.from_numpy(oc.sin_ic(P)), p, N=ah.multigrid(max_levels=4), jv="fd")
    assert r1.solved
    for r in ranks:
        assert r["newton_levels"] == local_levels("newton-4") and len(r["newton_levels"]) == 4
        for key in ("newton", "native"):
            assert r[key] == ranks[0][key] and r[key]["solved"]
            assert r[key]["outer"] == r1.stats.outer_iterations
            assert abs(r[key]["inner"] - r1.stats.inner_iterations) <= r1.stats.outer_iterations
    print(f"Newton 64 x 96: 4 ranks outer {ranks[0]['newton']['outer']} inner {ranks[0]['newton']['inner']}; one rank "
          f"outer {r1.stats.outer_iterations} inner {r1.stats.inner_iterations}")
    for key in ("u", "u_native"):
        np.testing.assert_allclose(arr[key], u1.to_numpy(), rtol=0, atol=1e-6 * np.abs(u1.to_numpy()).max())
    # one G_Euler_ step of the 3D heat case, against the same step on one rank
    arr, ranks, _ = ranks_run("heat3d-2", tmp_path_factory)
    kind, shape, R = CASES["heat3d-2"]
    a, dt = tm.A_DT
    P = oc.heat3d_euler(*shape, a=a, dt=dt)
    sp = (a, P.hx, P.hy, P.hz, ah.bc_zero_)
    stats = []
    un = ah.solve(ah.G_Euler_, ah.diffusion3d_, ah.DeviceArray.from_numpy(heat_start(P)), sp, dt, [0.0, dt],
                  krylov_kwargs={"N": ah.multigrid(max_levels=LEVELS["heat3d-2"])}, stats_out=stats)
    for r in ranks:
        assert r["heat"] == ranks[0]["heat"] and r["heat"]["solved"] and stats[0].solved
        assert r["heat"]["outer"] == stats[0].stats.outer_iterations
        assert abs(r["heat"]["inner"] - stats[0].stats.inner_iterations) <= stats[0].stats.outer_iterations
    # both satisfy ||G(u)|| = n_res; G is affine with J = -(I - a dt Δ_h), ||J^-1|| <= 1: ||u_a - u_b|| <= n_res_a + n_res_b
    assert np.linalg.norm(arr["heat_u"] - un.to_numpy()) <= ranks[0]["heat"]["n_res"] + stats[0].stats.n_res


@pytest.mark.gpu
def test_c_abi_refusals_on_a_two_rank_context(tmp_path_factory):
    _, ranks, _ = ranks_run("bratu-2", tmp_path_factory)
    for r in ranks:
        for key, word in (("blocks", "3D blocks"), ("periodic", "periodic"), ("levels", "level list"), ("odd", "odd number of planes")):
            rc, msg = r["abi"][key]
            assert rc == _lib.NK_E_ARG and word in msg, (key, rc, msg)
