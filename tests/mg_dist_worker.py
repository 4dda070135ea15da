"""Worker of tests/test_hip_multigrid_dist.py (started through test_hip_dist.run_ranks): one rank of a slab-distributed
multigrid hierarchy (distributed=True).

Every rank opens the peer mailbox (IPC handles over gloo, no RCCL: the ranks may share one GPU), owns an equal slab of
the global case of test_hip_multigrid_dist.CASES[--case] and runs everything the test asks of that shape; rank 0 writes
the gathered arrays to --out.npz and the scalars to --out.json.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402
import torch.distributed as dist  # noqa: E402
from ariadne_hip import _lib  # noqa: E402

import test_hip_multigrid as tm  # noqa: E402
import test_hip_multigrid_dist as td  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--case", required=True)
args = ap.parse_args()

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
device = 0 if os.environ.get("NK_WORKER_SHARED_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
ctx = ah.Context(device)
ah.set_default_context(ctx)
handles = [None] * world
dist.all_gather_object(handles, ctx.mailbox_handle())
ctx.mailbox_open(rank, world, b"".join(handles))

arrays, scalars = {}, {}  # this rank's slabs (gathered along the slab axis) and its scalars (one entry per rank)


def slab_of(a, grid):
    return np.ascontiguousarray(a[grid.offset:grid.offset + grid.shape_xyz[-1]])


def on_slab(a, grid):
    return ah.DeviceArray.from_numpy(slab_of(a, grid), grid, ctx)


def operator(kind, P, u0, grid):
    """the case's JacobianOperator on this rank's slab (as test_hip_multigrid.device_operator builds the global one)"""
    u = on_slab(u0, grid)
    res = u.zero()
    f = tm.RESIDUALS[kind]
    if kind.startswith("bratu"):
        p = (P.hx, P.hy, P.lam)
    else:
        sp = (P.a, P.hx, P.hy, ah.bc_zero_) if P.dim == 2 else (P.a, P.hx, P.hy, P.hz, ah.bc_zero_)
        p = (on_slab(P.un, grid), P.dt, u.zero(), sp, 0.0)
    f(res, u, p)
    return ah.JacobianOperator(f, res, u, p)


def krylov(J, algo, **kw):
    ws = ah.krylov_workspace(algo, ah.KrylovConstructor(J.res, memory=30))
    opts = dict(restart=True, itmax=60) if algo == "gmres" else {}
    ah.krylov_solve_(ws, J, J.res, atol=0.0, rtol=td.RTOL, history=True, **opts, **kw)
    out = ws.x.to_numpy(), dict(niter=int(ws.stats.niter), solved=bool(ws.stats.solved), h=[float(r) for r in ws.stats.residuals])
    ws.free()
    return out


def vcycle_case(name):
    kind, shape, R = td.CASES[name]
    assert R == world
    P, u0, k, s, h = tm.host_problem(kind, shape)
    v, v2, u2 = td.case_vectors(P, u0)
    grid = ah.slab(shape, rank, world)
    J = operator(kind, P, u0, grid)
    vd = on_slab(v, grid)
    mg = ah.MultigridPreconditioner(J, distributed=True)
    scalars["levels"] = [list(e) for e in mg.levels]
    arrays["z"] = mg.apply(J, vd).to_numpy()
    arrays["z_again"] = mg.apply(J, vd).to_numpy()
    zd, vz = mg.vcycle_dot(vd)
    arrays["z_dot"], scalars["vz"] = zd.to_numpy(), vz
    mg.spd = True
    scalars["levels_spd"] = [list(e) for e in mg.levels]
    arrays["z_spd"] = mg.apply(J, vd).to_numpy()
    zd, vz = mg.vcycle_dot(vd)
    arrays["z_spd_dot"], scalars["vz_spd"] = zd.to_numpy(), vz
    mg.spd = False
    # the level-0 operator follows update(J) at another u
    J2 = operator(kind, P, u2, grid)
    mg.update(J2)
    scalars["levels_updated"] = [list(e) for e in mg.levels]
    arrays["z_updated"] = mg.apply(J2, on_slab(v2, grid)).to_numpy()
    mg.free()
    # the solves: J x = F(u)
    arrays["b"] = J.res.to_numpy()
    arrays["x_gmres"], scalars["gmres"] = krylov(J, "gmres", N=ah.multigrid(distributed=True))
    if name == "bratu-2":
        for algo in ("cg", "minres"):
            arrays["x_" + algo], scalars[algo] = krylov(J, algo, M=ah.multigrid(spd=True, distributed=True))
        truncation_case()
        c_abi_refusals()  # last: it turns the context's slabs into blocks
    if kind.startswith("heat3d"):
        heat_step(P, grid)


def truncation_case():
    """set-up must truncate on every rank alike: only rank 1's slab has a positive diagonal entry on the fourth level"""
    shape, h, k, s, v = td.truncation_problem()
    grid = ah.slab(shape, rank, world)
    mg = ah.MultigridPreconditioner.from_coefficients(grid, k, on_slab(s, grid), ctx=ctx, distributed=True)
    scalars["trunc_levels"] = [list(e) for e in mg.levels]
    arrays["trunc_z"] = mg.vcycle(on_slab(v, grid)).to_numpy()
    mg.free()


def heat_step(P, grid):
    """one solve(G_Euler_, ...) step of the 3D heat case with the distributed V-cycle as N"""
    a, dt = tm.A_DT
    un0 = td.heat_start(P)
    sp = (a, P.hx, P.hy, P.hz, ah.bc_zero_)
    stats = []
    un = ah.solve(ah.G_Euler_, ah.diffusion3d_, on_slab(un0, grid), sp, dt, [0.0, dt],
                  krylov_kwargs={"N": ah.multigrid(distributed=True)}, stats_out=stats)
    arrays["heat_u"] = un.to_numpy()
    scalars["heat"] = dict(solved=bool(stats[0].solved), outer=int(stats[0].stats.outer_iterations),
                           inner=int(stats[0].stats.inner_iterations), n_res=float(stats[0].stats.n_res))


def newton_case(name):
    kind, shape, R = td.CASES[name]
    from oracle import oracle as oc

    P = oc.bratu2d(*shape)
    grid = ah.slab(shape, rank, world)
    fac = ah.multigrid(distributed=True)
    u, r = ah.newton_krylov_(ah.bratu2d_, on_slab(oc.sin_ic(P), grid), (P.hx, P.hy, P.lam), N=fac, jv="fd")
    arrays["u"] = u.to_numpy()
    scalars["newton"] = dict(solved=bool(r.solved), outer=int(r.stats.outer_iterations), inner=int(r.stats.inner_iterations))
    scalars["newton_levels"] = [list(e) for e in fac.mg.levels]
    fac.free()
    # the loop in the library refreshes the distributed hierarchy itself
    un, rn = ah.newton_krylov_native(ah.bratu2d_, on_slab(oc.sin_ic(P), grid), (P.hx, P.hy, P.lam),
                                     N=ah.multigrid(distributed=True), jv="fd")
    arrays["u_native"] = un.to_numpy()
    scalars["native"] = dict(solved=bool(rn.solved), outer=int(rn.stats[0]), inner=int(rn.stats[1]))


def c_abi_refusals():
    """NK_E_ARG with the reason, from the library on a distributed context; nothing is enqueued by a refused create"""
    lib = ah.load()
    h = C.c_void_p()
    out = {}

    def create(prob, levels=None):
        if levels is None:
            rc = lib.nk_mg_create(ctx.handle, C.byref(prob), None, C.byref(h))
        else:
            ext = (C.c_int64 * len(levels))(*levels)
            rc = lib.nk_mg_create_levels(ctx.handle, C.byref(prob), None, ext, len(levels) // 3, C.byref(h))
        return [rc, (lib.nk_last_error(ctx.handle) or b"").decode()]

    g2 = ah.Grid.full(24, 12)
    prob = g2.geometry_problem()
    prob.hx = prob.hy = 1.0 / 25
    out["levels"] = create(prob, [24, 12, 1, 12, 6, 1])
    odd = ah.Grid.full(24, 11).geometry_problem()
    out["odd"] = create(odd)
    heat = _lib.nk_problem(_lib.NK_HEAT2D_EULER, _lib.NK_BC_PERIODIC, 24, 12, 1, 0.04, 0.04, 1.0, 0.0, 0.01, 0.1, 8)
    out["periodic"] = create(heat)
    # 3D blocks: a process grid is set before any vector is allocated, so on a second context of its own mailbox
    # (the last thing this worker runs on the GPU: the newer context's mailbox is the one bound to the device)
    ctx2 = ah.Context(device)
    handles = [None] * world
    dist.all_gather_object(handles, ctx2.mailbox_handle())
    ctx2.mailbox_open(rank, world, b"".join(handles))
    ctx2.set_process_grid(2, 1, 1)
    g3 = ah.Grid.full(8, 8, 8).geometry_problem()
    rc = lib.nk_mg_create(ctx2.handle, C.byref(g3), None, C.byref(h))
    out["blocks"] = [rc, (lib.nk_last_error(ctx2.handle) or b"").decode()]
    dist.barrier()
    ctx2.close()
    scalars["abi"] = out


if args.case == "newton-4":
    newton_case(args.case)
else:
    vcycle_case(args.case)

parts = [None] * world
dist.all_gather_object(parts, dict(rank=rank, arrays=arrays, scalars=scalars))
if rank == 0:
    parts.sort(key=lambda d: d["rank"])
    np.savez(args.out + ".npz", **{k: np.concatenate([d["arrays"][k] for d in parts]) for k in arrays})
    json.dump(dict(world=world, ranks=[d["scalars"] for d in parts], path=ctx.path_info()), open(args.out + ".json", "w"))
dist.barrier()
ctx.sync()
