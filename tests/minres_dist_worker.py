"""Worker for the two-rank MINRES test (started by tests/test_hip_minres.py through test_hip_dist.run_ranks).

Every rank owns a slab of case A (2D Bratu 24 x 20 at sin_ic, b = F(u)), opens the peer mailbox (IPC handles over
gloo, no RCCL: both ranks may share one GPU; NK_DIST_MAILBOX=host puts the mailbox in host shared memory) and runs
`--itmax` MINRES iterations with atol = rtol = 0.  Rank 0 writes the gathered x, its history, every rank's count and
whether all ranks hold the same history.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402
import torch.distributed as dist  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--nx", type=int, default=24)
ap.add_argument("--ny", type=int, default=20)
ap.add_argument("--itmax", type=int, default=20)
args = ap.parse_args()

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
device = 0 if os.environ.get("NK_WORKER_SHARED_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
ctx = ah.Context(device)
ah.set_default_context(ctx)
handles = [None] * world
dist.all_gather_object(handles, ctx.mailbox_handle())
ctx.mailbox_open(rank, world, b"".join(handles))

nx, ny = args.nx, args.ny
grid = ah.slab((nx, ny), rank, world)
hx, hy, lam = 1.0 / (nx + 1), 1.0 / (ny + 1), 3.51382
xs = np.arange(1, nx + 1) * hx
y0, nyl = grid.offset, grid.shape_xyz[1]
ys = np.arange(y0 + 1, y0 + nyl + 1) * hy
u0 = np.sin(np.pi * ys)[:, None] * np.sin(np.pi * xs)[None, :]
p = (hx, hy, lam)
u = ah.DeviceArray.from_numpy(u0, grid, ctx)
res = u.zero()
ah.bratu2d_(res, u, p)
J = ah.JacobianOperator(ah.bratu2d_, res, u, p)
ws = ah.krylov_workspace("minres", ah.KrylovConstructor(res))
ah.krylov_solve_(ws, J, res, atol=0.0, rtol=0.0, itmax=args.itmax, history=True)
parts = [None] * world
dist.all_gather_object(parts, dict(y0=y0, x=ws.x.to_numpy(), h=list(ws.stats.residuals), niter=ws.stats.niter))
if rank == 0:
    parts.sort(key=lambda d: d["y0"])
    np.savez(args.out + ".npz", x=np.concatenate([d["x"] for d in parts]), h=np.array(parts[0]["h"]))
    json.dump(dict(niter=[d["niter"] for d in parts], histories_equal=all(d["h"] == parts[0]["h"] for d in parts),
                   world=world, path=ctx.path_info()), open(args.out + ".json", "w"))
dist.barrier()
ctx.sync()
