"""Worker for the two-rank line-search test (started by tests/test_hip_linesearch.py through test_hip_dist.run_ranks).

Every rank owns a y-slab of 2D Bratu 24 x 20 with lambda = 1 and u0 = 5 sin sin, opens the peer mailbox (IPC handles
over gloo, no RCCL: both ranks may share one GPU) and runs newton_krylov_ with the backtracking line search -- the
trial residuals exchange the ghost rows of u and of the step d, the trial norms are all-reduced, so every rank takes
the same decisions.  Rank 0 writes the gathered u, every rank's accepted step lengths and whether it solved.
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
args = ap.parse_args()

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
device = 0 if os.environ.get("NK_WORKER_SHARED_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
ctx = ah.Context(device)
ah.set_default_context(ctx)
handles = [None] * world
dist.all_gather_object(handles, ctx.mailbox_handle())
ctx.mailbox_open(rank, world, b"".join(handles))

nx, ny = 24, 20
grid = ah.slab((nx, ny), rank, world)
hx, hy, lam = 1.0 / (nx + 1), 1.0 / (ny + 1), 1.0
xs = np.arange(1, nx + 1) * hx
y0, nyl = grid.offset, grid.shape_xyz[1]
ys = np.arange(y0 + 1, y0 + nyl + 1) * hy
u0 = 5.0 * (np.sin(np.pi * ys)[:, None] * np.sin(np.pi * xs)[None, :])
p = (hx, hy, lam)
u = ah.DeviceArray.from_numpy(u0, grid, ctx)
res = u.zero()
_, r = ah.newton_krylov_(ah.bratu2d_, u, p, res, algo="gmres", memory=480, forcing=None, jv="exact",
                         linesearch=ah.Backtracking())
parts = [None] * world
dist.all_gather_object(parts, dict(y0=y0, u=u.to_numpy(), steps=list(r.steps), solved=bool(r.solved),
                                   n_backtrack=r.n_backtrack, outer=r.stats.outer_iterations))
if rank == 0:
    parts.sort(key=lambda d: d["y0"])
    np.savez(args.out + ".npz", u=np.concatenate([d["u"] for d in parts]))
    json.dump(dict(solved=[d["solved"] for d in parts], steps=parts[0]["steps"],
                   steps_equal=all(d["steps"] == parts[0]["steps"] for d in parts),
                   n_backtrack=[d["n_backtrack"] for d in parts], outer=[d["outer"] for d in parts], world=world,
                   path=ctx.path_info()), open(args.out + ".json", "w"))
dist.barrier()
ctx.sync()
