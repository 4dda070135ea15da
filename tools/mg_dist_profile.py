"""Profile the slab-distributed multigrid V-cycle (distributed=True): launches per cycle, the share of
the ghost-plane exchange in the cycle's time, and the peer waits of nk_dist_path.

    python tools/mg_dist_profile.py --world 8 --n 4096 --out profiles/mg_dist/vcycle_4096_8.json

starts `--world` ranks (this script again, with --rank), one per GPU when the box has that many and all on device 0
otherwise (the mailbox transport over IPC handles, no RCCL -- then the times describe ranks time-sharing one GPU, not
one GPU per slab).  Every rank owns n x (n / world) of 2D Bratu n x n at sin_ic and applies the V-cycle `--cycles`
times; rank 0 times every launch with nk_prof_enable and writes the JSON.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--cycles", type=int, default=20)
ap.add_argument("--coarse-sweeps", type=int, default=8)
ap.add_argument("--out", required=True)
ap.add_argument("--rank", type=int, default=-1)
ap.add_argument("--port", type=int, default=29411)
ap.add_argument("--shared", type=int, default=-1)
args = ap.parse_args()

if args.rank < 0:  # the launcher
    import _nkpath  # noqa: F401
    import ariadne_hip as ah

    shared = int(ah.device_count() < args.world)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(args.port), WORLD_SIZE=str(args.world))
    if shared:
        env["GPU_MAX_HW_QUEUES"] = "1"  # one hardware queue per rank process (as the tests' worker_env)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), "--shared", str(shared)] + sys.argv[1:],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(args.world)]
    end, rc = time.time() + 300, 0
    while any(p.poll() is None for p in procs):
        if time.time() > end or any(p.poll() not in (None, 0) for p in procs):
            for p in procs:
                if p.poll() is None:
                    p.kill()
            rc = 1
            break
        time.sleep(0.2)
    sys.exit(rc or max(p.wait() for p in procs))

import numpy as np  # noqa: E402

import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
ctx = ah.Context(0 if args.shared else rank)
ah.set_default_context(ctx)
handles = [None] * world
dist.all_gather_object(handles, ctx.mailbox_handle())
ctx.mailbox_open(rank, world, b"".join(handles))

n = args.n
grid = ah.slab((n, n), rank, world)
h, lam = 1.0 / (n + 1), 3.51382
xs = np.arange(1, n + 1) * h
ys = np.arange(grid.offset + 1, grid.offset + grid.shape_xyz[1] + 1) * h
u = ah.DeviceArray.from_numpy(np.sin(np.pi * ys)[:, None] * np.sin(np.pi * xs)[None, :], grid, ctx)
res = u.zero()
p = (h, h, lam)
ah.bratu2d_(res, u, p)
J = ah.JacobianOperator(ah.bratu2d_, res, u, p)
mg = ah.MultigridPreconditioner(J, distributed=True, coarse_sweeps=args.coarse_sweeps)
v = ah.DeviceArray.from_numpy(np.random.default_rng(7 + rank).standard_normal(grid.np_shape), grid, ctx)
z = v.zero()
for _ in range(3):  # warm-up
    mg.vcycle(v, z)
dist.barrier()
w0 = ctx.path_info()
if rank == 0:
    ctx.prof_enable(1)
    ctx.prof_reset()
t0 = time.perf_counter()
for _ in range(args.cycles):
    mg.vcycle(v, z)  # (synchronises after each cycle)
wall = (time.perf_counter() - t0) / args.cycles
w1 = ctx.path_info()
info = dict(rank=rank, wall_ms_per_cycle=1e3 * wall,
            halo_wait_us_per_cycle=(w1.get("halo_wait_us", 0.0) - w0.get("halo_wait_us", 0.0)) / args.cycles)
if rank == 0:
    prof = ctx.prof_read()
    total = sum(e["ms"] for e in prof.values())
    info["classes"] = {k: dict(launches_per_cycle=e["launches"] / args.cycles, ms_per_cycle=e["ms"] / args.cycles,
                               share=e["ms"] / total) for k, e in sorted(prof.items())}
    info["launches_per_cycle"] = sum(e["launches"] for e in prof.values()) / args.cycles
    info["kernel_ms_per_cycle"] = total / args.cycles
    info["halo_ipc_share"] = prof.get("halo_ipc", {"ms": 0.0})["ms"] / total
allinfo = [None] * world
dist.all_gather_object(allinfo, info)
if rank == 0:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(n=n, world=world, ranks_share_one_gpu=bool(args.shared), gpus=1 if args.shared else world,
                   local_levels=[list(e) for e in mg.levels], cycles=args.cycles, coarse_sweeps=args.coarse_sweeps,
                   path=w1, ranks=allinfo), open(args.out, "w"), indent=1)
    print(json.dumps({k: info[k] for k in ("launches_per_cycle", "kernel_ms_per_cycle", "halo_ipc_share", "wall_ms_per_cycle",
                                           "halo_wait_us_per_cycle")}))
dist.barrier()
ctx.sync()
