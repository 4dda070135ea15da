"""One rank of a 2-rank context (peer mailbox over IPC handles, no RCCL: both ranks may share a GPU) that asks the
library for 3D Bratu, as z-slabs and as 3D blocks; prints what the library answered as one JSON line per rank.
Started by tests/test_hip_bratu3d.py::test_two_rank_context_is_refused."""
import ctypes as C
import json
import os
import sys

import torch  # noqa: F401  (first: libnkhip.so binds torch's HIP runtime)
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402
from ariadne_hip import _lib  # noqa: E402

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
ctx = ah.Context(0 if os.environ.get("NK_WORKER_SHARED_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
handles = [None] * world
dist.all_gather_object(handles, ctx.mailbox_handle())
ctx.mailbox_open(rank, world, b"".join(handles))
lib = ah.load()
out = {"rank": rank, "nranks": ctx.path_info()["nranks"]}
prob = _lib.nk_problem(_lib.NK_BRATU3D, _lib.NK_BC_ZERO, 12, 10, 4, 0.1, 0.1, 0.1, 6.0, 0.0, 0.0, None)
for name, grid in (("slabs", None), ("blocks", (2, 1, 1))):
    if grid:
        ctx.set_process_grid(*grid)
    p = C.c_void_p()
    rc = lib.nk_vec_alloc(ctx.handle, C.byref(prob), C.byref(p))
    out[name] = [rc, (lib.nk_last_error(ctx.handle) or b"").decode()]
    if rc == 0:
        lib.nk_vec_free(ctx.handle, p)
dist.barrier()
print("BRATU3D_RANK " + json.dumps(out), flush=True)
dist.destroy_process_group()
