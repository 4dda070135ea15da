"""Worker of tests/test_hip_ilu.py::test_ilu0_timeout_recovers_on_one_rank, started with NK_ILU_SPIN_LIMIT=1
in a fresh interpreter: every strip poll of the pipelined ILU(0) solve sweeps gives up at once (the factor's
poll budget is not affected), so one rank's recovery runs -- the apply (nk_precond_apply) or the whole Krylov
solve (nk_krylov_solve) once more on the level sweep, which that context then keeps.

    ilu_timeout_worker.py IN.npz OUT.npz      IN: u0, v of 2D Bratu (x fastest);  OUT: see the end

(a) one context: factor, apply, and a second factor and apply;  (b) a fresh context: ILU(0)-preconditioned
restarted GMRES(10), 12 steps, atol = rtol = 0.  Launch counts per kernel class are saved as JSON.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402

inp = np.load(sys.argv[1])
u0, v = inp["u0"], inp["v"]
ny, nx = u0.shape
p = (1.0 / (nx + 1), 1.0 / (ny + 1), float(inp["lam"]))


def launches(ctx):
    return {k: e["launches"] for k, e in ctx.prof_read().items() if k.startswith("ilu0_")}


def setup():
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    u = ah.DeviceArray.from_numpy(u0, ctx=ctx)
    res = u.zero()
    ah.bratu2d_(res, u, p)
    ctx.prof_enable(1 << 20)
    return ctx, res, ah.JacobianOperator(ah.bratu2d_, res, u, p)


# (a) the apply times out and is redone; the context's second factor and apply run on the level sweep
ctx, res, J = setup()
N = ah.ilu0(J)
z1 = N.apply(J, ah.DeviceArray.from_numpy(v, ctx=ctx)).to_numpy()
prof_first = launches(ctx)
N2 = ah.ilu0(J)
z2 = N2.apply(J, ah.DeviceArray.from_numpy(v, ctx=ctx)).to_numpy()
out = dict(d=N.d.to_numpy(), d2=N2.d.to_numpy(), z1=z1, z2=z2, prof_first=json.dumps(prof_first),
           prof_a=json.dumps(launches(ctx)))
ctx.sync()

# (b) a fresh context: the first Arnoldi step's apply times out, the whole solve is redone
ctx, res, J = setup()
N = ah.ilu0(J)
ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(res, memory=10))
ah.krylov_solve_(ws, J, res, N=N, ldiv=True, history=True, restart=True, atol=0.0, rtol=0.0, itmax=12)
out.update(h=np.array(ws.stats.residuals), x=ws.x.to_numpy(), niter=ws.stats.niter, n_matvec=ws.stats.n_matvec,
           prof_b=json.dumps(launches(ctx)))
ctx.sync()
np.savez(sys.argv[2], **out)
