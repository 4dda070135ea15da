#!/usr/bin/env python3
"""MINRES on one MI355X against the parent's paths: 2D Bratu from sin_ic, FD Jv.

1. One linear solve J(u0) x = F(u0) with atol = rtol = 0: `--iters` iterations of MINRES and as many of GMRES(30) with
   restart (the headline's Krylov settings, the reference for time): ms per iteration and the true ||b - J x|| / ||b||
   from one extra exact Jv.
2. The Newton solve from the same start (the default Eisenstat-Walker forcing and tolerance): unpreconditioned MINRES,
   MINRES with M = multigrid(spd=True), CG with M = multigrid(spd=True): counts, final ||F||, wall time.
3. Per-launch times of minres_lanczos and minres_update (HIP events around every launch of a profiled run of part 1)
   against their byte models, as a fraction of 8 TB/s.

  python tools/minres_solve.py [--grid 4096x4096] [--iters 300] [--out profiles/minres] [--tag NAME] [--linear-only]

With the kernel-variant build (NK_KBENCH_LIB=1) and NK_MINRES_BLAS1=1 part 1 runs the Lanczos step assembled from the
BLAS-1 launches (--linear-only --tag blas1): the measured no-go of DESIGN.md §11.
Writes minres_solve[_TAG].{txt,json}.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _nkpath  # noqa: E402,F401
import ariadne_hip as ah  # noqa: E402

PEAK = 8.0e12  # B/s, the MI355X HBM3E peak the byte models are held against
LAMBDA = 3.51382


def sin_ic(nx, ny):
    x = np.sin(np.pi * np.arange(1, nx + 1) / (nx + 1))
    y = np.sin(np.pi * np.arange(1, ny + 1) / (ny + 1))
    return np.ascontiguousarray(y[:, None] * x[None, :])


def operator(ctx, nx, ny, jv):
    u = ah.DeviceArray.from_numpy(sin_ic(nx, ny), ctx=ctx)
    p = (1.0 / (nx + 1), 1.0 / (ny + 1), LAMBDA)
    res = u.zero()
    ah.bratu2d_(res, u, p)
    return ah.JacobianOperator(ah.bratu2d_, res, u, p, jv=jv)


def linear(ctx, nx, ny, algo, iters, profile=False, **kw):
    J = operator(ctx, nx, ny, "fd")
    ws = ah.krylov_workspace(algo, ah.KrylovConstructor(J.res, memory=30))
    ah.krylov_solve_(ws, J, J.res, atol=0.0, rtol=0.0, itmax=min(iters, 30), **kw)  # warm: kernels loaded, buffers touched
    if profile:
        ctx.prof_enable(1)
        ctx.prof_reset()
    ctx.sync()
    t0 = time.perf_counter()
    ah.krylov_solve_(ws, J, J.res, atol=0.0, rtol=0.0, itmax=iters, history=True, **kw)
    ctx.sync()
    secs = time.perf_counter() - t0
    prof = ctx.prof_read() if profile else {}
    if profile:
        ctx.prof_enable(0)
    out = J.res.zero()
    ah.mul_(out, ah.JacobianOperator(ah.bratu2d_, J.res, J.u, J.p, jv="exact"), ws.x)
    b = J.res.to_numpy()
    true = float(np.linalg.norm(b - out.to_numpy()) / np.linalg.norm(b))
    row = dict(algo=algo, niter=ws.stats.niter, n_matvec=ws.stats.n_matvec, seconds=secs, ms_per_iteration=1e3 * secs / max(1, ws.stats.niter),
               estimate_rel=ws.stats.residuals[-1] / ws.stats.residuals[0], true_rel_residual=true)
    ws.free()
    kernels = []
    for name, e in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        if e["timed"]:
            us = 1e3 * e["ms"] / e["timed"]
            bw = e["bytes"] / (e["ms"] * 1e-3) if e["ms"] > 0 else 0.0
            kernels.append(dict(kernel=name, timed=e["timed"], us_per_launch=us, model_bytes_per_launch=e["bytes"] / e["timed"],
                                model_gbs=bw / 1e9, fraction_of_peak=bw / PEAK))
    return row, kernels


def newton(ctx, nx, ny, max_niter, **kw):
    u = ah.DeviceArray.from_numpy(sin_ic(nx, ny), ctx=ctx)
    p = (1.0 / (nx + 1), 1.0 / (ny + 1), LAMBDA)
    ctx.sync()
    t0 = time.perf_counter()
    _, r = ah.newton_krylov_(ah.bratu2d_, u, p, max_niter=max_niter, **kw)
    ctx.sync()
    return dict(solved=bool(r.solved), outer=r.stats.outer_iterations, inner=r.stats.inner_iterations, n_matvec=r.n_matvec,
                n_res=r.stats.n_res, seconds=time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="4096x4096")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", default="profiles/minres")
    ap.add_argument("--tag", default="")
    ap.add_argument("--jv", default="fd", help="the Newton solves' Jv")
    ap.add_argument("--plain-itmax", type=int, default=20000, help="itmax of the unpreconditioned Newton-MINRES's inner solves")
    ap.add_argument("--plain-steps", type=int, default=50, help="Newton steps the unpreconditioned solve may take")
    ap.add_argument("--linear-only", action="store_true")
    args = ap.parse_args()
    nx, ny = (int(t) for t in args.grid.split("x"))
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    for algo, kw in (("minres", {}), ("gmres", dict(restart=True))):  # load every kernel before anything is timed
        linear(ctx, 96, 80, algo, 40, **kw)
    out = dict(grid=[nx, ny], settings=dict(jv="fd", iters=args.iters, kbench_lib=os.environ.get("NK_KBENCH_LIB", ""),
                                            minres_blas1=os.environ.get("NK_MINRES_BLAS1", "")))
    lines = [f"== 2D Bratu {nx} x {ny} at sin_ic, J(u0) x = F(u0), FD Jv, atol = rtol = 0, {args.iters} iterations"]
    rows = []
    for rep in range(2):  # alternating
        rows.append(linear(ctx, nx, ny, "minres", args.iters)[0])
        rows.append(linear(ctx, nx, ny, "gmres", args.iters, restart=True)[0])
    out["linear"] = rows
    for r in rows:
        lines.append(f"  {r['algo']:<6}: {r['niter']} iterations  {r['seconds']:.4f} s  {r['ms_per_iteration']:.4f} ms/iteration  "
                     f"estimate / ||b|| {r['estimate_rel']:.3e}  true ||b - J x|| / ||b|| {r['true_rel_residual']:.3e}")
    _, kernels = linear(ctx, nx, ny, "minres", args.iters, profile=True)
    out["minres_kernels"] = kernels
    lines.append("  per launch of the profiled MINRES run (HIP events around every launch):")
    for r in kernels:
        lines.append(f"    {r['kernel']:<22} x{r['timed']:<4} {r['us_per_launch']:9.2f} us  model {r['model_bytes_per_launch'] / 1e6:8.2f} MB  "
                     f"{r['model_gbs']:7.0f} GB/s  {r['fraction_of_peak']:.2f} of 8 TB/s")
    if not args.linear_only:
        lines.append(f"== Newton from sin_ic, {args.jv.upper()} Jv, Eisenstat-Walker, tol 1e-6 ||F(u0)|| + 1e-12")
        newton(ctx, 96, 80, 50, algo="minres", M=ah.multigrid(spd=True), jv=args.jv)
        newton(ctx, 96, 80, 50, algo="cg", M=ah.multigrid(spd=True), jv=args.jv)
        runs = [("minres, M = multigrid(spd)", dict(algo="minres", M=ah.multigrid(spd=True), max_niter=50)),
                ("cg, M = multigrid(spd)", dict(algo="cg", M=ah.multigrid(spd=True), max_niter=50)),
                ("minres, plain", dict(algo="minres", max_niter=args.plain_steps, krylov_kwargs=dict(itmax=args.plain_itmax)))]
        out["newton"] = []
        for tag, kw in runs:
            max_niter = kw.pop("max_niter")
            r = newton(ctx, nx, ny, max_niter, jv=args.jv, **kw)
            r["run"] = tag
            out["newton"].append(r)
            lines.append(f"  {tag:<28}: solved {r['solved']}  ||F|| {r['n_res']:.3e}  Newton {r['outer']}  Krylov {r['inner']}  "
                         f"matvecs {r['n_matvec']}  {r['seconds']:.4f} s")
    text = "\n".join(lines)
    print(text)
    stem = os.path.join(args.out, "minres_solve" + (f"_{args.tag}" if args.tag else ""))
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    with open(stem + ".txt", "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
