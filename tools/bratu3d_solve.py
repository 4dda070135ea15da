#!/usr/bin/env python3
"""3D Bratu (NK_BRATU3D) at scale: its stencil kernels against the heat kernel of the same march, Newton solves
with and without the multigrid V-cycle, and one V-cycle's kernel classes.

  python tools/bratu3d_solve.py --kernels [--sizes 256,512] [--reps 20] [--tag NAME]
      residual, exact Jv and FD Jv of bratu3d_ and -- in the same session -- G_Euler!'s FD Jv (k_st3l without an
      exp) at n^3: microseconds per launch from the library's event profile, the byte model of each launch and the
      fraction of 8 TB/s it amounts to, and each kernel's time per model byte relative to the heat kernel's.
      With NK_LIB_VARIANT=<TAG> the same table for a `make variant` build (the NK_ST3D_BRATU_DIV_RN and
      NK_ST3L_BRATU_WPE A/Bs).
  python tools/bratu3d_solve.py --solves [--sizes 256] [--lambdas 3.51382,6]
      Newton from the sine with GMRES(30) restart, itmax 300, FD Jv, default forcing and tolerance: unpreconditioned,
      N = multigrid, and CG with M = multigrid(spd=True); Newton / Krylov counts, final ||F||, wall time.  Then the
      per-kernel profile of one V-cycle at the first size.

Writes profiles/bratu3d/<kernels|solves>[_TAG].{txt,json}.
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


def sin_ic(n):
    s = np.sin(np.pi * np.arange(1, n + 1) / (n + 1))
    return np.ascontiguousarray(s[:, None, None] * s[None, :, None] * s[None, None, :])


def profiled(ctx, name, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(1)
    for _ in range(reps):
        fn()
    ctx.sync()
    e = ctx.prof_read()[name]
    ctx.prof_enable(0)
    us = 1e3 * e["ms"] / e["timed"]
    byt = e["bytes"] / e["timed"]
    return dict(launch=name, kernel=e["kernel"], us=us, model_bytes=byt, fraction_of_peak=byt / (us * 1e-6) / PEAK,
                ps_per_byte=1e6 * us / byt)


def kernels(ctx, n, reps):
    h = 1.0 / (n + 1)
    u = ah.DeviceArray.from_numpy(sin_ic(n), ctx=ctx)
    v = ah.DeviceArray.from_numpy(np.random.default_rng(0).standard_normal((n, n, n)), ctx=ctx)
    res, out = u.zero(), u.zero()
    rows = []
    # the yardstick: G_Euler!'s FD Jv, the same z-march without an exp
    un = u.copy()
    ph = (un, 1e-6, None, (0.01, h, h, h, ah.bc_zero_), 0.0)
    ah.heat3d_euler_(res, u, ph)
    Jh = ah.JacobianOperator(ah.heat3d_euler_, res, u, ph, jv="fd")
    rows.append(dict(profiled(ctx, "jv_fd", lambda: ah.mul_(out, Jh, v), reps), what="heat3d_euler FD Jv"))
    p = (h, h, h, 3.51382)
    rows.append(dict(profiled(ctx, "residual", lambda: ah.bratu3d_(res, u, p), reps), what="bratu3d residual"))
    for jv in ("exact", "fd"):
        J = ah.JacobianOperator(ah.bratu3d_, res, u, p, jv=jv)
        rows.append(dict(profiled(ctx, f"jv_{jv}", lambda: ah.mul_(out, J, v), reps), what=f"bratu3d {jv.upper()} Jv"))
    for r in rows:
        r["per_byte_vs_heat"] = r["ps_per_byte"] / rows[0]["ps_per_byte"]
    return rows


def newton(ctx, n, lam, algo="gmres", N=None, M=None):
    h = 1.0 / (n + 1)
    u = ah.DeviceArray.from_numpy(sin_ic(n), ctx=ctx)
    kw = dict(restart=True, itmax=300) if algo == "gmres" else dict(itmax=300)
    ctx.sync()
    t0 = time.perf_counter()
    _, r = ah.newton_krylov_(ah.bratu3d_, u, (h, h, h, lam), algo=algo, N=N, M=M, memory=30, jv="fd", krylov_kwargs=kw)
    ctx.sync()
    return dict(solved=bool(r.solved), outer=r.stats.outer_iterations, inner=r.stats.inner_iterations, n_matvec=r.n_matvec,
                n_res=r.stats.n_res, seconds=time.perf_counter() - t0)


def vcycle_profile(ctx, n, lam):
    h = 1.0 / (n + 1)
    u = ah.DeviceArray.from_numpy(sin_ic(n), ctx=ctx)
    p = (h, h, h, lam)
    res = u.zero()
    ah.bratu3d_(res, u, p)
    J = ah.JacobianOperator(ah.bratu3d_, res, u, p)
    mg = ah.MultigridPreconditioner(J)
    z = u.zero()
    for _ in range(2):
        mg.apply(J, res, z)
    ctx.prof_reset()
    ctx.prof_enable(1)
    mg.apply(J, res, z)
    prof = ctx.prof_read()
    ctx.prof_enable(0)
    rows = []
    for name, e in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        if name.startswith("mg_") and e["timed"]:
            bw = e["bytes"] / (e["ms"] * 1e-3) if e["ms"] > 0 else 0.0
            rows.append(dict(kernel=name, launches=e["launches"], ms=e["ms"], model_bytes=e["bytes"], fraction_of_peak=bw / PEAK))
    levels = mg.levels
    mg.free()
    return dict(levels=levels, kernel_ms=sum(r["ms"] for r in rows), kernels=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--solves", action="store_true")
    ap.add_argument("--sizes", default="256")
    ap.add_argument("--lambdas", default="3.51382,6")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="profiles/bratu3d")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    sizes = [int(s) for s in args.sizes.split(",")]
    variant = os.environ.get("NK_LIB_VARIANT", "")
    sfx = ("_" + args.tag) if args.tag else ""
    if args.kernels:
        out, lines = dict(library_variant=variant, reps=args.reps, sizes=[]), [f"library variant: {variant or '(the product)'}"]
        for n in sizes:
            rows = kernels(ctx, n, args.reps)
            out["sizes"].append(dict(n=n, kernels=rows))
            lines.append(f"== {n}^3, {args.reps} launches each")
            for r in rows:
                lines.append(f"  {r['what']:22s} {r['us']:9.1f} us  {r['model_bytes'] / n ** 3:4.0f} B/pt  "
                             f"{100 * r['fraction_of_peak']:5.1f} % of 8 TB/s  x{r['per_byte_vs_heat']:.3f} heat's time per byte  {r['kernel']}")
        name = "kernels" + sfx
    elif args.solves:
        out, lines = dict(library_variant=variant, solves=[]), []
        newton(ctx, 24, 6.0, N=ah.multigrid)  # load every kernel before anything is timed
        newton(ctx, 24, 6.0, algo="cg", M=ah.multigrid(spd=True))
        for n in sizes:
            for lam in (float(t) for t in args.lambdas.split(",")):
                lines.append(f"== 3D Bratu {n}^3, lambda {lam}, FD Jv, GMRES(30) restart itmax 300 / CG itmax 300")
                for what, kw in (("plain", {}), ("N=multigrid", dict(N=ah.multigrid)),
                                 ("cg M=multigrid(spd)", dict(algo="cg", M=ah.multigrid(spd=True)))):
                    r = dict(newton(ctx, n, lam, **kw), n=n, lam=lam, what=what)
                    out["solves"].append(r)
                    lines.append(f"  {what:22s} solved {r['solved']}  Newton {r['outer']:3d}  Krylov {r['inner']:5d}  "
                                 f"||F|| {r['n_res']:.3e}  {r['seconds']:.3f} s")
        vc = vcycle_profile(ctx, sizes[0], 6.0)
        out["vcycle"] = dict(n=sizes[0], **vc)
        lines.append(f"== one V-cycle at {sizes[0]}^3: levels {vc['levels']}, {vc['kernel_ms']:.3f} ms in kernels")
        for r in vc["kernels"]:
            lines.append(f"  {r['kernel']:18s} {r['launches']:3d} launches  {r['ms']:8.3f} ms  {100 * r['fraction_of_peak']:5.1f} % of 8 TB/s")
        name = "solves" + sfx
    else:
        ap.error("--kernels or --solves")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, name + ".txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, name + ".json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
