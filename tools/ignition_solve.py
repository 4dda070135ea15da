#!/usr/bin/env python3
"""The 2D ignition kinds (NK_IGNITION2D_*) at scale: their stencil kernels beside the heat kind of the same scheme and
Bratu 2D, and `solve` with and without the multigrid V-cycle.

  python tools/ignition_solve.py --kernels [--n 4096] [--reps 20] [--tag NAME]
      residual and FD Jv of ignition2d_{euler,midpoint,trapezoid}_ and -- in the same session -- of the heat kind of
      the same scheme and of bratu2d_ at n^2: microseconds per launch from the library's event profile, the byte model
      of each launch, the fraction of 8 TB/s it amounts to and the time per model byte relative to Bratu 2D's launch
      of the same mode.  With NK_LIB_VARIANT=<TAG> the same table for a `make variant` build (the NK_ST2D_IGN_WPE A/B).
  python tools/ignition_solve.py --solves [--n 4096] [--steps 20]
      one `solve` of G_Euler_ steps from u0 = 0 with a = 1, lambda = 6 and Δt = 10^3 h^2 (a Δt / h^2 = 10^3), GMRES(30)
      with restart, itmax 300, exact Jv: unpreconditioned and with N = multigrid; Newton and Krylov steps per time step,
      seconds.

Writes profiles/ignition/<kernels|solves>[_TAG].{txt,json}.
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
SCHEMES = (("euler", ah.G_Euler_), ("midpoint", ah.G_Midpoint_), ("trapezoid", ah.G_Trapezoid_))


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
    rng = np.random.default_rng(0)
    s = np.sin(np.pi * np.arange(1, n + 1) * h)
    u = ah.DeviceArray.from_numpy(np.ascontiguousarray(s[:, None] * s[None, :]), ctx=ctx)
    un = ah.DeviceArray.from_numpy(np.ascontiguousarray(0.9 * s[:, None] * s[None, :]), ctx=ctx)
    v = ah.DeviceArray.from_numpy(rng.standard_normal((n, n)), ctx=ctx)
    res, out = u.zero(), u.zero()
    dt = 10.0 * h * h
    cases = [("bratu2d", ah.bratu2d_, (h, h, 3.51382))]
    for name, G in SCHEMES:
        cases.append((f"heat2d_{name}", G.bind(ah.diffusion_), (un, dt, None, (1.0, h, h, ah.bc_zero_), 0.0)))
        cases.append((f"ignition2d_{name}", G.bind(ah.ignition_), (un, dt, None, (1.0, h, h, 3.51382, ah.bc_zero_), 0.0)))
    rows = []
    for what, F, p in cases:
        rows.append(dict(profiled(ctx, "residual", lambda: F(res, u, p), reps), what=f"{what} residual", mode="residual"))
        F(res, u, p)
        J = ah.JacobianOperator(F, res, u, p, jv="fd")
        rows.append(dict(profiled(ctx, "jv_fd", lambda: ah.mul_(out, J, v, eps=2.0 ** -26), reps), what=f"{what} FD Jv", mode="jv_fd"))
    base = {r["mode"]: r["ps_per_byte"] for r in rows[:2]}
    for r in rows:
        r["per_byte_vs_bratu2d"] = r["ps_per_byte"] / base[r["mode"]]
    return rows


def solve(ctx, n, steps, N=None):
    h = 1.0 / (n + 1)
    dt = 1.0e3 * h * h
    un = ah.DeviceArray(ah.Grid.full(n, n), ctx)
    stats = []
    ctx.sync()
    t0 = time.perf_counter()
    ah.solve(ah.G_Euler_, ah.ignition_, un, (1.0, h, h, 6.0, ah.bc_zero_), dt, [i * dt for i in range(steps + 1)], memory=30,
             krylov_kwargs=dict(restart=True, itmax=300), stats_out=stats, N=N)
    ctx.sync()
    secs = time.perf_counter() - t0
    return dict(n=n, steps=steps, dt=dt, seconds=secs, solved=[bool(r.solved) for r in stats],
                newton=[r.stats.outer_iterations for r in stats], krylov=[r.stats.inner_iterations for r in stats],
                u_max=float(np.max(un.to_numpy())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--solves", action="store_true")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="profiles/ignition")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    variant = os.environ.get("NK_LIB_VARIANT", "")
    sfx = ("_" + args.tag) if args.tag else ""
    n = args.n
    if args.kernels:
        rows = kernels(ctx, n, args.reps)
        out = dict(library_variant=variant, reps=args.reps, n=n, kernels=rows)
        lines = [f"library variant: {variant or '(the product)'}", f"== {n}^2, {args.reps} launches each"]
        for r in rows:
            lines.append(f"  {r['what']:30s} {r['us']:8.1f} us  {r['model_bytes'] / n ** 2:4.0f} B/pt  {100 * r['fraction_of_peak']:5.1f} % of 8 TB/s  "
                         f"{r['ps_per_byte']:.4f} ps/B  x{r['per_byte_vs_bratu2d']:.3f} bratu2d's  {r['kernel']}")
        name = "kernels" + sfx
    elif args.solves:
        solve(ctx, 64, 2, N=ah.multigrid())  # load every kernel before anything is timed
        out, lines = dict(library_variant=variant, solves=[]), []
        lines.append(f"== G_Euler ∘ ignition {n}^2, a = 1, lambda = 6, dt = 1e3 h^2, {args.steps} steps, exact Jv, GMRES(30) restart itmax 300")
        for what, fac in (("N=multigrid", ah.multigrid()), ("plain", None)):
            r = dict(solve(ctx, n, args.steps, N=fac), what=what)
            if fac is not None:
                fac.free()
            out["solves"].append(r)
            lines.append(f"  {what:12s} {r['seconds']:8.3f} s  solved {sum(r['solved'])}/{len(r['solved'])}  max u {r['u_max']:.6f}")
            lines.append(f"    Newton per step {r['newton']}")
            lines.append(f"    Krylov per step {r['krylov']}")
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
