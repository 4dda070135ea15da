#!/usr/bin/env python3
"""Time-to-solution of the multigrid-preconditioned Newton solve against the unpreconditioned one.

For each grid: one Newton solve of 2D Bratu from sin_ic with N = multigrid, then the same solve without a
preconditioner (the headline's Krylov settings: GMRES(30), restart, itmax 300, FD Jv), each timed per Newton step
(wall clock, stream synchronised by the ||F|| every step returns).  Reports the wall time to the same ||F|| (the
one the preconditioned solve ended at), the Newton / Krylov counts, and the per-kernel profile of ONE V-cycle
against each kernel's byte model as a fraction of 8 TB/s.

  python tools/mg_solve.py [--grids 4096x4096,16384x2048] [--out profiles/mg] [--plain-steps 50]

--coarsening semi | both: the semicoarsened hierarchy (N = multigrid(coarsening="semi")) instead of, or next to, the
fully coarsened one in the same session; the plain solve is left out, the V-cycle's result is identified by its
SHA-256 (equal plans must give equal bits) and the per-kernel table names the transfer kernels by their coarsened axes
(mg_restrict_x, mg_prolong_y, ...).  Writes mg_semi_solve.{txt,json}.  --vcycle-only skips the Newton solves: with
the kernel-variant build (NK_KBENCH_LIB=1) and NK_MG_GENERIC=1 the same level pairs run the general transfer kernels,
so two such runs compare each instantiation with the general one.

  python tools/mg_solve.py --coarsening both [--grids 16384x2048,4096x4096] [--vcycle-only] [--tag generic]

--algo cg: Newton-CG (examples/bratu.jl:59-63's algo = :cg, exact Jv) with M = the V-cycle in its SPD form against plain
Newton-CG; a grid given as one number is 1D Bratu (the default grids: 1000 -- BASELINE config 1 -- and bratu.jl's
10000), a 2D grid is run with M only, next to GMRES + N = multigrid on the same grid.  Then the kernels CG's fusion
is about, per launch from one profiled run each: the last level-0 sweep with <r, z> (mg_sweep_dot) against the plain
level-0 sweep (mg_sweep) and dot on a one-level hierarchy of every 2D grid, and the one-launch tail with <r, z>
(mg_tail_dot) against mg_tail and dot on every 1D grid of at most 1024 points.  Writes mg_cg_solve.{txt,json}.

  python tools/mg_solve.py --algo cg [--grids 1000,10000,4096x4096] [--plain-steps 50]

--workload heat2d | heat3d (with --scheme euler | midpoint | trapezoid, --bc periodic, --stiff = a Δt / h_x²): one stiff
implicit heat step on a periodic grid (h = 1 / n per axis, u_n random), the Newton solve with N = multigrid(periodic=True)
and without a preconditioner in one session, Newton / Krylov counts and wall time; then, per launch from the context's
profile classes over --reps profiled V-cycles each, the transfers of the finest level pair of the periodic hierarchy
(mg_restrict_per, mg_prolong_per) next to the Dirichlet hierarchy's (mg_restrict, mg_prolong) on the same extents, both
cut to two levels so that each class holds that pair alone.  Writes mg_periodic_<workload>.{txt,json}.

  python tools/mg_solve.py --workload heat2d --scheme trapezoid --bc periodic --stiff 1000 --grids 8192x8192 --out profiles/mg_periodic
"""
import argparse
import hashlib
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


def newton(ctx, nx, ny, N, max_niter, kw, memory, jv, workspace=None):
    u = ah.DeviceArray.from_numpy(sin_ic(nx, ny), ctx=ctx)
    p = (1.0 / (nx + 1), 1.0 / (ny + 1), LAMBDA)
    hist = []
    ctx.sync()
    t0 = time.perf_counter()
    _, r = ah.newton_krylov_(ah.bratu2d_, u, p, N=N, max_niter=max_niter, memory=memory, krylov_kwargs=kw, jv=jv,
                             workspace=workspace, callback=lambda _u, _res, n_res: hist.append((time.perf_counter() - t0, n_res)))
    ctx.sync()
    return dict(solved=bool(r.solved), outer=r.stats.outer_iterations, inner=r.stats.inner_iterations,
                n_matvec=r.n_matvec, n_res=r.stats.n_res, seconds=time.perf_counter() - t0,
                history=[dict(t=t, n_res=n) for t, n in hist])


def time_to(history, target):
    for h in history:
        if h["n_res"] <= target:
            return h["t"]
    return None


def vcycle_profile(ctx, nx, ny, **opts):
    u = ah.DeviceArray.from_numpy(sin_ic(nx, ny), ctx=ctx)
    p = (1.0 / (nx + 1), 1.0 / (ny + 1), LAMBDA)
    res = u.zero()
    ah.bratu2d_(res, u, p)
    J = ah.JacobianOperator(ah.bratu2d_, res, u, p)
    mg = ah.MultigridPreconditioner(J, **opts)
    z = u.zero()
    for _ in range(2):  # warm
        mg.apply(J, res, z)
    ctx.prof_enable(1)
    ctx.prof_reset()
    t0 = time.perf_counter()
    mg.apply(J, res, z)
    wall = time.perf_counter() - t0
    prof = ctx.prof_read()
    ctx.prof_enable(0)
    rows = []
    for name, e in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
        if not name.startswith("mg_") or not e["timed"]:
            continue
        bw = e["bytes"] / (e["ms"] * 1e-3) if e["ms"] > 0 else 0.0
        rows.append(dict(kernel=name, launches=e["launches"], ms=e["ms"], model_bytes=e["bytes"], model_gbs=bw / 1e9,
                         fraction_of_peak=bw / PEAK))
    levels = mg.levels
    mg.free()
    return dict(levels=levels, wall_ms=wall * 1e3, kernel_ms=sum(r["ms"] for r in rows), kernels=rows,
                z_sha256=hashlib.sha256(z.to_numpy().tobytes()).hexdigest())


def main_semi(args):
    """full and semicoarsened hierarchies in one session (no plain solve)"""
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    kw = dict(restart=True, itmax=300)
    kinds = ["full", "semi"] if args.coarsening == "both" else ["semi"]
    for c in kinds:  # load every kernel before anything is timed
        newton(ctx, 96, 12, ah.multigrid(coarsening=c), 50, kw, args.memory, args.jv)
    out = dict(settings=dict(krylov=kw, memory=args.memory, jv=args.jv, forcing="EisenstatWalker (the default)",
                             tol="1e-6 ||F(u0)|| + 1e-12 (the default)", kbench_lib=os.environ.get("NK_KBENCH_LIB", ""),
                             generic_transfers=os.environ.get("NK_MG_GENERIC", "")), grids=[])
    lines = []
    for g in args.grids.split(","):
        nx, ny = (int(t) for t in g.split("x"))
        row = dict(grid=[nx, ny])
        lines.append(f"== 2D Bratu {nx} x {ny}, GMRES({args.memory}) restart itmax 300, {args.jv.upper()} Jv")
        if not args.vcycle_only:
            # "alone": a solve by itself, as mg_solve.txt times it -- the hierarchy and the Krylov workspace (memory + 1
            # grid vectors) are allocated and freed inside the timed window.  "kept": one factory per hierarchy and one
            # workspace for all, allocated before: the solve's own time.  The two hierarchies alternate.
            for rep in range(2):
                for c in kinds:
                    r = newton(ctx, nx, ny, ah.multigrid(coarsening=c), 50, kw, args.memory, args.jv)
                    r["protocol"] = "alone"
                    row.setdefault(c, []).append(r)
            facs = {c: ah.multigrid(coarsening=c) for c in kinds}
            ws = ah.krylov_workspace("gmres", ah.KrylovConstructor(ah.DeviceArray.from_numpy(sin_ic(nx, ny), ctx=ctx), memory=args.memory))
            for rep in range(args.reps + 1):
                for c in kinds:
                    r = newton(ctx, nx, ny, facs[c], 50, kw, args.memory, args.jv, workspace=ws)
                    r["protocol"] = "kept" if rep else "kept, first (allocates the hierarchy)"
                    row[c].append(r)
            ws.free()
            for c in kinds:
                facs[c].free()
                for r in row[c]:
                    lines.append(f"  N = multigrid({c:<4}) {r['protocol']:<38}: solved {r['solved']}  ||F|| {r['n_res']:.3e}  "
                                 f"Newton {r['outer']}  Krylov {r['inner']}  matvecs {r['n_matvec']}  {r['seconds']:.4f} s")
                row[c + "_median_seconds"] = float(np.median([r["seconds"] for r in row[c] if r["protocol"] == "kept"]))
                lines.append(f"  N = multigrid({c:<4}) median of the {args.reps} solves on the kept hierarchy and workspace: "
                             f"{row[c + '_median_seconds']:.4f} s")
        for c in kinds:
            row["vcycle_" + c] = prof = vcycle_profile(ctx, nx, ny, coarsening=c)
            lines.append(f"  one V-cycle ({c}), {len(prof['levels'])} levels {prof['levels'][:5]} ...: kernels {prof['kernel_ms']:.3f} ms, "
                         f"wall {prof['wall_ms']:.3f} ms, sha256(z) {prof['z_sha256'][:16]}")
            for r in prof["kernels"]:
                lines.append(f"    {r['kernel']:<16} x{r['launches']:<3} {r['ms']:8.3f} ms  model {r['model_bytes'] / 1e6:9.1f} MB  "
                             f"{r['model_gbs']:7.0f} GB/s  {r['fraction_of_peak']:.2f} of 8 TB/s")
        if len(kinds) == 2:
            same_plan = row["vcycle_full"]["levels"] == row["vcycle_semi"]["levels"]
            same_bits = row["vcycle_full"]["z_sha256"] == row["vcycle_semi"]["z_sha256"]
            row["same_plan"], row["same_bits"] = same_plan, same_bits
            lines.append(f"  semi against full: the same plan {same_plan}, the same bits of z {same_bits}")
        out["grids"].append(row)
    text = "\n".join(lines)
    print(text)
    stem = os.path.join(args.out, "mg_semi_solve" + (f"_{args.tag}" if args.tag else ""))
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    with open(stem + ".txt", "w") as f:
        f.write(text + "\n")


def bratu(shape):
    """(residual, u0, p) of 1D / 2D Bratu at sin_ic"""
    if len(shape) == 1:
        n = shape[0]
        return ah.bratu_, np.sin(np.pi * np.arange(1, n + 1) / (n + 1)), (1.0 / (n + 1), LAMBDA)
    nx, ny = shape
    return ah.bratu2d_, sin_ic(nx, ny), (1.0 / (nx + 1), 1.0 / (ny + 1), LAMBDA)


def newton_any(ctx, shape, max_niter, **kw):
    f, u0, p = bratu(shape)
    u = ah.DeviceArray.from_numpy(u0, ctx=ctx)
    ctx.sync()
    t0 = time.perf_counter()
    _, r = ah.newton_krylov_(f, u, p, max_niter=max_niter, **kw)
    ctx.sync()
    return dict(solved=bool(r.solved), outer=r.stats.outer_iterations, inner=r.stats.inner_iterations,
                n_matvec=r.n_matvec, n_res=r.stats.n_res, seconds=time.perf_counter() - t0)


def fusion_profile(ctx, shape, reps=20):
    """per-launch means of the launches one PCG iteration's z = M r, <r, z> is made of, fused and not (one profiled run)"""
    f, u0, p = bratu(shape)
    u = ah.DeviceArray.from_numpy(u0, ctx=ctx)
    res = u.zero()
    f(res, u, p)
    J = ah.JacobianOperator(f, res, u, p)
    # 2D: one level, three sweeps -- every sweep is a level-0 sweep; 1D: the whole cycle is the one-launch tail
    opts = dict(max_levels=1, coarse_sweeps=3) if len(shape) == 2 else {}
    mg = ah.MultigridPreconditioner(J, spd=True, **opts)
    z = u.zero()

    def once():
        mg.vcycle_dot(res, z)
        if len(shape) == 1:
            mg.vcycle(res, z)
        ah.kdot(len(res), res, z)

    once()
    ctx.prof_enable(1)
    ctx.prof_reset()
    for _ in range(reps):
        once()
    prof = ctx.prof_read()
    ctx.prof_enable(0)
    mg.free()
    rows = []
    for name, e in sorted(prof.items()):
        if (name.startswith("mg_") or name == "dot") and e["timed"]:
            us = 1e3 * e["ms"] / e["timed"]
            gbs = e["bytes"] / (e["ms"] * 1e-3) / 1e9 if e["ms"] > 0 else 0.0
            rows.append(dict(kernel=name, timed=e["timed"], us_per_launch=us, model_bytes_per_launch=e["bytes"] / e["timed"],
                             model_gbs=gbs))
    return rows


def main_cg(args):
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    for shape in ((96,), (96, 80)):  # load every kernel before anything is timed
        newton_any(ctx, shape, 50, algo="cg", M=ah.multigrid(spd=True))
        newton_any(ctx, shape, 50, algo="cg")
    newton_any(ctx, (96, 80), 50, N=ah.multigrid, memory=args.memory, krylov_kwargs=dict(restart=True, itmax=300))
    out = dict(settings=dict(jv="exact", forcing="EisenstatWalker (the default)", tol="1e-6 ||F(u0)|| + 1e-12 (the default)",
                             gmres=dict(restart=True, itmax=300, memory=args.memory)), grids=[])
    lines = []
    for g in (args.grids or "1000,10000").split(","):
        shape = tuple(int(t) for t in g.split("x"))
        name = f"{len(shape)}D Bratu {' x '.join(map(str, shape))}"
        row = dict(grid=list(shape))
        row["cg_multigrid"] = mg = newton_any(ctx, shape, 50, algo="cg", M=ah.multigrid(spd=True))
        lines.append(f"== {name}, Newton-CG, exact Jv")
        fmt = "  {:<24}: solved {}  ||F|| {:.3e}  Newton {}  Krylov {}  matvecs {}  {:.4f} s"
        show = lambda tag, r: lines.append(fmt.format(tag, r["solved"], r["n_res"], r["outer"], r["inner"], r["n_matvec"],  # noqa: E731
                                                      r["seconds"]))
        show("cg, M = multigrid(spd)", mg)
        if len(shape) == 1:
            # cg!'s stopping test is on sqrt(<r, M r>), which for M ~ -J^-1 is about h / 2 times ||r|| on the smooth-free
            # residuals of a converging Newton solve: on fine grids Krylov's default atol = sqrt(eps) is met at
            # iteration 0 before Newton's tolerance is.  The same solve with atol = 0:
            row["cg_multigrid_atol0"] = newton_any(ctx, shape, 50, algo="cg", M=ah.multigrid(spd=True),
                                                   krylov_kwargs=dict(atol=0.0))
            show("cg, M, atol = 0", row["cg_multigrid_atol0"])
            row["cg_plain"] = newton_any(ctx, shape, args.plain_steps, algo="cg")
            show("cg, plain", row["cg_plain"])
        else:
            row["gmres_multigrid"] = newton_any(ctx, shape, 50, N=ah.multigrid(), memory=args.memory,
                                                krylov_kwargs=dict(restart=True, itmax=300))
            show(f"gmres({args.memory}), N = multigrid", row["gmres_multigrid"])
        if len(shape) == 2 or shape[0] <= 1024:
            row["fusion"] = fusion_profile(ctx, shape)
            lines.append("  per launch (HIP events), " + ("one-level hierarchy: level-0 sweeps" if len(shape) == 2 else "the one-launch tail"))
            for r in row["fusion"]:
                lines.append(f"    {r['kernel']:<14} x{r['timed']:<4} {r['us_per_launch']:9.2f} us  model {r['model_bytes_per_launch'] / 1e6:8.2f} MB  "
                             f"{r['model_gbs']:7.0f} GB/s")
        out["grids"].append(row)
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "mg_cg_solve.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out, "mg_cg_solve.txt"), "w") as f:
        f.write(text + "\n")


THETA = {"euler": 1.0, "midpoint": 0.5, "trapezoid": 0.5}  # (midpoint: the default α = 1/2)
HEAT_A = 0.01


def heat_step(ctx, shape, scheme, stiff, un0, N, kw, memory, jv, max_niter=50):
    """one implicit step from u_n with a Δt = stiff h_x²: the Newton solve, timed"""
    d = len(shape)
    h = [1.0 / n for n in shape]
    dt = stiff * h[0] * h[0] / HEAT_A
    f = getattr(ah, f"heat{d}d_{scheme}_")
    un = ah.DeviceArray.from_numpy(un0, ctx=ctx)
    p = (un, dt, un.zero(), (HEAT_A, *h, ah.bc_periodic_), 0.0)
    u = un.copy()
    ctx.sync()
    t0 = time.perf_counter()
    _, r = ah.newton_krylov_(f, u, p, N=N, memory=memory, krylov_kwargs=kw, jv=jv, tol_abs=6.0e-6, max_niter=max_niter)
    ctx.sync()
    return dict(solved=bool(r.solved), outer=r.stats.outer_iterations, inner=r.stats.inner_iterations, n_matvec=r.n_matvec,
                n_res=r.stats.n_res, seconds=time.perf_counter() - t0)


def transfer_profile(ctx, shape, k, periodic, reps):
    """per-launch times of the finest pair's transfers on a two-level hierarchy: one profiled V-cycle per repetition"""
    grid = ah.Grid.full(*shape)
    h = [1.0 / n for n in shape]
    mg = ah.MultigridPreconditioner.from_coefficients(grid, [k] * len(shape), -1.0, h=h, max_levels=2, periodic=periodic, ctx=ctx)
    v = ah.DeviceArray.from_numpy(np.random.default_rng(1).standard_normal(tuple(reversed(shape))), ctx=ctx)
    z = v.zero()
    for _ in range(2):
        mg.vcycle(v, z)
    ctx.prof_enable(1)
    per = {}
    for _ in range(reps):
        ctx.prof_reset()
        mg.vcycle(v, z)
        for name, e in ctx.prof_read().items():
            if name.startswith(("mg_restrict", "mg_prolong", "mg_resid", "mg_sweep")) and e["timed"]:
                per.setdefault(name, dict(us=[], model_bytes=e["bytes"] / e["timed"]))["us"].append(1e3 * e["ms"] / e["timed"])
    ctx.prof_enable(0)
    levels = mg.levels
    mg.free()
    return dict(levels=levels, kernels={n: dict(us_min=min(e["us"]), us_median=float(np.median(e["us"])), us_max=max(e["us"]),
                                               model_bytes=e["model_bytes"],
                                               fraction_of_peak_at_median=e["model_bytes"] / (np.median(e["us"]) * 1e-6) / PEAK)
                                           for n, e in sorted(per.items())})


def main_heat(args):
    if args.bc != "periodic":
        raise SystemExit("--workload heat2d / heat3d: only --bc periodic is implemented")
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    d = 2 if args.workload == "heat2d" else 3
    kw = dict(restart=True, itmax=args.itmax)
    small = (96, 48) if d == 2 else (24, 12, 12)
    un_small = np.random.default_rng(0).standard_normal(tuple(reversed(small)))
    for N in (ah.multigrid(periodic=True), None):  # load every kernel before anything is timed
        heat_step(ctx, small, args.scheme, args.stiff, un_small, N, kw, args.memory, args.jv)
    out = dict(settings=dict(workload=args.workload, scheme=args.scheme, bc=args.bc, a_dt_over_hx2=args.stiff, krylov=kw,
                             memory=args.memory, jv=args.jv, tol="6e-6 + 1e-6 ||F(u0)|| (solve's)", h="1 / n per axis"), grids=[])
    lines = []
    for g in args.grids.split(","):
        shape = tuple(int(t) for t in g.split("x"))
        assert len(shape) == d
        un0 = np.random.default_rng(0).standard_normal(tuple(reversed(shape)))
        row = dict(grid=list(shape), levels=ah.multigrid_plan(shape, periodic=True))
        lines.append(f"== {args.workload} {args.scheme} periodic {g}, a dt / hx^2 = {args.stiff:g}, GMRES({args.memory}) restart "
                     f"itmax {args.itmax}, {args.jv.upper()} Jv; {len(row['levels'])} levels")
        fac = ah.multigrid(periodic=True)
        row["multigrid"] = [heat_step(ctx, shape, args.scheme, args.stiff, un0, fac, kw, args.memory, args.jv) for _ in range(3)]
        fac.free()
        row["plain"] = [heat_step(ctx, shape, args.scheme, args.stiff, un0, None, kw, args.memory, args.jv, args.plain_steps)]
        for tag in ("multigrid", "plain"):
            for i, r in enumerate(row[tag]):
                note = " (allocates the hierarchy)" if tag == "multigrid" and i == 0 else ""
                if tag == "plain" and not r["solved"]:
                    note = f" (stopped after {args.plain_steps} Newton steps of itmax {args.itmax}: not solved)"
                lines.append(f"  {'N = multigrid(periodic)' if tag == 'multigrid' else 'plain':<24}: solved {r['solved']}  ||F|| {r['n_res']:.3e}  "
                             f"Newton {r['outer']}  Krylov {r['inner']}  matvecs {r['n_matvec']}  {r['seconds']:.4f} s{note}")
        theta = THETA[args.scheme]
        k = theta * args.stiff / shape[0] ** 2
        for tag, periodic in (("periodic", True), ("dirichlet", False), ("periodic_again", True), ("dirichlet_again", False)):
            row["transfers_" + tag] = prof = transfer_profile(ctx, shape, k, periodic, args.reps)
            lines.append(f"  two-level hierarchy {prof['levels']}, {tag}: per launch over {args.reps} profiled cycles (min / median / max us)")
            for n, e in prof["kernels"].items():
                lines.append(f"    {n:<20} {e['us_min']:9.1f} {e['us_median']:9.1f} {e['us_max']:9.1f}   model {e['model_bytes'] / 1e6:8.1f} MB  "
                             f"{e['fraction_of_peak_at_median']:.2f} of 8 TB/s")
        out["grids"].append(row)
    text = "\n".join(lines)
    print(text)
    stem = os.path.join(args.out, f"mg_periodic_{args.workload}")
    with open(stem + ".json", "w") as f:
        json.dump(out, f, indent=1)
    with open(stem + ".txt", "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="gmres", choices=["gmres", "cg"])
    ap.add_argument("--grids", default=None, help="gmres: 4096x4096,16384x2048; cg: 1000,10000 (one number: 1D Bratu)")
    ap.add_argument("--out", default="profiles/mg")
    ap.add_argument("--plain-steps", type=int, default=50, help="Newton steps the unpreconditioned solve may take")
    ap.add_argument("--memory", type=int, default=30)
    ap.add_argument("--jv", default="fd")
    ap.add_argument("--coarsening", default="full", choices=["full", "semi", "both"])
    ap.add_argument("--vcycle-only", action="store_true", help="--coarsening semi | both: the V-cycle profiles without the solves")
    ap.add_argument("--reps", type=int, default=5, help="--coarsening semi | both: timed solves per hierarchy")
    ap.add_argument("--tag", default="", help="--coarsening semi | both: suffix of the output files")
    ap.add_argument("--workload", default="bratu", choices=["bratu", "heat2d", "heat3d"])
    ap.add_argument("--scheme", default="trapezoid", choices=["euler", "midpoint", "trapezoid"])
    ap.add_argument("--bc", default="zero", choices=["zero", "periodic"])
    ap.add_argument("--stiff", type=float, default=1000.0, help="--workload heat*: a dt / h_x^2 of the step")
    ap.add_argument("--itmax", type=int, default=300, help="--workload heat*: Krylov itmax per Newton step")
    args = ap.parse_args()
    if args.workload != "bratu":
        if not args.grids:
            raise SystemExit("--workload heat*: give --grids")
        return main_heat(args)
    if args.algo == "cg":
        return main_cg(args)
    args.grids = args.grids or "4096x4096,16384x2048"
    if args.coarsening != "full":
        return main_semi(args)
    os.makedirs(args.out, exist_ok=True)
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    kw = dict(restart=True, itmax=300)
    for N in (ah.multigrid, None):  # load every kernel before anything is timed
        newton(ctx, 96, 80, N, 50, kw, args.memory, args.jv)
    out = dict(settings=dict(krylov=kw, memory=args.memory, jv=args.jv, forcing="EisenstatWalker (the default)",
                             tol="1e-6 ||F(u0)|| + 1e-12 (the default)"), grids=[])
    lines = []
    for g in args.grids.split(","):
        nx, ny = (int(t) for t in g.split("x"))
        mg = newton(ctx, nx, ny, ah.multigrid(), 50, kw, args.memory, args.jv)
        plain = newton(ctx, nx, ny, None, args.plain_steps, kw, args.memory, args.jv)
        target = mg["n_res"]
        t_plain = time_to(plain["history"], target)
        prof = vcycle_profile(ctx, nx, ny)
        out["grids"].append(dict(grid=[nx, ny], multigrid=mg, plain=plain, target_n_res=target,
                                 plain_seconds_to_target=t_plain, vcycle=prof))
        lines.append(f"== 2D Bratu {nx} x {ny}, GMRES({args.memory}) restart itmax 300, {args.jv.upper()} Jv")
        lines.append(f"  N = multigrid : solved {mg['solved']}  ||F|| {mg['n_res']:.3e}  Newton {mg['outer']}  Krylov {mg['inner']}  "
                     f"matvecs {mg['n_matvec']}  {mg['seconds']:.4f} s")
        reached = f"{t_plain:.4f} s" if t_plain is not None else f"not reached in {plain['outer']} Newton steps"
        lines.append(f"  plain         : solved {plain['solved']}  ||F|| {plain['n_res']:.3e}  Newton {plain['outer']}  Krylov {plain['inner']}  "
                     f"matvecs {plain['n_matvec']}  {plain['seconds']:.4f} s;  to ||F|| <= {target:.3e}: {reached}")
        lines.append(f"  one V-cycle, {len(prof['levels'])} levels: kernels {prof['kernel_ms']:.3f} ms, wall {prof['wall_ms']:.3f} ms")
        for r in prof["kernels"]:
            lines.append(f"    {r['kernel']:<12} x{r['launches']:<3} {r['ms']:8.3f} ms  model {r['model_bytes'] / 1e6:9.1f} MB  "
                         f"{r['model_gbs']:7.0f} GB/s  {r['fraction_of_peak']:.2f} of 8 TB/s")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(args.out, "mg_solve.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(args.out, "mg_solve.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
