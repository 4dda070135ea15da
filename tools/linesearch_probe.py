"""Time one line-search trial three ways on an MI355X: nk_residual_trial (the fused kernel: read u, read v, write F,
24 B/pt on the 2D Bratu byte model), the materialised sequence it replaces (copy + nk_axpy + nk_residual_norm,
56 B/pt) and nk_residual_norm alone (the floor: 16 B/pt), at 4096^2 Bratu 2D, 512^3 heat Euler and 256^3 Bratu 3D.
All three end in the norm's host synchronisation, as a line search uses them.  Then one end-to-end line: the
1D Bratu case whose full steps fail (N = 100, lambda = 3.5, u0 = 8 sin) with and without the line search.

    python tools/linesearch_probe.py [--out profiles/linesearch/probe.json] [--rounds 7] [--calls 20]

Per variant and shape: `rounds` timed windows of `calls` calls each, the variants alternating within a round, after
a warm-up of every variant; the median window and the spread (min .. max) are reported per call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402


def shapes():
    n2, n3h, n3b = 4096, 512, 256
    yield "bratu2d 4096^2", (n2, n2), ah.bratu2d_, lambda un: (1.0 / (n2 + 1), 1.0 / (n2 + 1), 3.51382), 0
    h = 1.0 / (n3h + 1)
    yield ("heat3d euler 512^3", (n3h, n3h, n3h), ah.G_Euler_.bind(ah.diffusion3d_),
           lambda un: (un, 0.1 * h * h / 0.01, None, (0.01, h, h, h, ah.bc_zero_), 0.0), 1)
    hb = 1.0 / (n3b + 1)
    yield "bratu3d 256^3", (n3b, n3b, n3b), ah.bratu3d_, lambda un: (hb, hb, hb, 3.51382), 0


def window(f, calls, ctx):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    ctx.sync()
    return (time.perf_counter() - t0) / calls * 1e6  # us per call


def probe(ctx, name, shape, F, mkp, n_un, rounds, calls):
    rng = np.random.default_rng(0)
    np_shape = shape[::-1]
    r = rng.standard_normal(np_shape)  # one draw, three fields (host time: the draw dominates at 512^3)
    u = ah.DeviceArray.from_numpy(0.5 * r)
    v = ah.DeviceArray.from_numpy(np.ascontiguousarray(r[..., ::-1]))
    un = ah.DeviceArray.from_numpy(np.ascontiguousarray(0.5 * r[::-1])) if n_un else None
    del r
    p = mkp(un)
    out, w = u.zero(), u.zero()
    n = len(u)
    s = -0.5

    def fused():
        return F.residual_trial(out, u, v, s, p)

    def materialised():
        ah.kcopy_(n, w, u)
        ah.kaxpy_(n, s, v, w)
        return F.residual_norm(out, w, p)

    def floor():
        return F.residual_norm(out, u, p)

    variants = {"residual_trial": fused, "copy+axpy+residual_norm": materialised, "residual_norm": floor}
    a, b = fused(), materialised()
    assert a == b, (name, a, b)  # the same bits, at the size that is timed
    for f in variants.values():
        for _ in range(5):
            f()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            times[k].append(window(f, calls, ctx))
    words = {"residual_trial": 3 + n_un, "copy+axpy+residual_norm": 7 + n_un, "residual_norm": 2 + n_un}
    row = {"shape": name, "points": n}
    for k, t in times.items():
        med = statistics.median(t)
        row[k] = dict(us=med, us_min=min(t), us_max=max(t), bytes_per_point=8 * words[k],
                      gb_per_s=8.0 * words[k] * n / med / 1e3)
    row["ratio_fused_over_materialised"] = row["residual_trial"]["us"] / row["copy+axpy+residual_norm"]["us"]
    row["ratio_model"] = words["residual_trial"] / words["copy+axpy+residual_norm"]
    row["ratio_fused_over_floor"] = row["residual_trial"]["us"] / row["residual_norm"]["us"]
    for x in (u, v, out, w) + ((un,) if un is not None else ()):
        x.free()
    return row


def end_to_end(ctx, repeats=5):
    N, lam = 100, 3.5
    p = (1.0 / (N + 1), lam)
    u0 = 8.0 * np.sin(np.pi * np.arange(1, N + 1) / (N + 1))
    out = {}
    for key, ls in (("full_step", None), ("backtracking", ah.Backtracking())):
        ts, r = [], None
        for _ in range(repeats + 1):
            u = ah.DeviceArray.from_numpy(u0)
            ctx.sync()
            t0 = time.perf_counter()
            _, r = ah.newton_krylov_(ah.bratu_, u, p, algo="gmres", memory=100, forcing=None, jv="exact", linesearch=ls)
            ctx.sync()
            ts.append(time.perf_counter() - t0)
        steps = max(1, r.stats.outer_iterations)
        trials = (r.stats.outer_iterations + r.n_backtrack) / steps if ls is not None else 0.0
        out[key] = dict(seconds=statistics.median(ts[1:]), solved=bool(r.solved), outer=r.stats.outer_iterations,
                        inner=r.stats.inner_iterations, n_backtrack=r.n_backtrack, trial_launches_per_step=trials,
                        n_res=r.stats.n_res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    ctx = ah.Context(0)
    ah.set_default_context(ctx)
    rows = [probe(ctx, *sh, args.rounds, args.calls) for sh in shapes()]
    res = dict(rows=rows, end_to_end_bratu1d=end_to_end(ctx), rounds=args.rounds, calls=args.calls)
    for r in rows:
        print(f"{r['shape']}: trial {r['residual_trial']['us']:.1f} us ({r['residual_trial']['gb_per_s']:.0f} GB/s), "
              f"materialised {r['copy+axpy+residual_norm']['us']:.1f} us, residual_norm {r['residual_norm']['us']:.1f} us; "
              f"trial / materialised = {r['ratio_fused_over_materialised']:.2f} (model {r['ratio_model']:.2f}), "
              f"trial / floor = {r['ratio_fused_over_floor']:.2f}")
    print("end to end, 1D Bratu N = 100:", json.dumps(res["end_to_end_bratu1d"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.sync()


if __name__ == "__main__":
    main()
