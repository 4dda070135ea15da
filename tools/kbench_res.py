"""A/B of the resident MGS sweep (one launch per Arnoldi step, q on chip) against the per-pass
chain of k_mgs_pass launches, on the same q and basis.  Not part of the product.

Usage (GPU box): python tools/kbench_res.py [--n 16777216] [--ks 8,16,30] [--rvs 0,16,32,48]
                 python tools/kbench_res.py --ks 2,3,16,30 --rvs 1000 --tails 0,8,16,24,32 [--rounds 3]

--tails: the tail-group sizes of the sweep, interleaved: every round times each tail once, in
order, in this one process; the table at the end gives each tail's median us per pass and its q and
Hessenberg column compared bit for bit with the first tail's.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NK_KBENCH_LIB", "1")  # the nkb_* hooks live in lib/libnkhip_kbench.so
import _nkpath  # noqa: F401,E402
import ariadne_hip as ah  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096 * 4096)
ap.add_argument("--ks", default="8,16,30")
ap.add_argument("--rvs", default="0,16,32,48")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tails", default="", help="tail-group sizes to interleave, e.g. 0,8,16,24,32")
ap.add_argument("--rounds", type=int, default=3, help="with --tails: interleaved rounds")
args = ap.parse_args()

ctx = ah.Context(0)
lib = ah.load()
PD = C.POINTER(C.c_double)
lib.nkb_mgs_res.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, PD, PD, PD]
lib.nkb_mgs_res_tail.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, PD, PD, PD, PD, PD,
                                 C.POINTER(C.c_int)]


def tail_run(k, rv, tail, keep):
    """One timed hook call at this tail: (us per pass, chain us per pass, the tail launched, q, column)."""
    import numpy as np

    us, ref, got = C.c_double(), C.c_double(), C.c_int()
    diff = (C.c_double * 4)()
    q = np.empty(args.n if keep else 0)
    col = np.empty(k + 1)
    rc = lib.nkb_mgs_res_tail(ctx.handle, args.n, k, rv, tail, args.reps, C.byref(us), C.byref(ref), diff,
                              q.ctypes.data_as(PD) if keep else None, col.ctypes.data_as(PD), C.byref(got))
    if rc != 0:
        print(f"k={k} rv={rv} tail={tail}: rc={rc} {lib.nk_last_error(ctx.handle)}", flush=True)
        sys.exit(1)
    return us.value, ref.value, got.value, q, col


for k in [int(x) for x in args.ks.split(",")]:
    for rv in [int(x) for x in args.rvs.split(",")]:
        if args.tails:
            import numpy as np

            tails = [int(x) for x in args.tails.split(",")]
            times = {t: [] for t in tails}
            first, same, launched = None, {}, {}
            for r in range(args.rounds):
                for t in tails:
                    us, ref, got, q, col = tail_run(k, rv, t, keep=(r == 0))
                    times[t].append(us)
                    launched[t] = got
                    if r == 0:
                        if first is None:
                            first = (q, col)
                        same[t] = bool(np.array_equal(q, first[0]) and np.array_equal(col, first[1]))
                    print(f"k={k:2d} rv={rv} round {r} tail {t:2d} (launched {got:2d})  {us:7.2f} us/pass   "
                          f"chain {ref:7.2f}", flush=True)
            base = statistics.median(times[tails[0]])
            for t in tails:
                m = statistics.median(times[t])
                print(f"k={k:2d} rv={rv} TAIL {t:2d} (launched {launched[t]:2d})  median {m:7.2f} us/pass  "
                      f"min {min(times[t]):7.2f}  max {max(times[t]):7.2f}  vs tail {tails[0]}: {100 * (m / base - 1):+5.2f} %  "
                      f"bitwise {'same' if same[t] else 'DIFFERENT'}", flush=True)
            continue
        us, ref = C.c_double(), C.c_double()
        diff = (C.c_double * 4)()
        rc = lib.nkb_mgs_res(ctx.handle, args.n, k, rv, args.reps, C.byref(us), C.byref(ref), diff)
        if rc != 0:
            print(f"k={k} rv={rv}: rc={rc} {lib.nk_last_error(ctx.handle)}", flush=True)
            sys.exit(1)
        print(f"k={k:2d} rv={rv:2d}  resident {us.value:7.2f} us/pass   chain {ref.value:7.2f} us/pass   "
              f"speedup {ref.value / us.value:5.2f}x   q diff {diff[0]:.2e}  h diff {diff[1]:.2e}  (LDS slots {diff[2]:.0f}, {diff[3]:.0f} blocks)", flush=True)
