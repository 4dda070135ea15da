"""The tail group of the fully resident MGS sweep (k_mgs_res in csrc/nk_resident.hip).

With a tail group of tg slots a pass runs in three phases: the last tg LDS slots are updated first (q -= h V_i, on
the lines the previous pass loaded last), then the register slots and the remaining LDS slots run the fused update +
dot as before, then the tail's dot runs, in slot order.  Only the order of the elementwise updates moves: the chain of
partial sums is the one of the schedule without a tail, so every result is the same bits.

`tail_plan` restates the host rule (res_plan, csrc/nk_plan.hpp) on top of test_hip_resident_variants.py's `sweep_plan`;
a CPU test holds every case of the table against the geometry it names (256 blocks, 39 LDS slots), and
tests/test_plan.py holds both restatements against the product's rule.  Each GPU case runs in a child process on the
kernel-variant build with NK_RES_TAIL=16, whatever size the product compiles in: short restarted GMRES solves (memory 8, itmax 12: sweeps of
2 to 8 passes, 2 to 16 with reorthogonalisation), plain and with reorthogonalisation, the history and x bit for bit
against the oracle in device order (test_hip_resident_variants.py's harness), the tail the rule predicts launched,
every step of two passes or more resident.  A one-pass step (the first of a cycle without reorthogonalisation) takes
the per-pass chain by design (test_hip_resident_variants.py's `sweep_steps`), so `mgs_passes` advances by exactly the
number of such steps and by 0 with reorthogonalisation.  The kbench case compares the hook's q and Hessenberg column
between tail sizes, and against kernel variant 1000 on the schedule without a tail.
"""
import json
import os
import subprocess
import sys
from collections import namedtuple

import pytest

import _nkpath  # noqa: F401
from ariadne_hip import _lib

from test_hip_resident_variants import K_RES_MAX, sweep_plan, whole_slots

G_TEST = 16  # the configured tail of the GPU cases (NK_RES_TAIL)


def tail_plan(n, g, G=256, rl=39):
    """The host rule: the tail is the configured g clamped to the LDS slots in use, and only at full residency."""
    rv, rl, full, _, _ = sweep_plan(n, G, rl)
    return min(g, rl) if full and g > 0 else 0


def geometry(n):
    """(whole, rv, rl, full) of n doubles on 256 blocks with 39 LDS slots."""
    return (whole_slots(n),) + sweep_plan(n)[:3]


def sweep_steps(itmax, memory, reorth):
    """(steps whose sweep is one resident launch, one-pass steps that take the chain) of a restarted solve."""
    steps = [k for c in range(0, itmax, memory) for k in range(1, min(memory, itmax - c) + 1)]
    np_ = [2 * k if reorth else k for k in steps]
    return sum(1 for p in np_ if 2 <= p <= K_RES_MAX), sum(1 for p in np_ if p < 2)


# fused = LDS slots left in the fused loop, tg = the tail launched (configured g = 16)
Case = namedtuple("Case", "nx ny whole rv rl full tg fused jacobi kresmax")
CASES = [
    Case(1024, 512, 4, 0, 4, True, 4, 0, False, False),  # tg clamps to rl = 4: the fused LDS loop is empty
    Case(1024, 1024, 8, 0, 8, True, 8, 0, False, True),  # same; + GMRES(32) with reorthogonalisation: 64 passes
    Case(2048, 1856, 29, 0, 29, True, 16, 13, False, False),  # 13 fused LDS slots (3 groups of 4 + 1) + 16 tail
    Case(2048, 2496, 39, 0, 39, True, 16, 23, False, False),  # all LDS slots in use
    Case(2048, 3520, 55, 16, 39, True, 16, 23, True, False),  # register slots + LDS + tail; plain and Jacobi N
    Case(2048, 2560, 40, 0, 39, False, 0, 39, False, False),  # one streamed slot: not full, the rule gives 0
]
KBENCH_SHAPES = [(2048, 1856), (4096, 4096)]
KBENCH_TAILS = (0, 8, 16, 24)


def case_id(c):
    return f"{c.nx}x{c.ny}-rv{c.rv}-rl{c.rl}-tg{c.tg}"


def test_cases_reach_the_geometry_they_name():
    for c in CASES:
        assert geometry(c.nx * c.ny) == (c.whole, c.rv, c.rl, c.full), c
        assert tail_plan(c.nx * c.ny, G_TEST) == c.tg, c
        assert c.rl - c.tg == c.fused, c
        assert tail_plan(c.nx * c.ny, 0) == 0
    assert [c.fused % 4 for c in CASES[2:4]] == [1, 3]  # fused loops that end in single slots
    assert sum(1 for c in CASES if c.full and c.fused == 0) == 2 and sum(1 for c in CASES if not c.full) == 1
    # the kbench case: what the rule predicts for each tail at its two shapes (4096^2: rv 89 + 39 LDS slots)
    assert geometry(4096 * 4096) == (128, 89, 39, True)
    assert [tail_plan(2048 * 1856, t) for t in KBENCH_TAILS] == [0, 8, 16, 24]
    assert [tail_plan(4096 * 4096, t) for t in KBENCH_TAILS + (64,)] == [0, 8, 16, 24, 39]
    # passes per launch: 2 .. 8 plain, 2 .. 16 with reorthogonalisation, 64 = kResMax at GMRES(32)
    assert sweep_steps(12, 8, False) == (10, 2) and sweep_steps(12, 8, True) == (12, 0)
    assert sweep_steps(32, 32, True) == (32, 0)


def test_tail_knob_is_absent_from_the_product_library():
    prod = open(_lib.PRODUCT_LIB, "rb").read()
    kb = open(_lib.KBENCH_LIB, "rb").read()
    assert b"NK_RES_TAIL" not in prod and b"NK_RES_TAIL" in kb
    for sym in (b"nkb_mgs_res_tail", b"nkb_res_tail_last"):
        assert sym not in prod and sym in kb, sym


# ----------------------------------------------------------------------------------------------- GPU
TESTS = os.path.dirname(os.path.abspath(__file__))

_SOLVE_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/..")
import test_hip_resident_variants as tv
import ariadne_hip as ah
from oracle import oracle as oc
nx, ny = int(sys.argv[2]), int(sys.argv[3])
runs = json.loads(sys.argv[4])
ctx = ah.Context(0)
ah.set_default_context(ctx)
lib = ah.load()
P, u, b = tv.problem(nx, ny)
out = []
for r in runs:
    run = tv.device_solve(ctx, P, u, b, memory=r["memory"], itmax=r["itmax"], reorth=r["reorth"], precond=r["jacobi"])
    tail = lib.nkb_res_tail_last()
    G = ctx.path_info()["resident_blocks"]
    kw = dict(jv="exact", memory=r["memory"], restart=True, reorthogonalization=r["reorth"], atol=0.0, rtol=0.0,
              itmax=r["itmax"])
    if r["jacobi"]:
        kw["N"] = ("diag", oc.jacobian_diag(P, u, reciprocal=True))
    oc.set_devred(True, cus=G)
    try:
        xr, _, hr = oc.krylov_solve(P, u, b, **kw)
    finally:
        oc.set_devred(False)
    h = np.array(run.stats.residuals)
    out.append(dict(run=r, G=G, tail=tail, kernel=run.prof.get("kernel", ""), launches=run.prof.get("launches", 0),
                    sweeps=run.sweeps_resident, passes=run.mgs_passes, niter=run.stats.niter,
                    h_equal=bool(h.shape == hr.shape and np.array_equal(h, hr)), x_equal=bool(np.array_equal(run.x, xr)),
                    h_dev=float(np.max(np.abs(h / hr - 1.0))) if h.shape == hr.shape else -1.0,
                    x_dev=float(np.max(np.abs(run.x - xr)) / np.max(np.abs(xr)))))
ctx.sync()
print("RESULT " + json.dumps(out))
"""


def child(code, argv, env, timeout):
    p = subprocess.run([sys.executable, "-c", code, TESTS] + [str(a) for a in argv],
                       env=dict(os.environ, NK_KBENCH_LIB="1", **env), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tail_solves_match_oracle(case):
    """GMRES(8), 12 steps, plain and with reorthogonalisation (+ a Jacobi N where the sweep writes q back, + GMRES(32)
    with reorthogonalisation at 1024^2: a sweep of kResMax passes) on the kernel-variant build with NK_RES_TAIL=16."""
    runs = [dict(memory=8, itmax=12, reorth=False, jacobi=False), dict(memory=8, itmax=12, reorth=True, jacobi=False)]
    if case.jacobi:
        runs.append(dict(memory=8, itmax=12, reorth=False, jacobi=True))
    if case.kresmax:
        runs.append(dict(memory=32, itmax=32, reorth=True, jacobi=False))
    res = child(_SOLVE_CHILD, [case.nx, case.ny, json.dumps(runs)], dict(NK_RES_TAIL=str(G_TEST)), 300)
    assert len(res) == len(runs)
    for r in res:
        print(f"\n{case_id(case)} {r}")
        if r["G"] != 256:
            pytest.skip(f"{r['G']} blocks: the case table is for 256")
        resident, one_pass = sweep_steps(r["run"]["itmax"], r["run"]["memory"], r["run"]["reorth"])
        assert r["kernel"].startswith(f"nk::k_mgs_res<{case.rv},"), r
        assert r["tail"] == case.tg, r
        assert r["niter"] == r["run"]["itmax"]
        assert r["launches"] >= resident > 0 and r["sweeps"] >= resident, r
        assert r["passes"] == one_pass, r  # no step of two passes or more took the per-pass chain
        assert r["h_equal"], r
        assert r["x_equal"], r


_KBENCH_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1] + "/..")
import _nkpath
import ariadne_hip as ah
n, k = int(sys.argv[2]), int(sys.argv[3])
calls = json.loads(sys.argv[4])  # [rv, tail] pairs; the first is the reference
ctx = ah.Context(0)
lib = ah.load()
PD = C.POINTER(C.c_double)
lib.nkb_mgs_res_tail.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, PD, PD, PD, PD, PD,
                                 C.POINTER(C.c_int)]
out, ref = [], None
for rv, tail in calls:
    us, chain, got = C.c_double(), C.c_double(), C.c_int()
    diff = (C.c_double * 4)()
    q, col = np.empty(n), np.empty(k + 1)
    rc = lib.nkb_mgs_res_tail(ctx.handle, n, k, rv, tail, 1, C.byref(us), C.byref(chain), diff, q.ctypes.data_as(PD),
                              col.ctypes.data_as(PD), C.byref(got))
    assert rc == 0, (rv, tail, rc, lib.nk_last_error(ctx.handle))
    if ref is None:
        ref = (q, col)
    out.append(dict(rv=rv, tail=tail, launched=got.value, q_equal=bool(np.array_equal(q, ref[0])),
                    col_equal=bool(np.array_equal(col, ref[1])), chain_q=diff[0], chain_h=diff[1],
                    finite=bool(np.all(np.isfinite(col)) and np.all(np.isfinite(q)) and np.any(q != 0.0))))
print("RESULT " + json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KBENCH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kbench_tails_are_bitwise(shape):
    """The hook's 5-pass sweep at tail 0 against 8, 16 and 24, one child process per shape: the same q and Hessenberg
    column, the launched tail the rule's.  At 4096^2 kernel variant 1000 (the headline instantiation, named
    explicitly) on the schedule without a tail gives the same bits too; at 2048 x 1856 its 89 register slots do not
    fit, and a second child checks that NK_RES_TAIL alone sets the tail."""
    n, k = shape[0] * shape[1], 5
    calls = [[-1, t] for t in KBENCH_TAILS] + ([[1000, 0], [1000, 16]] if shape == (4096, 4096) else [])
    res = child(_KBENCH_CHILD, [n, k, json.dumps(calls)], {}, 300)
    for r in res:
        print(f"\n{shape} {r}")
        assert r["launched"] == tail_plan(n, r["tail"]), r
        assert r["finite"] and r["q_equal"] and r["col_equal"], r
    if shape != (4096, 4096):
        res = child(_KBENCH_CHILD, [n, k, json.dumps([[-1, -1], [-1, 0]])], dict(NK_RES_TAIL="8"), 300)
        assert [r["launched"] for r in res] == [8, 0] and all(r["q_equal"] and r["col_equal"] for r in res), res
