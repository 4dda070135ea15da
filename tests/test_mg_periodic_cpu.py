"""The multigrid V-cycle on periodic grids (periodic=True; DESIGN.md §10 "Periodic grids"): everything that needs no GPU.

* the host-only rules of csrc/nk_mg_plan.hpp -- mg_plan_per and the periodic transfer index functions that the kernels
  call -- through a small g++ program (built under the address and undefined-behaviour sanitizers where the toolchain
  links them), against the Python restatements of this file; nk_mg_plan_periodic through ctypes;
* the numpy restatement of the periodic cycle (`PerCycle`, a subclass of test_hip_multigrid.py's `Cycle`: nested levels,
  wrapped neighbours, h_l = h_0 n_0 / n_l) against a second derivation, explicit long-double matrices with P built from
  the periodic hat function; the dense V is symmetric and σV positive definite for equal pre / post sweeps;
* the float64-versus-long-double sensitivities that the GPU file's tolerances are made of, recorded as constants and
  measured again here (within 1.5 x; no constant comes from device output);
* the host-only refusals of the Python layer;
* the restated GMRES counts of the GPU file's solver cases.

tests/test_hip_multigrid_periodic.py imports the restatement, the cases and the constants from here.
"""
import ctypes as C
import os
import subprocess
import tempfile
import types
from collections import namedtuple
from fractions import Fraction
from itertools import product

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from ariadne_hip import _lib
from oracle import oracle as oc

from test_hip_multigrid import ALPHA, Cycle, fake_operator, gmres_right, rel
from test_hip_multigrid_options import kron_axes, within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "newtonkrylov.jl_amd", "csrc")
MAX_LEVELS = 32  # kMgMaxLevels

# float64 versus long double, max-abs over the result relative to its max-abs (test_sensitivities_are_as_recorded
# measures each again and holds it within 1.5 x):
#   PER_DENSE_SENSITIVITY   the dense matrix recursion's V over DENSE_CASES                        measured 9.236e-16
#   PER_UNIT_SENSITIVITY    the restatement applied to the unit vectors of those cases             measured 6.063e-16
#   PER_CYCLE_SENSITIVITY   the restatement over CYCLE_CASES and the coefficient case              measured 3.728e-16
PER_DENSE_SENSITIVITY = 9.2e-16
PER_UNIT_SENSITIVITY = 6.1e-16
PER_CYCLE_SENSITIVITY = 3.7e-16


# ------------------------------------------------------------------------------------ the restatement
def halvable(n):
    return n % 2 == 0 and n >= 6


def plan_per(shape, max_levels=0):
    lv = [tuple(shape)]
    while any(halvable(n) for n in lv[-1]) and (max_levels == 0 or len(lv) < max_levels) and len(lv) < MAX_LEVELS:
        lv.append(tuple(n // 2 if halvable(n) else n for n in lv[-1]))
    return lv


def prolong_per_1d(nf, nc, dt):
    """an even fine i takes e_c[i / 2], an odd one half of each wrapped neighbour; a kept axis is the identity"""
    if nf == nc:
        return np.eye(nf, dtype=dt)
    assert nf == 2 * nc
    P = np.zeros((nf, nc), dtype=dt)
    for i in range(nf):
        if i % 2 == 0:
            P[i, i // 2] = 1
        else:
            P[i, (i - 1) // 2] += dt(1) / dt(2)
            P[i, ((i + 1) // 2) % nc] += dt(1) / dt(2)
    return P


def transfers_per(nf, nc, dt):
    P = prolong_per_1d(nf, nc, dt)
    return P, (P / P.sum(axis=0)).T


def d2_per(x, a):
    """x_- + x_+ - 2 x along grid axis a, neighbours wrap"""
    ax = x.ndim - 1 - a
    return np.roll(x, 1, ax) + np.roll(x, -1, ax) - 2 * x


class PerCycle(Cycle):
    """The cycle on a periodic grid: Cycle's smoother and recursion on nested levels, with wrapped neighbours, the
    periodic transfers and the coarse spacings h_l = h_0 (n_0 / n_l)."""

    def __init__(self, shape, h, k, s0, nu=2, coarse_sweeps=8, omega=None, max_levels=0, dt=np.float64):
        from test_hip_multigrid import along

        d = len(shape)
        self.dt, self.nu, self.cs = dt, nu, coarse_sweeps
        self.omega = dt(omega) if omega else dt(2 * d) / dt(2 * d + 1)
        self.levels = plan_per(shape, max_levels)
        self.c, self.s, self.diag, self.P, self.R = [], [], [], [], []
        s = np.asarray(s0, dtype=dt) * np.ones(tuple(reversed(shape)), dtype=dt)
        for l, ext in enumerate(self.levels):
            if l > 0:
                Ps, Rs = zip(*[transfers_per(nf, nc, dt) for nf, nc in zip(self.levels[l - 1], ext)])
                for a in range(d):
                    s = along(Rs[a], s, a)
            hl = [dt(h[a]) * dt(shape[a] // ext[a]) for a in range(d)]
            c = [dt(k[a]) / (hl[a] * hl[a]) for a in range(d)]
            diag = s - 2 * sum(c)
            if not (np.all(diag > 0) or np.all(diag < 0)):
                self.levels = self.levels[:l]
                break
            if l > 0:
                self.P.append(Ps)
                self.R.append(Rs)
            self.c.append(c)
            self.s.append(s)
            self.diag.append(diag)

    def A(self, l, x):
        return sum(self.c[l][a] * d2_per(x, a) for a in range(len(self.c[l]))) + self.s[l] * x

    def vcycle(self, b, l=0):
        """Cycle.vcycle over the grid axes only (counted from the last), so that b may carry leading batch axes"""
        from test_hip_multigrid import along

        b = np.asarray(b, dtype=self.dt)
        x, d = np.zeros_like(b), len(self.c[l])
        if l == len(self.levels) - 1:
            return self.smooth(l, x, b, self.cs)
        x = self.smooth(l, x, b, self.nu)
        r = b - self.A(l, x)
        for a in range(d):
            r = along(self.R[l][a], r, a)
        e = self.vcycle(r, l + 1)
        for a in range(d):
            e = along(self.P[l][a], e, a)
        return self.smooth(l, x + e, b, self.nu)


def unit_matrix(cyc, shape):
    """the matrix of the restated cycle: all unit vectors as one batch"""
    n = int(np.prod(shape))
    return cyc.vcycle(np.eye(n, dtype=cyc.dt).reshape((n,) + tuple(reversed(shape)))).reshape(n, n).T


# ------------------------------------------------------------------------------------ the dense form
DENSE_GRIDS = [(12, 6), (3, 12), (12, 6, 6), (6, 5, 12)]
DENSE_S = ["const", "var"]
DENSE_OPTS = [(1, 1), (1, 8), (2, 1), (2, 8)]
DENSE_CASES = [(g, sk, nu, cs) for g in DENSE_GRIDS for sk in DENSE_S for nu, cs in DENSE_OPTS]
DENSE_IDS = [f"{'x'.join(map(str, g))}-{sk}-nu{nu}-cs{cs}" for g, sk, nu, cs in DENSE_CASES]


def dense_coefficients(shape, skind):
    """(h, k, s_0): h = 1 / n, k = 1; s the constant -1, or a positive s that varies along every axis and is symmetric
    along none (below 2 Σ_a c_a on every level, so the diagonal keeps its sign)"""
    h = [1.0 / n for n in shape]
    if skind == "const":
        return h, [1.0] * len(shape), -1.0
    arg, tilt = 1.0, 0.0
    for a, n in enumerate(shape):
        x = (np.arange(n) * h[a]).reshape([-1 if b == len(shape) - 1 - a else 1 for b in range(len(shape))])
        arg, tilt = arg * np.sin(np.pi * (x + 0.1)), tilt + 0.3 * (a + 1) * x
    return h, [1.0] * len(shape), 3.5 * np.exp(arg + tilt)


def hat_prolongation_per(nf, nc, dt):
    """One axis of P from the definition: the levels are nested, fine point i sits at p = i / 2 in coarse index units on
    a ring of n_c points, and coarse point j carries the hat function max(0, 1 - dist(p, j)) there, dist the distance
    on the ring."""
    if nf == nc:
        return np.eye(nf, dtype=dt)
    P = np.zeros((nf, nc), dtype=dt)
    for i in range(nf):
        p = Fraction(i, 2)
        for j in range(nc):
            dist = min(abs(p - j), nc - abs(p - j))
            w = 1 - dist
            if w > 0:
                P[i, j] = dt(w.numerator) / dt(w.denominator)
    return P


def second_difference_per(n, dt):
    S = -2 * np.eye(n, dtype=dt)
    for i in range(n):
        S[i, (i + 1) % n] += 1
        S[i, (i - 1) % n] += 1
    return S


def dense_vcycle_matrix_per(shape, h, k, s0, nu, cs, dt, post=None):
    """V with z = V v for one cycle from x = 0, by the matrix recursion (post: other post-sweeps than nu)"""
    d = len(shape)
    post = nu if post is None else post
    omega = dt(2 * d) / dt(2 * d + 1)
    levels = plan_per(shape)
    s = (np.asarray(s0, dtype=dt) * np.ones(tuple(reversed(shape)), dtype=dt)).reshape(-1)
    A, P, R = [], [], []
    for l, ext in enumerate(levels):
        if l > 0:
            Pa = [hat_prolongation_per(nf, nc, dt) for nf, nc in zip(levels[l - 1], ext)]
            Ra = [(p.T / p.T.sum(axis=1)[:, None]) for p in Pa]
            P.append(kron_axes(Pa))
            R.append(kron_axes(Ra))
            s = R[-1] @ s
        Al = np.diag(s)
        for a in range(d):
            hl = dt(h[a]) * dt(shape[a] // ext[a])
            eyes = [np.eye(n, dtype=dt) for n in ext]
            eyes[a] = second_difference_per(ext[a], dt)
            Al = Al + (dt(k[a]) / (hl * hl)) * kron_axes(eyes)
        A.append(Al)

    # A_l X from the at most 2 d + 1 non-zero entries of each row of the dense A_l (numpy's long-double matrix product
    # of 432 x 432 matrices takes most of a second, and the recursion needs dozens)
    rows = []
    for Al in A:
        w = int((Al != 0).sum(axis=1).max())
        idx = np.argsort(Al == 0, axis=1, kind="stable")[:, :w]
        rows.append((idx, np.take_along_axis(Al, idx, 1)))

    def times_A(l, X):
        idx, val = rows[l]
        return sum(val[:, t, None] * X[idx[:, t]] for t in range(idx.shape[1]))

    def jacobi(l, X, sweeps):
        eye, dinv = np.eye(A[l].shape[0], dtype=dt), 1 / np.diag(A[l])
        for _ in range(sweeps):
            X = X + omega * (dinv[:, None] * (eye - times_A(l, X)))
        return X

    def M(l):
        n = A[l].shape[0]
        if l == len(levels) - 1:
            return jacobi(l, np.zeros((n, n), dtype=dt), cs)
        pre = jacobi(l, np.zeros((n, n), dtype=dt), nu)
        return jacobi(l, pre + P[l] @ (M(l + 1) @ (R[l] @ (np.eye(n, dtype=dt) - times_A(l, pre)))), post)

    return M(0)


_DENSE = {}


def dense_reference(case):
    """(h, k, s_0, V in long double, the float64 restatement on the unit vectors) of a dense case, computed once"""
    if case not in _DENSE:
        shape, skind, nu, cs = case
        h, k, s = dense_coefficients(shape, skind)
        cyc = PerCycle(shape, h, k, s, nu=nu, coarse_sweeps=cs)
        assert cyc.levels == plan_per(shape) and len(cyc.levels) >= 2
        _DENSE[case] = (h, k, s, dense_vcycle_matrix_per(shape, h, k, s, nu, cs, np.longdouble), unit_matrix(cyc, shape))
    return _DENSE[case]


# ------------------------------------------------------------------------------------ the cases of the GPU file
# k_a = theta a Δt = STIFF h_x² on every axis (a Δt / h² far beyond the explicit limit), h = 1 / n
Case = namedtuple("Case", "kind shape nu cs omega max_levels")
STIFF = {2: 1.0e3, 3: 1.0e2}
THETA = {"euler": 1.0, "midpoint": 1.0 - ALPHA, "trapezoid": 0.5}
HEAT_A = 0.01


def case(kind, shape, nu=2, cs=8, omega=None, max_levels=0):
    return Case(kind, shape, nu, cs, omega, max_levels)


CYCLE_CASES = [
    case("heat2d_trapezoid", (96, 48)),                 # two per-level pairs (4608, 1152 points), then the tail
    case("heat2d_euler", (130, 12)),                    # three x-blocks, the last 2 columns wide; x stops at 65
    case("heat2d_midpoint", (264, 12)),                 # coarse rows of 132: three x-blocks in the restriction
    case("heat3d_euler", (24, 12, 12)),                 # y and z wrap in the per-level kernels
    case("heat3d_trapezoid", (20, 9, 12)),              # a kept odd middle axis
    case("heat2d_euler", (64, 16)),                     # 1024 points exactly: level 0 in the tail
    case("heat2d_euler", (64, 32)),                     # level 0 per-level, level 1 the tail's first
    case("heat2d_trapezoid", (96, 48), max_levels=2),   # no tail: coarse sweeps on a per-level level
    case("heat2d_trapezoid", (96, 48), nu=1, cs=1),
    case("heat2d_trapezoid", (96, 48), nu=3, cs=3),
    case("heat3d_midpoint", (24, 12, 12), nu=1, cs=1),
    case("heat3d_midpoint", (24, 12, 12), nu=3, cs=3),
    case("heat2d_midpoint", (96, 48), omega=0.6),
]


def case_id(c):
    om = "" if c.omega is None else f"-om{c.omega}"
    ml = "" if not c.max_levels else f"-ml{c.max_levels}"
    return f"{c.kind}-{'x'.join(map(str, c.shape))}-nu{c.nu}-cs{c.cs}{om}{ml}"


def options(c):
    return dict(nu=c.nu, coarse_sweeps=c.cs, omega=c.omega, max_levels=c.max_levels)


def per_problem(kind, shape, stiff=None, seed=4):
    """(oracle problem with bc_periodic!, u, k per axis, s_0 = -1, h per axis): h = 1 / n, θ a Δt = stiff h_x²"""
    rng = np.random.default_rng(seed)
    d, scheme = len(shape), kind.split("_")[1]
    h = [1.0 / n for n in shape]
    k = (STIFF[d] if stiff is None else stiff) * h[0] * h[0]
    dt = k / (THETA[scheme] * HEAT_A)
    hs = dict(zip(("hx", "hy", "hz"), h))
    P = oc.Problem(oc.HEAT_KINDS[scheme, d], *shape, a=HEAT_A, dt=dt, bc=oc.BC_PERIODIC, alpha=ALPHA, **hs)
    P.un = rng.standard_normal(P.shape)
    # k as the library forms it: θ a Δt in this order
    theta = {"euler": 1.0, "midpoint": 1.0 - ALPHA, "trapezoid": 0.5}[scheme]
    return P, rng.standard_normal(P.shape), [theta * HEAT_A * dt] * d, -1.0, h


_REF = {}


def per_reference(c):
    """(P, u, k, s, h, v, the float64 restatement at the case's options, its V-cycle of v), computed once"""
    if c not in _REF:
        P, u, k, s, h = per_problem(c.kind, c.shape)
        v = np.random.default_rng(11).standard_normal(P.shape)
        cyc = PerCycle(c.shape, h, k, s, **options(c))
        _REF[c] = (P, u, k, s, h, v, cyc, cyc.vcycle(v))
    return _REF[c]


def coefficient_case():
    """from_coefficients(periodic=True) with a variable s on 96 x 48 and the default spacings 1 / n:
    (shape, h, k, s, v, the restatement, its V-cycle of v)"""
    if "coef" not in _REF:
        shape = (96, 48)
        h = [1.0 / n for n in shape]
        x, y = np.arange(96) * h[0], np.arange(48) * h[1]
        s = -1.0 - 40.0 * (1.0 + np.sin(2 * np.pi * y + 0.3)[:, None] * np.cos(4 * np.pi * x + 0.1)[None, :]) - 3.0 * x[None, :]
        k = [0.11, 0.07]
        v = np.random.default_rng(12).standard_normal(s.shape)
        cyc = PerCycle(shape, h, k, s)
        _REF["coef"] = (shape, h, k, s, v, cyc, cyc.vcycle(v))
    return _REF["coef"]


# the solver cases: (kind, shape); the right-hand side is the residual at u, as the Newton step has it
SOLVER_2D = ("heat2d_trapezoid", (96, 48))
SOLVER_3D = ("heat3d_euler", (24, 12, 12))
# restated GMRES(30) counts at rtol 1e-8, itmax 200 (test_restated_gmres_counts computes and asserts them):
# with the V-cycle as N / without (200: not solved within itmax)
RESTATED_COUNTS = {SOLVER_2D: (10, 200), SOLVER_3D: (10, 99)}


def jv_per(P, k, q):
    """J q of a periodic heat problem from its coefficients: Σ_a k_a δ²_a(h_a) q - q (J does not depend on u)"""
    h = [P.hx, P.hy, P.hz][: q.ndim]
    return sum(k[a] / (h[a] * h[a]) * d2_per(q, a) for a in range(q.ndim)) - q


_SOLVE = {}


def restated_solve(key):
    """(b, preconditioned count, unpreconditioned count, solved flags, the restatement) of a solver case"""
    if key not in _SOLVE:
        kind, shape = key
        P, u, k, s, h = per_problem(kind, shape)
        b = oc.residual(P, u)
        cyc = PerCycle(shape, h, k, s)
        A = lambda q: jv_per(P, k, q)  # noqa: E731
        x, it, ok = gmres_right(A, cyc.vcycle, b, 1e-8, itmax=200)
        _, it0, ok0 = gmres_right(A, lambda q: q, b, 1e-8, itmax=200)
        _SOLVE[key] = (P, u, k, b, x, it, ok, it0, ok0, cyc)
    return _SOLVE[key]


# ------------------------------------------------------------------------------------ the header's rules (g++)
SRC = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "nk_mg_plan.hpp"
using namespace nk;
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const char kind = line[0];
        std::vector<long long> v;
        const char* s = line.c_str() + 1;
        for (char* end = nullptr;; s = end) {
            const long long x = std::strtoll(s, &end, 10);
            if (end == s) break;
            v.push_back(x);
        }
        if (kind == 'P') {  // nx ny nz max_levels [dim]: mg_plan_per, or "0 why" (dim: the used axes; none: from the extents)
            const int64_t n[3] = {v[0], v[1], v[2]};
            int64_t ext[kMgMaxLevels + 1][3];
            if (const char* why = mg_plan_per_why(n, (int)(v.size() > 4 ? v[4] : 0))) {
                std::printf("0 %s\n", why);
                continue;
            }
            const int L = mg_plan_per(n, (int)v[3], ext);
            std::printf("%d", L);
            for (int l = 0; l < L; ++l) std::printf(" %" PRId64 " %" PRId64 " %" PRId64, ext[l][0], ext[l][1], ext[l][2]);
            std::printf("\n");
        } else if (kind == 'R') {  // nf: every mg_per_rax (m c p), then mg_per_rkeep of the first coarse points
            const int nf = (int)v[0];
            for (int j = 0; j < nf / 2; ++j) {
                const MgPerR a = mg_per_rax(nf, j), b = mg_per_rkeep(j);
                std::printf("%d %d %d %d %d %d ", a.m, a.c, a.p, b.m, b.c, b.p);
            }
            std::printf("\n");
        } else {  // Q nf: every mg_per_pax (j0 j1 w), with mg_per_pkeep
            const int nf = (int)v[0];
            for (int i = 0; i < nf; ++i) {
                const MgPerP a = mg_per_pax(nf / 2, i), b = mg_per_pkeep(i);
                std::printf("%d %d %a %d %d %a ", a.j0, a.j1, a.w, b.j0, b.j1, b.w);
            }
            std::printf("\n");
        }
    }
    return 0;
}
"""

EXAMPLES = {(8192, 8192): 12, (96, 48): [(96, 48), (48, 24), (24, 12), (12, 6), (6, 3), (3, 3)],
            (130, 12): [(130, 12), (65, 6), (65, 3)], (6, 5, 12): [(6, 5, 12), (3, 5, 6), (3, 5, 3)]}
EXTENTS = range(3, 41)
ALL_SHAPES = [s for d in (1, 2, 3) for s in product(EXTENTS, repeat=d)]
PLAN_QUERIES = [(s, 0) for s in ALL_SHAPES] + [(s, ml) for s in EXAMPLES for ml in (0, 1, 2, 3)]
REFUSED = [(2, 8), (8, 2), (8, 8, 2), (2,), (1, 8), (8, 1, 8)]
# a used axis of one point, which only the kind's dimension tells from an unused one: (extents, dim)
REFUSED_DIM = [((8, 1, 1), 2), ((8, 8, 1), 3), ((1, 1, 1), 1), ((8, 2, 1), 2)]
AXES = [n for n in range(6, 131, 2)]


def pad(e):
    return tuple((list(e) + [1, 1])[:3])


def q_plan(shape, ml=0):
    return "P %d %d %d %d" % (pad(shape) + (ml,))


@pytest.fixture(scope="module")
def ask():
    lines = [q_plan(s, ml) for s, ml in PLAN_QUERIES] + [q_plan(s) for s in REFUSED]
    lines += [q_plan(s) + " %d" % dim for s, dim in REFUSED_DIM] + [q_plan((8, 8)) + " 2", q_plan((8, 8, 8)) + " 3"]
    lines += ["R %d" % n for n in AXES] + ["Q %d" % n for n in AXES]
    lines = sorted(set(lines))
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "mg_per.cpp"), os.path.join(d, "mg_per")
        with open(src, "w") as f:
            f.write(SRC)
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src]
        if subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"],
                          capture_output=True).returncode != 0:
            subprocess.run(base, check=True)  # no sanitizer runtimes to link here
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
    return dict(zip(lines, out))


def levels_of(answer, dim):
    v = [int(t) for t in answer.split()]
    assert len(v) == 1 + 3 * v[0]
    return [tuple(v[1 + 3 * l:1 + 3 * l + dim]) for l in range(v[0])]


def test_plan_restatement_gives_the_examples():
    assert len(plan_per((8192, 8192))) == 12 and plan_per((8192, 8192))[-1] == (4, 4)
    for s, lv in EXAMPLES.items():
        if isinstance(lv, list):
            assert plan_per(s) == lv
    assert plan_per((96, 48), 2) == [(96, 48), (48, 24)]


def test_header_plan_matches_restatement(ask):
    for s, ml in PLAN_QUERIES:
        assert levels_of(ask[q_plan(s, ml)], len(s)) == plan_per(s, ml), (s, ml)
    for q in [q_plan(s) for s in REFUSED] + [q_plan(s) + " %d" % dim for s, dim in REFUSED_DIM]:
        assert ask[q].startswith("0 ") and "at least 3 points" in ask[q], q
    assert levels_of(ask[q_plan((8, 8)) + " 2"], 2) == plan_per((8, 8))
    assert levels_of(ask[q_plan((8, 8, 8)) + " 3"], 3) == plan_per((8, 8, 8))


def test_header_transfer_indices_match_the_matrices(ask):
    """mg_per_rax / mg_per_pax as the kernels call them, against P and R = D^-1 P^T of one axis"""
    for nf in AXES:
        nc = nf // 2
        P, R = transfers_per(nf, nc, np.float64)
        np.testing.assert_array_equal(P, hat_prolongation_per(nf, nc, np.float64))
        assert np.all(P.sum(axis=1) == 1.0) and np.all(R.sum(axis=1) == 1.0)
        r = [int(t) for t in ask["R %d" % nf].split()]
        Rh = np.zeros((nc, nf))
        for j in range(nc):
            m, c, p, km, kc, kp = r[6 * j:6 * j + 6]
            assert (m, c, p) == ((2 * j - 1) % nf, 2 * j, (2 * j + 1) % nf) and (km, kc, kp) == (j, j, j)
            for i, w in ((m, 1.0), (c, 2.0), (p, 1.0)):
                Rh[j, i] += w / 4.0
        np.testing.assert_array_equal(Rh, R)
        q = ask["Q %d" % nf].split()
        Ph = np.zeros((nf, nc))
        for i in range(nf):
            j0, j1, w = int(q[6 * i]), int(q[6 * i + 1]), float.fromhex(q[6 * i + 2])
            assert (int(q[6 * i + 3]), int(q[6 * i + 4]), float.fromhex(q[6 * i + 5])) == (i, i, 0.0)
            assert 0 <= j0 < nc and 0 <= j1 < nc and w == (0.5 if i % 2 else 0.0)
            Ph[i, j0] += 1.0 - w
            Ph[i, j1] += w
        np.testing.assert_array_equal(Ph, P)


def c_plan(shape, max_levels=0, cap=64):
    n = (C.c_int64 * 3)(*pad(shape))
    ext, nl = (C.c_int64 * (3 * 64))(), C.c_int32(0)
    rc = ah.load().nk_mg_plan_periodic(n, max_levels, ext, cap, C.byref(nl))
    return rc, [tuple(int(ext[3 * l + a]) for a in range(len(shape))) for l in range(min(nl.value, cap))], nl.value


def test_c_plan_matches_restatement():
    for s in [x for x in ALL_SHAPES if len(x) < 3 or max(x) <= 14] + list(EXAMPLES):
        for ml in (0, 2):
            rc, lv, n = c_plan(s, ml)
            assert rc == 0 and lv == plan_per(s, ml) and n == len(lv), (s, ml)
        assert ah.multigrid_plan(s, periodic=True) == plan_per(s)
    assert ah.multigrid_plan((96, 48), 3, periodic=True) == plan_per((96, 48), 3)
    rc, lv, n = c_plan((96, 48), 0, cap=2)  # a short buffer: the count is still the plan's
    assert rc == 0 and lv == plan_per((96, 48))[:2] and n == 6


def test_c_plan_rejects_bad_arguments():
    E = _lib.NK_E_ARG
    for s in REFUSED + [(0, 8), (8, -1)]:  # (a used axis needs 3 points; one of 1 point below a used one is refused too)
        assert c_plan(s)[0] == E, s
    assert c_plan((8, 8), -1)[0] == E
    nl = C.c_int32(0)
    n = (C.c_int64 * 3)(8, 8, 1)
    assert ah.load().nk_mg_plan_periodic(n, 0, None, 4, C.byref(nl)) == E
    assert ah.load().nk_mg_plan_periodic(n, 0, None, 0, None) == E
    assert ah.load().nk_mg_plan_periodic(None, 0, None, 0, C.byref(nl)) == E
    assert ah.load().nk_mg_plan_periodic(n, 0, None, 0, C.byref(nl)) == 0 and nl.value == 2
    with pytest.raises(ValueError, match="at least 3 points"):
        ah.multigrid_plan((8, 2), periodic=True)


# ------------------------------------------------------------------------------------ the cycle
@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_restatement_matches_dense_form(case):
    h, k, s, V, Z = dense_reference(case)
    err = rel(Z, V)
    print(f"{case}: restatement vs dense long double V {float(err):.3e} (allowed {16 * PER_DENSE_SENSITIVITY:.1e})")
    assert err <= 16 * PER_DENSE_SENSITIVITY


@pytest.mark.parametrize("case", DENSE_CASES, ids=DENSE_IDS)
def test_dense_cycle_is_symmetric_and_definite(case):
    """equal pre / post sweeps: V is symmetric to rounding and σ V = -V positive definite (the diagonal is negative)"""
    h, k, s, V, Z = dense_reference(case)
    V = V.astype(np.float64)
    scale = np.max(np.abs(V))
    assert np.max(np.abs(V - V.T)) <= 64 * np.finfo(np.float64).eps * scale
    ev = np.linalg.eigvalsh(-(V + V.T) / 2)
    assert ev.min() > 0
    # unequal sweeps are not symmetric: the check can fail
    shape, skind, nu, cs = case
    U = dense_vcycle_matrix_per(shape, h, k, s, nu, cs, np.float64, post=nu + 1)
    assert np.max(np.abs(U - U.T)) > 1e4 * np.finfo(np.float64).eps * scale


def test_restriction_reproduces_a_constant():
    for case in DENSE_CASES[::8]:
        shape = case[0]
        cyc = PerCycle(shape, *dense_coefficients(shape, "const"))
        assert all(np.all(s == -1.0) for s in cyc.s)


def measured_sensitivities():
    dense = unit = cycle = 0.0
    for case in DENSE_CASES:
        shape, skind, nu, cs = case
        h, k, s, V, Z = dense_reference(case)
        dense = max(dense, rel(dense_vcycle_matrix_per(shape, h, k, s, nu, cs, np.float64), V))
        Zl = unit_matrix(PerCycle(shape, h, k, s, nu=nu, coarse_sweeps=cs, dt=np.longdouble), shape)
        unit = max(unit, rel(Z, Zl))
        assert rel(Zl, V) <= 16 * PER_DENSE_SENSITIVITY * float(np.finfo(np.longdouble).eps) / np.finfo(np.float64).eps
    for c in CYCLE_CASES:
        P, u, k, s, h, v, cyc, z = per_reference(c)
        zl = PerCycle(c.shape, h, k, s, dt=np.longdouble, **options(c)).vcycle(v)
        cycle = max(cycle, rel(z, zl))
    shape, h, k, s, v, cyc, z = coefficient_case()
    cycle = max(cycle, rel(z, PerCycle(shape, h, k, s, dt=np.longdouble).vcycle(v)))
    return dense, unit, cycle


def test_sensitivities_are_as_recorded():
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double"
    dense, unit, cycle = measured_sensitivities()
    print(f"periodic dense form float64 vs longdouble: {dense:.3e}; restatement on the unit vectors: {unit:.3e}; "
          f"restatement over the cycle cases: {cycle:.3e}")
    assert within(PER_DENSE_SENSITIVITY, dense)
    assert within(PER_UNIT_SENSITIVITY, unit)
    assert within(PER_CYCLE_SENSITIVITY, cycle)


def test_cycle_cases_reach_the_named_edges():
    """the shapes of CYCLE_CASES are there for their plans: check that the plans are those"""
    lv = {c: per_reference(c)[6].levels for c in CYCLE_CASES}
    pts = lambda e: int(np.prod(e))  # noqa: E731
    assert [pts(e) > 1024 for e in lv[CYCLE_CASES[0]]] == [True, True, False, False, False, False]
    assert lv[CYCLE_CASES[1]] == [(130, 12), (65, 6), (65, 3)]
    assert lv[CYCLE_CASES[2]][:2] == [(264, 12), (132, 6)]
    assert lv[CYCLE_CASES[3]] == [(24, 12, 12), (12, 6, 6), (6, 3, 3), (3, 3, 3)]
    assert lv[CYCLE_CASES[4]] == [(20, 9, 12), (10, 9, 6), (5, 9, 3)]
    assert pts(lv[CYCLE_CASES[5]][0]) == 1024 and pts(lv[CYCLE_CASES[6]][0]) == 2048 and pts(lv[CYCLE_CASES[6]][1]) == 512
    assert lv[CYCLE_CASES[7]] == [(96, 48), (48, 24)]


# ------------------------------------------------------------------------------------ refusals (no device)
def test_python_refusals_need_no_device():
    g2 = ah.Grid.full(16, 12)
    heat_p = lambda bc: (lambda u: (u, 0.1, u, (0.01, 0.1, 0.1, bc), 0.0))  # noqa: E731
    per = fake_operator(ah.heat2d_euler_, g2, heat_p(ah.bc_periodic_))
    # the default path still refuses, and names the keyword
    for make in (ah.MultigridPreconditioner, ah.multigrid, ah.multigrid()):
        with pytest.raises(NotImplementedError, match="periodic") as e:
            make(per)
        assert "periodic=True" in str(e.value)
    zero = fake_operator(ah.heat2d_euler_, g2, heat_p(ah.bc_zero_))
    with pytest.raises(ValueError, match="bc_zero_"):
        ah.MultigridPreconditioner(zero, periodic=True)
    with pytest.raises(ValueError, match="bc_zero_"):
        ah.multigrid(periodic=True)(zero)
    with pytest.raises(NotImplementedError, match="distributed"):
        ah.MultigridPreconditioner(per, periodic=True, distributed=True)
    with pytest.raises(NotImplementedError, match="distributed"):
        ah.multigrid(periodic=True, distributed=True)(per)
    with pytest.raises(NotImplementedError, match="semi"):
        ah.MultigridPreconditioner(per, periodic=True, coarsening="semi")
    with pytest.raises(NotImplementedError, match="semi"):
        ah.multigrid(periodic=True, coarsening="semi")(per)
    with pytest.raises(NotImplementedError, match="one rank"):  # a context of several ranks is not covered either
        ah.MultigridPreconditioner(fake_operator(ah.heat2d_euler_, g2, heat_p(ah.bc_periodic_), nranks=2), periodic=True)
    ctx = types.SimpleNamespace(nranks=1, handle=None)
    with pytest.raises(NotImplementedError, match="2D and 3D"):
        ah.MultigridPreconditioner.from_coefficients(ah.Grid.full(16), [1.0], -1.0, ctx=ctx, periodic=True)
    with pytest.raises(NotImplementedError, match="distributed"):
        ah.MultigridPreconditioner.from_coefficients(g2, [1.0, 1.0], -1.0, ctx=ctx, periodic=True, distributed=True)
    with pytest.raises(NotImplementedError, match="semi"):
        ah.MultigridPreconditioner.from_coefficients(g2, [1.0, 1.0], -1.0, ctx=ctx, periodic=True, coarsening="semi")
    with pytest.raises(NotImplementedError, match="semi"):
        ah.multigrid_plan((16, 12), periodic=True, coarsening="semi", h=[0.1, 0.1])
    with pytest.raises(NotImplementedError, match="distributed"):
        ah.multigrid_plan((16, 12), periodic=True, nranks=2)


def test_header_ctypes_and_shim_agree_on_the_new_name():
    import re

    n = "nk_mg_plan_periodic"
    hdr = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "newtonkrylov.jl_amd", "julia", "AriadneHIP.jl")).read()
    args = re.search(rf"\bint {n}\(([^;]*?)\);", hdr, re.S).group(1)
    assert [a.strip() for a in args.split(",")] == ["const int64_t n[3]", "int32_t max_levels", "int64_t* extents", "int32_t cap",
                                                    "int32_t* nlevels"]
    assert _lib.SIGNATURES[n] == _lib.SIGNATURES["nk_mg_plan"] and hasattr(ah.load(), n)
    call = shim[shim.index(f"ccall((:{n}, libnkhip)"):]
    jl = re.match(r"ccall\(\(:\w+, libnkhip\), Cint,\s*\((.*?)\),\s", call, re.S).group(1)
    assert re.sub(r"\s", "", jl) == "Ref{NTuple{3,Int64}},Int32,Ptr{Int64},Int32,Ref{Int32}"
    assert C.sizeof(_lib.nk_mg_opts) == 24  # the options struct keeps its four fields


# ------------------------------------------------------------------------------------ the solver cases, restated
@pytest.mark.parametrize("key", [SOLVER_2D, SOLVER_3D], ids=["heat2d-96x48", "heat3d-24x12x12"])
def test_restated_gmres_counts(key):
    P, u, k, b, x, it, ok, it0, ok0, cyc = restated_solve(key)
    print(f"{key}: GMRES(30) with the restated V-cycle {it} steps (solved {ok}), without {it0} (solved {ok0})")
    assert ok and np.linalg.norm(b - jv_per(P, k, x)) <= 1e-7 * np.linalg.norm(b)
    assert (it, it0) == RESTATED_COUNTS[key]
    assert 4 * it <= it0
    # the operator of the restated solve is the oracle's Jacobian of the periodic problem
    q = np.random.default_rng(1).standard_normal(P.shape)
    assert rel(jv_per(P, k, q), oc.jv_exact(P, u, q)) <= 1e-13
