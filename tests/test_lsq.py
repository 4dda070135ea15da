"""The Krylov drivers' host algebra of csrc/nk_lsq.hpp (sym_givens, GMRES's least-squares state and stop rules,
MINRES's rotation scalars) against its references, bit for bit, on the CPU: oracle/ariadne_ref.py's gmres and
sym_givens, and test_hip_minres.py's minres_ref.

A small program includes the header (it needs no HIP), is built with g++ -ffp-contract=off -- under the address and
undefined-behaviour sanitizers where the toolchain links them -- and answers every query in one run.  For GMRES it
runs the host side of nk_krylov.cpp's gmres() loop over a stream of doubles: the reference's inner products in
order (its `dot=` hook, a norm's <w, w> under the root the reference takes of it), which are beta and then, per step,
the raw Hessenberg column as the kernels deliver it (k entries, k more when reorthogonalising, then h_{k+1,k}).  The
program decides by itself when a cycle ends, so a stop rule that moved would misread the stream.  The arithmetic is
the same sequence of IEEE operations on the same inputs: everything is compared with ==.
"""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _nkpath  # noqa: F401
from oracle import ariadne_ref as ar
from test_hip_minres import minres_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "newtonkrylov.jl_amd", "csrc")

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nk_lsq.hpp"
static double num() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) std::exit(3);
    return std::strtod(tok, nullptr);
}
// G a b: sym_givens
static void givens() {
    const double a = num(), b = num();
    double c, s, rho;
    nk::sym_givens(a, b, &c, &s, &rho);
    std::printf("%a %a %a\n", c, s, rho);
}
// M beta1 steps, then (alpha, beta2) per step: the rotation's (oldeps, delta, gamma, phi) and phibar
static void minres() {
    nk::MinresRot rot(num());
    const int steps = (int)num();
    for (int i = 0; i < steps; ++i) {
        const double alpha = num(), beta2 = num();
        const nk::MinresRot::Step s = rot.step(alpha, beta2);
        std::printf("%a %a %a %a %a\n", s.oldeps, s.delta, s.gamma, s.phi, rot.phibar);
    }
}
// K mem restart reorth itmax atol rtol count, then `count` doubles: the host side of gmres()
static void gmres() {
    const int mem = (int)num();
    const bool restart = num() != 0, reorth = num() != 0;
    const long long itmax = (long long)num();
    const double atol = num(), rtol = num();
    std::vector<double> in((size_t)num());
    for (double& v : in) v = num();
    size_t at = 0;
    double beta = in[at++];
    double rNorm = beta;
    std::vector<double> hist{rNorm};
    const double eps_ = atol + rtol * rNorm;
    const double btol = nk::gmres_btol();
    nk::GmresLsq lsq(mem);
    long long iter = 0, inner_itmax = itmax;
    bool breakdown = false, inconsistent = false, solved = rNorm <= eps_, tired = iter >= itmax;
    std::vector<std::vector<double>> ys;
    while (!(solved || tired || breakdown)) {
        beta = in.at(at++);
        lsq.start(beta);
        long long inner_iter = 0;
        bool inner_tired = false;
        while (!(solved || inner_tired || breakdown)) {
            inner_iter++;
            const int k = (int)inner_iter;
            const bool last = nk::gmres_last(restart, inner_iter, mem, inner_itmax);
            const size_t len = (size_t)(reorth ? 2 * k : k) + 1;
            if (at + len > in.size()) std::exit(4);
            const nk::GmresLsq::Col h = lsq.column(k, &in[at], reorth);
            at += len;
            rNorm = h.rNorm;
            hist.push_back(rNorm);
            solved = nk::gmres_solved(rNorm, eps_);
            breakdown = nk::gmres_breakdown(h.Hbis, btol);
            inner_tired = last;
            if (!(solved || inner_tired || breakdown)) lsq.accept(k, h.zeta);
        }
        const int kk = (int)inner_iter;
        if (lsq.solve(kk, btol)) inconsistent = true;
        ys.emplace_back(lsq.y(), lsq.y() + kk);
        iter += inner_iter;
        inner_itmax = itmax - iter;
        tired = iter >= itmax;
    }
    std::printf("%lld %d %d %d %d %d %zu %zu\n", iter, (int)solved, (int)tired, (int)breakdown, (int)inconsistent, lsq.cap,
                at, ys.size());
    for (double v : hist) std::printf("%a ", v);
    std::printf("\n");
    for (const auto& y : ys) {
        for (double v : y) std::printf("%a ", v);
        std::printf("\n");
    }
}
int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'G') givens();
        else if (kind == 'M') minres();
        else if (kind == 'K') gmres();
        else return 2;
    }
    return 0;
}
"""


def tridiag(n):
    """diag(2 + i/n) with -1 on both off-diagonals"""
    return np.diag(2.0 + np.arange(n) / n) - np.eye(n, k=1) - np.eye(n, k=-1)


def rand_b(n):
    return np.random.default_rng(0).standard_normal(n)


# name: (A, b, gmres keywords, path: niter, exit flag, final capacity, steps per cycle).  The capacity doubles
# when step k = capacity arrives (room for z[k]), so a restarted solve at memory 5 ends at 10
GMRES_CASES = {
    "inconsistent": (np.array([[0.0, 1.0], [0.0, 0.0]]), np.array([1.0, 0.0]), dict(memory=20, atol=0.0, rtol=0.0),
                     (1, "inconsistent", 20, [1])),
    "breakdown": (tridiag(12), rand_b(12), dict(memory=20, itmax=40, atol=0.0, rtol=0.0), (12, "breakdown", 20, [12])),
    "growth": (tridiag(40), rand_b(40), dict(memory=4, itmax=30, atol=0.0, rtol=0.0), (30, "tired", 32, [30])),
    "restart_reorth": (tridiag(40), rand_b(40),
                       dict(memory=5, restart=True, itmax=17, atol=0.0, rtol=0.0, reorthogonalization=True),
                       (17, "tired", 10, [5, 5, 5, 2])),
    "restart": (tridiag(40), rand_b(40), dict(memory=5, restart=True, itmax=17, atol=0.0, rtol=0.0),
                (17, "tired", 10, [5, 5, 5, 2])),
    "solved": (tridiag(40), rand_b(40), dict(memory=20, atol=1e-8, rtol=1e-8), (31, "solved", 40, [31])),
}
GIVENS_GRID = [(3.0, 4.0), (-2.0, 0.5), (0.0, 0.0), (0.0, -3.0), (1.5, 0.0), (1e-300, 1e300)]


class DotLog:
    """ariadne_ref.gmres's `dot=` hook: every inner product in order, and the basis of every cycle."""

    def __init__(self):
        self.values, self.cycles, self.step, self.after_norm = [], [], [], False

    def __call__(self, x, y):
        h = float(np.dot(x, y))
        self.values.append(math.sqrt(h) if x is y else h)  # the reference takes the same root of a norm's <w, w>
        if x is y:  # a norm: beta, a cycle's beta (the second norm in a row) or the h_{k+1,k} that ends a step
            if self.after_norm:
                self.cycles.append([])
            elif self.step:
                k = len(self.cycles[-1]) + 1
                self.cycles[-1] = self.step[:k]  # the first pass of step k pairs w with V_1 .. V_k
            self.step = []
        else:
            self.step.append(x)
        self.after_norm = x is y
        return h


def gmres_reference(name):
    A, b, kw, _ = GMRES_CASES[name]
    log = DotLog()
    x, st, hist = ar.gmres(lambda v: A @ v, b, dot=log, **kw)
    return x, st, hist, log


def minres_traces():
    """minres_ref in float64 on a 30 x 30 symmetric indefinite tridiagonal, without M (as the identity, which leaves
    every operation as it is and shows g = <r2, r2>) and with a diagonal SPD M: (beta1, history, trace) each."""
    n = 30
    A = np.diag(np.arange(n) - 11.3) - np.eye(n, k=1) - np.eye(n, k=-1)
    assert np.linalg.eigvalsh(A)[0] < 0 < np.linalg.eigvalsh(A)[-1]
    b = np.random.default_rng(1).standard_normal(n)
    d = 1.0 / (1.0 + np.arange(n) / 7.0)
    out = {}
    for name, M in (("none", lambda r: r), ("diag", lambda r: d * r)):
        trace = []
        _, hist, it, _ = minres_ref(A, b, M=M, itmax=25, trace=trace)
        assert it == len(trace) == 25
        out[name] = (hist[0], hist, trace)
    return out


def hexes(vals):
    return " ".join(float(v).hex() for v in vals)


@pytest.fixture(scope="module")
def run():
    """Build the program once, put every query to it in one run, and return the references with its answers."""
    refs = {name: gmres_reference(name) for name in GMRES_CASES}
    traces = minres_traces()
    lines = ["G %s" % hexes(ab) for ab in GIVENS_GRID]
    for name, (beta1, _, trace) in traces.items():
        lines.append("M %s %d %s" % (hexes([beta1]), len(trace), hexes(v for t in trace for v in t[:2])))
    for name, (_, b, kw, _) in GMRES_CASES.items():
        vals = refs[name][3].values
        lines.append("K %d %d %d %d %s %d %s" % (
            kw["memory"], kw.get("restart", False), kw.get("reorthogonalization", False), kw.get("itmax", 2 * b.size),
            hexes([kw["atol"], kw["rtol"]]), len(vals), hexes(vals)))
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "lsq.cpp"), os.path.join(d, "lsq")
        with open(src, "w") as f:
            f.write(SRC)
        base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src]
        if subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"],
                          capture_output=True).returncode != 0:
            subprocess.run(base, check=True)  # no sanitizer runtimes to link here
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    out = iter(p.stdout.splitlines())
    row = lambda: [float.fromhex(v) for v in next(out).split()]
    ans = {"givens": [tuple(row()) for _ in GIVENS_GRID], "minres": {}, "gmres": {}}
    for name, (_, _, trace) in traces.items():
        ans["minres"][name] = [row() for _ in trace]
    for name in GMRES_CASES:
        head = [int(v) for v in next(out).split()]
        hist = row()
        ans["gmres"][name] = (head, hist, [row() for _ in range(head[7])])
    assert next(out, None) is None
    return refs, traces, ans


def test_sym_givens_is_the_reference(run):
    for ab, got in zip(GIVENS_GRID, run[2]["givens"]):
        assert got == ar.sym_givens(*ab), ab


@pytest.mark.parametrize("name", ["none", "diag"])
def test_minres_rotation_is_minres_ref(run, name):
    """Every step's (oldeps, delta, gamma, phi) and the phibar history, from minres_ref's alpha and <r2, y>."""
    _, hist, trace = run[1][name]
    got = run[2]["minres"][name]
    assert [g[:4] for g in got] == [[float(v) for v in t[2:]] for t in trace]
    assert [g[4] for g in got] == [float(v) for v in hist[1:]]


@pytest.mark.parametrize("name", list(GMRES_CASES))
def test_gmres_host_loop_is_the_reference(run, name):
    """History, niter, the flags and x = sum y_i V_i equal ariadne_ref.gmres's, and the case takes the path it is
    here for: its step count, its exit, the capacity the arrays grew to, the cycle pattern."""
    A, b, kw, (niter, flag, cap, pattern) = GMRES_CASES[name]
    x, st, hist, log = run[0][name]
    (it, solved, tired, breakdown, inconsistent, gcap, consumed, ncycles), ghist, ys = run[2]["gmres"][name]
    assert ghist == hist
    assert it == st.niter == niter
    assert (bool(solved), bool(inconsistent)) == (st.solved, st.inconsistent)
    ref_status = "solved" if solved else ("tired" if tired else "breakdown")
    assert st.status == ref_status
    assert consumed == len(log.values)  # the program read the whole stream: every cycle ended where the reference's did
    assert [len(y) for y in ys] == [len(V) for V in log.cycles] == pattern
    assert gcap == cap
    if flag == "inconsistent":
        assert inconsistent and ys == [[0.0]] and hist[-1] == 0.0
    elif flag == "breakdown":
        assert breakdown and not solved and not tired
    elif flag == "tired":
        assert tired and not solved and not breakdown
    else:
        assert solved and not tired
    restart = kw.get("restart", False)
    xr = np.zeros(b.size)
    xs = np.zeros(b.size) if restart else xr
    for y, V in zip(ys, log.cycles):
        if restart:
            xr[:] = 0.0
        for yi, Vi in zip(y, V):
            xr += yi * Vi
        if restart:
            xs += xr
    assert np.array_equal(xs, x)
