"""The Newton step's line search of csrc/nk_linesearch.hpp (Kelley's three-point parabolic backtracking) on the CPU,
bit for bit against ariadne_hip.Backtracking and against a restatement written here.

A small program includes the header (it needs no HIP), is built with g++ -ffp-contract=off -- under the address and
undefined-behaviour sanitizers where the toolchain links them -- and answers every query in one run: parab3p on given
arguments, the validity of a set of options, and whole Newton steps driven by a stream of trial norms (the program
decides by itself how many of them it consumes and how the step ends, so a rule that moved would misread the stream).
The arithmetic is the same sequence of IEEE operations on the same inputs: everything is compared with ==.
Also here: the new names of include/nkhip.h against their ctypes mirrors, nk_newton_defaults, and the options
Backtracking refuses.
"""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _nkpath  # noqa: F401
import ariadne_hip as ah
from ariadne_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "newtonkrylov.jl_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "nkhip.h")

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nk_linesearch.hpp"
static double num() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) std::exit(3);
    return std::strtod(tok, nullptr);
}
static nk::LsOpts opts() {
    nk::LsOpts o;
    o.alpha = num();
    o.sigma0 = num();
    o.sigma1 = num();
    o.maxarm = (int)num();
    return o;
}
int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'D') {  // the defaults
            const nk::LsOpts o;
            std::printf("%a %a %a %d\n", o.alpha, o.sigma0, o.sigma1, o.maxarm);
        } else if (kind == 'O') {  // O opts: are they valid?
            std::printf("%d\n", (int)nk::ls_opts_ok(opts()));
        } else if (kind == 'P') {  // P opts lc lm ff0 ffc ffm
            const nk::LsOpts o = opts();
            const double lc = num(), lm = num(), ff0 = num(), ffc = num(), ffm = num();
            std::printf("%a\n", nk::parab3p(o, lc, lm, ff0, ffc, ffm));
        } else if (kind == 'S') {  // S opts n_res count, then `count` trial norms: one Newton step
            const nk::LsOpts o = opts();
            const double n_res = num();
            std::vector<double> in((size_t)num());
            for (double& v : in) v = num();
            nk::LsStep S;
            S.begin(o, n_res);
            size_t at = 0;
            std::vector<double> lams;
            nk::LsVerdict v;
            for (;;) {
                if (at >= in.size()) std::exit(4);
                lams.push_back(S.lam);
                v = S.feed(in[at++]);
                if (v != nk::LS_RETRY) break;
            }
            std::printf("%d %zu", (int)v, at);
            for (double l : lams) std::printf(" %a", l);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
"""

DEFAULTS = (1e-4, 0.1, 0.5, 20)
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------- the restatement written here
def parab3p_here(o, lc, lm, ff0, ffc, ffm):
    alpha, sigma0, sigma1, maxarm = o
    if math.isinf(ffc) or math.isnan(ffc) or math.isinf(ffm) or math.isnan(ffm):
        return sigma1 * lc
    c2 = lm * (ffc - ff0) - lc * (ffm - ff0)
    if not (c2 < 0):
        return sigma1 * lc
    c1 = lc * lc * (ffm - ff0) - lm * lm * (ffc - ff0)
    lp = ((-c1) * 0.5) / c2
    return min(max(lp, sigma0 * lc), sigma1 * lc)  # (lp is finite here: no NaN reaches min / max)


def step_here(o, n_res, stream):
    """One Newton step on a stream of trial norms: (accepted, trials consumed, the lam of every trial)."""
    alpha, sigma0, sigma1, maxarm = o
    it = iter(stream)
    lam = lm = lc = 1.0
    k = 0
    lams = [lam]
    n_t = next(it)
    ff0 = n_res * n_res
    ffc = ffm = n_t * n_t
    while not (n_t < (1.0 - alpha * lam) * n_res):
        if k == maxarm:
            return False, len(lams), lams
        lam = sigma1 * lam if k == 0 else parab3p_here(o, lc, lm, ff0, ffc, ffm)
        lm = lc
        lc = lam
        ffm = ffc
        lams.append(lam)
        n_t = next(it)
        ffc = n_t * n_t
        k += 1
    return True, len(lams), lams


def step_backtracking(bt, n_res, stream):
    """The same through ah.Backtracking.search."""
    it = iter(stream)
    lams = []

    def trial(s):
        lams.append(-s)
        return next(it)

    lam, n_t, nrej = bt.search(n_res, trial)
    assert nrej == len(lams) - (lam is not None)
    if lam is not None:
        assert lam == lams[-1]
    return lam is not None, len(lams), lams


# ---------------------------------------------------------------- the cases
def parab_cases():
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(200):  # random finite inputs
        lm = float(rng.uniform(0.01, 1.0))
        lc = lm * float(rng.uniform(0.1, 0.5))
        ff0, ffc, ffm = (float(v) for v in np.exp(rng.uniform(-5, 5, 3)))
        cases.append((DEFAULTS, lc, lm, ff0, ffc, ffm))
    for _ in range(40):  # other options
        o = (float(rng.uniform(1e-6, 0.5)), float(rng.uniform(0.01, 0.3)), float(rng.uniform(0.3, 0.9)), 5)
        cases.append((o, 0.25, 0.5, 1.0, float(rng.uniform(0.5, 3)), float(rng.uniform(0.5, 3))))
    cases += [
        (DEFAULTS, 0.5, 1.0, 1.0, 1.5, 4.0),      # c2 = 0.5 - 1.5 < 0: the minimiser 0.125, inside the clamps
        (DEFAULTS, 0.5, 1.0, 1.0, 2.0, 1.0),      # c2 = 1 > 0: no minimum
        (DEFAULTS, 0.5, 1.0, 1.0, 1.0, 1.0),      # c2 = 0
        (DEFAULTS, 0.5, 1.0, 4.0, 3.999, 100.0),  # minimiser far to the right: the upper clamp sigma1 lc
        (DEFAULTS, 0.5, 1.0, 1.0, 50.0, 110.0),   # minimiser close to 0: the lower clamp sigma0 lc
        (DEFAULTS, 0.5, 1.0, 1.0, INF, 2.0), (DEFAULTS, 0.5, 1.0, 1.0, 2.0, INF), (DEFAULTS, 0.5, 1.0, 1.0, NAN, 2.0),
        (DEFAULTS, 0.5, 1.0, 1.0, 2.0, NAN), (DEFAULTS, 0.5, 1.0, 1.0, INF, NAN),
    ]
    return cases


def step_cases():
    rng = np.random.default_rng(11)
    cases = {
        "accepted_at_once": (DEFAULTS, 10.0, [3.0]),
        "one_halving": (DEFAULTS, 10.0, [50.0, 9.0]),
        "parabola": (DEFAULTS, 10.0, [1e4, 300.0, 40.0, 12.0, 9.99]),
        "inf_then_nan": (DEFAULTS, 10.0, [INF, NAN, 1e300, 25.0, 9.0]),
        "equal_is_rejected": (DEFAULTS, 10.0, [10.0, 10.0 * (1.0 - 1e-4 * 0.5), 9.0]),
        "fails": (DEFAULTS, 10.0, [11.0] * 21),         # maxarm + 1 rejected trials
        "fails_nan": (DEFAULTS, 10.0, [NAN] * 21),
        "fails_maxarm_1": ((1e-4, 0.1, 0.5, 1), 10.0, [11.0, 12.0]),
        "accepted_on_last": (DEFAULTS, 10.0, [11.0] * 20 + [1.0]),
        "other_options": ((0.01, 0.25, 0.4, 6), 2.0, [5.0, 4.0, 3.0, 2.5, 1.97]),
    }
    for i in range(12):  # random streams: rejected a random number of times, then a decrease
        n_res = float(np.exp(rng.uniform(-3, 3)))
        rej = int(rng.integers(0, 8))
        cases[f"random{i}"] = (DEFAULTS, n_res, [n_res * float(np.exp(rng.uniform(0, 4))) for _ in range(rej)] + [0.5 * n_res])
    return cases


OPTION_SETS = [(DEFAULTS, 1), ((1e-4, 0.1, 0.5, 1), 1), ((1e-4, 0.5, 0.5, 20), 1), ((1e-4, 0.1, 0.5, 0), 0),
               ((1e-4, 0.1, 0.5, -3), 0), ((1e-4, 0.0, 0.5, 20), 0), ((1e-4, 0.6, 0.5, 20), 0), ((1e-4, 0.1, 1.0, 20), 0),
               ((1e-4, -0.1, 0.5, 20), 0), ((0.0, 0.1, 0.5, 20), 0), ((1.0, 0.1, 0.5, 20), 0), ((-1e-4, 0.1, 0.5, 20), 0),
               ((NAN, 0.1, 0.5, 20), 0), ((1e-4, NAN, 0.5, 20), 0), ((1e-4, 0.1, NAN, 20), 0)]


def hexes(vals):
    return " ".join(float(v).hex() for v in vals)


def opt_text(o):
    return "%s %d" % (hexes(o[:3]), o[3])


@pytest.fixture(scope="module")
def run():
    """Build the program once and put every query to it in one run."""
    pc, sc = parab_cases(), step_cases()
    lines = ["D"]
    lines += ["O " + opt_text(o) for o, _ in OPTION_SETS]
    lines += ["P %s %s" % (opt_text(c[0]), hexes(c[1:])) for c in pc]
    lines += ["S %s %s %d %s" % (opt_text(o), hexes([n_res]), len(st), hexes(st)) for o, n_res, st in sc.values()]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "ls.cpp"), os.path.join(d, "ls")
        with open(src, "w") as f:
            f.write(SRC)
        base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src]
        if subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"],
                          capture_output=True).returncode != 0:
            subprocess.run(base, check=True)  # no sanitizer runtimes to link here
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    out = iter(p.stdout.splitlines())
    ans = {"defaults": next(out).split()}
    ans["opts"] = [int(next(out)) for _ in OPTION_SETS]
    ans["parab"] = [float.fromhex(next(out)) for _ in pc]
    ans["steps"] = {}
    for name in sc:
        row = next(out).split()
        ans["steps"][name] = (int(row[0]), int(row[1]), [float.fromhex(v) for v in row[2:]])
    assert next(out, None) is None
    return pc, sc, ans


def test_defaults_agree(run):
    d = run[2]["defaults"]
    got = (float.fromhex(d[0]), float.fromhex(d[1]), float.fromhex(d[2]), int(d[3]))
    bt = ah.Backtracking()
    assert got == DEFAULTS == (bt.alpha, bt.sigma0, bt.sigma1, bt.maxarm)


def test_parab3p_three_ways(run):
    pc, _, ans = run
    seen = set()
    for c, got in zip(pc, ans["parab"]):
        o = c[0]
        here = parab3p_here(*c)
        py = ah.Backtracking(*o).parab3p(*c[1:])
        assert got == here == py, c
        lc = c[1]
        assert o[1] * lc <= got <= o[2] * lc
        seen.add("hi" if got == o[2] * lc else ("lo" if got == o[1] * lc else "in"))
    assert seen == {"hi", "lo", "in"}  # both clamps and the interior are exercised


def test_parab3p_special_cases():
    bt = ah.Backtracking()
    assert bt.parab3p(0.5, 1.0, 1.0, 2.0, 1.0) == 0.25  # c2 > 0
    assert bt.parab3p(0.5, 1.0, 1.0, 1.0, 1.0) == 0.25  # c2 = 0
    assert bt.parab3p(0.5, 1.0, 4.0, 3.999, 100.0) == 0.25  # upper clamp
    assert bt.parab3p(0.5, 1.0, 1.0, 50.0, 110.0) == 0.05  # lower clamp
    for ffc, ffm in ((INF, 2.0), (2.0, INF), (NAN, 2.0), (2.0, NAN)):
        assert bt.parab3p(0.5, 1.0, 1.0, ffc, ffm) == 0.25
    lp = bt.parab3p(0.5, 1.0, 1.0, 1.5, 4.0)  # c2 = 0.5 - 1.5 = -1, c1 = 0.75 - 0.5: the minimiser, unclamped
    assert lp == 0.125


@pytest.mark.parametrize("name", list(step_cases()))
def test_step_sequences_three_ways(run, name):
    """The lam of every trial, the number of trials and the verdict: header == Backtracking == the restatement."""
    _, sc, ans = run
    o, n_res, stream = sc[name]
    verdict, used, lams = ans["steps"][name]
    ok_h, used_h, lams_h = step_here(o, n_res, stream)
    ok_b, used_b, lams_b = step_backtracking(ah.Backtracking(*o), n_res, stream)
    assert verdict in (0, 2)
    assert (verdict == 0, used, lams) == (ok_h, used_h, lams_h) == (ok_b, used_b, lams_b)
    assert lams[0] == 1.0 and all(o[1] * a <= b <= o[2] * a for a, b in zip(lams, lams[1:]))
    if len(lams) > 1:
        assert lams[1] == o[2]  # the first reduction is sigma1, whatever the norms
    if name.startswith("fails"):
        assert verdict == 2 and used == o[3] + 1 == len(stream)
    if name in ("accepted_at_once",):
        assert verdict == 0 and used == 1
    if name == "accepted_on_last":
        assert verdict == 0 and used == 21
    if name == "equal_is_rejected":
        assert used == 3  # n_t == (1 - alpha lam) n_res is not a decrease


def test_options_validity(run):
    for (o, want), got in zip(OPTION_SETS, run[2]["opts"]):
        assert got == want, o
        if want:
            ah.Backtracking(*o)
        else:
            with pytest.raises(ValueError):
                ah.Backtracking(*o)


def test_backtracking_messages():
    with pytest.raises(ValueError, match="maxarm"):
        ah.Backtracking(maxarm=0)
    with pytest.raises(ValueError, match="sigma0 <= sigma1"):
        ah.Backtracking(sigma0=0.6, sigma1=0.5)
    with pytest.raises(ValueError, match="alpha"):
        ah.Backtracking(alpha=1.0)


# ---------------------------------------------------------------- header / ctypes / defaults
def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_constants_and_names():
    h = header_text()
    defs = dict(re.findall(r"#define\s+(NK_LINESEARCH_\w+)\s+(\d+)", h))
    assert defs == {"NK_LINESEARCH_NONE": "0", "NK_LINESEARCH_BACKTRACK": "1"}
    assert (_lib.NK_LINESEARCH_NONE, _lib.NK_LINESEARCH_BACKTRACK) == (0, 1)
    proto = re.search(r"int nk_residual_trial\(([^;]*)\);", h).group(1)
    args = [a.strip() for a in " ".join(proto.split()).split(",")]
    assert args == ["nk_ctx* ctx", "const nk_problem* p", "double* out", "const double* u", "const double* v", "double s",
                    "double* n_out"]
    lib = ah.load()
    assert lib.nk_residual_trial.argtypes[5] is _lib.C.c_double and len(lib.nk_residual_trial.argtypes) == 7

    def members(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.findall(r"(\w+)\s*$", part.strip())[0] for part in decl.split(",")]
        return names

    assert members("nk_newton_opts") == [n for n, _ in _lib.nk_newton_opts._fields_]
    assert members("nk_newton_stats") == [n for n, _ in _lib.nk_newton_stats._fields_]
    assert members("nk_newton_opts")[-7:] == ["linesearch", "ls_alpha", "ls_sigma0", "ls_sigma1", "ls_maxarm", "ls_hist",
                                              "ls_hist_cap"]
    assert members("nk_newton_stats")[-2:] == ["n_backtrack", "ls_failed"]


def test_newton_defaults():
    o = _lib.nk_newton_opts()
    assert ah.load().nk_newton_defaults(_lib.C.byref(o)) == 0
    assert o.linesearch == _lib.NK_LINESEARCH_NONE
    assert (o.ls_alpha, o.ls_sigma0, o.ls_sigma1, o.ls_maxarm) == DEFAULTS
    assert not o.ls_hist and o.ls_hist_cap == 0
    assert (o.tol_rel, o.tol_abs, o.max_niter, o.memory) == (1e-6, 1e-12, 50, 20)  # the others as before


def test_result_keeps_its_positional_form():
    r = ah.Result(True, ah.Stats(1, 2, 3.0), 0.5, 7)
    assert (r.n_backtrack, r.ls_failed, r.steps) == (0, False, ())
    assert tuple(r)[:4] == (True, ah.Stats(1, 2, 3.0), 0.5, 7)
