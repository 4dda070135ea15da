"""The kind table of csrc/nk_kind.hpp (kind_of, kStencilKinds, for_kind) against the facts other files keep on their
own: the #defines of include/nkhip.h (a kind's name says its family, dimension and scheme), ariadne_hip/_lib.py's
constants, the (scheme, dim) -> kind tables of the oracle and of ariadne_hip/problems.py, the Makefile's ST_KINDS
(one stencil object per kind), and the refusals the library has always made (periodic boundaries for the heat kinds
only, one rank for NK_BRATU3D and the ignition kinds, no F0R instance for the ignition kinds).

A small program includes the header (it needs no HIP), is built with g++ -- under the address and
undefined-behaviour sanitizers where the toolchain links them -- and prints every field of kind_of(k) for k in 0 .. 31,
kStencilKinds, and what for_kind does with every k in -1 .. 40.
"""
import os
import re
import subprocess
import tempfile

import pytest

import _nkpath  # noqa: F401
from ariadne_hip import _lib, problems
from oracle import oracle as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "newtonkrylov.jl_amd")
HEADER = os.path.join(ROOT, "include", "nkhip.h")

FIELDS = ("dim", "scheme", "heat", "bratu", "ignition", "user", "exp", "un", "periodic", "ranks", "blocks3d", "f0r",
          "stencil", "jexact_un")
SRC = r"""
#include <cstdio>
#include "nk_kind.hpp"
int main() {
    for (int k = 0; k < 32; ++k) {
        const nk::Kind K = nk::kind_of(k);
        std::printf("K %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", k, K.dim, K.scheme, (int)K.heat, (int)K.bratu,
                    (int)K.ignition, (int)K.user, (int)K.exp, (int)K.un, (int)K.periodic, (int)K.ranks, (int)K.blocks3d,
                    (int)K.f0r, (int)nk::stencil_kind(k), (int)nk::jexact_reads_un(k));
    }
    std::printf("S");
    for (int k : nk::kStencilKinds) std::printf(" %d", k);
    std::printf("\n");
    for (int k = -1; k <= 40; ++k) {  // F k: for_kind's return, the calls it made, the template argument of the last
        int calls = 0, arg = -1;
        const bool ok = nk::for_kind(k, [&](auto KC) { ++calls; arg = decltype(KC)::value; });
        std::printf("F %d %d %d %d\n", k, (int)ok, calls, arg);
    }
    return 0;
}
"""
SCHEME_OF = {"EULER": 0, "MIDPOINT": 1, "TRAPEZOID": 2}


@pytest.fixture(scope="module")
def table():
    """Build the program once: ({k: {field: value}}, kStencilKinds, {k: (returned, calls, argument)})."""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "kind.cpp"), os.path.join(d, "kind")
        with open(src, "w") as f:
            f.write(SRC)
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(AMD, "csrc"), "-I",
                os.path.join(ROOT, "include"), "-o", exe, src]
        if subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"],
                          capture_output=True).returncode != 0:
            subprocess.run(base, check=True)  # no sanitizer runtimes to link here
        p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    kinds, stencil, visits = {}, None, {}
    for line in p.stdout.splitlines():
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "K":
            kinds[v[0]] = dict(zip(FIELDS, v[1:]))
        elif tag == "S":
            stencil = v
        else:
            visits[v[0]] = tuple(v[1:])
    assert sorted(kinds) == list(range(32)) and sorted(visits) == list(range(-1, 41))
    return kinds, stencil, visits


def header_kinds():
    """{name: number} of the header's problem kinds"""
    hdr = open(HEADER).read()
    return {n: int(v) for n, v in re.findall(r"^#define (NK_(?:BRATU|HEAT|USER|IGNITION)\w+) (\d+)\b", hdr, re.M)}


def test_fields_follow_the_header_names(table):
    """A kind's name in nkhip.h says its family, its dimension and its scheme; exp and u_n follow from the family
    (Bratu and ignition have the exp term; the implicit schemes -- heat and ignition -- carry u_n).  The ignition
    Midpoint kind is the one whose exact tangent reads u_n.  A number the header does not define is no kind."""
    kinds, _, _ = table
    defined = header_kinds()
    assert len(defined) == 15 and len(set(defined.values())) == 15 and max(defined.values()) < 32
    for name, k in defined.items():
        fam, dim, sch = re.fullmatch(r"NK_(BRATU|HEAT|USER|IGNITION)(\d)D(?:_(\w+))?", name).groups()
        K = kinds[k]
        assert K["dim"] == int(dim) and K["scheme"] == (SCHEME_OF[sch] if sch else 0), name
        assert (K["bratu"], K["heat"], K["user"], K["ignition"]) == tuple(int(fam == f) for f in ("BRATU", "HEAT", "USER", "IGNITION")), name
        assert K["exp"] == int(fam in ("BRATU", "IGNITION")) and K["un"] == int(fam in ("HEAT", "IGNITION")), name
        assert K["stencil"] == int(fam != "USER"), name
        assert K["jexact_un"] == int(name == "NK_IGNITION2D_MIDPOINT"), name
    for k in set(range(32)) - set(defined.values()):
        assert not any(kinds[k].values()), k


def test_python_constants_and_tables_agree(table):
    """_lib.py's constants are the header's; the oracle's and problems.py's (scheme, dim) -> kind tables and
    problems.py's _IGNITION name kinds of that family, scheme and dimension."""
    kinds, _, _ = table
    defined = header_kinds()
    assert {n: getattr(_lib, n) for n in defined} == defined
    assert len(oc.HEAT_KINDS) == len(problems._SCHEMES) == 6 and len(problems._IGNITION) == 3
    for (scheme, dim), k in oc.HEAT_KINDS.items():
        assert (kinds[k]["heat"], kinds[k]["scheme"], kinds[k]["dim"]) == (1, SCHEME_OF[scheme.upper()], dim)
    for (scheme, dim), k in problems._SCHEMES.items():
        assert (kinds[k]["heat"], kinds[k]["scheme"], kinds[k]["dim"]) == (1, SCHEME_OF[scheme[2:-1].upper()], dim)
        assert k == oc.HEAT_KINDS[scheme[2:-1].lower(), dim]
    for scheme, k in problems._IGNITION.items():
        assert (kinds[k]["ignition"], kinds[k]["scheme"], kinds[k]["dim"]) == (1, SCHEME_OF[scheme[2:-1].upper()], 2)


def test_makefile_builds_one_object_per_stencil_kind(table):
    """ST_KINDS of the Makefile is kStencilKinds: ascending, and exactly the kinds that are not the caller's."""
    kinds, stencil, _ = table
    mk = open(os.path.join(AMD, "Makefile")).read()
    st_kinds = [int(v) for v in re.search(r"^ST_KINDS = ([\d ]+)$", mk, re.M).group(1).split()]
    assert st_kinds == stencil == sorted(stencil)
    assert stencil == [k for k in range(32) if kinds[k]["dim"] and not kinds[k]["user"]]
    assert stencil == [1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 21, 22]


def test_refusals_are_the_ones_the_library_has_always_made(table):
    """geometry()'s refusals as traits: periodic boundaries for the heat kinds only; one rank for NK_BRATU3D and the
    ignition kinds; 3D blocks for the built-in 3D kinds that run on several ranks; F0R instances for every built-in
    stencil kind but the ignition kinds (what nk_plan.hpp's st_kind_f0r said of them)."""
    kinds, stencil, _ = table
    real = [k for k in range(32) if kinds[k]["dim"]]
    assert [k for k in real if kinds[k]["periodic"]] == [k for k in real if kinds[k]["heat"]] == [3, 4, 5, 6, 7, 8]
    assert [k for k in real if not kinds[k]["ranks"]] == [9, 20, 21, 22]
    assert [k for k in real if kinds[k]["blocks3d"]] == [4, 6, 8]
    assert [k for k in stencil if not kinds[k]["f0r"]] == [20, 21, 22]
    assert not any(kinds[k]["f0r"] for k in range(32) if k not in stencil)


def test_for_kind_visits_each_stencil_kind_once(table):
    """for_kind(k, f) calls f exactly once, with k as the template argument, and returns true for the kinds of
    kStencilKinds; for every other number -- 0, 10 .. 19 (the user kinds among them), 23 and beyond -- it returns
    false without calling f."""
    _, stencil, visits = table
    assert [k for k, (ok, _, _) in sorted(visits.items()) if ok] == stencil
    for k, (ok, calls, arg) in visits.items():
        assert (ok, calls, arg) == ((1, 1, k) if k in stencil else (0, 0, -1)), k
    for k in [0, *range(10, 20), 23, _lib.NK_USER1D, _lib.NK_USER2D, _lib.NK_USER3D]:
        assert visits[k] == (0, 0, -1)
