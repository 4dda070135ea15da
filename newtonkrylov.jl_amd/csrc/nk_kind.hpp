// nk_kind.hpp -- the problem kinds of include/nkhip.h, each fact about a kind stated once: kind_of(kind) is the
// kind's row of traits, kStencilKinds the built-in stencil kinds, for_kind the one place where a runtime kind
// becomes a template argument.  Host launchers, the launch plan's callers and the kernels (as constant
// expressions) all read these; nothing else in csrc/ compares a kind against a list or a range.  No HIP header:
// this file compiles with a plain host compiler (tests/test_kind.py holds it against the header's #defines, the
// Python tables and the Makefile's ST_KINDS).
#pragma once

#include <type_traits>

#include "nkhip.h"

namespace nk {

struct Kind {
    int dim;        // 1, 2, 3; 0: the number is no kind
    int scheme;     // implicit.jl scheme: 0 G_Euler! (and the kinds without u_n), 1 G_Midpoint!, 2 G_Trapezoid!
    bool heat;      // an implicit scheme composed with diffusion! (heat_2D.jl)
    bool bratu;     // the Laplacian plus λ exp(u) (bratu.jl and its 2D / 3D generalisations)
    bool ignition;  // an implicit scheme composed with f(u) = a Δu + λ exp(u)
    bool user;      // the residual is the caller's (nk_user_ops): no stencil kernel
    bool exp;       // every point evaluates exp: the table in LDS and the per-lane exact phase
    bool un;        // the kind carries u_n (a, Δt, α with it): the implicit schemes, whatever f they are composed with
    bool periodic;  // bc_periodic! is defined for it (PER kernel instances exist)
    bool ranks;     // it runs on several ranks (slabs of the slowest axis)
    bool blocks3d;  // it runs on 3D blocks (nk_dist_grid with px * py > 1)
    bool f0r;       // it has F0R instances (k_st2d / k_st3l<..., F0R>: F0 recomputed from u); without them the
                    // launcher clears StShape::f0r and the FD launch reads F0
};

constexpr Kind kind_of(int kind) {
    constexpr bool Y = true, n = false;
    switch (kind) {  //                      dim sch heat bra ign usr exp un per rnk blk f0r
    case NK_BRATU1D:              return Kind{1, 0, n, Y, n, n, Y, n, n, Y, n, Y};
    case NK_BRATU2D:              return Kind{2, 0, n, Y, n, n, Y, n, n, Y, n, Y};
    case NK_HEAT2D_EULER:         return Kind{2, 0, Y, n, n, n, n, Y, Y, Y, n, Y};
    case NK_HEAT3D_EULER:         return Kind{3, 0, Y, n, n, n, n, Y, Y, Y, Y, Y};
    case NK_HEAT2D_MIDPOINT:      return Kind{2, 1, Y, n, n, n, n, Y, Y, Y, n, Y};
    case NK_HEAT3D_MIDPOINT:      return Kind{3, 1, Y, n, n, n, n, Y, Y, Y, Y, Y};
    case NK_HEAT2D_TRAPEZOID:     return Kind{2, 2, Y, n, n, n, n, Y, Y, Y, n, Y};
    case NK_HEAT3D_TRAPEZOID:     return Kind{3, 2, Y, n, n, n, n, Y, Y, Y, Y, Y};
    case NK_BRATU3D:              return Kind{3, 0, n, Y, n, n, Y, n, n, n, n, Y};
    case NK_USER1D:               return Kind{1, 0, n, n, n, Y, n, n, n, Y, n, n};
    case NK_USER2D:               return Kind{2, 0, n, n, n, Y, n, n, n, Y, n, n};
    case NK_USER3D:               return Kind{3, 0, n, n, n, Y, n, n, n, Y, n, n};
    case NK_IGNITION2D_EULER:     return Kind{2, 0, n, n, Y, n, Y, Y, n, n, n, n};
    case NK_IGNITION2D_MIDPOINT:  return Kind{2, 1, n, n, Y, n, Y, Y, n, n, n, n};
    case NK_IGNITION2D_TRAPEZOID: return Kind{2, 2, n, n, Y, n, Y, Y, n, n, n, n};
    default:                      return Kind{};
    }
}

// the exact tangent reads u_n: G_Midpoint! ∘ f with an exp term exponentiates m = α u_n + (1 - α) u (k_st2d's kUn
// for MODE_JEXACT, k_jdiag and the byte models of the stencil and the batched launch)
constexpr bool jexact_reads_un(int kind) { return kind_of(kind).un && kind_of(kind).exp && kind_of(kind).scheme == 1; }

// the built-in stencil kinds, ascending: one object of nk_stencil_inst.hip each (the Makefile's ST_KINDS)
constexpr int kStencilKinds[] = {NK_BRATU1D,          NK_BRATU2D,          NK_HEAT2D_EULER,     NK_HEAT3D_EULER,
                                 NK_HEAT2D_MIDPOINT,  NK_HEAT3D_MIDPOINT,  NK_HEAT2D_TRAPEZOID, NK_HEAT3D_TRAPEZOID,
                                 NK_BRATU3D,          NK_IGNITION2D_EULER, NK_IGNITION2D_MIDPOINT,
                                 NK_IGNITION2D_TRAPEZOID};
constexpr bool stencil_kind(int kind) {
    for (int k : kStencilKinds)
        if (k == kind) return true;
    return false;
}

// f(std::integral_constant<int, K>{}) for the built-in stencil kind K == kind; false (f not called) for any other
// number.  The only place where a runtime kind becomes a template argument.
template <int K>
using KindC = std::integral_constant<int, K>;
template <class F>
bool for_kind(int kind, F&& f) {
    switch (kind) {
    case NK_BRATU1D: f(KindC<NK_BRATU1D>{}); return true;
    case NK_BRATU2D: f(KindC<NK_BRATU2D>{}); return true;
    case NK_HEAT2D_EULER: f(KindC<NK_HEAT2D_EULER>{}); return true;
    case NK_HEAT3D_EULER: f(KindC<NK_HEAT3D_EULER>{}); return true;
    case NK_HEAT2D_MIDPOINT: f(KindC<NK_HEAT2D_MIDPOINT>{}); return true;
    case NK_HEAT3D_MIDPOINT: f(KindC<NK_HEAT3D_MIDPOINT>{}); return true;
    case NK_HEAT2D_TRAPEZOID: f(KindC<NK_HEAT2D_TRAPEZOID>{}); return true;
    case NK_HEAT3D_TRAPEZOID: f(KindC<NK_HEAT3D_TRAPEZOID>{}); return true;
    case NK_BRATU3D: f(KindC<NK_BRATU3D>{}); return true;
    case NK_IGNITION2D_EULER: f(KindC<NK_IGNITION2D_EULER>{}); return true;
    case NK_IGNITION2D_MIDPOINT: f(KindC<NK_IGNITION2D_MIDPOINT>{}); return true;
    case NK_IGNITION2D_TRAPEZOID: f(KindC<NK_IGNITION2D_TRAPEZOID>{}); return true;
    default: return false;
    }
}

// the three lists above name the same kinds: a stencil kind is a kind that is not the caller's, and the other
// way round (for_kind's cases: tests/test_kind.py)
constexpr bool kinds_consistent() {
    for (int k = -1; k < 64; ++k)
        if (stencil_kind(k) != (kind_of(k).dim != 0 && !kind_of(k).user)) return false;
    return true;
}
static_assert(kinds_consistent(), "kStencilKinds and kind_of disagree");

}  // namespace nk
