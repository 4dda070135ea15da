// nk_stencil_inst.hip -- instantiates the stencil kernels of ONE problem kind (NK_ST_KIND, set by
// the Makefile: one object per kind, compiled in parallel).
#include "nk_stencil_kern.hpp"

#ifndef NK_ST_KIND
#error "compile with -DNK_ST_KIND=<problem kind>"
#endif

namespace nk {

static_assert(stencil_kind(NK_ST_KIND), "NK_ST_KIND is not in kStencilKinds (nk_kind.hpp)");

template <int KIND>
StInst stencil_launch(const KArgs& A, int mode, int epi, int vec, int grid, hipStream_t s, bool per) {
    return go_stencil_mode<KIND>(A, mode, epi, vec, grid, s, per);
}

template <int KIND>
hipError_t stencil_bind_mb(const MbInfo& m) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_mb), &m, sizeof(m));
}

template StInst stencil_launch<NK_ST_KIND>(const KArgs&, int, int, int, int, hipStream_t, bool);
template hipError_t stencil_bind_mb<NK_ST_KIND>(const MbInfo&);

}  // namespace nk
