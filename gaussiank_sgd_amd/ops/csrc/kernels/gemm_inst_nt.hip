// Instantiation units of the LDS-DMA NT GEMM family (gemm_nt.h), one per operand type /
// row-vs-gather form, selected by -DGK_GEMM_UNIT=<n>; ops/build.py compiles them in parallel.
#include "gemm_nt.h"

#ifndef GK_GEMM_UNIT
#error "compile with -DGK_GEMM_UNIT=<unit>"
#endif

namespace gk {

#if GK_GEMM_UNIT == 0
int nt_b16_row(GK_NT_UNIT_ARGS) { return nt_dispatch<false, uint16_t>(GK_NT_UNIT_PASS); }
#elif GK_GEMM_UNIT == 1
int nt_b16_gat(GK_NT_UNIT_ARGS) { return nt_dispatch<true, uint16_t>(GK_NT_UNIT_PASS); }
#elif GK_GEMM_UNIT == 2
int nt_f32_row(GK_NT_UNIT_ARGS) { return nt_dispatch<false, float>(GK_NT_UNIT_PASS); }
#elif GK_GEMM_UNIT == 3
int nt_f32_gat(GK_NT_UNIT_ARGS) { return nt_dispatch<true, float>(GK_NT_UNIT_PASS); }
#elif GK_GEMM_UNIT == 5
int nt_x6_row(GK_NT_UNIT_ARGS) { return nt_dispatch<false, float, true>(GK_NT_UNIT_PASS); }
#elif GK_GEMM_UNIT == 6
int nt_x6_gat(GK_NT_UNIT_ARGS) { return nt_dispatch<true, float, true>(GK_NT_UNIT_PASS); }
#else
#error "unknown GK_GEMM_UNIT"
#endif

}  // namespace gk
