// Instantiation units of the register-staged bf16x6 NT GEMM family
// (gemm_nt_x62.h), selected by -DGK_GEMM_UNIT=<n>.
#include "gemm_nt_x62.h"

namespace gk {

#if GK_GEMM_UNIT == 8
int nt_x62_row(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
               const cfg::NtWord& w, int max_blocks, const float* bias, float* stats, int64_t stats_ld, int stats_rows,
               const BnBwd& bb, const uint16_t* b3, hipStream_t stream) {
  ConvGeo g{};
  g.b3 = b3;
  return nt_x62_dispatch<false>(A, lda, B, ldb, C, ldc, M, N, K, w, max_blocks, bias, stats, stats_ld, stats_rows, bb,
                                g, stream);
}
#elif GK_GEMM_UNIT == 10
int nt_x62_gat(const float* A, const float* B, float* C, int64_t M, int N, int K, const cfg::NtWord& w, int max_blocks,
               const ConvGeo& geo, float* stats, int64_t stats_ld, int stats_rows, const BnBwd& bb,
               hipStream_t stream) {
  return nt_x62_dispatch<true>(A, geo.C, B, K, C, N, M, N, K, w, max_blocks, geo.bias, stats, stats_ld, stats_rows,
                               bb, geo, stream);
}
#else
#error "compile with -DGK_GEMM_UNIT=<unit>"
#endif

}  // namespace gk
