// Instantiation units of the LDS-DMA grad-weight (TN) GEMM families (gemm_tn.h,
// gemm_tn_f32.h), selected by -DGK_GEMM_UNIT=<n>.
#include "gemm_tn.h"
#include "gemm_tn_f32.h"

namespace gk {

#if GK_GEMM_UNIT == 4
void tn_unit_b16(bool gather, const void* G, int64_t ldg, const void* X, int64_t ldx, float* W, int64_t ldw, int64_t M,
                 int N, int K, const cfg::TnWord& w, int splits, const ConvGeo& geo, hipStream_t stream) {
  if (gather) tn_dispatch<true>(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, geo, stream);
  else tn_dispatch<false>(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, geo, stream);
}
void tn_unit_f32(bool gather, const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw,
                 int64_t M, int N, int K, const cfg::TnF32Word& w, int splits, const ConvGeo& geo, const LazyArgs* lza,
                 hipStream_t stream) {
  if (gather) tn_f32_dispatch<true>(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, geo, lza, stream);
  else tn_f32_dispatch<false>(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, geo, lza, stream);
}
#elif GK_GEMM_UNIT == 7
void tn_unit_x6(bool gather, const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw,
                int64_t M, int N, int K, const cfg::TnF32Word& w, int splits, const ConvGeo& geo, const LazyArgs* lza,
                hipStream_t stream) {
  if (gather) tn_f32_dispatch<true, true>(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, geo, lza, stream);
  else tn_f32_dispatch<false, true>(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, geo, lza, stream);
}
#else
#error "compile with -DGK_GEMM_UNIT=<unit>"
#endif

}  // namespace gk
