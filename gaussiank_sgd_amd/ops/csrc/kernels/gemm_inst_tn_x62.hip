// The instantiation unit (9) of the register-staged bf16x6 grad-weight GEMM
// family (gemm_tn_x62.h).
#include "gemm_tn_x62.h"

namespace gk {

void tn_x62_row(const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw, int64_t M, int N,
                int K, const cfg::TnF32Word& w, int splits, hipStream_t stream) {
  tn_x62_dispatch(G, ldg, X, ldx, W, ldw, M, N, K, w, splits, stream);
}

}  // namespace gk
