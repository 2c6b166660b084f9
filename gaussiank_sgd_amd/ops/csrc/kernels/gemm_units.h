// What gemm.hip (the public entry points) and the GEMM instantiation units share:
// the operand descriptors and the per-unit entry points.  Declarations only -- the
// kernel templates are in the family headers (gemm_nt.h, gemm_tn*.h, gemm_*_x62.h).
#pragma once

#include <hip/hip_runtime.h>

#include "gemm_cfg.h"
#include "gk_kernels.h"

namespace gk {

// Implicit-GEMM convolution: row m of the A operand is output pixel
// (n, oh, ow) and K slice k0 (64 channels) is tap (kh, kw) of input channels
// c0..c0+63 (K = KH*KW*C, tap-major, matching a channels-last [Cout][KH][KW][C]
// weight).  Out-of-image taps read a zero row (padding) -- LDS-DMA cannot write
// zeros itself.
constexpr int kMaxTaps = 4;   // gemm_nt gather: at most 4 taps per kernel dimension

struct ConvGeo {
  const void* zero;       // >= 128 zero bytes (one K slice row of either element type)
  int H, W, C, OH, OW, S, P, KW;
  const float* bias;      // optional per-output-channel bias (gemm_nt / conv_nt epilogue)
  // gemm_nt output row remap (stride-2 grad-input parity classes): RH > 0 stores
  // row m = (n, oh, ow) of the OH x OW class grid at image row
  // (n * RH + 2 oh + RA) * RW + 2 ow + RB of the RH x RW output; RZ also writes
  // zeros to the three other parity positions (1x1 stride-2: those get no tap)
  int RH, RW, RA, RB, RZ;
  // gemm_nt split-K (row GEMMs only): KZ > 1 launches KZ planes along z, plane z
  // multiplies K slices [z K, (z + 1) K) of A and B into its own fp32 output
  // plane C + z M ldc (plain epilogue); nt_splitk_reduce_kernel sums the planes
  int KZ;
  // bf16x6 register-staged kernels, cfg family 3: the B operand already split
  // into three bf16 planes, [N][K / 32][3][32] (split3_rows); nullptr otherwise
  const uint16_t* b3;
};

// BatchNorm-backward epilogue (grad-input GEMM of the convolution that consumes
// a fused BN + ReLU [+ residual] output): instead of the plain gradient dy the
// kernel stores dz = relu_mask ? bf16(dy) + dy2 : 0 (dy2: the BN output's second
// consumer's gradient, ResNet shortcut) and reduces per-channel partials
// sum(dz) and sum(dz * h) (h: the BN input) into `stats`, which is what the BN
// backward's separate reduction pass would read dy, dy2, h and the mask for.
// The operands are loaded per output row in the epilogue (transient registers:
// the main loop's register budget is unchanged).
struct BnBwd {
  const void* h;          // BN input [M, N] (same ld and element type as C); nullptr: plain epilogue
  const void* dy2;        // optional second gradient [M, N]
  const uint8_t* mask;    // optional 1-bit ReLU mask, one byte per 16-byte vector: (m, n / V) at
                          // m * (N / V) + n / V, V = 8 (bf16) or 4 (fp32) -- bn_act.hip's layout
  // OW > 0: dy2 is compact (BnBwdArgs; gemm_nt_x62_kernel only): row m = (n, h, w) of the
  // H x W grid adds row (n OH + h / 2) OW + w / 2 of dy2 when h and w are even, else 0
  int H, W, OH, OW;
  // m / (H W) and m / W for m < 2^31 without a division: (umulhi(m, mg) + m) >> sh (magic_u32)
  uint32_t mg_hw, sh_hw, mg_w, sh_w;
};

// Round-up magic number of the divisor d >= 1: (umulhi(n, mg) + n) >> sh == n / d for
// every n < 2^31 (mg = floor(2^32 (2^sh - d) / d) + 1, sh = ceil(log2 d); umulhi(n, mg) < n,
// so the sum fits 32 bits)
inline void magic_u32(uint32_t d, uint32_t* mg, uint32_t* sh) {
  uint32_t s = 0;
  while (((uint64_t)1 << s) < d) ++s;
  *sh = s;
  *mg = (uint32_t)(((((uint64_t)1 << s) - d) << 32) / d + 1);
}

// Lazy BatchNorm-backward operand (fp32): the A operand (NT) / G operand (TN)
// is the gradient of a BN input, dx = k1 ((dz - k2) - (x - mu) k4), which is
// never materialised -- the kernel stages dz AND x tiles and applies the
// per-channel affine map after its LDS reads (bn_act.hip bn_bwd_finalize_lazy
// makes coef[c] = {k1, k2, mu, k4}).  Padding taps load the rows padz = k2 and
// padx = mu, so they contribute exactly 0.  The BN's apply pass (read dz and
// x, write dx) disappears; the two consumers (grad-input and grad-weight of
// the producing convolution) read dz and x instead of dx.
struct LazyA {
  const void* x;          // BN input, same layout / strides as the dz operand
  const float* coef;      // [C] x {k1, k2, mu, k4}
  const void* padz;       // [C] padding row of dz (k2)
  const void* padx;       // [C] padding row of x (mu)
  int C;                  // channels of dz (coefficient table length)
};

// per-unit dispatchers (gemm_inst_*.hip, one object per GK_GEMM_UNIT); w: the decoded
// configuration word (gemm_cfg.h) -- nothing below the gk:: entry points sees the integer
#define GK_NT_UNIT_ARGS                                                                                  \
  const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc, int64_t M, int N, int K, \
      const cfg::NtWord &w, int max_blocks, const ConvGeo &geo, float *stats, int64_t stats_ld,         \
      int stats_rows, const BnBwd &bb, const LazyArgs *lza, hipStream_t stream
#define GK_NT_UNIT_PASS A, lda, B, ldb, C, ldc, M, N, K, w, max_blocks, geo, stats, stats_ld, stats_rows, bb, lza, stream
int nt_b16_row(GK_NT_UNIT_ARGS);   // unit 0
int nt_b16_gat(GK_NT_UNIT_ARGS);   // unit 1
int nt_f32_row(GK_NT_UNIT_ARGS);   // unit 2
int nt_f32_gat(GK_NT_UNIT_ARGS);   // unit 3
int nt_x6_row(GK_NT_UNIT_ARGS);    // unit 5: fp32 operands, bf16x6 products
int nt_x6_gat(GK_NT_UNIT_ARGS);    // unit 6
// unit 8: fp32 row GEMMs, bf16x6 with register staging (gemm_nt_x62_kernel)
int nt_x62_row(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
               const cfg::NtWord& w, int max_blocks, const float* bias, float* stats, int64_t stats_ld, int stats_rows,
               const BnBwd& bb, const uint16_t* b3, hipStream_t stream);
// unit 10: implicit-GEMM convolutions, bf16x6 with register staging
int nt_x62_gat(const float* A, const float* B, float* C, int64_t M, int N, int K, const cfg::NtWord& w, int max_blocks,
               const ConvGeo& geo, float* stats, int64_t stats_ld, int stats_rows, const BnBwd& bb,
               hipStream_t stream);
// unit 9: fp32 row grad-weight GEMMs, bf16x6 with register staging (gemm_tn_x62_kernel)
void tn_x62_row(const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw, int64_t M, int N,
                int K, const cfg::TnF32Word& w, int splits, hipStream_t stream);
// unit 7: fp32 grad-weight (TN) GEMMs with bf16x6 products
void tn_unit_x6(bool gather, const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw,
                int64_t M, int N, int K, const cfg::TnF32Word& w, int splits, const ConvGeo& geo, const LazyArgs* lza,
                hipStream_t stream);
// unit 4: grad-weight (TN) GEMMs, both operand types and forms
void tn_unit_b16(bool gather, const void* G, int64_t ldg, const void* X, int64_t ldx, float* W, int64_t ldw, int64_t M,
                 int N, int K, const cfg::TnWord& w, int splits, const ConvGeo& geo, hipStream_t stream);
void tn_unit_f32(bool gather, const float* G, int64_t ldg, const float* X, int64_t ldx, float* W, int64_t ldw,
                 int64_t M, int N, int K, const cfg::TnF32Word& w, int splits, const ConvGeo& geo, const LazyArgs* lza,
                 hipStream_t stream);

}  // namespace gk
