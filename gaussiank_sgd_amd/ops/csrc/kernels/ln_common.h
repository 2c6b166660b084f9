// Shared by the LayerNorm row kernels (ln.hip: post-LN add+dropout+LN;
// ln_pre.hip: the pre-LN join that also returns the residual stream): the
// 8-element chunk loads / stores, the dropout hash, the row sum, the
// (chunks per lane, rows per wave) dispatch and the dgamma / dbeta reduction.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace gk {

// dgamma / dbeta (+)= column sums of the [P][H] per-block partials pg / pb
// (ln.hip, two levels, fp64 within each, deterministic); q: [2][kFinSplits][H]
// floats, the tail of the add_ln_partial_rows workspace.  P == 0 gives zero sums.
void ln_param_reduce(const float* pg, const float* pb, int64_t P, int H, float* q, float* dgamma, float* dbeta,
                     int accumulate, hipStream_t stream);

namespace {

constexpr int kLnMaxChunks = 8;          // per lane: H <= 64 * 8 * 8 = 4096
constexpr int kLnRowsPerWave = 4;        // backward: rows per wave (RPW at a time)
constexpr int kLnRowsPerBlock = kLnRowsPerWave * kWavesPerBlock;   // backward: one partial row per block

__device__ __forceinline__ void load8(const uint16_t* p, float* v) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ void load8f(const float* p, float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ uint32_t bf16r(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

__device__ __forceinline__ void store8(uint16_t* p, const float* v) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = bf16r(v[2 * i]) | (bf16r(v[2 * i + 1]) << 16);
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

// 8-element chunks of either storage type: 16 bytes of bf16 or 32 of fp32
__device__ __forceinline__ void ld8(const uint16_t* p, float* v) { load8(p, v); }
__device__ __forceinline__ void ld8(const float* p, float* v) { load8f(p, v); }
__device__ __forceinline__ void st8(uint16_t* p, const float* v) { store8(p, v); }
__device__ __forceinline__ void st8(float* p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// keep element (row, col) with probability 1 - p: hash < keep threshold
__device__ __forceinline__ bool keep(uint32_t seed, int64_t row, int col, uint32_t thr) {
  return hash_u32((uint32_t)(row * 8191 + col), seed ^ (uint32_t)(row >> 19)) < thr;
}

// keep threshold (0: no dropout) and the scale of the kept elements
inline uint32_t ln_keep_threshold(float p) { return p > 0.f ? (uint32_t)((1.0 - (double)p) * 4294967295.0) : 0u; }
inline float ln_keep_scale(float p) { return p > 0.f ? 1.f / (1.f - p) : 1.f; }

// sum over the L lanes of one row (L = 64 / rows-per-wave, a power of two)
template <int L>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// (CH, RPW) for a row of nc 16-byte chunks: two rows per wave up to 256
// chunks (H <= 2048), the fewest chunks per lane that cover the row
template <template <int, int> class Launch>
void ln_dispatch(int nc, Launch<1, 2> l12, Launch<2, 2> l22, Launch<3, 2> l32, Launch<4, 2> l42, Launch<6, 2> l62,
                 Launch<8, 2> l82, Launch<8, 1> l81) {
  if (nc <= 32) l12();
  else if (nc <= 64) l22();
  else if (nc <= 96) l32();
  else if (nc <= 128) l42();
  else if (nc <= 192) l62();
  else if (nc <= 256) l82();
  else l81();
}

}  // namespace
}  // namespace gk
