// Fused pre-LN residual join for decoder blocks (GPT-2), gfx950: one row pass
// that returns BOTH the new residual stream and its normalisation.
//
//   forward : h = x + dropout(a);  y = (h - mean) * rstd * gamma + beta
//   backward: t = rstd * (g - mean(g) - xhat * mean(g * xhat)) + dh,  g = dy * gamma
//             dx = t,  da = t * mask / (1 - p)
//             dgamma = sum_rows dy * xhat, dbeta = sum_rows dy
// Two storage types.  The residual STREAM (x, h, dh, dx) is always fp32: it is
// summed over 2 * layers joins and must not be rounded at each.  The BRANCH
// (a, y, dy, da) is what the linears produce and consume: bf16 under autocast,
// fp32 at the reference's precision.  Unfused, a bf16 join is a dropout
// kernel, an fp32 add, an fp32 LayerNorm and a cast back to bf16 (about 29
// bytes per element); here it reads a + x and writes h + y: 12.  The backward
// takes the gradient dh that arrives on the stream from the joins downstream
// (null for the last one), so the residual gradient add costs no pass either.
// Geometry, dropout hash and the dgamma / dbeta partial rows are those of
// ln.hip (ln_common.h): RPW rows per wave, the row in registers as fp32, no LDS
// for a row.
#include <hip/hip_runtime.h>

#include "common.h"
#include "gk_kernels.h"
#include "ln_common.h"

namespace gk {
namespace {

// HAS_A = false: the first LayerNorm of the model.  The stream is x itself,
// nothing is added and h is not written (fp32 in, TB out, no cast pass).
template <int CH, int RPW, typename TB, bool HAS_A>
__global__ __launch_bounds__(kBlock) void res_ln_fwd_kernel(const TB* __restrict__ a, const float* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, TB* __restrict__ y,
                                                            float* __restrict__ h, float* __restrict__ mean,
                                                            float* __restrict__ rstd, int64_t R, int H, float eps,
                                                            uint32_t seed, uint32_t thr, float scale,
                                                            const uint32_t* __restrict__ seed_dev) {
  if (HAS_A && seed_dev != nullptr) seed = hash_u32(__builtin_amdgcn_readfirstlane(*seed_dev), seed);
  constexpr int L = 64 / RPW;
  const int lane = threadIdx.x & 63, sl = lane % L;
  const int64_t row0 = ((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * RPW;
  if (row0 >= R) return;
  const int64_t row = row0 + lane / L;
  const bool rv = row < R;
  const int nc = H >> 3;
  float v[CH][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int c = sl + j * L;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[j][i] = 0.f;
    if (rv && c < nc) {
      load8f(x + row * H + c * 8, v[j]);
      if (HAS_A) {
        float av[8];
        ld8(a + row * H + c * 8, av);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[j][i] += thr ? (keep(seed, row, c * 8 + i, thr) ? av[i] * scale : 0.f) : av[i];
        st8(h + row * H + c * 8, v[j]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[j][i];
    }
  }
  const float mu = row_sum<L>(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < CH; ++j)
    if (rv && sl + j * L < nc)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = v[j][i] - mu;
        q = fmaf(d, d, q);
      }
  const float rs = rsqrtf(row_sum<L>(q) / (float)H + eps);
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int c = sl + j * L;
    if (rv && c < nc) {
      float gv[8], bv[8], o[8];
      load8f(gamma + c * 8, gv);
      load8f(beta + c * 8, bv);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = (v[j][i] - mu) * rs * gv[i] + bv[i];
      st8(y + row * H + c * 8, o);
    }
  }
  if (rv && sl == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// The block walk of add_ln_bwd_kernel: kLnRowsPerBlock rows per block, the
// lanes' dgamma / dbeta column partials folded over the waves through LDS in a
// fixed order into ONE partial row per block (deterministic, no atomics).  dh
// is read in the second loop, where it is first needed: at CH = 8 the first
// loop already holds four fp32 rows (g, xhat and the two accumulators).
template <int CH, int RPW, typename TB>
__global__ __launch_bounds__(kBlock) void res_ln_bwd_kernel(
    const TB* __restrict__ dy, const float* __restrict__ h, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ dh,
    float* __restrict__ dx, TB* __restrict__ da, float* __restrict__ pg, float* __restrict__ pb, int64_t R, int H,
    uint32_t seed, uint32_t thr, float scale, const uint32_t* __restrict__ seed_dev) {
  if (seed_dev != nullptr) seed = hash_u32(__builtin_amdgcn_readfirstlane(*seed_dev), seed);
  constexpr int L = 64 / RPW;
  __shared__ float red[2][64 * 8 * kLnMaxChunks];
  const int lane = threadIdx.x & 63, sl = lane % L, wave = threadIdx.x >> 6;
  const int nc = H >> 3;
  float accg[CH][8], accb[CH][8];
#pragma unroll
  for (int j = 0; j < CH; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) accg[j][i] = accb[j][i] = 0.f;
  const int64_t wrow = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kLnRowsPerWave;
#pragma unroll 1
  for (int rr = 0; rr < kLnRowsPerWave; rr += RPW) {
    const int64_t row = wrow + rr + lane / L;
    const bool rv = row < R;
    const float mu = rv ? mean[row] : 0.f, rs = rv ? rstd[row] : 0.f;
    float g[CH][8], xh[CH][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int c = sl + j * L;
#pragma unroll
      for (int i = 0; i < 8; ++i) g[j][i] = xh[j][i] = 0.f;
      if (rv && c < nc) {
        float dv[8], hv[8], gv[8];
        ld8(dy + row * H + c * 8, dv);
        load8f(h + row * H + c * 8, hv);
        load8f(gamma + c * 8, gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          xh[j][i] = (hv[i] - mu) * rs;
          g[j][i] = dv[i] * gv[i];
          s1 += g[j][i];
          s2 = fmaf(g[j][i], xh[j][i], s2);
          accg[j][i] = fmaf(dv[i], xh[j][i], accg[j][i]);
          accb[j][i] += dv[i];
        }
      }
    }
    const float m1 = row_sum<L>(s1) / (float)H, m2 = row_sum<L>(s2) / (float)H;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int c = sl + j * L;
      if (rv && c < nc) {
        float t[8], od[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = 0.f;
        if (dh) load8f(dh + row * H + c * 8, t);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          t[i] += rs * (g[j][i] - m1 - xh[j][i] * m2);
          if (da) od[i] = thr ? (keep(seed, row, c * 8 + i, thr) ? t[i] * scale : 0.f) : t[i];
        }
        st8(dx + row * H + c * 8, t);
        if (da) st8(da + row * H + c * 8, od);
      }
    }
  }
  // the row halves of a wave own the same columns: fold them first
  if (RPW == 2) {
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        accg[j][i] += __shfl_xor(accg[j][i], 32, 64);
        accb[j][i] += __shfl_xor(accb[j][i], 32, 64);
      }
  }
  // waves 0, 1, 2, 3 in turn into the block's LDS row (fixed order)
  for (int w = 0; w < kWavesPerBlock; ++w) {
    if (wave == w && lane < L) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int c = sl + j * L;
        if (c < nc)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            red[0][c * 8 + i] = w ? red[0][c * 8 + i] + accg[j][i] : accg[j][i];
            red[1][c * 8 + i] = w ? red[1][c * 8 + i] + accb[j][i] : accb[j][i];
          }
      }
    }
    __syncthreads();
  }
  for (int c4 = threadIdx.x; c4 < (H >> 2); c4 += kBlock) {
    reinterpret_cast<float4*>(pg + (int64_t)blockIdx.x * H)[c4] = reinterpret_cast<const float4*>(red[0])[c4];
    reinterpret_cast<float4*>(pb + (int64_t)blockIdx.x * H)[c4] = reinterpret_cast<const float4*>(red[1])[c4];
  }
}

struct ResFwdArgs {
  const void* a;
  const float *x, *gamma, *beta;
  void* y;
  float *h, *mean, *rstd;
  int64_t R;
  int H;
  float eps;
  uint32_t seed, thr;
  float scale;
  const uint32_t* seed_dev;
  hipStream_t stream;
  bool f32;
};

template <int CH, int RPW>
struct ResFwdLaunch {
  const ResFwdArgs* p;
  template <typename TB, bool HAS_A>
  void go() const {
    const int64_t waves = (p->R + RPW - 1) / RPW;
    const unsigned grid = (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL((res_ln_fwd_kernel<CH, RPW, TB, HAS_A>), dim3(grid), dim3(kBlock), 0, p->stream,
                       static_cast<const TB*>(p->a), p->x, p->gamma, p->beta, static_cast<TB*>(p->y), p->h, p->mean,
                       p->rstd, p->R, p->H, p->eps, p->seed, p->thr, p->scale, p->seed_dev);
  }
  void operator()() const {
    if (p->f32) p->a ? go<float, true>() : go<float, false>();
    else p->a ? go<uint16_t, true>() : go<uint16_t, false>();
  }
};

struct ResBwdArgs {
  const void* dy;
  const float *h, *mean, *rstd, *gamma, *dh;
  float* dx;
  void* da;
  float *pg, *pb;
  int64_t R;
  int H;
  uint32_t seed, thr;
  float scale;
  const uint32_t* seed_dev;
  hipStream_t stream;
  bool f32;
};

template <int CH, int RPW>
struct ResBwdLaunch {
  const ResBwdArgs* p;
  template <typename TB>
  void go() const {
    hipLaunchKernelGGL((res_ln_bwd_kernel<CH, RPW, TB>), dim3((unsigned)((p->R + kLnRowsPerBlock - 1) / kLnRowsPerBlock)),
                       dim3(kBlock), 0, p->stream, static_cast<const TB*>(p->dy), p->h, p->mean, p->rstd, p->gamma,
                       p->dh, p->dx, static_cast<TB*>(p->da), p->pg, p->pb, p->R, p->H, p->seed, p->thr, p->scale,
                       p->seed_dev);
  }
  void operator()() const {
    if (p->f32) go<float>();
    else go<uint16_t>();
  }
};

}  // namespace

void res_ln_forward(const void* a, const float* x, const float* gamma, const float* beta, void* y, float* h,
                    float* mean, float* rstd, int64_t R, int H, float eps, float p, uint32_t seed,
                    const uint32_t* seed_dev, hipStream_t stream, bool f32) {
  if (R <= 0) return;   // no rows: nothing to launch (a zero-sized grid is a launch error)
  const uint32_t thr = ln_keep_threshold(p);
  const float scale = ln_keep_scale(p);
  const ResFwdArgs args{a, x, gamma, beta, y, h, mean, rstd, R, H, eps, seed, thr, scale, seed_dev, stream, f32};
  ln_dispatch<ResFwdLaunch>(H >> 3, {&args}, {&args}, {&args}, {&args}, {&args}, {&args}, {&args});
}

void res_ln_backward(const void* dy, const float* h, const float* mean, const float* rstd, const float* gamma,
                     const float* dh, float* dx, void* da, float* dgamma, float* dbeta, int accumulate, float* ws,
                     int64_t R, int H, float p, uint32_t seed, const uint32_t* seed_dev, hipStream_t stream, bool f32) {
  if (R <= 0 && accumulate) return;   // no rows: dx / da are empty and the sums to add are zero
  const int64_t P = R > 0 ? (R + kLnRowsPerBlock - 1) / kLnRowsPerBlock : 0;
  float* pg = ws;
  float* pb = ws + P * H;
  float* q = ws + 2 * P * H;   // [2][kFinSplits][H]: fits the 2 * add_ln_partial_rows(R) * H of the workspace
  if (R > 0) {
    const uint32_t thr = ln_keep_threshold(p);
    const float scale = ln_keep_scale(p);
    const ResBwdArgs args{dy, h, mean, rstd, gamma, dh, dx, da, pg, pb, R, H, seed, thr, scale, seed_dev, stream, f32};
    ln_dispatch<ResBwdLaunch>(H >> 3, {&args}, {&args}, {&args}, {&args}, {&args}, {&args}, {&args});
  }
  // no rows: P = 0 gives the zero sums through the same two kernels (no memset, which a graph capture cannot take)
  if (dgamma || dbeta) ln_param_reduce(pg, pb, P, H, q, dgamma, dbeta, accumulate, stream);
}

}  // namespace gk
