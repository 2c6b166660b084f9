// Fused optimizer kernels over flat parameter / momentum / gradient arenas.
//
//   fused_sgd        K12: torch.optim.SGD semantics (weight decay, momentum,
//                    dampening, nesterov; first step buf = d) for every param
//                    group in ONE launch, plus optional gradient zeroing and a
//                    device-side gradient scale (clip coefficient, K14).
//                    Reference: dl_trainer.py:212-228 (two param groups),
//                    dl_trainer.py:839-873 (_step), torch SGD via
//                    distributed_optimizer.py:546.
//   fused_adam       torch.optim.Adam / AdamW (single-tensor, no amsgrad) with the
//                    same chunk table, gradient zeroing, bf16 shadow and device
//                    scalars; the step count is a device scalar bumped by a
//                    one-thread launch ahead of the update, so eager steps and
//                    HIP-graph replays take one path with no host read.
//   fused_lamb       LAMB (You et al. 2020): the Adam direction u with decoupled
//                    decay, scaled per tensor by ||w|| / ||u||.  Three launches
//                    after the step tick (moments + chunk partials, one wave per
//                    tensor for the ratio, apply); the norms are reduced in a
//                    fixed order, so replicas stay bit-identical.
//   segmented_sumsq  per-tensor ||w||^2, ||g||^2 (LARS trust ratios)
//   fused_lars       K13: lars.py:67-134 (trust ratio clamp [0,50], grad clamp
//                    +-10, acceleration buffer initialised to ones)
//   clip_grad_norm   K14: global-norm clip with no host sync
//                    (dist_trainer.py:80-85 clip after synchronize()).
//
// The arenas are float4-aligned per tensor (the Python arena pads every tensor
// to 64 elements), so each workgroup streams one <=16K-element chunk with
// 16-byte loads.  for_chunk() is that loop: every chunk kernel states its
// per-element arithmetic once, as a body over Vec<N>, and for_chunk runs it
// with N = 4 over the chunk's float4s and with N = 1 over the up to 3 elements
// left (a length the arena's padding never produces, but the ops accept it).
#include "common.h"
#include "gk_kernels.h"

namespace gk {
namespace {

__device__ __forceinline__ uint16_t f2bf(float f) {  // round-to-nearest-even, NaN kept quiet
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// ---- streaming one chunk --------------------------------------------------------
// N consecutive floats in registers, moved by load / store as ONE access: 16 bytes for N = 4, a float for N = 1.
template <int N>
struct Vec {
  float e[N];
  __device__ __forceinline__ float& operator[](int j) { return e[j]; }
  __device__ __forceinline__ float operator[](int j) const { return e[j]; }
};
template <int N>
struct Width { static constexpr int value = N; };

template <int N>
using Packed = float __attribute__((ext_vector_type(N)));   // the access: global_load / global_store_dwordx4 for N = 4
template <int N>
__device__ __forceinline__ Vec<N> load(const float* p, int i) {
  const Packed<N> t = reinterpret_cast<const Packed<N>*>(p)[i];
  Vec<N> v;
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = t[j];
  return v;
}
template <int N>
__device__ __forceinline__ void store(float* p, int i, const Vec<N>& v) {
  Packed<N> t;
#pragma unroll
  for (int j = 0; j < N; ++j) t[j] = v[j];
  reinterpret_cast<Packed<N>*>(p)[i] = t;
}

// bf16 shadow of N new weights: one 8-byte store for N = 4
template <int N>
__device__ __forceinline__ void store_shadow(uint16_t* s, int i, const Vec<N>& w) {
  if constexpr (N == 4) {
    const uint32_t lo = (uint32_t)f2bf(w[0]) | ((uint32_t)f2bf(w[1]) << 16);
    const uint32_t hi = (uint32_t)f2bf(w[2]) | ((uint32_t)f2bf(w[3]) << 16);
    reinterpret_cast<uint2*>(s)[i] = make_uint2(lo, hi);
  } else {
    s[i] = f2bf(w[0]);
  }
}

// The sum of squares as the norms (LAMB, LARS) define it: (x^2 + y^2) + (z^2 + w^2) for a float4, one square at a
// time in the tail.  The trust ratios are bit-identical across replicas only while this association holds.
template <int N>
__device__ __forceinline__ float sumsq(const Vec<N>& a) {
  if constexpr (N == 4) return (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
  else return a[0] * a[0];
}

// body(Width<4>(), i) for every float4 i of a chunk of `len` elements, then body(Width<1>(), i) for the elements
// behind the last whole float4; i indexes units of N floats from the chunk's start, as load / store take it.
template <class Body>
__device__ __forceinline__ void for_chunk(int len, Body body) {
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += kBlock) body(Width<4>(), i);
  for (int i = (n4 << 2) + threadIdx.x; i < len; i += kBlock) body(Width<1>(), i);
}

__device__ __forceinline__ float sgd_elem(float w, float& m, float g, const SgdGroup& p, float gs) {
  float d = g * gs;
  if (p.weight_decay != 0.f) d = fmaf(p.weight_decay, w, d);
  if (p.momentum != 0.f) {
    if (p.first_step) m = d;
    else m = fmaf(p.momentum, m, (1.f - p.dampening) * d);
    d = p.nesterov ? fmaf(p.momentum, m, d) : m;
  }
  return fmaf(-p.lr, d, w);
}

__global__ __launch_bounds__(kBlock) void fused_sgd_kernel(SgdArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  SgdGroup p = a.groups[c.group];
  if (a.lr_mult) p.lr *= *a.lr_mult;   // lr schedule of a captured graph, read at replay time
  const float gs = a.grad_scale ? *a.grad_scale : 1.f;
  float* w = a.w + c.start;
  float* m = a.m ? a.m + c.start : nullptr;
  float* g = a.g + c.start;
  uint16_t* shadow = a.w_bf16 ? a.w_bf16 + c.start : nullptr;
  const bool use_m = p.momentum != 0.f;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    Vec<N> wv = load<N>(w, i);
    const Vec<N> gv = load<N>(g, i);
    Vec<N> mv = {};
    if (use_m && !p.first_step) mv = load<N>(m, i);
#pragma unroll
    for (int j = 0; j < N; ++j) wv[j] = sgd_elem(wv[j], mv[j], gv[j], p, gs);
    store<N>(w, i, wv);
    if (use_m) store<N>(m, i, mv);
    if (a.zero_grad) store<N>(g, i, Vec<N>{});
    if (shadow) store_shadow<N>(shadow, i, wv);
  });
}

// ---- Adam / AdamW and LAMB: one core --------------------------------------------
// Per-workgroup constants of one chunk's param group at the current step.
struct AdamCoef {
  float omb1, beta2, omb2;   // 1 - beta1, beta2, 1 - beta2
  float bc1;                 // 1 - beta1^t
  float bc2_sqrt;            // sqrt(1 - beta2^t)
  float eps;
  float wd;                  // weight decay added as wd * w: to the gradient (Adam, 0 when decoupled), to u (LAMB)
  float decay;               // AdamW: 1 - lr * wd (1 when coupled)
  float step_size;           // lr / (1 - beta1^t)
  double lr;                 // lr * lr_mult; read by lamb_apply_kernel alone, which scales it by the trust ratio
};                           // (a kernel's unused fields cost nothing: the compiler drops them from its LDS copy)

// Thread 0 of a workgroup: the bias corrections from the device step count, in double (torch derives them, lr / bc1
// and 1 - lr * wd from Python floats before it rounds); once per workgroup, then through LDS -- a per-element pow
// would make the streaming passes compute-bound.
__device__ __forceinline__ AdamCoef adam_coef(const AdamHyper& p, bool decoupled, const float* step,
                                              const float* lr_mult) {
  const double t = (double)*step;
  AdamCoef k;
  k.lr = p.lr;
  if (lr_mult) k.lr *= (double)*lr_mult;   // lr schedule of a captured graph; scales the decoupled decay too
  const double bc1 = 1.0 - pow(p.beta1, t);
  const double bc2 = 1.0 - pow(p.beta2, t);
  k.omb1 = (float)(1.0 - p.beta1);
  k.beta2 = (float)p.beta2;
  k.omb2 = (float)(1.0 - p.beta2);
  k.bc1 = (float)bc1;
  k.bc2_sqrt = (float)sqrt(bc2);
  k.eps = (float)p.eps;
  k.wd = decoupled ? 0.f : (float)p.weight_decay;
  k.decay = decoupled ? (float)(1.0 - k.lr * p.weight_decay) : 1.f;
  k.step_size = (float)(k.lr / bc1);
  return k;
}

__global__ void adam_tick_kernel(float* __restrict__ step) { *step += 1.f; }

// The moments from the scaled gradient d, in torch's forms (lerp; mul, addcmul).  Adam and LAMB share state that a
// wrapped optimizer hands from one to the other, and LAMB without adaptation is bit-for-bit AdamW: one copy.
__device__ __forceinline__ void adam_moments(float& m, float& v, float d, const AdamCoef& k) {
  m = fmaf(k.omb1, d - m, m);
  v = fmaf(k.omb2 * d, d, k.beta2 * v);
}

// sqrt(vhat) + eps.  sqrtf and '/' are the correctly rounded ones (with eps = 1e-8 and the tiny v of a sparsified
// gradient the approximate rcp / rsq are visible).
__device__ __forceinline__ float adam_denom(float v, const AdamCoef& k) { return sqrtf(v) / k.bc2_sqrt + k.eps; }

// torch's single-tensor order of operations.  A slot with w = g = m = v = 0 (padding) stays exactly 0 because
// eps > 0 (checked by the binding): 0 / (0 + eps).
__device__ __forceinline__ float adam_elem(float w, float& m, float& v, float g, const AdamCoef& k, float gs) {
  float d = g * gs;
  if (k.wd != 0.f) d = fmaf(k.wd, w, d);
  w *= k.decay;
  adam_moments(m, v, d, k);
  return fmaf(-k.step_size, m / adam_denom(v, k), w);
}

__global__ __launch_bounds__(kBlock) void fused_adam_kernel(AdamArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  __shared__ AdamCoef sk;
  if (threadIdx.x == 0) {
    const AdamGroup p = a.groups[c.group];
    sk = adam_coef(p, p.decoupled != 0, a.step, a.lr_mult);
  }
  __syncthreads();
  const AdamCoef k = sk;
  const float gs = a.grad_scale ? *a.grad_scale : 1.f;
  float* w = a.w + c.start;
  float* m = a.m + c.start;
  float* v = a.v + c.start;
  float* g = a.g + c.start;
  uint16_t* shadow = a.w_bf16 ? a.w_bf16 + c.start : nullptr;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    Vec<N> wv = load<N>(w, i), mv = load<N>(m, i), vv = load<N>(v, i);
    const Vec<N> gv = load<N>(g, i);
#pragma unroll
    for (int j = 0; j < N; ++j) wv[j] = adam_elem(wv[j], mv[j], vv[j], gv[j], k, gs);
    store<N>(w, i, wv);
    store<N>(m, i, mv);
    store<N>(v, i, vv);
    if (a.zero_grad) store<N>(g, i, Vec<N>{});
    if (shadow) store_shadow<N>(shadow, i, wv);
  });
}

// ---- LAMB ---------------------------------------------------------------------
// LAMB's coefficients: Adam's with the decay kept out of the gradient (k.wd goes into u).
__device__ __forceinline__ AdamCoef lamb_coef(const LambArgs& a, const Chunk& c) {
  return adam_coef(a.groups[c.group], false, a.step, a.lr_mult);
}

// The update direction from the UPDATED moments; both streaming passes call
// this, so the u whose norm was taken is the u that is applied.  A slot with
// w = m = v = 0 (padding) gives 0 / (0 + eps) + wd * 0 = 0 because eps > 0.
__device__ __forceinline__ float lamb_u(float w, float m, float v, const AdamCoef& k) {
  return fmaf(k.wd, w, (m / k.bc1) / adam_denom(v, k));
}

// Pass 1: m, v updated in place; the chunk's sum of w^2 and of u^2 to part[2 * chunk], part[2 * chunk + 1].
// Each lane adds at most kChunkElems / kBlock = 64 squares in fp32; everything above that is double.
__global__ __launch_bounds__(kBlock) void lamb_moments_kernel(LambArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  __shared__ AdamCoef sk;
  __shared__ double sh[kWavesPerBlock];
  if (threadIdx.x == 0) sk = lamb_coef(a, c);
  __syncthreads();
  const AdamCoef k = sk;
  const float gs = a.grad_scale ? *a.grad_scale : 1.f;
  const float* w = a.w + c.start;
  float* m = a.m + c.start;
  float* v = a.v + c.start;
  const float* g = a.g + c.start;
  float sw = 0.f, su = 0.f;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    const Vec<N> wv = load<N>(w, i), gv = load<N>(g, i);
    Vec<N> mv = load<N>(m, i), vv = load<N>(v, i), u;
#pragma unroll
    for (int j = 0; j < N; ++j) adam_moments(mv[j], vv[j], gv[j] * gs, k);
    store<N>(m, i, mv);
    store<N>(v, i, vv);
#pragma unroll
    for (int j = 0; j < N; ++j) u[j] = lamb_u(wv[j], mv[j], vv[j], k);
    sw += sumsq<N>(wv);
    su += sumsq<N>(u);
  });
  const double bw = block_sum((double)sw, sh);
  const double bu = block_sum((double)su, sh);
  if (threadIdx.x == 0) {
    a.part[2 * (int64_t)blockIdx.x] = bw;
    a.part[2 * (int64_t)blockIdx.x + 1] = bu;
  }
}

// Pass 2: one wave per tensor.  Lane l adds the partials of chunks first + l, first + l + 64, ... in ascending
// order, then the xor butterfly of wave_sum: the order depends on the table alone, never on arrival.
__global__ __launch_bounds__(kBlock) void lamb_trust_kernel(LambArgs a) {
  const int seg = blockIdx.x * kWavesPerBlock + wave_id();
  if (seg >= a.nseg) return;
  const int first = a.seg_range[2 * seg];
  int n = a.seg_range[2 * seg + 1];
  if (first < 0 || first + n > a.nchunks) n = 0;   // a workspace of another table: read nothing outside part
  double sw = 0.0, su = 0.0;
  for (int c = first + lane_id(); c < first + n; c += kWave) {
    sw += a.part[2 * (int64_t)c];
    su += a.part[2 * (int64_t)c + 1];
  }
  sw = wave_sum(sw);
  su = wave_sum(su);
  if (lane_id() != 0) return;
  float trust = 1.f;
  if (n > 0) {
    const LambGroup p = a.groups[a.chunks[first].group];
    const float wn = (float)sqrt(sw), un = (float)sqrt(su);
    if (p.adapt && wn > 0.f && un > 0.f) trust = wn / un;
    if (p.trust_clip > 0.0) trust = fminf(trust, (float)p.trust_clip);
  }
  a.trust[seg] = trust;
}

// Pass 3: w -= (lr * lr_mult * trust[seg]) * u, u recomputed from the updated moments.
__global__ __launch_bounds__(kBlock) void lamb_apply_kernel(LambArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  __shared__ AdamCoef sk;
  __shared__ float s_slr;
  if (threadIdx.x == 0) {
    const AdamCoef k = lamb_coef(a, c);
    const float trust = (c.seg >= 0 && c.seg < a.nseg) ? a.trust[c.seg] : 1.f;
    s_slr = (float)(k.lr * (double)trust);
    sk = k;
  }
  __syncthreads();
  const AdamCoef k = sk;
  const float nslr = -s_slr;
  float* w = a.w + c.start;
  const float* m = a.m + c.start;
  const float* v = a.v + c.start;
  float* g = a.g + c.start;
  uint16_t* shadow = a.w_bf16 ? a.w_bf16 + c.start : nullptr;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    Vec<N> wv = load<N>(w, i);
    const Vec<N> mv = load<N>(m, i), vv = load<N>(v, i);
#pragma unroll
    for (int j = 0; j < N; ++j) wv[j] = fmaf(nslr, lamb_u(wv[j], mv[j], vv[j], k), wv[j]);
    store<N>(w, i, wv);
    if (a.zero_grad) store<N>(g, i, Vec<N>{});
    if (shadow) store_shadow<N>(shadow, i, wv);
  });
}

// DGC momentum correction: u = mu*u + (g + wd*w); g = u (the compressor then
// sparsifies the locally accumulated velocity instead of the raw gradient).
__global__ __launch_bounds__(kBlock) void momentum_correct_kernel(McArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  const float mu = a.momentum[c.group];
  const float wd = a.weight_decay[c.group];
  float* u = a.u + c.start;
  float* g = a.g + c.start;
  const float* w = a.w + c.start;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    Vec<N> uv = load<N>(u, i);
    const Vec<N> gv = load<N>(g, i), wv = load<N>(w, i);
#pragma unroll
    for (int j = 0; j < N; ++j) uv[j] = fmaf(mu, uv[j], fmaf(wd, wv[j], gv[j]));
    store<N>(u, i, uv);
    store<N>(g, i, uv);
  });
}

// Momentum factor masking: u[idx] = 0 for every index this rank sent.
__global__ __launch_bounds__(kBlock) void mask_records_kernel(float* __restrict__ u, const int32_t* __restrict__ rec,
                                                              int64_t k_cap) {
  const int64_t sent = rec[0];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < sent && i < k_cap;
       i += (int64_t)gridDim.x * kBlock)
    u[rec[kRecHdr + i]] = 0.f;
}

__global__ __launch_bounds__(kBlock) void accum_grad_bf16_kernel(float* __restrict__ dst,
                                                                 const uint16_t* __restrict__ src, int64_t n,
                                                                 int vec) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t n8 = vec ? (n >> 3) : 0;
  for (int64_t i = tid; i < n8; i += stride) {
    const uint4 u = reinterpret_cast<const uint4*>(src)[i];
    float4 a = reinterpret_cast<float4*>(dst)[2 * i];
    float4 b = reinterpret_cast<float4*>(dst)[2 * i + 1];
    a.x += __uint_as_float(u.x << 16); a.y += __uint_as_float(u.x & 0xffff0000u);
    a.z += __uint_as_float(u.y << 16); a.w += __uint_as_float(u.y & 0xffff0000u);
    b.x += __uint_as_float(u.z << 16); b.y += __uint_as_float(u.z & 0xffff0000u);
    b.z += __uint_as_float(u.w << 16); b.w += __uint_as_float(u.w & 0xffff0000u);
    reinterpret_cast<float4*>(dst)[2 * i] = a;
    reinterpret_cast<float4*>(dst)[2 * i + 1] = b;
  }
  for (int64_t i = (n8 << 3) + tid; i < n; i += stride) dst[i] += __uint_as_float(((uint32_t)src[i]) << 16);
}

__global__ __launch_bounds__(kBlock) void accum_grad_f32_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                                int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = tid; i < n; i += stride) dst[i] += src[i];
}

__global__ __launch_bounds__(kBlock) void cast_bf16_kernel(uint16_t* __restrict__ dst, const float* __restrict__ src,
                                                           int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = tid; i < n; i += stride) dst[i] = f2bf(src[i]);
}

__global__ __launch_bounds__(kBlock) void segmented_sumsq_kernel(const float* __restrict__ w,
                                                                 const float* __restrict__ g,
                                                                 const Chunk* __restrict__ chunks,
                                                                 double* __restrict__ out) {
  const Chunk c = chunks[blockIdx.x];
  const float* wp = w + c.start;
  const float* gp = g + c.start;
  float sw = 0.f, sg = 0.f;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    sw += sumsq<N>(load<N>(wp, i));
    sg += sumsq<N>(load<N>(gp, i));
  });
  __shared__ double sh[kWavesPerBlock];
  const double bw = block_sum((double)sw, sh);
  const double bg = block_sum((double)sg, sh);
  if (threadIdx.x == 0) {
    atomicAdd(out + 2 * c.seg, bw);
    atomicAdd(out + 2 * c.seg + 1, bg);
  }
}

__device__ __forceinline__ float lars_elem(float w, float& acc, float g, float wd, float mom, float slr) {
  float d = fmaf(wd, w, g);
  d = fminf(fmaxf(d, -10.f), 10.f);
  acc = fmaf(mom, acc, slr * d);
  return w - acc;
}

__global__ __launch_bounds__(kBlock) void fused_lars_kernel(LarsArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  const int gi = c.group;
  const float lr = a.lr[gi], mom = a.momentum[gi], wd = a.weight_decay[gi], eeta = a.eeta[gi], eps = a.epsilon[gi];
  const float wn = (float)sqrt(a.seg_sumsq[2 * c.seg]);
  const float gn = (float)sqrt(a.seg_sumsq[2 * c.seg + 1]);
  float trust = 1.f;
  if (wn > 0.f && gn > 0.f) trust = eeta * wn / (gn + wd * wn + eps);
  trust = fminf(fmaxf(trust, 0.f), 50.f);
  const float slr = lr * trust;
  float* w = a.w + c.start;
  float* m = a.m + c.start;
  const float* g = a.g + c.start;
  for_chunk(c.len, [&](auto width, int i) {
    constexpr int N = decltype(width)::value;
    Vec<N> wv = load<N>(w, i), mv = load<N>(m, i);
    const Vec<N> gv = load<N>(g, i);
#pragma unroll
    for (int j = 0; j < N; ++j) wv[j] = lars_elem(wv[j], mv[j], gv[j], wd, mom, slr);
    store<N>(w, i, wv);
    store<N>(m, i, mv);
  });
}

// ---- global-norm clip -------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sumsq_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
  float s = 0.f;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += stride) s += x[i] * x[i];
  } else {
    for (int64_t i = tid; i < n; i += stride) s += x[i] * x[i];
  }
  __shared__ double sh[kWavesPerBlock];
  const double b = block_sum((double)s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

__global__ __launch_bounds__(kBlock) void clip_coef_kernel(const double* __restrict__ part, int nparts, float max_norm,
                                                           float* __restrict__ coef, float* __restrict__ norm_out) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nparts; b += kBlock) s += part[b];
  __shared__ double sh[kWavesPerBlock];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float nrm = (float)sqrt(s);
    float c = max_norm / (nrm + 1e-6f);
    if (c > 1.f) c = 1.f;
    *coef = c;
    if (norm_out) *norm_out = nrm;
  }
}

__global__ __launch_bounds__(kBlock) void scale_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ coef) {
  const float c = *coef;
  if (c == 1.f) return;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = tid; i < n; i += stride) x[i] *= c;
}

}  // namespace

void fused_sgd(const SgdArgs& a, hipStream_t s) {
  if (a.nchunks <= 0) return;
  hipLaunchKernelGGL(fused_sgd_kernel, dim3(a.nchunks), dim3(kBlock), 0, s, a);
}

void fused_adam(const AdamArgs& a, hipStream_t s) {
  if (a.nchunks <= 0) return;
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, a.step);
  hipLaunchKernelGGL(fused_adam_kernel, dim3(a.nchunks), dim3(kBlock), 0, s, a);
}

void fused_lamb(const LambArgs& a, hipStream_t s) {
  if (a.nchunks <= 0 || a.nseg <= 0) return;
  if (a.passes & 1) {
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, s, a.step);
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(a.nchunks), dim3(kBlock), 0, s, a);
  }
  if (a.passes & 2)
    hipLaunchKernelGGL(lamb_trust_kernel, dim3((a.nseg + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, s,
                       a);
  if (a.passes & 4) hipLaunchKernelGGL(lamb_apply_kernel, dim3(a.nchunks), dim3(kBlock), 0, s, a);
}

void momentum_correct(const McArgs& a, hipStream_t s) {
  if (a.nchunks <= 0) return;
  hipLaunchKernelGGL(momentum_correct_kernel, dim3(a.nchunks), dim3(kBlock), 0, s, a);
}

void mask_records(float* u, const int32_t* record, int64_t k_cap, hipStream_t s) {
  int64_t G = ceil_div(k_cap, (int64_t)kBlock);
  if (G < 1) G = 1;
  if (G > 1024) G = 1024;
  hipLaunchKernelGGL(mask_records_kernel, dim3((int)G), dim3(kBlock), 0, s, u, record, k_cap);
}

void accum_grad(float* dst, const void* src, int64_t n, int src_bytes, hipStream_t s) {
  if (n <= 0) return;
  int64_t G = ceil_div(n, (int64_t)kBlock * 8);
  if (G < 1) G = 1;
  if (G > 2048) G = 2048;
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
  if (src_bytes == 2)  // unaligned pointers: the scalar tail loop covers every element
    hipLaunchKernelGGL(accum_grad_bf16_kernel, dim3((int)G), dim3(kBlock), 0, s, dst, (const uint16_t*)src, n,
                       vec ? 1 : 0);
  else
    hipLaunchKernelGGL(accum_grad_f32_kernel, dim3((int)G), dim3(kBlock), 0, s, dst, (const float*)src, n);
}

void cast_bf16(uint16_t* dst, const float* src, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  int64_t G = ceil_div(n, (int64_t)kBlock * 8);
  if (G < 1) G = 1;
  if (G > 2048) G = 2048;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3((int)G), dim3(kBlock), 0, s, dst, src, n);
}

void segmented_sumsq(const float* w, const float* g, const Chunk* chunks, int nchunks, double* out, hipStream_t s) {
  if (nchunks <= 0) return;
  hipLaunchKernelGGL(segmented_sumsq_kernel, dim3(nchunks), dim3(kBlock), 0, s, w, g, chunks, out);
}

void fused_lars(const LarsArgs& a, hipStream_t s) {
  if (a.nchunks <= 0) return;
  hipLaunchKernelGGL(fused_lars_kernel, dim3(a.nchunks), dim3(kBlock), 0, s, a);
}

void clip_grad_norm(float* g, int64_t n, float max_norm, double* ws, float* coef_out, float* norm_out,
                    hipStream_t s) {
  int G = (int)ceil_div(n, (int64_t)kBlock * 16);
  if (G < 1) G = 1;
  if (G > 1024) G = 1024;
  hipLaunchKernelGGL(sumsq_kernel, dim3(G), dim3(kBlock), 0, s, g, n, ws);
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(kBlock), 0, s, ws, G, max_norm, coef_out, norm_out);
  int Gs = (int)ceil_div(n, (int64_t)kBlock * 8);
  if (Gs < 1) Gs = 1;
  if (Gs > 2048) Gs = 2048;
  hipLaunchKernelGGL(scale_kernel, dim3(Gs), dim3(kBlock), 0, s, g, n, coef_out);
}

}  // namespace gk
