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
// 16-byte loads.
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
  const bool use_m = p.momentum != 0.f;
  const int n4 = c.len >> 2;
  float4* w4 = reinterpret_cast<float4*>(w);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    float4 wv = w4[i];
    const float4 gv = g4[i];
    float4 mv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (use_m && !p.first_step) mv = m4[i];
    wv.x = sgd_elem(wv.x, mv.x, gv.x, p, gs);
    wv.y = sgd_elem(wv.y, mv.y, gv.y, p, gs);
    wv.z = sgd_elem(wv.z, mv.z, gv.z, p, gs);
    wv.w = sgd_elem(wv.w, mv.w, gv.w, p, gs);
    w4[i] = wv;
    if (use_m) m4[i] = mv;
    if (a.zero_grad) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.w_bf16) {
      const uint32_t lo = (uint32_t)f2bf(wv.x) | ((uint32_t)f2bf(wv.y) << 16);
      const uint32_t hi = (uint32_t)f2bf(wv.z) | ((uint32_t)f2bf(wv.w) << 16);
      reinterpret_cast<uint2*>(a.w_bf16 + c.start)[i] = make_uint2(lo, hi);
    }
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    float mv = (use_m && !p.first_step) ? m[i] : 0.f;
    w[i] = sgd_elem(w[i], mv, g[i], p, gs);
    if (use_m) m[i] = mv;
    if (a.zero_grad) g[i] = 0.f;
    if (a.w_bf16) a.w_bf16[c.start + i] = f2bf(w[i]);
  }
}

// ---- Adam / AdamW -------------------------------------------------------------
// Per-workgroup constants of one chunk's param group at the current step.
struct AdamCoef {
  float omb1, beta2, omb2;   // 1 - beta1, beta2, 1 - beta2
  float decay;               // AdamW: 1 - lr * wd (1 when coupled)
  float wd;                  // Adam: wd added to the gradient (0 when decoupled)
  float step_size;           // lr / (1 - beta1^t)
  float bc2_sqrt;            // sqrt(1 - beta2^t)
  float eps;
};

__global__ void adam_tick_kernel(float* __restrict__ step) { *step += 1.f; }

// torch's single-tensor order of operations; sqrtf and '/' are the correctly
// rounded ones (with eps = 1e-8 and the tiny v of a sparsified gradient the
// approximate rcp / rsq are visible).  A slot with w = g = m = v = 0 (padding)
// stays exactly 0 because eps > 0 (checked by the binding): 0 / (0 + eps).
__device__ __forceinline__ float adam_elem(float w, float& m, float& v, float g, const AdamCoef& k, float gs) {
  float d = g * gs;
  if (k.wd != 0.f) d = fmaf(k.wd, w, d);
  w *= k.decay;
  m = fmaf(k.omb1, d - m, m);
  v = fmaf(k.omb2 * d, d, k.beta2 * v);
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  return fmaf(-k.step_size, m / denom, w);
}

__global__ __launch_bounds__(kBlock) void fused_adam_kernel(AdamArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  // bias corrections from the device step count, in double, once per workgroup
  // (a per-element pow would make this streaming pass compute-bound)
  __shared__ AdamCoef sk;
  if (threadIdx.x == 0) {
    const AdamGroup p = a.groups[c.group];
    const double t = (double)*a.step;
    double lr = p.lr;
    if (a.lr_mult) lr *= (double)*a.lr_mult;   // lr schedule of a captured graph; scales the decoupled decay too
    const double bc1 = 1.0 - pow(p.beta1, t);
    const double bc2 = 1.0 - pow(p.beta2, t);
    AdamCoef k;
    k.omb1 = (float)(1.0 - p.beta1);
    k.beta2 = (float)p.beta2;
    k.omb2 = (float)(1.0 - p.beta2);
    k.decay = p.decoupled ? (float)(1.0 - lr * p.weight_decay) : 1.f;
    k.wd = p.decoupled ? 0.f : (float)p.weight_decay;
    k.step_size = (float)(lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = (float)p.eps;
    sk = k;
  }
  __syncthreads();
  const AdamCoef k = sk;
  const float gs = a.grad_scale ? *a.grad_scale : 1.f;
  float* w = a.w + c.start;
  float* m = a.m + c.start;
  float* v = a.v + c.start;
  float* g = a.g + c.start;
  const int n4 = c.len >> 2;
  float4* w4 = reinterpret_cast<float4*>(w);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  float4* g4 = reinterpret_cast<float4*>(g);
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    float4 wv = w4[i];
    float4 mv = m4[i];
    float4 vv = v4[i];
    const float4 gv = g4[i];
    wv.x = adam_elem(wv.x, mv.x, vv.x, gv.x, k, gs);
    wv.y = adam_elem(wv.y, mv.y, vv.y, gv.y, k, gs);
    wv.z = adam_elem(wv.z, mv.z, vv.z, gv.z, k, gs);
    wv.w = adam_elem(wv.w, mv.w, vv.w, gv.w, k, gs);
    w4[i] = wv;
    m4[i] = mv;
    v4[i] = vv;
    if (a.zero_grad) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.w_bf16) {
      const uint32_t lo = (uint32_t)f2bf(wv.x) | ((uint32_t)f2bf(wv.y) << 16);
      const uint32_t hi = (uint32_t)f2bf(wv.z) | ((uint32_t)f2bf(wv.w) << 16);
      reinterpret_cast<uint2*>(a.w_bf16 + c.start)[i] = make_uint2(lo, hi);
    }
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    float mv = m[i], vv = v[i];
    const float wn = adam_elem(w[i], mv, vv, g[i], k, gs);
    w[i] = wn;
    m[i] = mv;
    v[i] = vv;
    if (a.zero_grad) g[i] = 0.f;
    if (a.w_bf16) a.w_bf16[c.start + i] = f2bf(wn);
  }
}

// ---- LAMB ---------------------------------------------------------------------
// Per-workgroup constants of one chunk's param group at the current step.
struct LambCoef {
  float omb1, beta2, omb2;   // 1 - beta1, beta2, 1 - beta2
  float bc1;                 // 1 - beta1^t
  float bc2_sqrt;            // sqrt(1 - beta2^t)
  float eps, wd;
};

// thread 0 of the workgroup; bias corrections in double from the device step count, as fused_adam_kernel
__device__ __forceinline__ LambCoef lamb_coef(const LambGroup& p, const float* step) {
  const double t = (double)*step;
  LambCoef k;
  k.omb1 = (float)(1.0 - p.beta1);
  k.beta2 = (float)p.beta2;
  k.omb2 = (float)(1.0 - p.beta2);
  k.bc1 = (float)(1.0 - pow(p.beta1, t));
  k.bc2_sqrt = (float)sqrt(1.0 - pow(p.beta2, t));
  k.eps = (float)p.eps;
  k.wd = (float)p.weight_decay;
  return k;
}

// The moment update of adam_elem (same forms).
__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, const LambCoef& k, float gs) {
  const float d = g * gs;
  m = fmaf(k.omb1, d - m, m);
  v = fmaf(k.omb2 * d, d, k.beta2 * v);
}

// The update direction from the UPDATED moments; both streaming passes call
// this, so the u whose norm was taken is the u that is applied.  IEEE sqrt and
// divisions for the reason given at adam_elem; a slot with w = m = v = 0
// (padding) gives 0 / (0 + eps) + wd * 0 = 0 because eps > 0.
__device__ __forceinline__ float lamb_u(float w, float m, float v, const LambCoef& k) {
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  return fmaf(k.wd, w, (m / k.bc1) / denom);
}

// Pass 1: m, v updated in place; the chunk's sum of w^2 and of u^2 to part[2 * chunk], part[2 * chunk + 1].
// Each lane adds at most kChunkElems / kBlock = 64 squares in fp32; everything above that is double.
__global__ __launch_bounds__(kBlock) void lamb_moments_kernel(LambArgs a) {
  const Chunk c = a.chunks[blockIdx.x];
  __shared__ LambCoef sk;
  __shared__ double sh[kWavesPerBlock];
  if (threadIdx.x == 0) sk = lamb_coef(a.groups[c.group], a.step);
  __syncthreads();
  const LambCoef k = sk;
  const float gs = a.grad_scale ? *a.grad_scale : 1.f;
  const float* w = a.w + c.start;
  float* m = a.m + c.start;
  float* v = a.v + c.start;
  const float* g = a.g + c.start;
  const int n4 = c.len >> 2;
  const float4* w4 = reinterpret_cast<const float4*>(w);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float sw = 0.f, su = 0.f;
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    const float4 wv = w4[i];
    float4 mv = m4[i];
    float4 vv = v4[i];
    const float4 gv = g4[i];
    lamb_moments(mv.x, vv.x, gv.x, k, gs);
    lamb_moments(mv.y, vv.y, gv.y, k, gs);
    lamb_moments(mv.z, vv.z, gv.z, k, gs);
    lamb_moments(mv.w, vv.w, gv.w, k, gs);
    m4[i] = mv;
    v4[i] = vv;
    const float ux = lamb_u(wv.x, mv.x, vv.x, k), uy = lamb_u(wv.y, mv.y, vv.y, k);
    const float uz = lamb_u(wv.z, mv.z, vv.z, k), uw = lamb_u(wv.w, mv.w, vv.w, k);
    sw += (wv.x * wv.x + wv.y * wv.y) + (wv.z * wv.z + wv.w * wv.w);
    su += (ux * ux + uy * uy) + (uz * uz + uw * uw);
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    float mv = m[i], vv = v[i];
    const float wv = w[i];
    lamb_moments(mv, vv, g[i], k, gs);
    m[i] = mv;
    v[i] = vv;
    const float u = lamb_u(wv, mv, vv, k);
    sw += wv * wv;
    su += u * u;
  }
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
  __shared__ LambCoef sk;
  __shared__ float s_slr;
  if (threadIdx.x == 0) {
    const LambGroup p = a.groups[c.group];
    sk = lamb_coef(p, a.step);
    double lr = p.lr;
    if (a.lr_mult) lr *= (double)*a.lr_mult;   // lr schedule of a captured graph
    const float trust = (c.seg >= 0 && c.seg < a.nseg) ? a.trust[c.seg] : 1.f;
    s_slr = (float)(lr * (double)trust);
  }
  __syncthreads();
  const LambCoef k = sk;
  const float nslr = -s_slr;
  float* w = a.w + c.start;
  const float* m = a.m + c.start;
  const float* v = a.v + c.start;
  float* g = a.g + c.start;
  const int n4 = c.len >> 2;
  float4* w4 = reinterpret_cast<float4*>(w);
  const float4* m4 = reinterpret_cast<const float4*>(m);
  const float4* v4 = reinterpret_cast<const float4*>(v);
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    float4 wv = w4[i];
    const float4 mv = m4[i];
    const float4 vv = v4[i];
    wv.x = fmaf(nslr, lamb_u(wv.x, mv.x, vv.x, k), wv.x);
    wv.y = fmaf(nslr, lamb_u(wv.y, mv.y, vv.y, k), wv.y);
    wv.z = fmaf(nslr, lamb_u(wv.z, mv.z, vv.z, k), wv.z);
    wv.w = fmaf(nslr, lamb_u(wv.w, mv.w, vv.w, k), wv.w);
    w4[i] = wv;
    if (a.zero_grad) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.w_bf16) {
      const uint32_t lo = (uint32_t)f2bf(wv.x) | ((uint32_t)f2bf(wv.y) << 16);
      const uint32_t hi = (uint32_t)f2bf(wv.z) | ((uint32_t)f2bf(wv.w) << 16);
      reinterpret_cast<uint2*>(a.w_bf16 + c.start)[i] = make_uint2(lo, hi);
    }
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    const float wn = fmaf(nslr, lamb_u(w[i], m[i], v[i], k), w[i]);
    w[i] = wn;
    if (a.zero_grad) g[i] = 0.f;
    if (a.w_bf16) a.w_bf16[c.start + i] = f2bf(wn);
  }
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
  const int n4 = c.len >> 2;
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    float4 uv = reinterpret_cast<float4*>(u)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    const float4 wv = reinterpret_cast<const float4*>(w)[i];
    uv.x = fmaf(mu, uv.x, fmaf(wd, wv.x, gv.x));
    uv.y = fmaf(mu, uv.y, fmaf(wd, wv.y, gv.y));
    uv.z = fmaf(mu, uv.z, fmaf(wd, wv.z, gv.z));
    uv.w = fmaf(mu, uv.w, fmaf(wd, wv.w, gv.w));
    reinterpret_cast<float4*>(u)[i] = uv;
    reinterpret_cast<float4*>(g)[i] = uv;
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    const float uv = fmaf(mu, u[i], fmaf(wd, w[i], g[i]));
    u[i] = uv;
    g[i] = uv;
  }
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
  const int n4 = c.len >> 2;
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    const float4 a = reinterpret_cast<const float4*>(wp)[i];
    const float4 b = reinterpret_cast<const float4*>(gp)[i];
    sw += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
    sg += (b.x * b.x + b.y * b.y) + (b.z * b.z + b.w * b.w);
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    sw += wp[i] * wp[i];
    sg += gp[i] * gp[i];
  }
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
  const int n4 = c.len >> 2;
  for (int i = threadIdx.x; i < n4; i += kBlock) {
    float4 wv = reinterpret_cast<float4*>(w)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    wv.x = lars_elem(wv.x, mv.x, gv.x, wd, mom, slr);
    wv.y = lars_elem(wv.y, mv.y, gv.y, wd, mom, slr);
    wv.z = lars_elem(wv.z, mv.z, gv.z, wd, mom, slr);
    wv.w = lars_elem(wv.w, mv.w, gv.w, wd, mom, slr);
    reinterpret_cast<float4*>(w)[i] = wv;
    reinterpret_cast<float4*>(m)[i] = mv;
  }
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += kBlock) {
    float mv = m[i];
    w[i] = lars_elem(w[i], mv, g[i], wd, mom, slr);
    m[i] = mv;
  }
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
