// Selection-quality metrics of one compressed bucket, on device.
//
// After compress() the residual r holds the accumulator with the sent entries
// zeroed and the record holds the sent (idx, val) pairs, so
//
//   acc[i] = r[i]  except  acc[idx[j]] = val[j]  (j < sent),   r[idx[j]] == 0.
//
// The metrics compare the record with the exact top-k of acc by abs_key:
// K = the k_eff-th largest key, c_gt = #{key > K}, the record's overlap with
// the top-k, and the energies sum val^2 / sum of the top-k acc^2 / sum acc^2
// (QualityOut in gk_kernels.h).  acc is never materialised: r and the record
// values are streamed separately.  The key histogram of acc is that of r plus
// that of val[0:sent], minus `sent` keys of 0 (the zeroed slots of r).
//
//   hist<0> (grid)  11-bit histogram of key[31:21] over r and val; sum x^2
//   hist<1> (grid)  picks digit d0 from hist 0 (every block, redundantly),
//                   histogram of key[20:10] among keys with prefix d0;
//                   sum x^2 of the keys above d0
//   hist<2> (grid)  picks d1; count AND energy histogram of key[9:0] among
//                   keys with prefix (d0, d1); sum x^2 of prefix d0, above d1
//   final  (1 WG)   picks d2 -> K; c_gt and the energy above K from the
//                   histograms; one scan of the record for overlap and e_sel
//
// Passes are separated by launch boundaries only: no block ever waits on
// another (no grid barrier, no spin, no arrival counter), so nothing here can
// hang beside the backward pass.  The workspace is zeroed by the call itself.
// Energies accumulate in fp64 (per-thread registers, one atomic per block
// spread over kSlots slots); the integer fields are exact.
#include "common.h"
#include "gk_kernels.h"

namespace gk {
namespace {

constexpr int kQTile = kBlock * 16;   // 4 float4 per thread per tile
constexpr int kQMaxBlocks = 1024;
// per-block energy partials land in kSlots accumulators kSlotStride doubles
// apart (different 256-byte lines): 1024 blocks do not queue on one address
constexpr int kSlots = 32, kSlotStride = 32;

struct QWs {
  uint32_t hist0[kRadixBins0];
  uint32_t hist1[kRadixBins1];
  uint32_t hist2[kRadixBins2];
  double ehist2[kRadixBins2];           // sum x^2 per bin of the last pass
  double e_all[kSlots * kSlotStride];   // sum x^2 over everything
  double e_gt[kSlots * kSlotStride];    // sum x^2 of the keys known to be above K after passes 1, 2
};

__device__ __forceinline__ int64_t clamp_sent(const int32_t* __restrict__ rec, int64_t k_cap) {
  int64_t s = rec[0];
  if (s < 0) s = 0;
  return s < k_cap ? s : k_cap;
}

// Exclusive scan of a u64 over the 256 threads of the block, in thread order.
__device__ __forceinline__ uint64_t q_block_excl_scan(uint64_t v, uint64_t* sh /*kWavesPerBlock*/) {
  uint64_t inc = v;
  const int l = lane_id();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = __shfl_up(inc, off, 64);
    if (l >= off) inc += o;
  }
  __syncthreads();
  if (l == 63) sh[wave_id()] = inc;
  __syncthreads();
  uint64_t before = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w)
    if (w < wave_id()) before += sh[w];
  return before + inc - v;
}

// The digit holding the kr-th largest key (1-based) of a histogram of NB bins,
// with `zeros` keys taken out of bin 0 (the zeroed slots of r).  Broadcast to
// every thread; *kr_out is the rank inside the digit's bin, so kr - *kr_out
// keys lie in the bins above it.  Thread t owns the NB/256 bins below
// NB - t * NB/256, highest first.
template <int NB>
__device__ int q_find(const uint32_t* __restrict__ hist, uint32_t zeros, int64_t kr, uint64_t* sh, int64_t* kr_out) {
  constexpr int PER = NB / kBlock;
  static_assert(NB % kBlock == 0 && PER >= 1 && PER <= 8, "bins per thread");
  __shared__ int s_digit;
  __shared__ int64_t s_kr;
  const int hi = NB - (int)threadIdx.x * PER;
  uint32_t hv[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) hv[q] = hist[hi - 1 - q];
  if (hi == PER) hv[PER - 1] = hv[PER - 1] > zeros ? hv[PER - 1] - zeros : 0u;   // bin 0
  uint64_t ls = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) ls += hv[q];
  const uint64_t before = q_block_excl_scan(ls, sh);
  if (threadIdx.x == 0) { s_digit = 0; s_kr = 1; }
  __syncthreads();
  if ((int64_t)before < kr && kr <= (int64_t)(before + ls)) {   // at most one thread
    int64_t cum = (int64_t)before;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int64_t h = hv[q];
      if (cum + h >= kr) { s_digit = hi - 1 - q; s_kr = kr - cum; break; }
      cum += h;
    }
  }
  __syncthreads();
  const int d = s_digit;
  *kr_out = s_kr;
  __syncthreads();
  return d;
}

struct QPick {
  uint32_t d0, d1;
};

// One element of acc (from r or from the record) in pass PASS.
template <int PASS>
__device__ __forceinline__ void q_visit(float x, const QPick& p, uint32_t* __restrict__ my, double* __restrict__ eh,
                                        double& e) {
  const uint32_t key = abs_key(x);
  const double xx = (double)x * (double)x;
  if (PASS == 0) {
    atomicAdd(&my[key >> 21], 1u);
    e += xx;
  } else if (PASS == 1) {
    const uint32_t a = key >> 21;
    if (a > p.d0) e += xx;
    else if (a == p.d0) atomicAdd(&my[(key >> 10) & 0x7ffu], 1u);
  } else {
    if ((key >> 21) == p.d0) {
      const uint32_t b = (key >> 10) & 0x7ffu;
      if (b > p.d1) {
        e += xx;
      } else if (b == p.d1) {
        atomicAdd(&my[key & 0x3ffu], 1u);
        if (x != 0.f) atomicAdd(&eh[key & 0x3ffu], xx);
      }
    }
  }
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void quality_hist_kernel(const float* __restrict__ r, int64_t n,
                                                              const int32_t* __restrict__ rec, int64_t k,
                                                              int64_t k_cap, QWs* __restrict__ ws) {
  constexpr int NB = PASS == 0 ? kRadixBins0 : (PASS == 1 ? kRadixBins1 : kRadixBins2);
  __shared__ uint32_t sh_hist[kWavesPerBlock * NB];   // one copy per wave
  __shared__ double sh_eh[PASS == 2 ? kRadixBins2 : 1];
  __shared__ uint64_t sh_scan[kWavesPerBlock];
  __shared__ double sh_red[kWavesPerBlock];
  const int64_t sent = clamp_sent(rec, k_cap);
  QPick p = {0u, 0u};
  if (PASS >= 1) {
    // the bin picked from the passes before this launch, redundantly per block
    const int64_t keff = k < n ? k : n;
    int64_t kr1, kr2;
    p.d0 = (uint32_t)q_find<kRadixBins0>(ws->hist0, (uint32_t)sent, keff, sh_scan, &kr1);
    if (PASS == 2) p.d1 = (uint32_t)q_find<kRadixBins1>(ws->hist1, p.d0 == 0u ? (uint32_t)sent : 0u, kr1, sh_scan, &kr2);
  }
  for (int i = threadIdx.x; i < kWavesPerBlock * NB; i += kBlock) sh_hist[i] = 0u;
  if (PASS == 2)
    for (int i = threadIdx.x; i < kRadixBins2; i += kBlock) sh_eh[i] = 0.0;
  __syncthreads();
  uint32_t* my = sh_hist + wave_id() * NB;
  double e = 0.0;

  // r: float4 body between a scalar head (up to 16-byte alignment) and tail
  int64_t head = (int64_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(r) & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const int64_t nbody = (n - head) & ~(int64_t)3;
  const float* body = r + head;
  const int64_t ntiles = ceil_div(nbody, (int64_t)kQTile);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t base = t * kQTile + (int64_t)threadIdx.x * 4;
    float4 v[4];
    if (base + 3 * kBlock * 4 + 4 <= nbody) {   // whole tile in range for this thread: all loads in flight
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4*>(body + base + q * kBlock * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        q_visit<PASS>(v[q].x, p, my, sh_eh, e);
        q_visit<PASS>(v[q].y, p, my, sh_eh, e);
        q_visit<PASS>(v[q].z, p, my, sh_eh, e);
        q_visit<PASS>(v[q].w, p, my, sh_eh, e);
      }
    } else {                                    // ragged last tile
      for (int q = 0; q < 4; ++q) {
        const int64_t o = base + q * kBlock * 4;
        if (o + 4 <= nbody) {
          const float4 f = *reinterpret_cast<const float4*>(body + o);
          q_visit<PASS>(f.x, p, my, sh_eh, e);
          q_visit<PASS>(f.y, p, my, sh_eh, e);
          q_visit<PASS>(f.z, p, my, sh_eh, e);
          q_visit<PASS>(f.w, p, my, sh_eh, e);
        }
      }
    }
  }
  if (blockIdx.x == 0) {
    // head and tail elements (at most 3 + 3), one thread each
    const int64_t ntail = n - head - nbody;
    if ((int64_t)threadIdx.x < head) q_visit<PASS>(r[threadIdx.x], p, my, sh_eh, e);
    else if ((int64_t)threadIdx.x - head < ntail) q_visit<PASS>(r[nbody + threadIdx.x], p, my, sh_eh, e);
  }
  // the record's values: every entry once, grid-strided over the blocks
  const float* val = reinterpret_cast<const float*>(rec + kRecHdr + k_cap);
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < sent; j += (int64_t)gridDim.x * kBlock)
    q_visit<PASS>(val[j], p, my, sh_eh, e);
  __syncthreads();

  uint32_t* out = PASS == 0 ? ws->hist0 : (PASS == 1 ? ws->hist1 : ws->hist2);
  for (int b = threadIdx.x; b < NB; b += kBlock) {
    const uint32_t c = sh_hist[b] + sh_hist[NB + b] + sh_hist[2 * NB + b] + sh_hist[3 * NB + b];
    if (c) atomicAdd(&out[b], c);
    if (PASS == 2) {
      const double eb = sh_eh[b];
      if (eb != 0.0) atomicAdd(&ws->ehist2[b], eb);
    }
  }
  const double eblk = block_sum(e, sh_red);
  if (threadIdx.x == 0 && eblk != 0.0)
    atomicAdd((PASS == 0 ? ws->e_all : ws->e_gt) + (blockIdx.x % kSlots) * kSlotStride, eblk);
}

__global__ __launch_bounds__(kBlock) void quality_final_kernel(int64_t n, const int32_t* __restrict__ rec, int64_t k,
                                                               int64_t k_cap, const QWs* __restrict__ ws,
                                                               double* __restrict__ outp) {
  __shared__ uint64_t sh_scan[kWavesPerBlock];
  __shared__ double sh_red[kWavesPerBlock];
  const int64_t sent = clamp_sent(rec, k_cap);
  const int64_t keff = k < n ? k : n;
  int64_t kr1, kr2, kr3;
  const uint32_t d0 = (uint32_t)q_find<kRadixBins0>(ws->hist0, (uint32_t)sent, keff, sh_scan, &kr1);
  const uint32_t d1 = (uint32_t)q_find<kRadixBins1>(ws->hist1, d0 == 0u ? (uint32_t)sent : 0u, kr1, sh_scan, &kr2);
  const uint32_t d2 =
      (uint32_t)q_find<kRadixBins2>(ws->hist2, (d0 | d1) == 0u ? (uint32_t)sent : 0u, kr2, sh_scan, &kr3);
  const uint32_t K = (d0 << 21) | (d1 << 10) | d2;
  // kr3 of the k_eff largest keys equal K; the rest are above it
  const int64_t c_gt = keff - kr3;

  double e = 0.0;
  for (int b = threadIdx.x; b < kRadixBins2; b += kBlock)
    if ((uint32_t)b > d2) e += ws->ehist2[b];
  if (threadIdx.x < kSlots) e += ws->e_gt[threadIdx.x * kSlotStride];
  const double e_gt = block_sum(e, sh_red);
  const double e_all = block_sum(threadIdx.x < kSlots ? ws->e_all[threadIdx.x * kSlotStride] : 0.0, sh_red);

  const float* val = reinterpret_cast<const float*>(rec + kRecHdr + k_cap);
  double es = 0.0;
  uint64_t cnt = 0;   // low half: #key > K, high half: #key == K  (both <= k_cap < 2^31)
  for (int64_t j = threadIdx.x; j < sent; j += kBlock) {
    const float x = val[j];
    const uint32_t key = abs_key(x);
    es += (double)x * (double)x;
    cnt += key > K ? 1ull : (key == K ? (1ull << 32) : 0ull);
  }
  const double e_sel = block_sum(es, sh_red);
  cnt = wave_sum(cnt);
  __syncthreads();
  if (lane_id() == 0) sh_scan[wave_id()] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t c = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) c += sh_scan[w];
    const int64_t rec_gt = (int64_t)(c & 0xffffffffull), rec_eq = (int64_t)(c >> 32);
    const int64_t slots = keff - c_gt;
    const double fK = (double)__uint_as_float(K);
    outp[kQualK] = (double)K;
    outp[kQualCgt] = (double)c_gt;
    outp[kQualOverlap] = (double)(rec_gt + (rec_eq < slots ? rec_eq : slots));
    outp[kQualEsel] = e_sel;
    outp[kQualEtop] = e_gt + (double)slots * fK * fK;
    outp[kQualEall] = e_all;
    outp[kQualSent] = (double)sent;
    outp[kQualKeff] = (double)keff;
  }
}

}  // namespace

size_t quality_workspace_bytes() { return (sizeof(QWs) + 255) / 256 * 256; }

void selection_quality(const float* r, int64_t n, const int32_t* record, int64_t k, int64_t k_cap, double* out,
                       void* ws, hipStream_t s) {
  QWs* w = reinterpret_cast<QWs*>(ws);
  int64_t G = ceil_div(n, (int64_t)kQTile);
  if (G < 1) G = 1;
  if (G > kQMaxBlocks) G = kQMaxBlocks;
  (void)hipMemsetAsync(ws, 0, sizeof(QWs), s);
  hipLaunchKernelGGL(quality_hist_kernel<0>, dim3((int)G), dim3(kBlock), 0, s, r, n, record, k, k_cap, w);
  hipLaunchKernelGGL(quality_hist_kernel<1>, dim3((int)G), dim3(kBlock), 0, s, r, n, record, k, k_cap, w);
  hipLaunchKernelGGL(quality_hist_kernel<2>, dim3((int)G), dim3(kBlock), 0, s, r, n, record, k, k_cap, w);
  hipLaunchKernelGGL(quality_final_kernel, dim3(1), dim3(kBlock), 0, s, n, record, k, k_cap, w, out);
}

}  // namespace gk
