// Compact wire records: 16-bit segment indices and bf16 values (4 bytes per entry).
//
//   hdr[4] | seg_off[nseg + 1] | idx16[k_cap] (two per word) | val16[k_cap] (bf16, two per word)
//
// The arena is cut into segments of 65,536 elements (nseg = ceil(n / 65536)).  The select kernel
// emits ascending indices, so the entries of segment s are the positions [seg_off[s], seg_off[s+1])
// of the record and an index is (s << 16) | idx16; seg_off[nseg] = min(sent, k_cap).
//
//   pack_records16: one launch over the rank's full record {hdr | idx[k_cap] | val[k_cap]}.  A thread
//     takes the two entries of one payload word.  val16 = RNE bf16(val); the rounding residue
//     val - float(val16) is exact in fp32 and goes into the error-feedback slot the select kernel
//     cleared at idx (plain store: indices of one record are unique), and the full record's value is
//     overwritten with the rounded one, so residual + record is still the accumulator.  Segment
//     boundaries come from neighbouring entries: entry j writes j into
//     seg_off[(idx[j-1] >> 16) + 1 .. idx[j] >> 16], the first entry the leading offsets, the last one
//     the trailing ones.
//   reduce_records16<APPLY>: reduce_records_kernel's semantics (scatter.hip: the first rank holding an
//     index owns it and sums the P contributions in rank order, fp32, one scale; no atomics) straight
//     from the P gathered compact records.  A workgroup takes kR16Tile consecutive entries of one rank
//     -- a run spans many segments at the usual densities (a segment holds ~65 entries at 0.001), so the
//     grid does not depend on how the entries fall into segments.  Two searches in the rank's OWN table
//     give the run's segments [s_lo, s_hi]; every other rank's window is then seg_off_q[s_lo] ..
//     seg_off_q[s_hi + 1], two table look-ups.  The tables' slices and the 16-bit windows are staged in
//     LDS; an entry finds its segment in the staged slice of its own table and searches only that
//     segment's few entries of every other rank.  Runs over more than kR16Segs segments, windows over
//     kR16Win entries and ranks from kR16MaxP on read global memory instead.
// Compiled with -ffp-contract=off like scatter.hip (product and sum round separately).
#include "common.h"
#include "gk_kernels.h"

namespace gk {
namespace {

constexpr int kSegShift = 16;                    // 65,536 elements per segment
constexpr int kR16Per = 2;                       // entries per thread
constexpr int kR16Tile = kBlock * kR16Per;       // entries of the owner rank per workgroup
constexpr int kR16Win = 1024;                    // LDS window per other rank (16-bit keys)
constexpr int kR16Segs = 64;                     // segments of a run whose offsets are staged
constexpr int kR16MaxP = 16;                     // ranks staged in LDS; more go through global memory

__device__ __forceinline__ uint16_t f2bf_rne(float f) {   // scatter.hip's rule, NaN kept quiet
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the geometry of one compact record, in int32 words from its start
struct Rec16 {
  int nseg;
  int64_t k_cap, idx_at, val_at, words;
};

__host__ __device__ inline Rec16 rec16_of(int64_t n, int64_t k_cap) {
  Rec16 g;
  g.nseg = (int)((n + (1 << kSegShift) - 1) >> kSegShift);
  if (g.nseg < 1) g.nseg = 1;
  g.k_cap = k_cap;
  g.idx_at = kRecHdr + g.nseg + 1;
  g.val_at = g.idx_at + ((k_cap + 1) >> 1);
  g.words = g.val_at + ((k_cap + 1) >> 1);
  return g;
}

__global__ __launch_bounds__(kBlock) void pack_records16_kernel(int32_t* __restrict__ full, Rec16 g, int64_t n,
                                                                float* __restrict__ resid,
                                                                int32_t* __restrict__ out) {
  int64_t sent = full[0];
  sent = sent < 0 ? 0 : (sent > g.k_cap ? g.k_cap : sent);
  const int32_t* idx = full + kRecHdr;
  float* val = reinterpret_cast<float*>(full + kRecHdr + g.k_cap);
  int32_t* soff = out + kRecHdr;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  if (tid < kRecHdr) out[tid] = full[tid];
  if (sent == 0) {
    for (int64_t s = tid; s <= g.nseg; s += stride) soff[s] = 0;
  }
  const int64_t pairs = (g.k_cap + 1) >> 1;
  for (int64_t p = tid; p < pairs; p += stride) {
    uint32_t iw = 0, vw = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t j = 2 * p + h;
      if (j >= sent) continue;
      const int32_t i = idx[j];
      const float v = val[j];
      const uint16_t b = f2bf_rne(v);
      const float vr = bf2f(b);
      if (i >= 0 && i < n) resid[i] = v - vr;              // exact: v and vr share sign and binade (or vr is one up)
      val[j] = vr;
      iw |= (uint32_t)(i & 0xffff) << (16 * h);
      vw |= (uint32_t)b << (16 * h);
      const int s_cur = clampi(i >> kSegShift, 0, g.nseg - 1);
      const int s_prev = j == 0 ? -1 : clampi(idx[j - 1] >> kSegShift, 0, g.nseg - 1);
      for (int s = s_prev + 1; s <= s_cur; ++s) soff[s] = (int32_t)j;
      if (j == sent - 1)
        for (int s = s_cur + 1; s <= g.nseg; ++s) soff[s] = (int32_t)sent;
    }
    out[g.idx_at + p] = (int32_t)iw;
    out[g.val_at + p] = (int32_t)vw;
  }
}

// largest s in [0, len) with tab[s] <= j (tab ascending, tab[0] <= j)
template <typename T>
__device__ __forceinline__ int seg_of(const T* tab, int len, int j) {
  int lo = 1, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] <= j) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

__device__ __forceinline__ int lower_bound_u16(const uint16_t* a, int lo, int hi, uint32_t key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <bool APPLY>
__global__ __launch_bounds__(kBlock) void reduce_records16_kernel(float* __restrict__ dst, int64_t n,
                                                                  const int32_t* __restrict__ records, int P, Rec16 g,
                                                                  float scale, const float* __restrict__ lr_ptr,
                                                                  float lr, uint16_t* __restrict__ shadow) {
  __shared__ uint32_t win[kR16MaxP][kR16Win / 2];          // 16-bit keys, two per word, from an even position
  __shared__ int32_t soff[kR16MaxP][kR16Segs + 1];         // seg_off_q[s_lo .. s_hi + 1]
  __shared__ int s_wlo[kR16MaxP], s_whi[kR16MaxP];         // record positions of rank q's window
  __shared__ int s_fit[kR16MaxP];                          // ... and whether it is staged in win[q]
  __shared__ int s_seg[2];
  const int r = blockIdx.y;
  const int kc = (int)g.k_cap;
  const int32_t* rec = records + (int64_t)r * g.words;
  const int32_t* so = rec + kRecHdr;
  const int cnt = clampi(so[g.nseg], 0, kc);
  const int t0 = blockIdx.x * kR16Tile;
  if (t0 >= cnt) return;                                   // block-uniform
  const int t1 = t0 + kR16Tile < cnt ? t0 + kR16Tile : cnt;
  // the run's segments, from this rank's own table
  if (threadIdx.x < 2) s_seg[threadIdx.x] = seg_of(so, g.nseg, threadIdx.x == 0 ? t0 : t1 - 1);
  __syncthreads();
  const int s_lo = s_seg[0], s_hi = s_seg[1];
  const int span = s_hi - s_lo + 1;
  const bool tab_lds = span <= kR16Segs;                   // block-uniform
  const int Ps = P < kR16MaxP ? P : kR16MaxP;
  if (threadIdx.x < Ps) {                                  // every rank's window: two table look-ups
    const int q = threadIdx.x;
    const int32_t* sq = records + (int64_t)q * g.words + kRecHdr;
    const int wlo = clampi(sq[s_lo], 0, kc);
    const int whi = clampi(sq[s_hi + 1], wlo, kc);
    s_wlo[q] = wlo;
    s_whi[q] = whi;
    s_fit[q] = q != r && whi - (wlo & ~1) <= kR16Win;
  }
  if (tab_lds) {
    for (int i = threadIdx.x; i < Ps * (span + 1); i += kBlock) {
      const int q = i / (span + 1), s = i - q * (span + 1);
      soff[q][s] = clampi(records[(int64_t)q * g.words + kRecHdr + s_lo + s], 0, kc);
    }
  }
  __syncthreads();
  for (int q = 0; q < Ps; ++q) {
    if (!s_fit[q]) continue;
    const int w0 = s_wlo[q] >> 1, w1 = (s_whi[q] + 1) >> 1;
    const int32_t* src = records + (int64_t)q * g.words + g.idx_at;
    for (int i = w0 + threadIdx.x; i < w1; i += kBlock) win[q][i - w0] = (uint32_t)src[i];
  }
  __syncthreads();
  const float lr_eff = APPLY ? (lr_ptr ? lr * *lr_ptr : lr) : 0.f;
  const uint16_t* idx16 = reinterpret_cast<const uint16_t*>(rec + g.idx_at);
  const uint16_t* val16 = reinterpret_cast<const uint16_t*>(rec + g.val_at);
#pragma unroll
  for (int e = 0; e < kR16Per; ++e) {
    const int j = t0 + e * kBlock + threadIdx.x;
    if (j >= t1) continue;
    // this entry's segment: its own table, staged slice or global
    const int s = (tab_lds && r < kR16MaxP) ? s_lo + seg_of(soff[r], span, j) : s_lo + seg_of(so + s_lo, span, j);
    const uint32_t k16 = idx16[j];
    const int64_t key = ((int64_t)s << kSegShift) | k16;
    bool owner = true;
    float sum = 0.f;
    for (int q = 0; q < P && owner; ++q) {
      float v = 0.f;
      if (q == r) {
        v = bf2f(val16[j]);
      } else {
        const int32_t* rq = records + (int64_t)q * g.words;
        int lo, hi;                                        // segment s of rank q: record positions [lo, hi)
        if (tab_lds && q < kR16MaxP) {
          lo = soff[q][s - s_lo];
          hi = soff[q][s - s_lo + 1];
        } else {
          lo = clampi(rq[kRecHdr + s], 0, kc);
          hi = clampi(rq[kRecHdr + s + 1], 0, kc);
        }
        int pos;
        bool hit;
        if (q < kR16MaxP && s_fit[q] && lo >= s_wlo[q] && hi <= s_whi[q]) {
          const uint16_t* w = reinterpret_cast<const uint16_t*>(win[q]);
          const int base = s_wlo[q] & ~1;
          pos = lower_bound_u16(w, lo - base, hi - base, k16);
          hit = pos < hi - base && w[pos] == k16;
          pos += base;
        } else {
          const uint16_t* iq = reinterpret_cast<const uint16_t*>(rq + g.idx_at);
          pos = lower_bound_u16(iq, lo, hi, k16);
          hit = pos < hi && iq[pos] == k16;
        }
        if (hit) {
          if (q < r) owner = false;                        // an earlier rank owns this index
          else v = bf2f(reinterpret_cast<const uint16_t*>(rq + g.val_at)[pos]);
        }
      }
      sum = sum + v;                                       // rank order: ((0 + v0) + v1) + ...
    }
    if (!owner || key >= n) continue;
    const float avg = sum * scale;
    if (APPLY) {
      const float wn = dst[key] - lr_eff * avg;
      dst[key] = wn;
      if (shadow) shadow[key] = f2bf_rne(wn);
    } else {
      dst[key] = dst[key] + avg;
    }
  }
}

template <bool APPLY>
void launch_reduce16(float* dst, int64_t n, const int32_t* records, int P, int64_t k_cap, float scale,
                     const float* lr_mult, float lr, uint16_t* shadow, hipStream_t s) {
  const Rec16 g = rec16_of(n, k_cap);
  const int gx = (int)ceil_div(k_cap, (int64_t)kR16Tile);
  hipLaunchKernelGGL((reduce_records16_kernel<APPLY>), dim3(gx < 1 ? 1 : gx, P), dim3(kBlock), 0, s, dst, n, records,
                     P, g, scale, lr_mult, lr, shadow);
}

}  // namespace

int64_t record16_words(int64_t n, int64_t k_cap) { return rec16_of(n, k_cap).words; }

void pack_records16(int32_t* full, int64_t k_cap, float* resid, int64_t n, int32_t* out, hipStream_t s) {
  const Rec16 g = rec16_of(n, k_cap);
  int64_t gx = ceil_div((k_cap + 1) >> 1, (int64_t)kBlock);
  if (gx < 1) gx = 1;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(pack_records16_kernel, dim3((int)gx), dim3(kBlock), 0, s, full, g, n, resid, out);
}

void reduce_records16(float* dst, int64_t n, const int32_t* records, int P, int64_t k_cap, float scale,
                      hipStream_t s) {
  launch_reduce16<false>(dst, n, records, P, k_cap, scale, nullptr, 0.f, nullptr, s);
}

void apply_records16_sgd(float* w, uint16_t* w_bf16, int64_t n, const int32_t* records, int P, int64_t k_cap,
                         float scale, float lr, const float* lr_mult, hipStream_t s) {
  launch_reduce16<true>(w, n, records, P, k_cap, scale, lr_mult, lr, w_bf16, s);
}

}  // namespace gk
