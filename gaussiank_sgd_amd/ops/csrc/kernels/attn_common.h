// What the bf16 and the fp32 fused attention kernels (attn.hip, attn_f32.hip)
// share: the argument struct, the block mapping, the key-padding and causal
// mask policy, the forward's online softmax with its lazy running max, the
// dropout pair hash, the dQ kernel's dS step and the host dispatch.  The two
// files keep what differs: LDS layout, staging, operand reads, MFMA sequences
// and stores.  Every device helper here works on f32x4 accumulators in the
// layout both precisions' MFMAs produce (lane = 16 g + li holds D[4g + r][li])
// and never on operand fragments.
//
// Key-padding mask (MASK instantiations).  key_bits: uint32 [B, T / 32]; bit j
// of word w of a sequence is key 32 w + j, set = valid.  A 64-key tile is two
// words, the 128 keys of a dK/dV workgroup four; both are read through a
// workgroup-uniform address.  Masked keys get the score -inf, so P is exactly
// 0, lse runs over the valid keys, and dK / dV of masked keys are written as
// zeros.  The forward and the dQ kernel skip the arithmetic of key tiles
// without a valid key and stop at the last tile that has one; the dK/dV kernel
// returns early for 128 masked keys.  Every skip is uniform over the workgroup
// (or, inside the dK/dV loop, leaves the wave on its barriers and staging
// duty).  The masked bf16 forward can also store what the bf16 rounding of the
// output dropped (out_lo), which the dQ kernel adds back for delta =
// rowsum(dO * O): rows with few valid keys have concentrated P, where dP and
// delta nearly cancel.  The MASK = false instantiations are the code without
// any of this.
//
// Causal mask (CAUSAL instantiations): query q sees key k iff k <= q, ANDed
// with the key bits under MASK.  The forward and the dQ kernel stop at tile
// 2 qb + 2 (the last one their query 128 qb + 127 sees); per wave a tile is
// fully visible (no mask work), diagonal (masked element-wise through the
// accumulator init) or past the wave's last query (waves 0 and 1 on the
// workgroup's last tile: arithmetic skipped, barrier and staging kept).  The
// dK/dV kernel starts its query tiles at 2 kb; waves 2 and 3 skip the
// arithmetic of that tile.  Every case is wave-uniform.  The forward's lazy
// running max is then kept per row: a row below the threshold does not move
// its m when another row of the wave does, so nothing a later query sees
// changes an earlier row's bits, and under MASK a row whose scores have all
// been -inf so far (left padding) waits for its first finite one; a query
// without any visible valid key gives out = 0, lse = 0 and zero dQ.  out_lo is
// kept as under MASK: the first rows of a sequence see few keys.
// The CAUSAL = false instantiations are the code without any of this.
//
// Lazy running max (forward): only when some row's tile max exceeds the
// current m by kLazy (log2 units, so p <= 256) does the wave take the textbook
// update (cross-lane row max, O and l rescale).  The first tile always takes
// it, so m starts at the first tile's row max.
//
// Dropout: keep(query, key) = half (key & 1) of pair_hash(seed, (bh*T + q)*T/2
// + key/2) >= round(p * 65536), in all kernels of both precisions and in
// attn_dropout_mask (for tests); the mask is regenerated, never stored.
#pragma once
#include <type_traits>

#include "common.h"
#include "mfma_util.h"

namespace gk {

// the geometry both precisions share (the mask words and the tile cases below assume it)
constexpr int kHD = 64;          // head dim
constexpr int kKT = 64;          // rows per LDS tile (keys, or queries in the dK/dV kernels): two mask words
constexpr int kRows = 128;       // rows per workgroup: 4 waves x 32
constexpr float kLazy = 8.f;     // forward: rescale when a row max grows by more than this (log2)

// E: the element type of qkv / out / dout / dqkv (uint16_t = bf16 bits, or float)
template <typename E>
struct AttnArgsT {
  const E* qkv;
  const E* out;
  const E* dout;
  E* o;               // forward output
  E* dqkv;
  float* lse;
  float* delta;
  int T, H;
  float sc;           // log2(e) / sqrt(64)
  float qscale;       // 1 / sqrt(64)
  float dscale;       // 1 / (1 - p_effective)
  uint32_t thr;       // drop threshold on 16 hash bits
  uint32_t seed;
  const uint32_t* key_bits;   // optional [B, T / 32] valid-key bits, MASK kernels only
  // optional, bf16 MASK / CAUSAL kernels only (null for fp32): what the bf16 rounding of the output dropped,
  // out_lo = bf16(O - out) [B, T, H, 64], written by the forward and added back by the dQ kernel for delta
  E* out_lo;
  // optional replay word (graph capture): the effective seed mixes it in, so
  // a replayed step draws a fresh mask while forward and backward of one
  // replay read the same word
  const uint32_t* seed_dev;
};

template <typename E>
__device__ __forceinline__ uint32_t eff_seed(const AttnArgsT<E>& a) {
  if (a.seed_dev == nullptr) return a.seed;
  return hash_u32(__builtin_amdgcn_readfirstlane(*a.seed_dev), a.seed);
}

template <typename E>
AttnArgsT<E> make_args(int T, int H, float p, uint32_t seed, const uint32_t* seed_dev) {
  AttnArgsT<E> a{};
  a.seed_dev = seed_dev;
  a.T = T;
  a.H = H;
  a.qscale = 0.125f;                       // 1 / sqrt(64)
  a.sc = 1.4426950408889634f * 0.125f;     // log2(e) / sqrt(64)
  uint32_t thr = p > 0.f ? (uint32_t)lrintf(p * 65536.f) : 0u;
  if (thr > 65535u) thr = 65535u;
  a.thr = thr;
  a.dscale = thr ? 65536.f / (float)(65536u - thr) : 1.f;
  a.seed = seed;
  return a;
}

// (thr != 0, key_bits != nullptr, causal) -> f(DROP, MASK, CAUSAL) with std::bool_constant arguments
template <typename F>
void attn_dispatch(bool drop, bool mask, bool causal, F&& f) {
  auto with_causal = [&](auto d, auto m) {
    if (causal) f(d, m, std::true_type{});
    else f(d, m, std::false_type{});
  };
  auto with_mask = [&](auto d) {
    if (mask) with_causal(d, std::true_type{});
    else with_causal(d, std::false_type{});
  };
  if (drop) with_mask(std::true_type{});
  else with_mask(std::false_type{});
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ f32x4 splat4(float v) { return f32x4{v, v, v, v}; }

// dropout uniforms of keys (2j, 2j + 1) of one (bh, query): 16 bits each
__device__ __forceinline__ uint32_t pair_hash(uint32_t seed, uint32_t pidx) { return hash_u32(pidx, seed); }

// Workgroups are dispatched round-robin over the 8 XCDs (each with its own
// L2): give every XCD a contiguous range of logical blocks, so the row blocks
// of one (batch, head) -- which all stream the same K / V (or Q / dO) -- run
// on one XCD and share its L2 instead of fetching them once per XCD.
__device__ __forceinline__ int xcd_block() {
  const int n = gridDim.x, b = blockIdx.x;
  if (n % 8) return b;
  return (b & 7) * (n >> 3) + (b >> 3);
}

// CAUSAL block order.  Row block r of a (batch, head) costs 2 r + 2 key tiles in the forward and dQ kernels
// and (T / 64 - 2 r) query tiles in the dK/dV kernel, and workgroups start in block order: with the row
// blocks of a (batch, head) adjacent, every round of resident workgroups lasts as long as its heaviest
// member, and the pass takes nearly the dense time (0.87 of it measured where the tile count says 0.625).
// So each XCD's share of the grid -- whole (batch, head)s, as xcd_block() arranges, so that their K / V (or
// Q / dO) stay in one L2 -- is handed out by cost instead: slot k = 0 first, for all of the XCD's (batch,
// head)s, then k = 1, ...  The caller maps k to its heaviest-first row block.  nrb: row blocks per (batch,
// head).  A grid that does not split into whole (batch, head)s per XCD is ordered as one range.
__device__ __forceinline__ void causal_block(int nrb, int& bh, int& k) {
  const int n = gridDim.x, b = blockIdx.x;
  int x = 0, j = b, nbx = n / nrb;
  if (n % 8 == 0 && (n >> 3) % nrb == 0) {
    x = b & 7;
    j = b >> 3;
    nbx = (n >> 3) / nrb;
  }
  k = j / nbx;
  bh = x * nbx + (j - k * nbx);
}

// this workgroup's (batch, head) and row block.  CAUSAL hands the heaviest row blocks out first:
// HEAVIEST_LAST says that those are the last ones of a (batch, head) (forward, dQ: query block qb visits
// 2 qb + 2 tiles) and not the first (dK/dV: key block kb visits the query tiles from 2 kb on).
template <bool CAUSAL, bool HEAVIEST_LAST>
__device__ __forceinline__ void attn_block(int nrb, int& bh, int& rb) {
  if constexpr (CAUSAL) {
    causal_block(nrb, bh, rb);
    if (HEAVIEST_LAST) rb = nrb - 1 - rb;
  } else {
    const int blk = xcd_block();
    bh = blk / nrb;
    rb = blk - bh * nrb;
  }
}

// one past the last 64-key tile of a sequence that holds a valid key (0: the
// sequence has none).  kb: the sequence's nw = T / 32 words.  Every lane of
// every wave reads the same words, so the result is workgroup-uniform.
__device__ __forceinline__ int mask_tiles(const uint32_t* kb, int nw, int lane) {
  int last = -1;   // last non-zero word
  for (int c = 0; c < nw; c += 64) {
    const uint32_t v = c + lane < nw ? kb[c + lane] : 0u;
    const uint64_t bal = __ballot(v != 0u);
    if (bal) last = c + 63 - __builtin_clzll(bal);
  }
  return (last >> 1) + 1;
}

// key tiles of query block qb in the forward and dQ kernels.  MASK: stop after the last tile with a valid
// key (0 tiles: an empty sequence); CAUSAL: and after the workgroup's last visible tile, the one of its
// query 128 qb + 127
template <bool MASK, bool CAUSAL>
__device__ __forceinline__ int key_tiles(const uint32_t* kbits, int T, int qb, int lane) {
  const int ntm = MASK ? mask_tiles(kbits, T >> 5, lane) : T / kKT;
  return CAUSAL ? min(ntm, 2 * qb + 2) : ntm;
}

// scores of one 64-key tile in the transposed layout of the forward and dQ
// kernels (the lane holds keys 16 kt + 4g + r): -inf where the key's bit is
// clear.  lo / hi: the tile's two mask words shifted right by 4g, so every bit
// position is a constant.  min(s, +-inf) with the sign taken from the bit: a
// few in-place integer ops per score and no compare masks -- the select form
// (32 lane masks alive at once) cost the bf16 forward its third workgroup per CU.
__device__ __forceinline__ void mask_scores_t(f32x4 (&s)[2][4], uint32_t lo, uint32_t hi) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t w = kt < 2 ? lo : hi;
        const uint32_t neg = ((w << (31 - (16 * (kt & 1) + r))) & 0x80000000u) ^ 0x80000000u;   // sign set = masked
        s[qt][kt][r] = fminf(s[qt][kt][r], __uint_as_float(0x7f800000u | neg));
      }
}

// causal mask on a diagonal tile, same layout: the lane's query of block qt
// against its keys 16 kt + 4g + r.  d = (query of qt = 0) - (tile's first
// key) - 4g, so key (kt, r) of query block qt is hidden iff
// d - (16 kt + r - 16 qt) < 0: that sign is the sign of the +-inf, as above.
__device__ __forceinline__ void causal_scores_t(f32x4 (&s)[2][4], int d) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t neg = (uint32_t)(d - (16 * kt + r - 16 * qt)) & 0x80000000u;   // sign set = hidden
        s[qt][kt][r] = fminf(s[qt][kt][r], __uint_as_float(0x7f800000u | neg));
      }
}

// the same in the dK/dV kernels' layout (key on the lane, query on 4g + r):
// d = (query of r = 0) - (lane's key); score r is hidden iff d + r < 0
__device__ __forceinline__ void causal_scores_q(f32x4& s, int d) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t neg = (uint32_t)(d + r) & 0x80000000u;
    s[r] = fminf(s[r], __uint_as_float(0x7f800000u | neg));
  }
}

// Per-tile mask front end of the forward and dQ kernels, in the order a kernel needs it: load() before
// the tile's wait and barrier, skip() after the next tile is staged, init() ahead of the operand reads.
template <bool MASK, bool CAUSAL>
struct TileMask {
  uint32_t w0, w1;   // valid bits of the tile's 64 keys (workgroup-uniform)
  int qrel;          // CAUSAL: (wave's first query) - (tile's first key)

  __device__ __forceinline__ void load(const uint32_t* kbits, int t) {
    w0 = w1 = ~0u;
    if (MASK) {
      w0 = kbits[2 * t];
      w1 = kbits[2 * t + 1];
    }
  }
  // No valid / no visible key: the tile is staged and waited for, its arithmetic skipped (P = 0).
  // q0: the wave's first query, wave-uniform.  CAUSAL, per wave: the tile is fully visible (qrel >= 63),
  // diagonal, or past the wave's last query (qrel < -31: waves 0 and 1 on the workgroup's last tile)
  __device__ __forceinline__ bool skip(int q0, int t) {
    qrel = CAUSAL ? q0 - kKT * t : 0;
    return (MASK && (w0 | w1) == 0u) || (CAUSAL && qrel < -31);
  }
  // the scores' initial accumulator: the row constant c[qt], and -inf for a masked or hidden key, which the
  // MFMAs carry through (P = exp2(-inf) and with it dS are exactly 0).  Set before the operand reads so that
  // the tile's arithmetic stays one scheduling region.  Without MASK and CAUSAL this is only the splat, and
  // a kernel may pass the splat to its first MFMA instead.
  __device__ __forceinline__ void init(f32x4 (&s)[2][4], const float (&c)[2], int li, int g) const {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) s[qt][kt] = splat4(c[qt]);
    if (MASK && (w0 & w1) != ~0u) mask_scores_t(s, w0 >> (4 * g), w1 >> (4 * g));
    if (CAUSAL && qrel < 63) causal_scores_t(s, qrel + li - 4 * g);
  }
};

// the forward's first tile (MASK: the first with a valid key, where every row has a finite max; CAUSAL alone:
// tile 0, key 0 is visible to every query; CAUSAL && MASK: per row, fresh[] below).  started: MASK, a tile
// with a valid key has been seen
template <bool MASK>
__device__ __forceinline__ bool first_tile(bool& started, int t) {
  const bool first = MASK ? !started : t == 0;
  started = true;
  return first;
}

// Forward online-softmax step of one 16-query row block on tile t: s = S^T - m on entry (log2 units), the
// dropped-out P on exit; o, m, l: the row block's accumulator, running max and row sum (this lane's part).
// fresh (CAUSAL && MASK): the row has had no finite score yet.  Left padding or a hole over keys 0 .. q
// leaves a row's first tiles all -inf; such a row does not move m and takes the first-tile step at its
// first finite score (a row that never has one ends with l = 0: out = 0, lse = 0).
// hrow: pair-hash index of key 4g of tile 0.
template <bool DROP, bool MASK, bool CAUSAL>
__device__ __forceinline__ void softmax_step(f32x4 (&s)[4], f32x4 (&o)[4], float& m, float& l, bool& fresh, bool first,
                                             uint32_t hrow, int t, uint32_t seed, uint32_t thr) {
  float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
  for (int kt = 1; kt < 4; ++kt) mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
  // wave-uniform, rare after the first tile
  if ((CAUSAL && MASK) ? __ballot(fresh || mx > kLazy) != 0 : first || __ballot(mx > kLazy) != 0) {
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float d;
    if constexpr (CAUSAL) {
      // per row: a row below the threshold keeps its m bit for bit (d = 0 changes nothing), so what
      // another row of the wave scores -- a later query sees keys this one does not -- cannot reach it
      const bool fr = MASK ? fresh : first;
      const bool dark = MASK && mx == -INFINITY;   // no finite score in this tile
      d = fr ? (dark ? 0.f : mx) : (mx > kLazy ? mx : 0.f);
      if (MASK) fresh = fr && dark;
    } else {
      d = first ? mx : fmaxf(mx, 0.f);
    }
    m += d;
    const float al = fexp2(-d);
    l *= al;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= al;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) s[kt] -= splat4(d);
  }
  float ls = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    uint32_t hh[2];
    if (DROP) {
      const uint32_t pi = hrow + t * (kKT / 2) + 8 * kt;
      hh[0] = pair_hash(seed, pi);
      hh[1] = pair_hash(seed, pi + 1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float p = fexp2(s[kt][r]);
      ls += p;
      if (DROP) {
        const uint32_t u = (r & 1) ? hh[r >> 1] >> 16 : hh[r >> 1] & 0xffffu;
        p = u >= thr ? p : 0.f;
      }
      s[kt][r] = p;
    }
  }
  l += ls;
}

// Forward epilogue of one row: the row sum over the lane groups, lse (stored by g = 0 at lse_q) and the
// output scale.  MASK, a row without a visible valid key (l = 0; an empty sequence: no tile was waited
// for): out = 0 and lse = 0
template <bool MASK>
__device__ __forceinline__ float finish_row(float l, float m, float dscale, float* lse_q, int g) {
  float lt = l;
  lt += __shfl_xor(lt, 16, 64);
  lt += __shfl_xor(lt, 32, 64);
  const bool none = MASK && lt == 0.f;
  if (g == 0) *lse_q = none ? 0.f : m + __log2f(lt);
  return none ? 0.f : dscale / lt;
}

// dQ kernel, elementwise on one tile: s = c q.k - lse and dz = dP - delta' on entry (delta' = delta /
// dscale under DROP), s = dS = P (keep ? dscale dP - delta : -delta) on exit
template <bool DROP>
__device__ __forceinline__ void ds_step(f32x4 (&s)[2][4], const f32x4 (&dz)[2][4], const float (&del)[2],
                                        const uint32_t (&hrow)[2], int t, uint32_t seed, uint32_t thr, float dscale) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      uint32_t hh[2];
      if (DROP) {
        const uint32_t pi = hrow[qt] + t * (kKT / 2) + 8 * kt;
        hh[0] = pair_hash(seed, pi);
        hh[1] = pair_hash(seed, pi + 1);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fexp2(s[qt][kt][r]);
        float dd = dz[qt][kt][r];   // dP - delta (no dropout)
        if (DROP) {
          const uint32_t u = (r & 1) ? hh[r >> 1] >> 16 : hh[r >> 1] & 0xffffu;
          dd = u >= thr ? dd * dscale : -del[qt];
        }
        s[qt][kt][r] = p * dd;
      }
    }
}

}  // namespace gk
