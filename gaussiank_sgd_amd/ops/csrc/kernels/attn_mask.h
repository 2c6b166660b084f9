// Key-padding mask and causal mask of the fused attention kernels (attn.hip,
// attn_f32.hip).
//
// key_bits: uint32 [B, T / 32]; bit j of word w of a sequence is key 32 w + j,
// set = valid.  A 64-key tile is two words, the 128 keys of a dK/dV workgroup
// four; both are read through a workgroup-uniform address.
#pragma once
#include "common.h"
#include "mfma_util.h"

namespace gk {

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

// causal mask (CAUSAL instantiations: query q sees key k iff k <= q) on a
// diagonal tile, same layout: the lane's query of block qt against its keys
// 16 kt + 4g + r.  d = (query of qt = 0) - (tile's first key) - 4g, so key
// (kt, r) of query block qt is hidden iff d - (16 kt + r - 16 qt) < 0: that
// sign is the sign of the +-inf, as above.
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

}  // namespace gk
