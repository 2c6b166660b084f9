"""Fused multi-head self-attention (``csrc/kernels/attn.hip``), head dim 64.

``self_attention(qkv, heads, p)`` takes the packed QKV projection
``[B, T, 3 * heads * 64]`` (the ``[B, T, 3, heads, 64]`` layout of BERT's fused
QKV linear) and returns ``softmax(q k^T / 8) -> dropout_p -> @ v`` merged back
to ``[B, T, heads * 64]`` -- the input layout of the attention-output linear.
On a GPU with bf16 activations (or fp32, the reference's precision:
``csrc/kernels/attn_f32.hip`` on fp32 MFMA) this is one flash-style HIP kernel forward and
two backward (dQ with ``delta = rowsum(dO * O)``, then dK / dV); nothing of
size T x T is stored and there are no head split / merge copies: the kernels
read q, k, v with the packed row stride and write ``dqkv`` in the projection's
own layout.  The dropout mask is a hash of (seed, b*heads + h, query, key),
regenerated in the backward.

``key_mask`` is a key-padding mask: ``[B, T]`` (nonzero = real token) or the
packed bits of ``pack_key_mask`` (int32 ``[B, T // 32]``, bit ``j`` of word
``w`` = key ``32 w + j``).  The kernels take the bits: masked keys get
probability 0 (``softmax(q k^T / 8 + (valid ? 0 : -inf))``) and zero dK / dV,
key tiles without a valid key cost no arithmetic, and every query row --
padded ones too -- is computed, as SDPA does with a key mask.  The masked
bf16 forward also keeps the rounding residue of its output (``out_lo``) for the
backward's ``delta``, which short sequences need (few keys, concentrated
probabilities).  A sequence
without any valid key gives zeros (output and gradients) where SDPA gives NaN.

``causal=True`` is the lower-triangular mask of a decoder: query ``q`` sees key
``k`` iff ``k <= q``, ANDed with ``key_mask`` when both are given.  The kernels
take it as a compile-time variant (a Python bool here, so a captured step
replays it): key tiles past a workgroup's last query are never visited, tiles
below the diagonal carry no mask work, and only the diagonal tiles are masked
element by element.  A query without a visible valid key (left padding, a hole
over keys ``0 .. q``) gives output 0, zero dQ and adds nothing to dK / dV, where
SDPA gives NaN.  The causal bf16 forward keeps ``out_lo`` too, with or without
a key mask: the first rows of a sequence see few keys.

Elsewhere (CPU, ``attn_mask``, other head dims) it is
``F.scaled_dot_product_attention`` with identical semantics (``is_causal``, or
the lower triangle merged into the mask).

Not in the reference (its model zoo has no transformer); BASELINE config 5
(BERT-base MLM) runs it.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import capture_seed_word, hash_u32, load, seed_generator

HEAD_DIM = 64


def _ops():
    return torch.ops.gksgd


def drop_threshold(p: float) -> int:
    """16-bit drop threshold of the kernels (keep iff hash >> 16 >= thr)."""
    if p <= 0.0:
        return 0
    return min(int(round(p * 65536.0)), 65535)


def drop_scale(p: float) -> float:
    thr = drop_threshold(p)
    return 65536.0 / (65536 - thr) if thr else 1.0


def dropout_mask(B: int, heads: int, T: int, p: float, seed: int, device, seed_dev=None) -> torch.Tensor:
    """The kernels' keep mask as bool [B, heads, T, T] (tests / CPU mirror);
    ``seed_dev``: the replay word the captured kernels mixed in."""
    device = torch.device(device)
    if device.type == "cuda":
        load()
        m = torch.empty(B, heads, T, T, dtype=torch.uint8, device=device)
        _ops().attn_dropout_mask(m, B, heads, T, float(p), int(seed), seed_dev)
        return m.bool()
    # one 32-bit hash per pair of keys: low half -> even key, high half -> odd key
    h = hash_u32(torch.arange(B * heads * T * T // 2, dtype=torch.int64), int(seed) & 0xFFFFFFFF)
    u = torch.stack([h & 0xFFFF, h >> 16], dim=1)
    return (u >= drop_threshold(p)).view(B, heads, T, T)


def pack_key_mask(mask: torch.Tensor) -> torch.Tensor:
    """``[B, T]`` key mask (any dtype, nonzero = valid) -> packed bits, int32
    ``[B, T // 32]``: bit ``j`` of word ``w`` is key ``32 w + j``.  One HIP launch
    on the GPU, a torch expression on the CPU; nothing is read back to the host."""
    if mask.dim() != 2 or mask.shape[1] % 32:
        raise ValueError("key mask must be [B, T] with T a multiple of 32, got %s" % (tuple(mask.shape),))
    B, T = mask.shape
    if mask.is_cuda and load():
        bits = torch.empty(B, T // 32, dtype=torch.int32, device=mask.device)
        _ops().attn_pack_key_mask(mask.contiguous(), bits)
        return bits
    m = (mask != 0).view(B, T // 32, 32).to(torch.int64)
    w = (m << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_key_mask(bits: torch.Tensor, T: int) -> torch.Tensor:
    """Packed bits int32 ``[B, T // 32]`` -> bool ``[B, T]`` (True = valid)."""
    B = bits.shape[0]
    sh = torch.arange(32, device=bits.device)
    return ((bits.reshape(B, T // 32, 1).to(torch.int64) >> sh) & 1).bool().view(B, T)


def _is_packed(key_mask: torch.Tensor, B: int, T: int) -> bool:
    """A packed int32 [B, T // 32] mask, as opposed to a [B, T] one (dtype and shape tell)."""
    if key_mask.dtype == torch.int32 and tuple(key_mask.shape) == (B, T // 32) and T % 32 == 0:
        return True
    if tuple(key_mask.shape) != (B, T):
        raise ValueError("key_mask must be [B, T] = [%d, %d] or packed int32 [B, T // 32], got %s %s"
                         % (B, T, tuple(key_mask.shape), key_mask.dtype))
    return False


def _key_bits(key_mask: torch.Tensor, B: int, T: int) -> torch.Tensor:
    return key_mask.contiguous() if _is_packed(key_mask, B, T) else pack_key_mask(key_mask)


def key_mask_bool(key_mask: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """Either form of a key mask as bool ``[B, T]``."""
    return unpack_key_mask(key_mask, T) if _is_packed(key_mask, B, T) else key_mask != 0


def merge_masks(attn_mask, key_mask, B: int, T: int):
    """The SDPA mask of ``attn_mask`` (bool or additive, or None) and a key mask
    (either form, or None): masked keys are excluded for every query."""
    if key_mask is None:
        return attn_mask
    km = key_mask_bool(key_mask, B, T)[:, None, None, :]
    if attn_mask is None:
        return km
    if attn_mask.dtype == torch.bool:
        return attn_mask & km
    return attn_mask.masked_fill(~km, float("-inf"))


def causal_mask(T: int, device) -> torch.Tensor:
    """bool ``[T, T]``, True where query (row) sees key (column): ``k <= q``."""
    return torch.ones(T, T, dtype=torch.bool, device=device).tril_()


def reference_attention(qkv: torch.Tensor, heads: int, p: float = 0.0, seed: int = 0,
                        key_mask=None, causal: bool = False) -> torch.Tensor:
    """fp32 composition with the kernels' exact dropout mask (autograd-able);
    ``key_mask``: masked keys score -inf; ``causal``: so do keys after the
    query.  A row without a visible valid key gives zeros, not NaN."""
    B, T, H3 = qkv.shape
    d = H3 // (3 * heads)
    x = qkv.float().view(B, T, 3, heads, d)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) / d ** 0.5
    if key_mask is not None:
        s = s.masked_fill(~key_mask_bool(key_mask, B, T)[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill(~causal_mask(T, s.device), float("-inf"))
        if key_mask is not None:
            # rows that see nothing: a finite score row (so that softmax and its gradient stay finite), zeroed after
            dark = torch.isinf(s).all(dim=-1, keepdim=True)
            a = torch.softmax(s.masked_fill(dark, 0.0), dim=-1).masked_fill(dark, 0.0)
        else:
            a = torch.softmax(s, dim=-1)
    else:
        a = torch.softmax(s, dim=-1)
    if p > 0:
        keep = dropout_mask(B, heads, T, p, seed, qkv.device)
        a = a * keep.to(a.dtype) * drop_scale(p)
    o = torch.matmul(a, v)
    return o.transpose(1, 2).reshape(B, T, heads * d)


def _flash_attn_fn(name: str, dtype, fwd: str, bwd: str, keep_lo: bool):
    """The autograd function over the native ops ``fwd`` / ``bwd`` for activations of ``dtype``.
    ``keep_lo``: with a mask, rows with few valid keys have concentrated probabilities, where dP and
    delta = rowsum(dO * O) nearly cancel, so the bf16 forward also keeps what the rounding of O dropped
    (``out_lo``; causal: the first rows of a sequence are such rows) and both ops take it."""

    def forward(ctx, qkv, heads, p, seed, seed_dev=None, key_bits=None, causal=False):
        # seed_dev: the graph replay word (ops.graph_seed_word) under capture --
        # forward and backward of one replay read the same word
        # key_bits: the packed key mask (pack_key_mask), shared with the backward
        # causal: a Python bool, it picks the kernels' CAUSAL instantiations
        B, T, _ = qkv.shape
        out = torch.empty(B, T, heads * HEAD_DIM, dtype=dtype, device=qkv.device)
        lse = torch.empty(B * heads * T, dtype=torch.float32, device=qkv.device)
        lo = (None if key_bits is None and not causal else torch.empty_like(out),) if keep_lo else ()
        getattr(_ops(), fwd)(qkv, out, lse, int(heads), float(p), int(seed), seed_dev, key_bits, *lo,
                             bool(causal))
        ctx.save_for_backward(qkv, out, lse, key_bits, *lo)
        ctx.heads, ctx.p, ctx.seed, ctx.seed_dev = int(heads), float(p), int(seed), seed_dev
        ctx.causal = bool(causal)
        return out

    def backward(ctx, dout):
        qkv, out, lse, key_bits, *lo = ctx.saved_tensors
        dout = dout.to(dtype).contiguous()
        delta = torch.empty_like(lse)
        dqkv = torch.empty_like(qkv)
        getattr(_ops(), bwd)(qkv, out, dout, lse, delta, dqkv, ctx.heads, ctx.p, ctx.seed, ctx.seed_dev, key_bits,
                             *lo, ctx.causal)
        return dqkv, None, None, None, None, None, None

    # the class statement's own call, so that the class and its autograd node carry ``name``
    return type(torch.autograd.Function)(name, (torch.autograd.Function,),
                                         {"forward": staticmethod(forward), "backward": staticmethod(backward)})


_FlashAttnFn = _flash_attn_fn("_FlashAttnFn", torch.bfloat16, "attn_fwd", "attn_bwd", keep_lo=True)
# the fp32 twin (csrc/kernels/attn_f32.hip): fp32 operands on v_mfma_f32_16x16x4_f32, the same dropout hashes
_FlashAttnF32Fn = _flash_attn_fn("_FlashAttnF32Fn", torch.float32, "attn_f32_fwd", "attn_f32_bwd", keep_lo=False)


def _compute_dtype(qkv: torch.Tensor):
    """bf16 under bf16 autocast; otherwise the storage dtype -- but an
    autocast to any OTHER dtype (fp16) takes the SDPA composition, which
    follows autocast (as ops/ln.py and ops/linear.py do)."""
    if torch.is_autocast_enabled("cuda"):
        return torch.bfloat16 if torch.get_autocast_dtype("cuda") == torch.bfloat16 else None
    return qkv.dtype if qkv.dtype in (torch.bfloat16, torch.float32) else None


def _kernels_take(t: torch.Tensor, T: int, heads: int, width: int) -> bool:
    """The one rule behind ``fused_available`` and ``fused_available_for``: ``t``
    gives the device and the compute dtype, ``width`` is heads * head dim."""
    if not t.is_cuda or width != heads * HEAD_DIM:
        return False
    dt = _compute_dtype(t)
    if dt is None or not load():
        return False
    if dt == torch.float32:
        return bool(_ops().attn_f32_supported(T, HEAD_DIM))
    return bool(_ops().attn_supported(T, HEAD_DIM))


def fused_available(qkv: torch.Tensor, heads: int) -> bool:
    """The HIP kernels take this call: bf16 (autocast or bf16 activations) or
    fp32 (no autocast: the reference's precision), head dim 64, T % 128 == 0."""
    if qkv.dim() != 3:
        return False
    return _kernels_take(qkv, qkv.shape[1], heads, qkv.shape[-1] // 3 if qkv.shape[-1] % 3 == 0 else -1)


def fused_available_for(x: torch.Tensor, T: int, heads: int, width: int) -> bool:
    """``fused_available`` for the QKV projection of activations ``x`` ([B, T,
    width]) before it is computed: same device, same compute dtype."""
    return _kernels_take(x, T, heads, width)


def merge_causal(attn_mask, T: int, device):
    """``attn_mask`` (bool or additive, or None) with the lower triangle merged in."""
    tri = causal_mask(T, device)
    if attn_mask is None:
        return tri
    if attn_mask.dtype == torch.bool:
        return attn_mask & tri
    return attn_mask.masked_fill(~tri, float("-inf"))


def _sdpa(qkv: torch.Tensor, heads: int, p: float, attn_mask=None, causal: bool = False) -> torch.Tensor:
    B, T, H3 = qkv.shape
    d = H3 // (3 * heads)
    x = qkv.view(B, T, 3, heads, d)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    if causal and attn_mask is not None:   # SDPA takes is_causal or a mask, not both
        attn_mask, causal = merge_causal(attn_mask, T, qkv.device), False
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, dropout_p=p, is_causal=causal)
    return o.transpose(1, 2).reshape(B, T, heads * d)


def self_attention(qkv: torch.Tensor, heads: int, p: float = 0.0, training: bool = True,
                   attn_mask=None, seed: int = None, key_mask=None, causal: bool = False) -> torch.Tensor:
    """``[B, T, 3*heads*d]`` packed projection -> ``[B, T, heads*d]`` attention output.
    ``causal``: query ``q`` sees keys ``k <= q`` only (ANDed with ``key_mask``);
    the fused kernels take it (and then keep ``out_lo``, as with a key mask).  On
    the SDPA path a query without a visible valid key gives NaN, in the kernels 0.
    ``key_mask``: a key-padding mask, ``[B, T]`` (nonzero = valid) or packed
    (``pack_key_mask``); the fused kernels take it, ``attn_mask`` forces SDPA.
    An all-valid mask gives the unmasked call's output bit for bit; its bf16
    gradients agree with it only to rounding, because the masked backward forms
    ``delta`` from the output plus its saved rounding residue (``out_lo``, one
    more bf16 [B, T, heads*d] activation kept per call)."""
    p = float(p) if training else 0.0
    B, T = qkv.shape[0], qkv.shape[1]
    if attn_mask is None and fused_available(qkv, heads):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=seed_generator())) if p > 0 else 0
        seed_dev = capture_seed_word(qkv.device) if p > 0 else None
        bits = None if key_mask is None else _key_bits(key_mask, B, T)   # packed once, kept for the backward
        if _compute_dtype(qkv) == torch.float32:
            return _FlashAttnF32Fn.apply(qkv.contiguous(), heads, p, seed, seed_dev, bits, bool(causal))
        return _FlashAttnFn.apply(qkv.to(torch.bfloat16).contiguous(), heads, p, seed, seed_dev, bits, bool(causal))
    return _sdpa(qkv, heads, p, merge_masks(attn_mask, key_mask, B, T), bool(causal))
