"""FP8 operands for the linear layers (``csrc/kernels/fp8.hip``): per-tensor
power-of-two quantisers and a GEMM on ``v_mfma_scale_f32_16x16x128_f8f6f4``.

The numerics, stated once (the kernels, the emulation below and the tests
follow them):

* Scaling is per tensor and current: the scale comes from the tensor being
  quantised, there is no amax history and no state.  It is a power of two,
  ``2^e``, with ``e`` the largest integer such that ``amax * 2^e <= FMAX``;
  ``FMAX`` is 448 for e4m3 (OCP ``e4m3fn``) and 57344 for e5m2.  ``e`` is
  clamped to [-64, 64] and is 0 when ``amax`` is 0.  It is derived from the
  exponent and mantissa bits of ``amax`` (``scale_exponent``), not through a
  logarithm, so the CPU and the GPU agree exactly.  ``x * 2^e`` is exact in
  fp32 and ``|x * 2^e| <= FMAX`` by construction, so the saturation and NaN
  behaviour of the conversion is never reached.
* Rounding: ``q = rne(x * 2^e)``, round to nearest even -- what
  ``v_cvt_pk_fp8_f32`` / ``v_cvt_pk_bf8_f32`` do and what
  ``(x.float() * 2**e).to(torch.float8_e4m3fn)`` (or ``float8_e5m2``) does.
* Forward: ``y = bf16((X8 . W8^T) * 2^-(ex + ew) + bias)``; ``X8`` and ``W8``
  are e4m3, accumulation is fp32, the bias is fp32 and is added before the
  single rounding to bf16.
* Grad-input: ``dx = bf16((dY8 . W8) * 2^-(ed + ew))`` with ``dY8`` in e5m2
  and ``W8`` the same e4m3 values as in the forward (kept transposed,
  ``w8t``, because this product contracts over the output features).
* Grad-weight and bias gradient stay on the bf16 kernels (ops/linear.py).
* A scale is a one-element fp32 tensor on the operand's device holding the
  dequantising factor ``2^-e``.  No value is read by the host anywhere, so a
  forward and backward can be captured in a HIP graph.
* Non-finite inputs give non-finite (or meaningless) outputs and are not
  otherwise handled.

Off the GPU every function is a PyTorch emulation of these rules (torch
float8 casts, an fp32 matmul of the dequantised operands).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import require_native

FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
DTYPE = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
_FMT_ID = {"e4m3": 0, "e5m2": 1}
_P = {"e4m3": 8, "e5m2": 15}   # FMAX = 1.75 * 2^P
_PARTS = 1024                  # amax partials (kFp8MaxParts)


def _g():
    return torch.ops.gksgd


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for an int32 tensor e in [-126, 127], built from the bits."""
    return ((e + 127) << 23).to(torch.int32).view(torch.float32)


def scale_exponent(amax: torch.Tensor, fmt: str) -> torch.Tensor:
    """The int32 exponent ``e`` of the rule above for a non-negative fp32 ``amax`` (any shape)."""
    bits = amax.float().contiguous().view(torch.int32) & 0x7FFFFFFF
    x = (bits >> 23) - 127
    e = _P[fmt] - x - ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    return torch.where(bits == 0, torch.zeros_like(e), e.clamp(-64, 64))


def _emulate(x: torch.Tensor, fmt: str) -> Tuple[torch.Tensor, torch.Tensor]:
    e = scale_exponent(x.detach().abs().max().float().reshape(1), fmt)
    return (x.float() * _pow2(e)).to(DTYPE[fmt]), _pow2(-e)


def _native(x: torch.Tensor) -> bool:
    return x.is_cuda


def quantize(x: torch.Tensor, fmt: str = "e4m3") -> Tuple[torch.Tensor, torch.Tensor]:
    """``(q, scale)``: ``q`` the ``torch.float8_*`` image of the 2-D bf16 / fp32 ``x``, ``scale`` = 2^-e."""
    if not _native(x):
        return _emulate(x, fmt)
    require_native(x)
    x = x.contiguous()
    parts = torch.empty(_PARTS, dtype=torch.int32, device=x.device)
    q = torch.empty(x.shape, dtype=DTYPE[fmt], device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    _g().fp8_amax(x, parts)
    _g().fp8_quantize(x, parts, q, scale, _FMT_ID[fmt])
    return q, scale


def quantize_weight(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(w8, w8t, scale)`` of a weight ``[N, K]``: e4m3 as ``[N, K]`` and as ``[K, N]``, one scale."""
    if not _native(w):
        q, scale = _emulate(w, "e4m3")
        return q, q.t().contiguous(), scale
    require_native(w)
    w = w.contiguous()
    N, K = w.shape
    parts = torch.empty(_PARTS, dtype=torch.int32, device=w.device)
    w8 = torch.empty(N, K, dtype=DTYPE["e4m3"], device=w.device)
    w8t = torch.empty(K, N, dtype=DTYPE["e4m3"], device=w.device)
    scale = torch.empty(1, dtype=torch.float32, device=w.device)
    _g().fp8_amax(w, parts)
    _g().fp8_quantize_t(w, parts, w8, w8t, scale)
    return w8, w8t, scale


def gemm_supported(M: int, N: int, K: int) -> bool:
    return M >= 1 and N >= 128 and K >= 128 and N % 128 == 0 and K % 128 == 0


def gemm_nt(a8: torch.Tensor, sa: torch.Tensor, b8: torch.Tensor, sb: torch.Tensor,
            bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 ``(a8 [M, K] . b8 [N, K]^T) * sa * sb + bias``; ``a8`` e4m3 or e5m2, ``b8`` e4m3, ``bias`` fp32."""
    if b8.dtype != DTYPE["e4m3"] or a8.dtype not in (DTYPE["e4m3"], DTYPE["e5m2"]):
        raise TypeError("fp8.gemm_nt: a8 must be e4m3 or e5m2 and b8 e4m3, got %s, %s" % (a8.dtype, b8.dtype))
    if not _native(a8):
        y = (a8.float() @ b8.float().t()) * (sa * sb)
        return (y + bias.float() if bias is not None else y).to(torch.bfloat16)
    require_native(a8)
    out = torch.empty(a8.shape[0], b8.shape[0], dtype=torch.bfloat16, device=a8.device)
    _g().fp8_gemm_nt(a8, sa, b8, sb, bias, out, 0 if a8.dtype == DTYPE["e4m3"] else 1)
    return out
