"""Fused self-attention (ops/attention.py) vs torch SDPA on BERT-base's shape
(B 32, heads 12, T 512, d 64, dropout 0.1): forward and forward+backward
times per call and the achieved MFMA rate (fwd 4*B*H*T^2*d FLOPs, bwd 2.5x).

    python bench/attn_probe.py [--B 32] [--T 512] [--heads 12] [--p 0.1] [--dtype bf16|fp32] [--pad] [--causal]
                                 [--iters 20]

--pad: a key-padding mask with per-sequence valid lengths drawn uniformly from
[T/4, T] (fixed seed).  Times ours with the mask ("ours_masked") against SDPA
with the same boolean mask ("sdpa_masked"), and ours with an all-valid mask
("ours_allvalid") against ours without one ("ours"); the TFLOP/s of the masked
rows count the dense op's FLOPs.

--causal: ours with causal=True ("ours_causal") against ours without it at
the same shape ("ours") and against SDPA with is_causal=True ("sdpa_causal");
with --pad also "ours_causal_masked" against "ours_masked" and against SDPA
with the merged boolean mask ("sdpa_causal_masked").  "causal" then holds the
measured causal / non-causal time ratios, forward and backward, next to the
tile model: per (batch, head) the forward and dQ kernels visit nqb (nqb + 1) of
2 nqb^2 key tiles and the dK/dV kernel as many query tiles, nqb = T / 128
(0.625 at T = 512, 0.5625 at T = 1024).  The TFLOP/s of causal rows count the
dense op's FLOPs.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiank_sgd_amd import ops  # noqa: E402
from gaussiank_sgd_amd.ops import attention  # noqa: E402


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--pad", action="store_true", help="key-padding mask, valid lengths uniform in [T/4, T]")
    ap.add_argument("--causal", action="store_true", help="causal=True against the same shape without it")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per row (after iters / 4 warm-up calls)")
    ap.add_argument("--only", default="", help="comma-separated rows to time (default: all)")
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    assert ops.load(), ops._load_error
    B, T, Hh, p = a.B, a.T, a.heads, a.p
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    fn = attention._FlashAttnFn if a.dtype == "bf16" else attention._FlashAttnF32Fn
    torch.manual_seed(0)
    qkv = torch.randn(B, T, 3 * Hh * 64, device="cuda").to(dtype).requires_grad_(True)
    dout = torch.randn(B, T, Hh * 64, device="cuda").to(dtype)
    flops = 4.0 * B * Hh * T * T * 64
    res = {"shape": [B, Hh, T, 64], "p": p, "dtype": a.dtype}

    def pair(call):
        def f():
            with torch.no_grad():
                call()

        def fb():
            call().backward(dout)
        return f, fb

    rows = [("ours", *pair(lambda: fn.apply(qkv, Hh, p, 1))),
            ("sdpa", *pair(lambda: attention._sdpa(qkv, Hh, p)))]
    if a.pad:
        g = torch.Generator().manual_seed(1234)
        lengths = torch.randint(T // 4, T + 1, (B,), generator=g).cuda()
        valid = torch.arange(T, device="cuda")[None, :] < lengths[:, None]
        bits = attention.pack_key_mask(valid)
        ones = attention.pack_key_mask(torch.ones_like(valid))
        bmask = valid[:, None, None, :]
        res["pad"] = {"mean_valid": round(float(valid.float().mean()), 4), "min_len": int(lengths.min()),
                      "max_len": int(lengths.max())}
        rows += [("ours_masked", *pair(lambda: fn.apply(qkv, Hh, p, 1, None, bits))),
                 ("ours_allvalid", *pair(lambda: fn.apply(qkv, Hh, p, 1, None, ones))),
                 ("sdpa_masked", *pair(lambda: attention._sdpa(qkv, Hh, p, bmask)))]
    if a.causal:
        rows += [("ours_causal", *pair(lambda: fn.apply(qkv, Hh, p, 1, None, None, True))),
                 ("sdpa_causal", *pair(lambda: attention._sdpa(qkv, Hh, p, None, True)))]
        if a.pad:
            rows += [("ours_causal_masked", *pair(lambda: fn.apply(qkv, Hh, p, 1, None, bits, True))),
                     ("sdpa_causal_masked", *pair(lambda: attention._sdpa(qkv, Hh, p, bmask, True)))]

    only = set(filter(None, a.only.split(",")))
    for name, f, fb in rows:
        if only and name not in only:
            continue
        tf = timeit(f, a.iters, max(5, a.iters // 4))
        tfb = timeit(fb, a.iters, max(5, a.iters // 4))
        res[name] = {"fwd_us": round(tf, 1), "fwd_bwd_us": round(tfb, 1), "bwd_us": round(tfb - tf, 1),
                     "fwd_tflops": round(flops / tf / 1e6, 1), "bwd_tflops": round(2.5 * flops / max(tfb - tf, 1e-3) / 1e6, 1)}
    if a.causal:
        nqb = T // 128
        res["causal"] = {"tile_model": round((nqb + 1) / (2.0 * nqb), 4)}
        for c, d in (("ours_causal", "ours"), ("ours_causal_masked", "ours_masked")):
            if c in res and d in res:
                res["causal"][c + "/" + d] = {k: round(res[c][k + "_us"] / res[d][k + "_us"], 4) for k in ("fwd", "bwd")}
    print(json.dumps(res))
    if a.json_out:
        with open(a.json_out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
