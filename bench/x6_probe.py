#!/usr/bin/env python3
"""fp32 GEMMs on the fp32 MFMA (v_mfma_f32_16x16x4_f32) vs the bf16x6
fp32-accurate products (gemm_nt.h X6: exact 3-way bf16 split, six part
products on v_mfma_f32_16x16x32_bf16): best time over a set of tile configs
and the error of each against an fp64 reference, on the ResNet-50 bs512 1x1 /
implicit-GEMM shapes and the BERT-base linear shapes.

Usage (GPU): python bench/x6_probe.py [--json-out FILE] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CFGS = [0, 1, 2, 3, 4, 11, 12, 13, 14, 101, 102, 103, 104, 201, 203, 1001, 1002, 1005]
X6 = 100000

# (name, M, N, K) row GEMMs: ResNet-50 bs512 stride-1 1x1 forward shapes and BERT-base (bs32 x 512 tokens)
ROW = [("r50 64->256 @56", 512 * 56 * 56, 256, 64), ("r50 256->64 @56", 512 * 56 * 56, 64, 256),
       ("r50 128->512 @28", 512 * 28 * 28, 512, 128), ("r50 512->128 @28", 512 * 28 * 28, 128, 512),
       ("r50 256->1024 @14", 512 * 14 * 14, 1024, 256), ("r50 1024->256 @14", 512 * 14 * 14, 256, 1024),
       ("r50 512->2048 @7", 512 * 7 * 7, 2048, 512), ("r50 2048->512 @7", 512 * 7 * 7, 512, 2048),
       ("bert qkv", 16384, 2304, 768), ("bert out", 16384, 768, 768), ("bert ffn1", 16384, 3072, 768),
       ("bert ffn2", 16384, 768, 3072)]
# (name, N, H, C, Cout, S) 3x3 implicit GEMMs (pad 1)
CONV = [("r50 3x3 64 @56", 512, 56, 64, 64, 1), ("r50 3x3 128 @28", 512, 28, 128, 128, 1),
        ("r50 3x3 256 @14", 512, 14, 256, 256, 1), ("r50 3x3 512 @7", 512, 7, 512, 512, 1)]


def timeit(fn, iters=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def rel_err(C, ref):
    d = (C.double() - ref)
    return (d.norm() / ref.norm()).item(), (d.abs().max() / ref.abs().max()).item()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--quick", action="store_true", help="three configs per shape")
    args = ap.parse_args()
    from gaussiank_sgd_amd import ops
    assert ops.load(), ops._load_error
    g = torch.ops.gksgd
    dev = torch.device("cuda", 0)
    cfgs = [0, 2, 3] if args.quick else CFGS
    out = []
    torch.manual_seed(0)
    for name, M, N, K in ROW:
        A = torch.randn(M, K, device=dev)
        B = torch.randn(N, K, device=dev) * K ** -0.5
        C = torch.empty(M, N, device=dev)
        rec = {"name": name, "M": M, "N": N, "K": K, "flop": 2.0 * M * N * K}
        for mode, off in (("f32", 0), ("x6", X6)):
            best = (1e9, None)
            for c in cfgs:
                try:
                    t = timeit(lambda: g.gemm_nt(A, B, C, c + off, 0))
                except RuntimeError as e:
                    print("cfg", c + off, "error:", str(e).splitlines()[0][:300], flush=True)
                    continue
                best = min(best, (t, c))
            g.gemm_nt(A, B, C, best[1] + off, 0)
            rows = min(M, 4096)
            ref = A[:rows].double() @ B.double().t()
            rms, mx = rel_err(C[:rows], ref)
            rec[mode] = {"us": best[0] * 1e6, "cfg": best[1], "tflops": rec["flop"] / best[0] / 1e12,
                         "rel_rms_err": rms, "rel_max_err": mx}
        rec["speedup"] = rec["f32"]["us"] / rec["x6"]["us"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del A, B, C
    CL = torch.channels_last
    for name, Nb, H, Cin, Cout, S in CONV:
        x = torch.randn(Nb, Cin, H, H, device=dev).contiguous(memory_format=CL)
        w = (torch.randn(Cout, Cin, 3, 3, device=dev) * (9 * Cin) ** -0.5).contiguous(memory_format=CL)
        OH = (H + 2 - 3) // S + 1
        M = Nb * OH * OH
        y = torch.empty(Nb, Cout, OH, OH, device=dev).contiguous(memory_format=CL)
        zero = torch.zeros(64, device=dev)
        rec = {"name": name, "M": M, "N": Cout, "K": 9 * Cin, "flop": 2.0 * M * Cout * 9 * Cin}
        for mode, off in (("f32", 0), ("x6", X6)):
            best = (1e9, None)
            for c in cfgs:
                try:
                    t = timeit(lambda: g.conv_nt(x, w, y, zero, S, 1, c + off, 0))
                except RuntimeError as e:
                    print("cfg", c + off, "error:", str(e).splitlines()[0][:300], flush=True)
                    continue
                best = min(best, (t, c))
            g.conv_nt(x, w, y, zero, S, 1, best[1] + off, 0)
            ref = torch.nn.functional.conv2d(x[:2].double(), w.double(), stride=S, padding=1)
            rms, mx = rel_err(y[:2], ref)
            rec[mode] = {"us": best[0] * 1e6, "cfg": best[1], "tflops": rec["flop"] / best[0] / 1e12,
                         "rel_rms_err": rms, "rel_max_err": mx}
        rec["speedup"] = rec["f32"]["us"] / rec["x6"]["us"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del x, w, y
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
