"""FP8 linear probe: call times of the quantisers and the K = 128 MFMA GEMM against the bf16
FastLinear kernel the tuner picks, at the GPT-2 / BERT-base layer shapes; optionally the GPT-2
step time and the gpt_tiny loss with and without the FP8 path.

    python bench/fp8_probe.py [--iters 50] [--step] [--loss] [--out profiles/fp8_linear_probe.txt]

Times are device-event times of calls (launch overhead included), every shape warmed first, the
fp8 and the bf16 call alternated inside the same timed loop.  Reported, not gated.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiank_sgd_amd.ops import fp8, linear, load  # noqa: E402

M = 16384
SHAPES = [(768, 2304), (768, 768), (768, 3072), (3072, 768)]   # (K, N)


def _alternate(fns, iters):
    """Mean ms of each callable, all of them run once per iteration of one loop."""
    for f in fns:
        for _ in range(3):
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
          for _ in range(iters)]
    for row in ev:
        for f, (a, b) in zip(fns, row):
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return [sum(row[i][0].elapsed_time(row[i][1]) for row in ev) / iters for i in range(len(fns))]


def probe_shapes(iters, out):
    dev = torch.device("cuda")
    out("shape            pass     quant ms  fp8 gemm ms  fp8 sum ms   bf16 ms  fp8 gemm TFLOP/s  bf16 TFLOP/s")
    for K, N in SHAPES:
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        dy = torch.randn(M, N, device=dev).to(torch.bfloat16)
        w = (0.02 * torch.randn(N, K, device=dev)).to(torch.bfloat16)
        b = torch.zeros(N, device=dev)
        w8, w8t, sw = fp8.quantize_weight(w)
        x8, sx = fp8.quantize(x, "e4m3")
        d8, sd = fp8.quantize(dy, "e5m2")
        linear._fwd(x, w, b)     # tunes the bf16 kernels for this shape
        linear._dgrad(dy, w)
        flop = 2.0 * M * K * N
        for name, fns in (
                ("fwd", [lambda: fp8.quantize(x, "e4m3"), lambda: fp8.gemm_nt(x8, sx, w8, sw, b),
                         lambda: linear._fwd(x, w, b)]),
                ("dgrad", [lambda: fp8.quantize(dy, "e5m2"), lambda: fp8.gemm_nt(d8, sd, w8t, sw),
                           lambda: linear._dgrad(dy, w)])):
            q, g, ref = _alternate(fns, iters)
            out("K%-5d N%-5d   %-6s %9.4f %12.4f %11.4f %9.4f %17.1f %13.1f" %
                (K, N, name, q, g, q + g, ref, flop / g / 1e9, flop / ref / 1e9))
        wq = _alternate([lambda: fp8.quantize_weight(w)], iters)[0]
        out("K%-5d N%-5d   weight quantise + transpose (once per forward): %.4f ms" % (K, N, wq))


def train_run(dnn, batch, iters, timed, on):
    from gaussiank_sgd_amd.train.single import train_with_single   # builds the trainer as the entry point does
    linear.set_fp8(on)
    losses, t0 = [], None
    trainer = train_with_single(dnn, "openwebtext", "./data", 1, 1e-3 if dnn == "gpt_tiny" else 1e-4, batch, 1, 1,
                                amp="bf16", max_iters=1, optimizer="adamw")
    for i in range(iters):
        if i == iters - timed:
            torch.cuda.synchronize()
            t0 = time.time()
        trainer.optimizer.zero_grad()
        trainer.train(1)
        trainer.update_model()
        if dnn == "gpt_tiny" and (i + 1) % 20 == 0:
            losses.append(trainer.current_loss())
    torch.cuda.synchronize()
    linear.set_fp8(False)
    return (time.time() - t0) / timed * 1e3, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step", action="store_true", help="GPT-2 batch-16 step time, bf16 and fp8")
    ap.add_argument("--loss", action="store_true", help="gpt_tiny loss over 200 steps, bf16 and fp8")
    ap.add_argument("--out", default="profiles/fp8_linear_probe.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available() and load(), "needs a GPU and the native extension"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    f = open(args.out, "w")

    def out(s):
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()
    out("# bench/fp8_probe.py: M = %d, %d iterations, device-event call times (launches included)" % (M, args.iters))
    probe_shapes(args.iters, out)
    if args.step:
        for on in (False, True):
            ms, _ = train_run("gpt2", 16, 30, 20, on)
            out("train.single gpt2 adamw amp bf16 batch 16%s: %.2f ms / step (wall clock, 20 steps)" %
                (" --fp8-linear" if on else "", ms))
    if args.loss:
        for on in (False, True):
            _, losses = train_run("gpt_tiny", 16, 200, 100, on)
            out("gpt_tiny adamw amp bf16 batch 16%s, loss every 20 steps: %s" %
                (" --fp8-linear" if on else "", " ".join("%.3f" % v for v in losses)))
    f.close()


if __name__ == "__main__":
    main()
