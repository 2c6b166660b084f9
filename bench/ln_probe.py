"""Fused residual-add + dropout + LayerNorm (ops/ln.py) at BERT-base's shape
(32 x 512 rows of 768, p = 0.1): forward / backward microseconds per call and
the achieved bandwidth (forward moves 4 row tensors, backward 4 + the
column partials), against the unfused PyTorch composition.

    python bench/ln_probe.py [--rows 16384] [--hidden 768] [--p 0.1]

``--pre``: the pre-LN join of GPT-2 instead (``residual_layernorm``; 16 x 1024
rows of 768 unless ``--rows`` is given): fp32 residual stream, the branch in
bf16 under autocast and in fp32, against the composition GPT-2 ran before it
(dropout, add into the fp32 stream, LayerNorm -- fp32 under autocast -- and
the cast back to bf16 that the next linear makes).  The two alternate inside
the process; the figures are medians over the rounds, and the bandwidth is
the bytes one fused pass has to move over the time: per element, forward
a + x in and h + y out (bf16 branch 12, fp32 16), backward dy + h + dh in and
dx + da out (16 / 20).

    python bench/ln_probe.py --pre [--rows 16384] [--hidden 768] [--p 0.1] [--rounds 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiank_sgd_amd import ops  # noqa: E402
from gaussiank_sgd_amd.ops.ln import add_layernorm, residual_layernorm  # noqa: E402


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
    return e0.elapsed_time(e1) / iters * 1e3


def pre_ln(R, H, p, rounds):
    """The pre-LN join, fused against the composition, alternating; see the module docstring."""
    import statistics
    import torch.nn.functional as F
    ln = torch.nn.LayerNorm(H).cuda()
    x = torch.randn(R, H, device="cuda").requires_grad_(True)
    dh = torch.randn(R, H, device="cuda")
    res = {"rows": R, "hidden": H, "p": p, "rounds": rounds}
    for mode, cd, fwd_b, bwd_b in [("bf16", torch.bfloat16, 12, 16), ("fp32", torch.float32, 16, 20)]:
        bf16 = cd == torch.bfloat16
        a = torch.randn(R, H, device="cuda").to(cd).requires_grad_(True)
        dy = torch.randn(R, H, device="cuda").to(cd)

        def fused():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                return residual_layernorm(a, x, ln, p, True)

        def plain():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                h = x + F.dropout(a, p, True)
                return h, ln(h).to(cd)

        def nograd(f):
            def g():
                with torch.no_grad():
                    f()
            return g

        def both(f):
            def g():
                h, y = f()
                torch.autograd.backward([y, h], [dy, dh])
                x.grad = a.grad = None      # the next backward stores its gradients, it does not add to these
            return g

        t = {k: [] for k in ("fused_f", "plain_f", "fused_fb", "plain_fb")}
        for _ in range(rounds):
            for name, f in (("fused", fused), ("plain", plain)):
                t[name + "_f"].append(timeit(nograd(f), iters=200, warmup=10))
                t[name + "_fb"].append(timeit(both(f), iters=200, warmup=10))
        for name in ("fused", "plain"):
            tf = statistics.median(t[name + "_f"])
            tb = statistics.median(t[name + "_fb"]) - tf
            res[mode + "_" + name] = {"fwd_us": round(tf, 1), "bwd_us": round(tb, 1),
                                      "fwd_TBps": round(R * H * fwd_b / 1e6 / tf, 2),
                                      "bwd_TBps": round(R * H * bwd_b / 1e6 / max(tb, 1e-3), 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pre", action="store_true", help="the pre-LN join (residual_layernorm) instead")
    ap.add_argument("--rounds", type=int, default=5, help="--pre: alternations of fused and composition")
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--json-out", default="")
    a = ap.parse_args()
    assert ops.load(), ops._load_error
    R, H, p = a.rows, a.hidden, a.p
    if a.pre:
        res = pre_ln(R, H, p, a.rounds)
        print(json.dumps(res))
        if a.json_out:
            with open(a.json_out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    ln = torch.nn.LayerNorm(H).cuda()
    x = torch.randn(R, H, device="cuda").to(torch.bfloat16).requires_grad_(True)
    y = torch.randn(R, H, device="cuda").to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(R, H, device="cuda").to(torch.bfloat16)
    mb = R * H * 2 / 1e6
    res = {"rows": R, "hidden": H, "p": p}

    def fused_f():
        with torch.no_grad():
            add_layernorm(y, x, ln, p, True)

    def fused_fb():
        add_layernorm(y, x, ln, p, True).backward(dy)

    def eager_f():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            ln(x + torch.nn.functional.dropout(y, p))

    def eager_fb():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = ln(x + torch.nn.functional.dropout(y, p))
        out.backward(dy.float())

    for name, f, fb in [("fused", fused_f, fused_fb), ("torch", eager_f, eager_fb)]:
        tf, tfb = timeit(f), timeit(fb)
        res[name] = {"fwd_us": round(tf, 1), "bwd_us": round(tfb - tf, 1),
                     "fwd_TBps": round(4 * mb / tf, 2), "bwd_TBps": round(4 * mb / max(tfb - tf, 1e-3), 2)}
    print(json.dumps(res))
    if a.json_out:
        with open(a.json_out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
