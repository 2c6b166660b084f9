"""Wire-record probe: the full-format reduce against pack + 16-bit reduce of the compact format, for
P = 8 synthetic records of the ResNet-50 bucket (n = 25.6 M, k = 25.6 K) on one GPU; optionally the
end losses of 200 training steps in either format.

    python bench/records_probe.py [--iters 200] [--loss] [--out profiles/records16_probe.txt]

Index sets: independent (every rank draws its own k indices) and overlapping (every rank draws k of
one shared pool of 1.25 k).  Times are device-event times of calls (launch overhead included), all
calls warmed first, the formats alternated inside one timed loop.  pack is the one launch a rank adds
per step (its own record); both reduces read all P records.  Before timing, the 16-bit reduce is
compared bit for bit with the full reduce over the same bf16-rounded values.  Reported, not gated.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiank_sgd_amd import ops  # noqa: E402

N, K, P = 25_600_000, 25_600, 8
K_CAP = (4 * K + 2) // 3


def _records(overlap, dev, gen):
    pool = torch.randperm(N, device=dev, generator=gen)[:K + K // 4] if overlap else None
    full = torch.zeros(P, ops.REC_HDR + 2 * K_CAP, dtype=torch.int32, device=dev)
    for q in range(P):
        if overlap:
            idx = pool[torch.randperm(pool.numel(), device=dev, generator=gen)[:K]]
        else:
            idx = torch.randperm(N, device=dev, generator=gen)[:K]
        full[q, 0] = full[q, 1] = K
        full[q, ops.REC_HDR:ops.REC_HDR + K] = torch.sort(idx).values.to(torch.int32)
        full[q, ops.REC_HDR + K_CAP:ops.REC_HDR + K_CAP + K] = \
            torch.randn(K, device=dev, generator=gen).view(torch.int32)
    return full


def _alternate(fns, iters):
    """Mean ms of each callable, all of them run once per iteration of one loop."""
    for f in fns:
        for _ in range(5):
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


def probe(iters, out):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    words = ops.record16_words(N, K_CAP)
    out("record words per rank: full %d, compact %d (%.3fx); dense fp32 bucket / record: %.0fx -> %.0fx" % (
        full_words(), words, full_words() / words, N / full_words(), N / words))
    out("index sets     full reduce ms   pack ms   reduce16 ms   pack + reduce16 ms   faster")
    for overlap in (False, True):
        full = _records(overlap, dev, gen)
        resid = torch.zeros(N, device=dev)
        compact = torch.zeros(P, words, dtype=torch.int32, device=dev)
        for q in range(P):                       # rounds full's values too: both reduces see the same numbers
            ops.pack_records16_(full[q], K_CAP, resid, compact[q])
        a, b = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        ops.scatter_add_records_(a, full.view(-1), P, K_CAP, 1.0 / P, True)
        ops.reduce_records16_(b, compact.view(-1), P, K_CAP, 1.0 / P)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the two reduces disagree"
        tf, tp, tr = _alternate([lambda: ops.scatter_add_records_(a, full.view(-1), P, K_CAP, 1.0 / P, True),
                                 lambda: ops.pack_records16_(full[0], K_CAP, resid, compact[0]),
                                 lambda: ops.reduce_records16_(b, compact.view(-1), P, K_CAP, 1.0 / P)], iters)
        out("%-12s %16.4f %9.4f %13.4f %20.4f   %s" % ("overlapping" if overlap else "independent", tf, tp, tr,
                                                     tp + tr, "compact" if tp + tr < tf else "full"))


def full_words():
    return ops.REC_HDR + 2 * K_CAP


def end_loss(dnn, record_format, steps=200):
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm
    from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer
    from gaussiank_sgd_amd.train import DLTrainer
    comm.init()
    gpt = dnn == "gpt_tiny"
    t = DLTrainer(0, 1, dnn=dnn, dataset="openwebtext" if gpt else "cifar10", batch_size=16 if gpt else 128,
                  lr=1e-3 if gpt else 0.1, device="cuda:0", amp="bf16", channels_last=not gpt, seed=0,
                  optimizer="adamw" if gpt else "sgd")
    opt = DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                               compression=compressors["gaussian"], is_sparse=True, density=0.001,
                               threshold=524288000, compress_single_rank=True, density_warmup=False,
                               record_format=record_format)
    t.update_optimizer(opt)
    t.display = 10 ** 9
    tail = []
    for i in range(steps):
        opt.zero_grad()
        t.train(1)
        t.update_model()
        if i >= steps - 10:
            tail.append(t.current_loss())
    return tail[-1], sum(tail) / len(tail), opt.wire_compression_ratio()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--loss", action="store_true", help="200 steps of gpt_tiny and resnet20 (synthetic data) per format")
    ap.add_argument("--out", default="profiles/records16_probe.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.load(), "needs a GPU and the native extension"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    f = open(args.out, "w")

    def out(s):
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()
    out("# bench/records_probe.py: P = %d records, n = %d, k = %d, k_cap = %d, %d iterations, device-event call "
        "times (launches included)" % (P, N, K, K_CAP, args.iters))
    probe(args.iters, out)
    if args.loss:
        out("200 steps, gaussian, density 0.001, one GPU, synthetic data: loss at step 200, mean of the last 10, "
            "wire compression ratio")
        for dnn in ("gpt_tiny", "resnet20"):
            for fmt in ("full", "compact"):
                out("%-9s %-8s %8.4f %8.4f %8.1fx" % ((dnn, fmt) + end_loss(dnn, fmt)))
    f.close()


if __name__ == "__main__":
    main()
