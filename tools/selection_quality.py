#!/usr/bin/env python3
"""Selection-quality table of the sparsifiers.

For every (model, compressor) and for two bucket plans -- one merged bucket and
one bucket per tensor (``threshold=0``) -- runs a short seeded training loop on
synthetic data in one process with ``selection_quality_every=1`` and prints a
markdown table of the four metrics of ``DistributedOptimizer.collect_selection_quality``:
mean and min over the bucket-steps after the first ``--skip`` steps.

    record_occupancy  sent / k_cap
    topk_overlap      share of the exact top-k (of the error-feedback accumulator) that was sent
    energy_captured   sum of sent^2 / sum of the exact top-k's squares
    energy_fraction   sum of sent^2 / sum of the whole accumulator's squares

Usage: python tools/selection_quality.py [--models resnet20,vgg16,lstm,bert_tiny]
           [--compressors gaussian,gaussian_cal,topk,dgcsampling,redsync] [--steps 30] [--out FILE.md]
Runs on the CPU too (slowly: keep it to ``--models fcn5net``).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODELS = {   # dnn -> (dataset, batch size, lr, gradient-norm clip)
    "resnet20": ("cifar10", 32, 0.05, None),
    "vgg16": ("cifar10", 32, 0.01, None),
    "lstm": ("ptb", 20, 1.0, 0.25),
    "bert_tiny": ("wikipedia", 8, 0.01, None),
    "fcn5net": ("mnist", 32, 0.05, None),
}
METRICS = ("record_occupancy", "topk_overlap", "energy_captured", "energy_fraction")
MERGED = 524288000


def run_one(dnn, comp, threshold, steps, density, device, seed=0):
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm
    from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer
    from gaussiank_sgd_amd.train import DLTrainer
    dataset, bs, lr, clip = MODELS[dnn]
    torch.manual_seed(seed)
    comm.init()
    compressors[comp].clear()
    t = DLTrainer(0, 1, dnn=dnn, dataset=dataset, batch_size=bs, lr=lr, device=device, data_pool=4, seed=seed)
    opt = DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(), compression=compressors[comp],
                               is_sparse=True, density=density, compress_single_rank=True, density_warmup=False,
                               threshold=threshold, selection_quality_every=1)
    if t.is_cuda:
        from gaussiank_sgd_amd.parallel import install_direct_grads
        install_direct_grads(t.net, opt)
    t.update_optimizer(opt)
    hidden = t.net.init_hidden() if dnn == "lstm" else None
    for _ in range(steps):
        opt.zero_grad()
        if dnn == "lstm":
            _, hidden = t.train(1, hidden=hidden)
        else:
            t.train(1)
        if clip is not None:
            opt.synchronize()
            opt.clip_grad_norm_(clip)
        t.update_model()
    rows = opt.collect_selection_quality()
    return rows, len(opt.arena.buckets), float(t.current_loss())


def summarise(rows, skip):
    rows = [r for r in rows if r["iter"] >= skip]
    out = {}
    for m in METRICS:
        v = [r[m] for r in rows]
        out[m] = (float(np.mean(v)), float(np.min(v))) if v else (float("nan"), float("nan"))
    return out, len(rows)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", default="resnet20,vgg16,lstm,bert_tiny")
    ap.add_argument("--compressors", default="gaussian,gaussian_cal,topk,dgcsampling,redsync")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip", type=int, default=5, help="leave out the bucket-steps of the first SKIP steps")
    ap.add_argument("--density", type=float, default=0.001)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--out", default=None, help="also write the table to this file (appended row by row)")
    args = ap.parse_args(argv)
    head = ["| model | plan | buckets | compressor | bucket-steps | " +
            " | ".join("%s mean / min" % m for m in METRICS) + " | loss |",
            "|---|---|---|---|---|" + "---|" * (len(METRICS) + 1)]
    title = "Selection quality, density %g, %d steps (first %d left out), device %s%s" % (
        args.density, args.steps, args.skip, args.device,
        " (%s)" % torch.cuda.get_device_name(0) if args.device.startswith("cuda") else "")
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    emit(title)
    emit("")
    for line in head:
        emit(line)
    for dnn in args.models.split(","):
        for plan, threshold in (("merged", MERGED), ("per-tensor", 0)):
            for comp in args.compressors.split(","):
                t0 = time.time()
                rows, nb, loss = run_one(dnn, comp, threshold, args.steps, args.density, args.device)
                s, cnt = summarise(rows, args.skip)
                emit("| %s | %s | %d | %s | %d | %s | %.4f |" % (
                    dnn, plan, nb, comp, cnt, " | ".join("%.3f / %.3f" % s[m] for m in METRICS), loss))
                print("  (%s %s %s: %.1f s)" % (dnn, plan, comp, time.time() - t0), file=sys.stderr, flush=True)
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
