"""Multi-rank checkpoint / resume under LAMB (2 processes, gloo, CPU).

The pattern of tests/test_adam_resume_gloo.py with ``optimizer="adamw",
trust_ratio=True``: 4 steps
that save (every rank its own file), resumed in FRESH processes for 4 more,
must end bit-identical to 8 uninterrupted steps -- weights, both moment
arenas, the step count and every rank's residuals -- and the two replicas
must agree.  The density warm-up's epoch boundary (0.004 -> 0.001, another
record size) falls exactly at the resume point.  The moments and the step
count are replicated state: rank 0's are broadcast (``broadcast_state``)."""
import glob
import os
import socket

import torch
import torch.multiprocessing as mp

BS = 16
SAMPLES = 64          # 2 ranks x bs 16 -> 2 iterations per epoch


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, outdir, max_epochs, pretrain, save_final, tag):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                      LOCAL_RANK=str(rank))
    from gaussiank_sgd_amd.parallel import distributed_optimizer as hvd
    from gaussiank_sgd_amd.train.dist_trainer import ssgd
    hvd.init(device="cpu")
    try:
        trainer, opt = ssgd("fcn5net", "mnist", os.path.join(outdir, "nodata"), 2, 1e-3, BS, 1, max_epochs, 1,
                            pretrain, 35, "gaussian", 0.001, 524288000, saved_dir=outdir, train_samples=SAMPLES,
                            checkpoint_every=2, save_final=save_final, metrics_dir=outdir, optimizer="adamw",
                            trust_ratio=True, trust_clip=10.0)
        a = opt.arena
        assert opt._fused_kind == "lamb"
        steps = {float(st["step"]) for st in opt.state.values()}
        assert steps == {float(opt._adam_step)}, steps
        res = {"w": a.weights.clone(), "m": a.momentum.clone(), "v": a.second_moment.clone(),
               "r": a.residuals.clone(), "step": opt._adam_step.clone(), "trust": opt._lamb_ws.trust.clone(),
               "iter": torch.tensor([opt.train_iter, opt.train_epoch, trainer.train_iter, trainer.train_epoch])}
        torch.save(res, os.path.join(outdir, "%s-rank%d.pt" % (tag, rank)))
    finally:
        hvd.comm.shutdown()


def _run(outdir, max_epochs, pretrain, save_final, tag):
    mp.spawn(_worker, args=(_free_port(), outdir, max_epochs, pretrain, save_final, tag), nprocs=2, join=True)


def _load(outdir, tag, r):
    return torch.load(os.path.join(outdir, "%s-rank%d.pt" % (tag, r)), weights_only=True)


def test_lamb_resume_two_ranks_equals_uninterrupted(tmp_path):
    full = str(tmp_path / "full")
    part = str(tmp_path / "part")
    os.makedirs(full)
    os.makedirs(part)
    _run(full, 4, None, False, "full")            # 8 steps, epochs 0-3
    _run(part, 2, None, True, "first")            # 4 steps, then every rank saves
    cks = sorted(glob.glob(os.path.join(part, "weights", "**", "*-rank*-epoch*.pth"), recursive=True))
    r0 = [c for c in cks if "-rank0-" in os.path.basename(c)]
    assert r0 and any("-rank1-" in os.path.basename(c) for c in cks), cks
    assert float(_load(part, "first", 0)["step"]) == 4.0
    _run(part, 4, r0[-1], False, "resumed")       # fresh processes: 4 more steps
    for r in range(2):
        a, b = _load(full, "full", r), _load(part, "resumed", r)
        assert a["iter"].tolist() == b["iter"].tolist() == [8, 4, 8, 3], (a["iter"], b["iter"])
        assert float(a["step"]) == float(b["step"]) == 8.0
        assert set(a) == set(b)
        for key in a:
            assert torch.equal(a[key], b[key]), "rank %d: %s differs after resume" % (r, key)
        assert float(a["m"].abs().sum()) > 0 and float(a["v"].abs().sum()) > 0
    s0, s1 = _load(part, "resumed", 0), _load(part, "resumed", 1)
    for key in ("w", "m", "v", "step", "trust"):
        assert torch.equal(s0[key], s1[key]), "replicas diverged after resume: %s" % key
    # the residuals are per rank (not broadcast): they differ between ranks
    assert not torch.equal(s0["r"], s1["r"])
