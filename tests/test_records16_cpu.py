"""Compact wire records on the CPU: the PyTorch fallbacks against the reference of records16_cases.py, the
record size, the refusals, and loopback worlds training one step with record_format='compact'."""
import pytest
import torch

from gaussiank_sgd_amd import ops
from records16_cases import CASES, check_reduce


@pytest.mark.parametrize("apply", [False, True], ids=["reduce", "apply"])
@pytest.mark.parametrize("name", CASES)
def test_fallback_pack_and_reduce(name, apply):
    check_reduce(name, "cpu", apply)


@pytest.mark.parametrize("n,k_cap,words", [(64, 8, 14), (65536, 7, 14), (65537, 1, 9), (25_600_000, 25_600, 25_996)])
def test_record16_words(n, k_cap, words):
    assert ops.record16_words(n, k_cap) == words


def _world(P, comp="gaussian", density=0.01, **kw):
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm, distributed_optimizer as hvd
    from gaussiank_sgd_amd.train import DLTrainer
    trainers = []
    for r in range(P):
        torch.manual_seed(0)
        trainers.append(DLTrainer(r, P, dnn="fcn5net", dataset="mnist", batch_size=32, lr=0.5, nworkers=P,
                                  device="cpu", learnable_data=True, seed=r))

    def body(r):
        t = trainers[r]
        opt = hvd.DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                                       compression=compressors[comp], is_sparse=density < 1, density=density,
                                       density_warmup=False, record_format="compact", **kw)
        hvd.broadcast_parameters(t.net.state_dict(), root_rank=0)
        t.update_optimizer(opt)
        opt.zero_grad()
        t.train(1)
        acc = opt.arena.grads.clone() + opt.arena.residuals      # this step's accumulator (exchange is in step())
        t.update_model()
        return opt, acc
    return comm.loopback_world(P, body)


@pytest.mark.parametrize("P", [2, 4])
def test_loopback_step_compact(P):
    res = _world(P)
    for opt, acc in res:
        assert torch.equal(opt.arena.weights, res[0][0].arena.weights), "replicas diverged"
        words = []
        for b in opt.arena.buckets:
            k_cap = opt._compression.k_cap_for(opt._compression.k_of(b.numel, 0.01), b.numel)
            words.append(ops.record16_words(b.span, k_cap))
            assert opt._exchange_words(b, 0.01) == words[-1] and b.extra["agg"][0].numel() == P * words[-1]
            # conservation: the rank's contribution (its record, values as sent) + residual == accumulator
            back = b.slice(opt.arena.residuals).clone()
            ops.scatter_add_records_(back, b.bufs.record, 1, k_cap, 1.0)
            assert torch.equal(back, b.slice(acc))
        assert sum(int(b.bufs.record[0]) for b in opt.arena.buckets) > 0 and opt.wire_bytes_per_step() == 4 * sum(words)


@pytest.mark.parametrize("comp,density", [("gaussian2", 0.01), ("randomk", 0.01), ("none", 1.0), ("bucket", 1.0),
                                          ("topk_legacy", 0.01)])
def test_compact_refused(comp, density):    # no residual for the rounding residue, or no records at all
    with pytest.raises(ValueError, match="record_format"):
        _world(1, comp=comp, density=density, compress_single_rank=True)
