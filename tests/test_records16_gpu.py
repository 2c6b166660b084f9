"""records16.hip against the plain reference of records16_cases.py, bit for bit; a captured compact-format step."""
import pytest
import torch

from records16_cases import CASES, check_reduce

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("apply", [False, True], ids=["reduce", "apply"])
@pytest.mark.parametrize("name", CASES)
def test_pack_and_reduce(name, apply):
    check_reduce(name, "cuda", apply)


def _graphed():
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm, install_bf16_shadow
    from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer
    from gaussiank_sgd_amd.train import DLTrainer
    from gaussiank_sgd_amd.train.graph import GraphedStep
    comm.init()
    t = DLTrainer(0, 1, dnn="resnet20", dataset="cifar10", batch_size=16, lr=0.05, device="cuda", amp="bf16",
                  channels_last=True, data_pool=1, seed=0)
    opt = DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                               compression=compressors["gaussian"], is_sparse=True, density=0.01,
                               compress_single_rank=True, density_warmup=False, record_format="compact")
    install_bf16_shadow(t.net, opt)
    t.update_optimizer(opt)
    t.display = 10 ** 9
    return t, opt, GraphedStep(t, opt)


def test_graph_replay_compact():
    """The whole step captured in the compact format: test_graph_gpu.py's checks of the full format, and with
    their 0.5 loss margin a replayed run against an eager run of as many steps."""
    from gaussiank_sgd_amd import ops
    t, opt, step = _graphed()
    step()                                  # 3 eager warm-up steps, the capture, the first replay
    losses, w_prev = [], opt.arena.weights.clone()
    for _ in range(4):
        step()
        torch.cuda.synchronize()
        losses.append(t.current_loss())
        assert (opt.arena.weights - w_prev).abs().max().item() > 0, "a replay did not update the weights"
        w_prev = opt.arena.weights.clone()
    assert step.captures == 1 and all(l == l for l in losses) and losses[-1] < losses[0] + 0.5
    b = max(opt.arena.buckets, key=lambda b: b.numel)     # the compact record is what the step went through
    sent = min(int(b.bufs.record[0]), b.bufs.k_cap)
    assert sent > 0 and int(b.extra["rec16"][ops.REC_HDR + (b.span + 65535) // 65536]) == sent
    te, _, eager = _graphed()
    for _ in range(3 + 5):
        eager._body()
    torch.cuda.synchronize()
    assert abs(te.current_loss() - losses[-1]) < 0.5
