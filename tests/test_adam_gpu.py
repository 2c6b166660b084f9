"""Fused Adam / AdamW HIP kernel (ops/csrc/kernels/optim.hip) and its users on
the GPU: numerics against torch's optimizers (tests/adam_cases.py: within 2x
torch's own fp32-vs-fp64 difference), gradient zeroing, bf16 shadow, padding,
the device scalars, the device-side step count under eager calls and HIP-graph
replays, the whole-step graph of the trainer, and two ranks on one GPU.

Largest err / yardstick ratio measured on an MI355X: see
profiles/fused_adam_kernels.txt."""
import pytest
import torch

import adam_cases as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant,sparse", ac.CASES, ids=ac.CASE_IDS)
def test_fused_adam_vs_torch(cuda, variant, sparse):
    """The arena's layout: every tensor padded to 64 elements, so (1000, 64) spans 4 chunks and (7,) is
    7 elements plus 57 padding slots, all on the float4 path (the scalar tail: the ragged test below)."""
    pad = ac.padding_mask().to(cuda)

    def on_step(t, w, m, v, g, step, shadow):
        assert not g.any(), "the gradient arena is zeroed in the same pass"
        assert torch.equal(shadow, w.to(torch.bfloat16))
        assert not w[pad].any() and not m[pad].any() and not v[pad].any(), "padding slots must stay exactly 0"

    worst = ac.run_case(variant, sparse, 4, cuda, with_shadow=True, on_step=on_step)
    print("%s/%s largest ratio %.3f" % (variant, "sparse" if sparse else "dense", worst))


@pytest.mark.parametrize("variant,sparse", ac.CASES, ids=ac.CASE_IDS)
def test_fused_adam_ragged_lengths_run_the_scalar_tail(cuda, variant, sparse):
    """Chunk lengths 1727, 63, 63999, 1001 and 7 at 64-aligned starts (the op and the binding take any
    length): every chunk ends in the kernel's scalar tail.  Same rule on the covered slots, their
    gradients zeroed, their shadow bf16(w); every slot beyond a length untouched."""
    worst = ac.run_ragged(variant, sparse, 4, cuda)
    print("ragged %s/%s largest ratio %.3f" % (variant, "sparse" if sparse else "dense", worst))


def _state(cuda, steps=0, variant="adamw"):
    from gaussiank_sgd_amd import ops
    w0, grads, _, _ = ac.reference(variant, False)
    st = {"w": w0.clone().to(cuda), "m": torch.zeros(ac.TOTAL, device=cuda), "v": torch.zeros(ac.TOTAL, device=cuda),
          "step": torch.zeros((), dtype=torch.float32, device=cuda)}
    chunks, groups = ac.chunk_table(cuda), ac.groups_for(variant)
    for t in range(steps):
        ops.fused_adam_(st["w"], st["m"], st["v"], grads[t].to(cuda), chunks, groups, st["step"])
    return st, [g.to(cuda) for g in grads], chunks, groups


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def test_fused_adam_device_scalars(cuda):
    from gaussiank_sgd_amd import ops
    st, grads, chunks, groups = _state(cuda, steps=1)
    a = _clone(st)
    ops.fused_adam_(a["w"], a["m"], a["v"], grads[1].clone(), chunks, groups, a["step"],
                    lr_mult=torch.zeros(1, device=cuda))
    assert torch.equal(a["w"], st["w"]), "lr_mult = 0 must leave w bit-unchanged (decoupled decay included)"
    assert not torch.equal(a["m"], st["m"]) and not torch.equal(a["v"], st["v"])
    assert float(a["step"]) == 2.0
    b, c = _clone(st), _clone(st)
    ops.fused_adam_(b["w"], b["m"], b["v"], grads[1].clone(), chunks, groups, b["step"],
                    grad_scale=torch.full((1,), 0.5, device=cuda))
    ops.fused_adam_(c["w"], c["m"], c["v"], grads[1] * 0.5, chunks, groups, c["step"])
    for k in b:
        assert torch.equal(b[k], c[k]), k
    # zero_grad=False keeps the gradient; no shadow is written unless asked for
    g = grads[2].clone()
    ops.fused_adam_(c["w"], c["m"], c["v"], g, chunks, groups, c["step"], zero_grad=False)
    assert torch.equal(g, grads[2])


def test_fused_adam_device_step_eager_and_graph_replay(cuda):
    from gaussiank_sgd_amd import ops
    st, grads, chunks, groups = _state(cuda)
    for want in (1.0, 2.0):            # no host-supplied count: the kernel pair keeps it
        ops.fused_adam_(st["w"], st["m"], st["v"], grads[int(want) - 1].clone(), chunks, groups, st["step"])
        assert float(st["step"]) == want
    eager = _clone(st)
    for t in range(2, 5):
        ops.fused_adam_(eager["w"], eager["m"], eager["v"], grads[t].clone(), chunks, groups, eager["step"])
    gbuf = torch.zeros(ac.TOTAL, device=cuda)
    scratch = _clone(st)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):         # eager warm-up outside the capture, on state the comparison does not use
        ops.fused_adam_(scratch["w"], scratch["m"], scratch["v"], gbuf, chunks, groups, scratch["step"])
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # tick + update, one stream
        ops.fused_adam_(st["w"], st["m"], st["v"], gbuf, chunks, groups, st["step"])
    assert float(st["step"]) == 2.0, "capturing must not run the step"
    for t in range(2, 5):
        gbuf.copy_(grads[t])
        graph.replay()
    torch.cuda.synchronize()
    assert float(st["step"]) == 5.0
    for k in st:
        assert torch.equal(st[k], eager[k]), "%s: 3 replays differ from 3 eager calls" % k


def test_graphed_step_adamw_trains(cuda):
    """The setup of tests/test_graph_gpu.py under AdamW: one capture, every replay moves the weights,
    the device step count equals warm-ups + replays."""
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm, install_bf16_shadow
    from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer
    from gaussiank_sgd_amd.train import DLTrainer
    from gaussiank_sgd_amd.train.graph import GraphedStep
    comm.init()
    t = DLTrainer(0, 1, dnn="resnet20", dataset="cifar10", batch_size=16, lr=1e-3, device="cuda", amp="bf16",
                  channels_last=True, data_pool=1, seed=0, optimizer="adamw")
    opt = DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                               compression=compressors["gaussian"], is_sparse=True, density=0.01,
                               compress_single_rank=True, density_warmup=False)
    assert opt._fused_kind == "adam"
    install_bf16_shadow(t.net, opt)
    t.update_optimizer(opt)
    t.display = 10 ** 9
    step = GraphedStep(t, opt)
    step()                                  # warm-up + capture + first replay
    w_prev = opt.arena.weights.clone()
    losses = []
    for _ in range(6):
        step()
        torch.cuda.synchronize()
        losses.append(t.current_loss())
        w = opt.arena.weights
        assert (w - w_prev).abs().max().item() > 0, "a replay did not update the weights"
        w_prev = w.clone()
    assert step.captures == 1, "unexpected re-capture"
    assert float(opt._adam_step) == step.warmup + step.replays == 10.0
    assert all(torch.isfinite(torch.tensor(l)) for l in losses), losses
    assert torch.equal(opt.arena.shadow, opt.arena.weights.to(torch.bfloat16))


def test_loopback_two_ranks_topk_adamw_on_one_gpu(cuda):
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import comm
    from gaussiank_sgd_amd.parallel import distributed_optimizer as hvd
    from gaussiank_sgd_amd.train import DLTrainer
    compressors["topk"].clear()
    trainers = []
    for r in range(2):
        torch.manual_seed(0)
        trainers.append(DLTrainer(r, 2, dnn="fcn5net", dataset="mnist", batch_size=16, lr=1e-3, nworkers=2,
                                  device="cuda", learnable_data=True, seed=r, optimizer="adamw"))

    def body(r):
        torch.cuda.set_device(0)
        t = trainers[r]
        opt = hvd.DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                                       compression=compressors["topk"], is_sparse=True, density=0.05,
                                       density_warmup=False)
        assert opt._fused_kind == "adam"
        hvd.broadcast_parameters(t.net.state_dict(), root_rank=0)
        t.update_optimizer(opt)
        w0 = opt.arena.weights.clone()
        for _ in range(3):
            opt.zero_grad()
            t.train(1)
            t.update_model()
        torch.cuda.synchronize()
        a = opt.arena
        assert float(opt._adam_step) == 3.0 and not torch.equal(a.weights, w0)
        return a.weights.cpu(), a.momentum.cpu(), a.second_moment.cpu()

    r0, r1 = comm.loopback_world(2, body)
    for x, y, name in zip(r0, r1, ("weights", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), "replicas diverged: %s" % name
