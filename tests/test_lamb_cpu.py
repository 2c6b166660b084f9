"""Fused LAMB on the CPU: the pure-torch fallback of ``ops.fused_lamb_`` (the
rules themselves: tests/lamb_cases.py), the workspace validation, ``optim.LAMB``
inside ``DistributedOptimizer`` (arena state, trust_ratios(), state_dict round
trips with a plain LAMB, differing step counts, compressed exchange), the
trainer and both CLIs.

Tolerance: tests/lamb_cases.py -- ours against a plain fp64 implementation
within 2x the same implementation's fp32-vs-fp64 difference for w, exp_avg and
exp_avg_sq; trust ratios within a relative 2e-5 of the fp64 run."""
import copy

import pytest
import torch

import adam_cases as ac
import lamb_cases as lc
from gaussiank_sgd_amd import ops
from gaussiank_sgd_amd.optim import LAMB
from gaussiank_sgd_amd.parallel import comm
from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer


@pytest.mark.parametrize("variant,sparse", lc.CASES, ids=lc.CASE_IDS)
def test_fused_lamb_fallback_vs_plain(variant, sparse):
    lc.case_yardstick(variant, sparse, "cpu")


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse1pct"])
def test_fused_lamb_fallback_without_adapt_is_adamw(sparse):
    lc.case_noadapt_is_adamw(sparse, "cpu")


def test_fused_lamb_fallback_degenerate_tensors():
    lc.case_degenerate("cpu")


@pytest.mark.parametrize("variant,sparse", lc.CASES, ids=lc.CASE_IDS)
def test_fused_lamb_fallback_ragged_lengths(variant, sparse):
    lc.case_ragged(variant, sparse, "cpu")


def test_fused_lamb_fallback_zero_grad_false():
    lc.case_zero_grad_false("cpu")


def test_fused_lamb_fallback_device_scalars():
    lc.case_device_scalars("cpu")


def test_fused_lamb_fallback_same_result_under_permuted_group_ids():
    lc.case_determinism("cpu")


def test_lamb_workspace_validation():
    ws = ops.make_lamb_workspace(lc.chunk_table("cpu"), "cpu")
    assert ws.seg_range.dtype == torch.int32 and ws.seg_range.tolist() == [0, 1, 1, 1, 2, 4, 6, 1, 7, 1]
    assert ws.part.dtype == torch.float64 and ws.part.numel() == 2 * 8
    assert ws.trust.dtype == torch.float32 and ws.trust.numel() == 5
    # a segment's chunks interleaved with another's
    table = ops.make_chunk_table([(0, 64, 0, 0), (64, 64, 0, 1), (128, 64, 0, 0)], "cpu")
    with pytest.raises(ValueError, match="consecutive"):
        ops.make_lamb_workspace(table, "cpu")
    # a segment id beyond the 15-bit field: the 16th bit of the id is the word's sign bit
    word = 64 | (1 << 63)
    bad = torch.tensor([0, word - (1 << 64)], dtype=torch.int64)
    with pytest.raises(ValueError, match="15-bit"):
        ops.make_lamb_workspace(bad, "cpu")
    # eps = 0 and a workspace of another table
    w = torch.zeros(64)
    one = ops.make_chunk_table([(0, 64, 0, 0)], "cpu")
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=0.0, weight_decay=0.0, adapt=True, trust_clip=None)]
    with pytest.raises(ValueError, match="eps"):
        ops.fused_lamb_(w, w.clone(), w.clone(), w.clone(), one, groups, torch.zeros(()),
                        ops.make_lamb_workspace(one, "cpu"))
    groups[0]["eps"] = 1e-6
    with pytest.raises(ValueError, match="workspace"):
        ops.fused_lamb_(w, w.clone(), w.clone(), w.clone(), one, groups, torch.zeros(()), ws)
    with pytest.raises(ValueError):
        LAMB([torch.zeros(3, requires_grad=True)], eps=0.0)


# ---------------------------------------------------------------------------
# DistributedOptimizer(LAMB)
# ---------------------------------------------------------------------------
def mlp(dtype=torch.float32, device="cpu"):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(20, 37), torch.nn.Tanh(), torch.nn.Linear(37, 29), torch.nn.Tanh(),
                              torch.nn.Linear(29, 5))
    return net.to(dtype).to(device)


def lamb(net):
    decay = [p for p in net.parameters() if p.dim() > 1]
    rest = [p for p in net.parameters() if p.dim() <= 1]
    return LAMB([{"params": decay, "weight_decay": 0.05, "adapt": True, "trust_clip": 3.0},
                 {"params": rest, "weight_decay": 0.0, "adapt": False}], lr=2e-3, betas=(0.9, 0.99), eps=1e-6)


def batches(n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(16, 20, generator=gen), torch.randn(16, 5, generator=gen)) for _ in range(n)]


def train(net, opt, data):
    p0 = next(net.parameters())
    for x, y in data:
        opt.zero_grad()
        ((net(x.to(p0)) - y.to(p0)) ** 2).mean().backward()
        opt.step()


def snapshot(net, opt):
    ps = list(net.parameters())
    cat = lambda ts: torch.cat([t.detach().reshape(-1).double().cpu() for t in ts])   # noqa: E731
    return {"w": cat(ps), "m": cat([opt.state[p]["exp_avg"] for p in ps]),
            "v": cat([opt.state[p]["exp_avg_sq"] for p in ps])}


def check(label, ours, plain32, plain64):
    ac.check_step(label, snapshot(*ours), snapshot(*plain64), snapshot(*plain32))


def wrap(net, **kw):
    return DistributedOptimizer(lamb(net), named_parameters=net.named_parameters(), compression="none", **kw)


def wrapped_lamb_round_trip(device):
    """5 steps against LAMB.step() on plain fp32 / fp64 copies, trust_ratios(), then the state through
    state_dict() into a plain LAMB and a plain LAMB's state into a wrapped one, 3 more steps each."""
    first, more = batches(5), batches(3, seed=12)
    # the plain copies live on the same device, so that every run's gradients come from the same GEMMs
    n32, n64, nw = mlp(device=device), mlp(torch.float64, device), mlp(device=device)
    o32, o64 = lamb(n32), lamb(n64)
    ow = wrap(nw)
    assert ow._fused_kind == "lamb"
    train(n32, o32, first)
    train(n64, o64, first)
    train(nw, ow, first)
    check("wrapped LAMB, 5 steps", (nw, ow), (n32, o32), (n64, o64))
    arena = ow.arena
    for p in nw.parameters():
        st = ow.state[p]
        key = ow._parameter_names[p]
        assert st["exp_avg"].data_ptr() == arena.view_of(arena.momentum, key).data_ptr()
        assert st["exp_avg_sq"].data_ptr() == arena.view_of(arena.second_moment, key).data_ptr()
        assert st["step"].data_ptr() == ow._adam_step.data_ptr()
    assert float(ow._adam_step) == 5.0
    ratios = ow.trust_ratios()
    assert sorted(ratios) == sorted(n for n, _ in nw.named_parameters())
    for name, p in nw.named_parameters():
        r = ratios[name]
        assert r.dim() == 0 and r.dtype == torch.float32 and r.device == p.device
        if p.dim() <= 1:
            assert float(r) == 1.0, "the no-adapt group"
        else:
            assert 0.0 < float(r) <= 3.0 and float(r) != 1.0

    sd = copy.deepcopy(ow.state_dict())
    steps = [st["step"] for st in sd["state"].values()]
    assert len({s.data_ptr() for s in steps}) == len(steps) and all(float(s) == 5.0 for s in steps)
    np_ = mlp(device=device)
    np_.load_state_dict(copy.deepcopy(nw.state_dict()))
    op = lamb(np_)
    op.load_state_dict(sd)
    nq = mlp(device=device)
    nq.load_state_dict(copy.deepcopy(n32.state_dict()))
    oq = wrap(nq)
    oq.load_state_dict(copy.deepcopy(o32.state_dict()))
    assert oq._fused_kind == "lamb" and float(oq._adam_step) == 5.0
    for net, opt in ((n32, o32), (n64, o64), (nw, ow), (np_, op), (nq, oq)):
        train(net, opt, more)
    assert float(ow._adam_step) == 8.0 and float(oq._adam_step) == 8.0
    check("wrapped LAMB, 8 steps", (nw, ow), (n32, o32), (n64, o64))
    check("wrapped -> plain LAMB, 5 + 3 steps", (np_, op), (n32, o32), (n64, o64))
    check("plain -> wrapped LAMB, 5 + 3 steps", (nq, oq), (n32, o32), (n64, o64))


def differing_step_counts(device):
    nw = mlp(device=device)
    op = lamb(nw)
    train(nw, op, batches(2))
    op.state[next(iter(nw.parameters()))]["step"] += 3
    ow = DistributedOptimizer(op, named_parameters=nw.named_parameters(), compression="none")
    train(nw, ow, batches(1))
    assert ow._fused_kind is None
    assert sorted({float(st["step"]) for st in ow.state.values()}) == [3.0, 6.0]
    n2 = mlp()
    o2 = lamb(n2)
    train(n2, o2, batches(2))
    ow.load_state_dict(copy.deepcopy(o2.state_dict()))
    assert ow._fused_kind == "lamb" and float(ow._adam_step) == 2.0
    train(nw, ow, batches(1))
    assert ow._fused_kind == "lamb" and float(ow._adam_step) == 3.0


def loopback_gaussian_replicas(device):
    """Two virtual ranks, the gaussian compressor: the sparse aggregate feeds the dense LAMB passes; the
    replicas' weight arenas stay bit-identical, the residuals stay per rank."""
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import distributed_optimizer as hvd
    from gaussiank_sgd_amd.train import DLTrainer
    compressors["gaussian"].clear()
    trainers = []
    for r in range(2):
        torch.manual_seed(0)
        trainers.append(DLTrainer(r, 2, dnn="fcn5net", dataset="mnist", batch_size=16, lr=1e-3, nworkers=2,
                                  device=device, learnable_data=True, seed=r, optimizer="adamw", trust_ratio=True))

    def body(r):
        if device != "cpu":
            torch.cuda.set_device(0)
        t = trainers[r]
        opt = hvd.DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                                       compression=compressors["gaussian"], is_sparse=True, density=0.05,
                                       density_warmup=False)
        assert opt._fused_kind == "lamb"
        hvd.broadcast_parameters(t.net.state_dict(), root_rank=0)
        t.update_optimizer(opt)
        w0 = opt.arena.weights.clone()
        for _ in range(4):
            opt.zero_grad()
            t.train(1)
            t.update_model()
        a = opt.arena
        assert float(opt._adam_step) == 4.0 and not torch.equal(a.weights, w0)
        ratios = torch.stack(list(opt.trust_ratios().values()))
        assert torch.isfinite(ratios).all() and (ratios != 1.0).any()
        return a.weights.cpu(), a.momentum.cpu(), a.second_moment.cpu(), ratios.cpu(), a.residuals.cpu()

    r0, r1 = comm.loopback_world(2, body)
    for x, y, name in zip(r0[:4], r1[:4], ("weights", "exp_avg", "exp_avg_sq", "trust")):
        assert torch.equal(x, y), "replicas diverged: %s" % name
    assert not torch.equal(r0[4], r1[4])          # error feedback stays per rank


def test_wrapped_lamb_matches_plain_and_state_dict_round_trips():
    wrapped_lamb_round_trip("cpu")


def test_lamb_differing_step_counts_keep_the_unfused_update():
    differing_step_counts("cpu")


def test_loopback_gaussian_lamb_replicas_identical():
    loopback_gaussian_replicas("cpu")


def test_momentum_correction_with_lamb_raises():
    from gaussiank_sgd_amd.compression import compressors
    net = mlp()
    with pytest.raises(ValueError, match="momentum_correction"):
        DistributedOptimizer(lamb(net), named_parameters=net.named_parameters(),
                             compression=compressors["gaussian"], is_sparse=True, density=0.01,
                             compress_single_rank=True, momentum_correction=True)


def test_trust_ratios_needs_lamb():
    net = mlp()
    ow = DistributedOptimizer(torch.optim.AdamW(net.parameters(), lr=1e-3), named_parameters=net.named_parameters(),
                              compression="none")
    with pytest.raises(RuntimeError, match="LAMB"):
        ow.trust_ratios()


# ---------------------------------------------------------------------------
# trainer and CLI
# ---------------------------------------------------------------------------
def test_cli_and_trainer_build_lamb():
    from gaussiank_sgd_amd.train import dist_trainer, single
    for mod in (dist_trainer, single):
        args = mod.build_parser().parse_args(["--optimizer", "adamw", "--trust-ratio", "--trust-clip", "10"])
        assert (args.optimizer, args.trust_ratio, args.trust_clip) == ("adamw", True, 10.0)
        args = mod.build_parser().parse_args(["--optimizer", "adamw"])
        assert args.trust_ratio is False and args.trust_clip is None
        for other in ("sgd", "adam"):
            with pytest.raises(SystemExit):
                mod.build_parser().parse_args(["--optimizer", other, "--trust-ratio"])


def test_cli_error_names_adamw(capsys):
    from gaussiank_sgd_amd.train import dist_trainer
    with pytest.raises(SystemExit):
        dist_trainer.build_parser().parse_args(["--trust-ratio"])
    assert "adamw" in capsys.readouterr().err


def test_trainer_builds_lamb_only_with_the_flag():
    from gaussiank_sgd_amd.train import DLTrainer
    t = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer="adamw", trust_ratio=True,
                  trust_clip=10.0, weight_decay=0.02)
    assert type(t.optimizer) is LAMB
    assert [g["adapt"] for g in t.optimizer.param_groups] == [False, True]
    assert [g["weight_decay"] for g in t.optimizer.param_groups] == [0.0, 0.02]
    assert all(g["trust_clip"] == 10.0 for g in t.optimizer.param_groups)
    assert all(p.dim() == 1 for p in t.optimizer.param_groups[0]["params"])
    d = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer="adamw", trust_ratio=True)
    assert [g["adapt"] for g in d.optimizer.param_groups] == [False, True]
    a = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer="adamw")
    assert type(a.optimizer) is torch.optim.AdamW
    for other in ("sgd", "adam"):
        with pytest.raises(ValueError, match="adamw"):
            DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer=other, trust_ratio=True)
