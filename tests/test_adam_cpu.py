"""Fused Adam / AdamW on the CPU: the pure-torch fallback of ``ops.fused_adam_``
and its integration into ``DistributedOptimizer`` (arena state, state_dict
round trips with plain torch optimizers, compressed exchange, trainer, CLI).

Tolerance: tests/adam_cases.py -- ours against torch's fp64 optimizer within
2x torch's own fp32-vs-fp64 difference, for w, exp_avg and exp_avg_sq."""
import copy

import pytest
import torch

import adam_cases as ac
from gaussiank_sgd_amd import ops
from gaussiank_sgd_amd.parallel import comm
from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer


@pytest.mark.parametrize("variant,sparse", ac.CASES, ids=ac.CASE_IDS)
def test_fused_adam_fallback_vs_torch(variant, sparse):
    pad = ac.padding_mask()

    def on_step(t, w, m, v, g, step, shadow):
        assert not g.any()
        assert torch.equal(shadow, w.to(torch.bfloat16))
        assert not w[pad].any() and not m[pad].any() and not v[pad].any()

    ac.run_case(variant, sparse, ac.STEPS_MAX, "cpu", with_shadow=True, on_step=on_step)


@pytest.mark.parametrize("variant", list(ac.VARIANTS))
def test_fused_adam_fallback_ragged_lengths(variant):
    """Chunk lengths that are no multiple of 4 (nor of 64): the public op takes them."""
    ac.run_ragged(variant, False, 3, "cpu")


def test_fused_adam_rejects_non_positive_eps():
    """eps = 0 would turn the all-zero padding slots into 0 / 0: refused on every path."""
    w = torch.zeros(64)
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=0.0, weight_decay=0.0, decoupled=True)]
    with pytest.raises(ValueError, match="eps"):
        ops.fused_adam_(w, w.clone(), w.clone(), w.clone(), ops.make_chunk_table([(0, 64, 0, 0)], "cpu"), groups,
                        torch.zeros(()))
    net = _mlp()
    ow = DistributedOptimizer(torch.optim.AdamW(net.parameters(), lr=1e-3, eps=0.0),
                              named_parameters=net.named_parameters(), compression="none")
    assert ow._fused_kind is None       # torch's own update, which has no padding


def test_fused_adam_fallback_scalars():
    """lr_mult = 0 freezes w while the moments and the step advance; grad_scale = 0.5 halves the gradient."""
    w0, grads, _, _ = ac.reference("adamw", False)
    chunks, groups = ac.chunk_table("cpu"), ac.groups_for("adamw")

    def run(g, **kw):
        w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
        step = torch.zeros((), dtype=torch.float32)
        ops.fused_adam_(w, m, v, g.clone(), chunks, groups, step, **kw)
        return w, m, v, float(step)

    w, m, v, s = run(grads[0], lr_mult=torch.zeros(1))
    assert torch.equal(w, w0) and m.any() and v.any() and s == 1.0
    a = run(grads[0], grad_scale=torch.full((1,), 0.5))
    b = run(grads[0] * 0.5)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ---------------------------------------------------------------------------
# DistributedOptimizer(torch.optim.AdamW)
# ---------------------------------------------------------------------------
def _mlp(dtype=torch.float32):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(20, 37), torch.nn.Tanh(), torch.nn.Linear(37, 29), torch.nn.Tanh(),
                              torch.nn.Linear(29, 5))
    return net.to(dtype)


def _adamw(net):
    decay = [p for p in net.parameters() if p.dim() > 1]
    rest = [p for p in net.parameters() if p.dim() <= 1]
    return torch.optim.AdamW([{"params": decay, "weight_decay": 0.05}, {"params": rest, "weight_decay": 0.0}],
                             lr=2e-3, betas=(0.9, 0.99), eps=1e-8, foreach=False)


def _batches(n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(16, 20, generator=gen), torch.randn(16, 5, generator=gen)) for _ in range(n)]


def _train(net, opt, batches):
    dtype = next(net.parameters()).dtype
    for x, y in batches:
        opt.zero_grad()
        ((net(x.to(dtype)) - y.to(dtype)) ** 2).mean().backward()
        opt.step()


def _snapshot(net, opt):
    ps = list(net.parameters())
    cat = lambda ts: torch.cat([t.detach().reshape(-1).double() for t in ts])   # noqa: E731
    return {"w": cat(ps), "m": cat([opt.state[p]["exp_avg"] for p in ps]),
            "v": cat([opt.state[p]["exp_avg_sq"] for p in ps])}


def _check(label, ours, plain32, plain64):
    s64 = _snapshot(*plain64)
    s32 = _snapshot(*plain32)
    ac.check_step(label, _snapshot(*ours), s64, s32)


def _wrap(net):
    return DistributedOptimizer(_adamw(net), named_parameters=net.named_parameters(), compression="none")


def test_wrapped_adamw_matches_plain_and_state_dict_round_trips():
    first, more = _batches(5), _batches(3, seed=12)
    n32, n64, nw = _mlp(), _mlp(torch.float64), _mlp()
    o32, o64 = _adamw(n32), _adamw(n64)
    ow = _wrap(nw)
    assert ow._fused_kind == "adam"
    _train(n32, o32, first)
    _train(n64, o64, first)
    _train(nw, ow, first)
    _check("wrapped, 5 steps", (nw, ow), (n32, o32), (n64, o64))
    arena = ow.arena
    for p in nw.parameters():
        st = ow.state[p]
        key = ow._parameter_names[p]
        assert st["exp_avg"].data_ptr() == arena.view_of(arena.momentum, key).data_ptr()
        assert st["exp_avg_sq"].data_ptr() == arena.view_of(arena.second_moment, key).data_ptr()
        assert st["step"].data_ptr() == ow._adam_step.data_ptr()
    assert float(ow._adam_step) == 5.0

    # wrapped -> a fresh plain AdamW on a copy of the wrapped model (through a deep copy, as a checkpoint would)
    sd = copy.deepcopy(ow.state_dict())
    steps = [st["step"] for st in sd["state"].values()]
    assert len({s.data_ptr() for s in steps}) == len(steps) and all(float(s) == 5.0 for s in steps)
    np_ = _mlp()
    np_.load_state_dict(copy.deepcopy(nw.state_dict()))
    op = _adamw(np_)
    op.load_state_dict(sd)
    # plain -> wrapped: a model copy of the plain fp32 run, wrapped, loading the plain state
    nq = _mlp()
    nq.load_state_dict(copy.deepcopy(n32.state_dict()))
    oq = _wrap(nq)
    oq.load_state_dict(copy.deepcopy(o32.state_dict()))
    assert oq._fused_kind == "adam" and float(oq._adam_step) == 5.0
    for net, opt in ((n32, o32), (n64, o64), (nw, ow), (np_, op), (nq, oq)):
        _train(net, opt, more)
    assert float(ow._adam_step) == 8.0 and float(oq._adam_step) == 8.0
    _check("wrapped, 8 steps", (nw, ow), (n32, o32), (n64, o64))
    _check("wrapped -> plain, 5 + 3 steps", (np_, op), (n32, o32), (n64, o64))
    _check("plain -> wrapped, 5 + 3 steps", (nq, oq), (n32, o32), (n64, o64))


def test_state_handed_in_through_the_factory_is_adopted():
    batches = _batches(4)
    n32, n64, nw = _mlp(), _mlp(torch.float64), _mlp()
    o32, o64, op = _adamw(n32), _adamw(n64), _adamw(nw)
    _train(n32, o32, batches[:2])
    _train(n64, o64, batches[:2])
    _train(nw, op, batches[:2])
    ow = DistributedOptimizer(op, named_parameters=nw.named_parameters(), compression="none")
    _train(n32, o32, batches[2:])
    _train(n64, o64, batches[2:])
    _train(nw, ow, batches[2:])
    assert ow._fused_kind == "adam" and float(ow._adam_step) == 4.0
    _check("factory hand-in, 2 + 2 steps", (nw, ow), (n32, o32), (n64, o64))


def test_differing_step_counts_keep_the_unfused_update():
    nw = _mlp()
    op = _adamw(nw)
    _train(nw, op, _batches(2))
    op.state[next(iter(nw.parameters()))]["step"] += 3
    ow = DistributedOptimizer(op, named_parameters=nw.named_parameters(), compression="none")
    _train(nw, ow, _batches(1))
    assert ow._fused_kind is None
    assert sorted({float(st["step"]) for st in ow.state.values()}) == [3.0, 6.0]
    # state at one step count, loaded later, returns to the fused update
    n2 = _mlp()
    o2 = _adamw(n2)
    _train(n2, o2, _batches(2))
    ow.load_state_dict(copy.deepcopy(o2.state_dict()))
    assert ow._fused_kind == "adam" and float(ow._adam_step) == 2.0
    _train(nw, ow, _batches(1))
    assert ow._fused_kind == "adam" and float(ow._adam_step) == 3.0


def test_amsgrad_keeps_the_unfused_update():
    nw = _mlp()
    ow = DistributedOptimizer(torch.optim.AdamW(nw.parameters(), lr=1e-3, amsgrad=True),
                              named_parameters=nw.named_parameters(), compression="none")
    assert ow._fused_kind is None


def test_adam_decoupled_flag():
    for cls, kw, want in ((torch.optim.AdamW, {}, True), (torch.optim.Adam, {}, False),
                          (torch.optim.Adam, {"decoupled_weight_decay": True}, True)):
        if kw and "decoupled_weight_decay" not in torch.optim.Adam([torch.zeros(1)]).defaults:
            continue
        nw = _mlp()
        ow = DistributedOptimizer(cls(nw.parameters(), lr=1e-3, weight_decay=0.1, **kw),
                                  named_parameters=nw.named_parameters(), compression="none")
        assert ow._fused_kind == "adam"
        assert all(ow._adam_decoupled(g) == want for g in ow.param_groups)


# ---------------------------------------------------------------------------
# compressed exchange + Adam
# ---------------------------------------------------------------------------
def test_loopback_topk_adamw_replicas_identical_and_equal_dense_adamw():
    """Two virtual ranks, top-k at density 0.05: every step equals a plain ``torch.optim.AdamW`` applied by
    hand to ``aggregated_grads()`` (fp32 and fp64 copies fed the same aggregate: the rule of
    tests/adam_cases.py), and the replicas stay bit-identical."""
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import distributed_optimizer as hvd
    from gaussiank_sgd_amd.train import DLTrainer
    compressors["topk"].clear()
    trainers = []
    for r in range(2):
        torch.manual_seed(0)
        trainers.append(DLTrainer(r, 2, dnn="fcn5net", dataset="mnist", batch_size=16, lr=1e-3, nworkers=2,
                                  device="cpu", learnable_data=True, seed=r, optimizer="adamw"))

    def body(r):
        t = trainers[r]
        opt = hvd.DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                                       compression=compressors["topk"], is_sparse=True, density=0.05,
                                       density_warmup=False)
        assert opt._fused_kind == "adam"
        hvd.broadcast_parameters(t.net.state_dict(), root_rank=0)
        t.update_optimizer(opt)
        a = opt.arena
        params = [p for g in opt.param_groups for p in g["params"]]
        hand = {}
        for dtype in (torch.float32, torch.float64):     # plain torch AdamW on copies, same param groups
            copies = {p: p.detach().to(dtype).clone().requires_grad_(True) for p in params}
            hopt = torch.optim.AdamW([dict({k: v for k, v in g.items() if k != "params"},
                                           params=[copies[p] for p in g["params"]]) for g in opt.param_groups],
                                     foreach=False)
            hand[dtype] = (copies, hopt)

        def snap(ws, state_of):
            cat = lambda ts: torch.cat([x.detach().reshape(-1).double() for x in ts])   # noqa: E731
            return {"w": cat(ws), "m": cat([state_of(i)["exp_avg"] for i in range(len(ws))]),
                    "v": cat([state_of(i)["exp_avg_sq"] for i in range(len(ws))])}

        for i in range(4):
            opt.zero_grad()
            t.train(1)
            opt.synchronize()
            agg = opt.aggregated_grads()
            nz = int((agg != 0).sum())
            assert 0 < nz <= 0.25 * a.total, "the aggregate of two top-5 %% selections must be sparse (%d)" % nz
            for dtype, (copies, hopt) in hand.items():
                for hg, g in zip(hopt.param_groups, opt.param_groups):
                    hg["lr"] = g["lr"]                 # the trainer's schedule sets it every step
                for p in params:
                    copies[p].grad = p.grad.detach().to(dtype).clone()    # p.grad: a view of the aggregate
                hopt.step()
            t.update_model()
            refs = [snap([c[p] for p in params], lambda k, c=c, o=o: o.state[c[params[k]]])
                    for c, o in (hand[torch.float64], hand[torch.float32])]
            ac.check_step("rank %d step %d" % (r, i + 1), snap(params, lambda k: opt.state[params[k]]), *refs)
        assert float(opt._adam_step) == 4.0
        return a.weights.clone(), a.residuals.clone()

    (w0, r0), (w1, r1) = comm.loopback_world(2, body)
    assert torch.equal(w0, w1), "replicas diverged"
    assert not torch.equal(r0, r1)          # error feedback stays per rank


def test_momentum_correction_with_adamw_raises():
    from gaussiank_sgd_amd.compression import compressors
    net = _mlp()
    with pytest.raises(ValueError, match="momentum_correction"):
        DistributedOptimizer(_adamw(net), named_parameters=net.named_parameters(),
                             compression=compressors["gaussian"], is_sparse=True, density=0.01,
                             compress_single_rank=True, momentum_correction=True)


# ---------------------------------------------------------------------------
# trainer and CLI
# ---------------------------------------------------------------------------
def test_cli_and_trainer_accept_adamw():
    from gaussiank_sgd_amd.train import DLTrainer, dist_trainer, single
    for mod in (dist_trainer, single):
        args = mod.build_parser().parse_args(["--optimizer", "adamw", "--adam-beta1", "0.8", "--adam-beta2", "0.95",
                                              "--adam-eps", "1e-6", "--weight-decay", "0.02"])
        assert (args.optimizer, args.adam_beta1, args.adam_beta2, args.adam_eps, args.weight_decay) == \
            ("adamw", 0.8, 0.95, 1e-6, 0.02)
        assert mod.build_parser().parse_args([]).optimizer == "sgd"
    t = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer="adamw", betas=(0.8, 0.95),
                  adam_eps=1e-6, weight_decay=0.02)
    assert type(t.optimizer) is torch.optim.AdamW
    assert [g["weight_decay"] for g in t.optimizer.param_groups] == [0.0, 0.02]
    assert all(g["betas"] == (0.8, 0.95) and g["eps"] == 1e-6 for g in t.optimizer.param_groups)
    assert all(p.dim() == 1 for p in t.optimizer.param_groups[0]["params"])
    assert all(p.dim() > 1 for p in t.optimizer.param_groups[1]["params"])
    d = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer="adam")
    assert type(d.optimizer) is torch.optim.Adam and d.optimizer.param_groups[1]["weight_decay"] == 1e-4
    s = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu")
    assert type(s.optimizer) is torch.optim.SGD and s.optimizer.param_groups[1]["weight_decay"] == 1e-4
    with pytest.raises(ValueError):
        DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", device="cpu", optimizer="lamb")
