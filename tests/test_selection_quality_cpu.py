"""Selection-quality metrics: the pure-torch mirror of ops.selection_quality_
against the in-test fp64 reference (tests/selection_quality_cases.py), the
DistributedOptimizer sampling in a two-rank loopback world and the
dist_trainer flag / metrics keys."""
import json
import os

import pytest
import torch

import selection_quality_cases as sq
from gaussiank_sgd_amd import ops
from gaussiank_sgd_amd.parallel import comm

CPU = "cpu"


@pytest.mark.parametrize("dist", ["normal", "t"])
@pytest.mark.parametrize("n", sq.SIZES)
def test_topk_record(n, dist):
    sq.case_topk(CPU, n, dist)


@pytest.mark.parametrize("mode", [ops.MODE_GAUSSIAN, ops.MODE_GAUSSIAN_CAL])
@pytest.mark.parametrize("dist", ["normal", "t"])
@pytest.mark.parametrize("n", sq.SIZES)
def test_gaussian_records(n, dist, mode):
    sq.case_gaussian(CPU, n, dist, mode)


@pytest.mark.parametrize("more", [False, True])
def test_ties_at_kth_magnitude(more):
    sq.case_ties(CPU, more)


@pytest.mark.parametrize("mode", [ops.MODE_TOPK, ops.MODE_GAUSSIAN])
def test_third_radix_pass(mode):
    sq.case_low_bits(CPU, mode)


@pytest.mark.parametrize("mode", [ops.MODE_TOPK, ops.MODE_GAUSSIAN])
def test_all_zero(mode):
    sq.case_all_zero(CPU, mode)


@pytest.mark.parametrize("mode", [ops.MODE_TOPK, ops.MODE_THRESHOLD])
def test_fewer_than_k_nonzeros(mode):
    sq.case_few_nonzeros(CPU, mode)


@pytest.mark.parametrize("n", [100, sq.N_RAGGED])
def test_empty_record(n):
    sq.case_empty_record(CPU, n)


@pytest.mark.parametrize("extra", [0, 50])
def test_k_at_least_n(extra):
    sq.case_k_ge_n(CPU, extra)


def test_second_call_same_buffers():
    sq.case_second_call(CPU)


# ---------------------------------------------------------------------------
# DistributedOptimizer: two loopback ranks on fcn5net
# ---------------------------------------------------------------------------
STEPS = 6


def _loopback(comp, every):
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel import distributed_optimizer as hvd
    from gaussiank_sgd_amd.train import DLTrainer
    compressors[comp].clear()
    P = 2
    trainers = []
    for r in range(P):          # built serially: model init draws from the global RNG
        torch.manual_seed(0)
        trainers.append(DLTrainer(r, P, dnn="fcn5net", dataset="mnist", batch_size=32, lr=0.5, nworkers=P,
                                  device="cpu", learnable_data=True, seed=r))

    def body(r):
        t = trainers[r]
        opt = hvd.DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                                       compression=compressors[comp], is_sparse=True, density=0.01,
                                       density_warmup=False, threshold=10_000, selection_quality_every=every)
        hvd.broadcast_parameters(t.net.state_dict(), root_rank=0)
        t.update_optimizer(opt)
        t.base_lr = 0.5
        for _ in range(STEPS):
            opt.zero_grad()
            t.train(1)
            t.update_model()
        arena = opt.arena
        state = (arena.weights.detach().clone(), arena.residuals.detach().clone(),
                 [b.bufs.record.detach().clone() for b in arena.buckets])
        return opt.collect_selection_quality(), state, len(arena.buckets), opt._q_dev is None

    return comm.loopback_world(P, body)


@pytest.mark.parametrize("comp", ["topk", "gaussian"])
def test_loopback_optimizer_sampling(comp):
    on = _loopback(comp, 2)
    off = _loopback(comp, 0)
    for (rows, state, nb, unallocated), (rows0, state0, nb0, unallocated0) in zip(on, off):
        sq.check_rows(rows, nb, 2, STEPS, comp)
        assert not unallocated
        # sampling off: no rows, nothing allocated, and the training is bit-identical
        assert rows0 == [] and unallocated0 and nb0 == nb
        assert sq.states_equal(state, state0)


def test_env_default(monkeypatch):
    monkeypatch.setenv("GKSGD_SELECTION_QUALITY_EVERY", "3")
    from gaussiank_sgd_amd.compression import compressors
    from gaussiank_sgd_amd.parallel.distributed_optimizer import DistributedOptimizer
    from gaussiank_sgd_amd.train import DLTrainer
    comm.init()
    t = DLTrainer(0, 1, dnn="fcn5net", dataset="mnist", batch_size=8, lr=0.05, device="cpu", learnable_data=True)

    def mk(**kw):
        return DistributedOptimizer(t.optimizer, named_parameters=t.net.named_parameters(),
                                    compression=compressors["gaussian"], is_sparse=True, density=0.01,
                                    compress_single_rank=True, density_warmup=False, **kw)
    assert mk()._quality_every == 3
    assert mk(selection_quality_every=0)._quality_every == 0
    monkeypatch.delenv("GKSGD_SELECTION_QUALITY_EVERY")
    assert mk()._quality_every == 0


# ---------------------------------------------------------------------------
# dist_trainer: flag and metrics keys
# ---------------------------------------------------------------------------
QUALITY_KEYS = {"record_occupancy", "topk_overlap", "energy_captured", "energy_fraction", "compression_ratio_used"}


def test_dist_trainer_flag_parses():
    from gaussiank_sgd_amd.train import dist_trainer
    p = dist_trainer.build_parser()
    assert p.parse_args([]).selection_quality_every is None
    assert p.parse_args(["--selection-quality-every", "5"]).selection_quality_every == 5


@pytest.mark.parametrize("every", [2, 0])
def test_dist_trainer_metrics_keys(tmp_path, every, monkeypatch):
    from gaussiank_sgd_amd.train import dist_trainer
    monkeypatch.delenv("GKSGD_SELECTION_QUALITY_EVERY", raising=False)
    comm.init()
    # 5 iterations per epoch: one metrics line per epoch (at i == 4)
    dist_trainer.ssgd("fcn5net", "mnist", str(tmp_path), 1, 0.05, 8, 1, 1, 1, None, 35, "gaussian", 0.01, 10_000,
                      density_warmup=False, compress_single_rank=True, saved_dir=str(tmp_path),
                      metrics_dir=str(tmp_path), train_samples=40, max_iters=5, selection_quality_every=every)
    lines = [json.loads(s) for s in open(os.path.join(str(tmp_path), "metrics-rank0.jsonl")) if s.strip()]
    assert lines, "no metrics line written"
    for d in lines:
        if every:
            assert QUALITY_KEYS <= set(d), sorted(d)
            assert 0.0 < d["topk_overlap"] <= 1.0 and d["compression_ratio_used"] > 0.0
        else:
            assert not (QUALITY_KEYS & set(d)), sorted(d)
