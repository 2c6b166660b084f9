"""Selection-quality metrics on the GPU: the HIP kernels of
ops/csrc/kernels/quality.hip after a HIP ops.compress_, against the in-test
fp64 reference (tests/selection_quality_cases.py: integer fields exactly,
energies to relative 1e-5), and the DistributedOptimizer sampling on one GPU."""
import pytest
import torch

import selection_quality_cases as sq
from gaussiank_sgd_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dist", ["normal", "t"])
@pytest.mark.parametrize("n", sq.SIZES)
def test_topk_record(cuda, n, dist):
    sq.case_topk(cuda, n, dist)


@pytest.mark.parametrize("mode", [ops.MODE_GAUSSIAN, ops.MODE_GAUSSIAN_CAL])
@pytest.mark.parametrize("dist", ["normal", "t"])
@pytest.mark.parametrize("n", sq.SIZES)
def test_gaussian_records(cuda, n, dist, mode):
    sq.case_gaussian(cuda, n, dist, mode)


@pytest.mark.parametrize("more", [False, True])
def test_ties_at_kth_magnitude(cuda, more):
    sq.case_ties(cuda, more)


@pytest.mark.parametrize("mode", [ops.MODE_TOPK, ops.MODE_GAUSSIAN])
def test_third_radix_pass(cuda, mode):
    sq.case_low_bits(cuda, mode)


@pytest.mark.parametrize("mode", [ops.MODE_TOPK, ops.MODE_GAUSSIAN])
def test_all_zero(cuda, mode):
    sq.case_all_zero(cuda, mode)


@pytest.mark.parametrize("mode", [ops.MODE_TOPK, ops.MODE_THRESHOLD])
def test_fewer_than_k_nonzeros(cuda, mode):
    sq.case_few_nonzeros(cuda, mode)


@pytest.mark.parametrize("n", [100, sq.N_RAGGED])
def test_empty_record(cuda, n):
    sq.case_empty_record(cuda, n)


@pytest.mark.parametrize("extra", [0, 50])
def test_k_at_least_n(cuda, extra):
    sq.case_k_ge_n(cuda, extra)


def test_second_call_same_buffers(cuda):
    sq.case_second_call(cuda)


def test_unaligned_slice(cuda):
    """A residual slice that starts 4 bytes past a 16-byte boundary (scalar head
    and tail around the float4 body)."""
    n = sq.N_RAGGED
    k = sq.k_for(n)
    x, r = sq.pair(n, seed=17, dist="t")
    bufs = ops.CompressBuffers(k, cuda)
    base = torch.zeros(n + 8, device=cuda)
    rs = base[1:1 + n]
    assert rs.data_ptr() % 16 == 4
    rs.copy_(r)
    ops.compress_(x.to(cuda), rs, bufs, ops.MODE_TOPK, ec=True, zero_g=True, k=k, k_cap=k)
    out = torch.zeros(8, dtype=torch.float64, device=cuda)
    ops.selection_quality_(rs, bufs.record, k, k, out)
    sq.check(ops.quality_fields(out, k), sq.reference(rs.cpu(), bufs.record.cpu(), k, k))


@pytest.mark.parametrize("comp", ["topk", "gaussian"])
def test_optimizer_sampling_one_gpu(cuda, comp):
    steps, every = 6, 2
    rows, state, nb, opt = sq.optimizer_run("cuda", comp, every, steps)
    sq.check_rows(rows, nb, every, steps, comp)
    assert all("quality_ws" in b.extra for b in opt.arena.buckets)
    rows0, state0, nb0, opt0 = sq.optimizer_run("cuda", comp, 0, steps)
    # sampling off: no rows, nothing allocated; arena and records bit-identical
    assert rows0 == [] and opt0._q_dev is None and not any("quality_ws" in b.extra for b in opt0.arena.buckets)
    assert nb0 == nb and sq.states_equal(state, state0)
    # the sampled rows match the reference on the final step's buffers when it was sampled
    # (steps - 1 is odd: not sampled), so re-score the last records by hand
    for b in opt.arena.buckets:
        k_cap = min(opt._compression.k_cap_for(opt._compression.k_of(b.numel, 0.01), b.numel), b.bufs.k_cap)
        k = max(int(opt._compression.k_of(b.numel, 0.01)), 1)
        out = torch.zeros(8, dtype=torch.float64, device=cuda)
        r = b.slice(opt.arena.residuals)
        ops.selection_quality_(r, b.bufs.record, k, k_cap, out, b.extra["quality_ws"])
        sq.check(ops.quality_fields(out, k_cap), sq.reference(r.cpu(), b.bufs.record.cpu(), k, k_cap))
