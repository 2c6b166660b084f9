"""Fused LAMB HIP kernels (ops/csrc/kernels/optim.hip: lamb_moments_kernel,
lamb_trust_kernel, lamb_apply_kernel) and their users on the GPU: the cases of
tests/lamb_cases.py (numerics within 2x a plain implementation's own
fp32-vs-fp64 difference, trust ratios within a relative 2e-5, padding, ragged
lengths through the scalar tail, degenerate tensors, zero_grad=False, the
device scalars), bit-identical repeat runs and group-id permutations, the
device-side step count under HIP-graph replays, and ``optim.LAMB`` inside
``DistributedOptimizer`` (tests/test_lamb_cpu.py holds the bodies).

Largest err / yardstick ratios measured on an MI355X: see
profiles/fused_lamb_kernels.txt."""
import pytest
import torch

import lamb_cases as lc
import test_lamb_cpu as cpu_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant,sparse", lc.CASES, ids=lc.CASE_IDS)
def test_fused_lamb_vs_plain(cuda, variant, sparse):
    """The arena's layout: (1000, 64) spans 4 chunks, so its ratio combines the partials of 4 workgroups;
    (7,) is 7 elements plus 57 padding slots."""
    lc.case_yardstick(variant, sparse, cuda)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse1pct"])
def test_fused_lamb_without_adapt_is_adamw(cuda, sparse):
    lc.case_noadapt_is_adamw(sparse, cuda)


def test_fused_lamb_degenerate_tensors(cuda):
    lc.case_degenerate(cuda)


@pytest.mark.parametrize("variant,sparse", lc.CASES, ids=lc.CASE_IDS)
def test_fused_lamb_ragged_lengths_run_the_scalar_tail(cuda, variant, sparse):
    lc.case_ragged(variant, sparse, cuda)


def test_fused_lamb_zero_grad_false(cuda):
    lc.case_zero_grad_false(cuda)


def test_fused_lamb_device_scalars(cuda):
    lc.case_device_scalars(cuda)


def test_fused_lamb_is_deterministic(cuda):
    """No atomics: repeat runs and permuted group ids are bit-identical in w, m, v and the ratios."""
    lc.case_determinism(cuda)


def test_fused_lamb_device_step_under_graph_replay(cuda):
    """One captured step (tick, moments, trust, apply on one stream) replayed on a refilled static
    gradient buffer: replays 2 to 4 equal eager steps 2 to 4, so the bias corrections follow the device count."""
    w0, grads = lc.inputs(False)
    groups = lc.VARIANTS["mixed"]
    eager, graphed, scratch = lc.State(w0, cuda), lc.State(w0, cuda), lc.State(w0, cuda)
    for st in (eager, graphed):
        st.run(grads[0].clone().to(cuda), groups)
    for t in range(1, 4):
        eager.run(grads[t].clone().to(cuda), groups)
    gbuf = torch.zeros(lc.ac.TOTAL, device=cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):         # eager warm-up outside the capture, on state the comparison does not use
        scratch.run(gbuf, groups)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.run(gbuf, groups)
    assert float(graphed.step) == 1.0, "capturing must not run the step"
    for t in range(1, 4):
        gbuf.copy_(grads[t])
        graph.replay()
    torch.cuda.synchronize()
    assert float(graphed.step) == 4.0
    for k, x in eager.tensors().items():
        assert torch.equal(x, graphed.tensors()[k]), "%s: replays 2-4 differ from eager steps 2-4" % k


def test_wrapped_lamb_matches_plain_and_state_dict_round_trips(cuda):
    cpu_cases.wrapped_lamb_round_trip("cuda")


def test_lamb_differing_step_counts_keep_the_unfused_update(cuda):
    cpu_cases.differing_step_counts("cuda")


def test_loopback_gaussian_lamb_replicas_identical(cuda):
    cpu_cases.loopback_gaussian_replicas("cuda")


def test_wrapped_lamb_writes_the_bf16_shadow(cuda):
    nw = cpu_cases.mlp(device="cuda")
    ow = cpu_cases.wrap(nw)
    shadow = ow._ensure_shadow()
    cpu_cases.train(nw, ow, cpu_cases.batches(3))
    assert ow._fused_kind == "lamb" and float(ow._adam_step) == 3.0
    assert shadow.data_ptr() == ow.arena.shadow.data_ptr() and shadow.any()
    assert torch.equal(ow.arena.shadow, ow.arena.weights.to(torch.bfloat16))
