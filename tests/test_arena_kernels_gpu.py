"""The chunk-streaming HIP kernels of ops/csrc/kernels/optim.hip beside fused
Adam and LAMB (fused SGD, momentum correction, the LARS norms and update) on
chunk lengths that end in the scalar tail (tests/arena_cases.py), and the
bindings' checks of malformed input."""
import pytest
import torch

import arena_cases as arc
from gaussiank_sgd_amd import ops

pytestmark = pytest.mark.gpu


def test_fused_sgd_ragged_lengths(cuda):
    arc.run_sgd(cuda)


def test_momentum_correct_ragged_lengths(cuda):
    arc.run_momentum_correct(cuda)


def test_lars_ragged_lengths(cuda):
    """Largest relative error of segmented_sumsq against the float64 sums of the same weights, measured on an
    MI355X: 1.4e-8 and 7.6e-8 (bound 1.19e-6, derived in arena_cases.py); see profiles/optim_refactor_ab.txt."""
    arc.run_lars(cuda)


def test_lars_and_momentum_correct_reject_malformed_input(cuda):
    n = 256
    w, m, g = (torch.zeros(n, device=cuda) for _ in range(3))
    chunks = ops.make_chunk_table([(0, n, 0, 0)], cuda)
    ss = torch.ones(2, dtype=torch.float64, device=cuda)
    lars = dict(lr=[0.1], momentum=[0.9], weight_decay=[0.0], eeta=[1e-3], epsilon=[1e-5])
    ops._ops().fused_lars(w, m, g, chunks, ss, *lars.values())
    with pytest.raises(RuntimeError, match="one entry per group"):
        ops._ops().fused_lars(w, m, g, chunks, ss, *dict(lars, eeta=[]).values())
    with pytest.raises(RuntimeError, match="size mismatch"):
        ops._ops().fused_lars(w, m[:128], g, chunks, ss, *lars.values())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops._ops().fused_lars(w[1:], m[1:], g[1:], chunks, ss, *lars.values())
    with pytest.raises(RuntimeError, match="param groups"):
        ops._ops().momentum_correct(m, g, w, chunks, 0, 1, [0.9, 0.9], [0.0])
    with pytest.raises(RuntimeError, match="size mismatch"):
        ops._ops().momentum_correct(m[:128], g, w, chunks, 0, 1, [0.9], [0.0])
    assert not w.any() and not m.any() and not g.any()
