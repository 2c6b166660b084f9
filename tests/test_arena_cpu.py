"""The pure-torch fallbacks of fused SGD, momentum correction and LARS on the
ragged chunk table of tests/arena_cases.py.  On the CPU the cases compare a
fallback with itself, so their numeric comparisons say nothing here; what these
tests check is that nothing beyond a chunk's length is touched, that gradients
are zeroed and that the shadow follows w.  The GPU tests run the same cases to
compare the HIP kernels with these fallbacks."""
import arena_cases as arc


def test_fused_sgd_fallback_ragged_lengths():
    arc.run_sgd("cpu")


def test_momentum_correct_fallback_ragged_lengths():
    arc.run_momentum_correct("cpu")


def test_lars_fallback_ragged_lengths():
    assert arc.run_lars("cpu") == 0.0
