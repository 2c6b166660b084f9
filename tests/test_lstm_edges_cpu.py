"""The cases of tests/lstm_cases.py without a GPU: the step-GEMM scenarios through the torch mirrors (slice by
slice, K batch by K batch, in the kernel's precision), the cell scenarios through ``_cell_fwd_ref`` /
``_cell_bwd_ref`` of ops/lstm.py.  The fp64 references, the bounds and the case table hold before a GPU is
involved (the HIP kernels: tests/test_lstm_edges_gpu.py)."""
import pytest
import torch

import lstm_cases as lc

CPU = torch.device("cpu")
CDS = pytest.mark.parametrize("cd", [lc.F32, lc.BF16], ids=["fp32", "bf16"])
KINDS = pytest.mark.parametrize("kind", lc.KINDS)


def test_case_table_reaches_every_variant():
    lc.assert_case_table()


def test_dispatch_mirror_by_hand():
    """Three slice depths worked out by hand from the ladders of lstm_rec_gemm* (a batch is D steps of 32 bf16
    or 16 fp32 K elements)."""
    # ks = 64: no multiple of 128 -> bf16 D = 2 (64 deep: 1 trip), fp32 D = 4 (64 deep: 1 trip)
    assert [lc.rec_variant(k, 64) for k in lc.KINDS] == [(2, 1), (4, 1), (2, 1)]
    # ks = 384 = 3 * 128: bf16 D = 4 (128 deep: 3 trips), fp32 D = 8 (128 deep: 3 trips), x6 64 deep: 6 trips
    assert [lc.rec_variant(k, 384) for k in lc.KINDS] == [(4, 3), (8, 3), (2, 6)]
    # ks = 512 = 2 * 256: bf16 D = 8 (256 deep: 2 trips), fp32 D = 8 (128 deep: 4 trips), x6: 8 trips
    assert [lc.rec_variant(k, 512) for k in lc.KINDS] == [(8, 2), (8, 4), (2, 8)]
    with pytest.raises(AssertionError):
        lc.rec_variant("bf16", 96)


@KINDS
def test_gemm_exact(kind):
    lc.scenario_gemm_exact(CPU, kind)


@KINDS
def test_gemm_random(kind):
    lc.scenario_gemm_random(CPU, kind)


@KINDS
def test_gemm_strided(kind):
    lc.scenario_gemm_strided(CPU, kind)


@KINDS
def test_gemm_refusals(kind):
    lc.scenario_gemm_refusals(CPU, kind)


@CDS
def test_cell_forward(cd):
    lc.scenario_cell_fwd(CPU, cd)


@CDS
def test_cell_backward(cd):
    lc.scenario_cell_bwd(CPU, cd)


@CDS
def test_cell_saturation(cd):
    lc.scenario_cell_saturation(CPU, cd)


def test_splits_and_forced_step_plan(monkeypatch):
    """``_splits`` and the forced-rule branch of ``_step_plan`` over H in 1 .. 2048: S divides the 64-block
    count of K, the padded operands satisfy the binding's K % (64 S) == 0, and S > 1 leaves every slice at
    least two blocks deep.  The last assertion holds ``_step_plan`` against the same ``_splits`` call, so it pins
    only the batch threshold (hipBLASLt above it) and which block counts and target each direction passes."""
    from gaussiank_sgd_amd.ops import lstm as L
    monkeypatch.setitem(L.SPLITK_MAX_BATCH, "fwd", 256)
    monkeypatch.setitem(L.SPLITK_MAX_BATCH, "bwd", 128)
    for H in range(1, 2049):
        Hp = lc.pad64(H)
        for B in (1, 20, 128, 129, 300):
            mb = -(-B // 128)
            for direction, K, N, target, mx in (("fwd", Hp, 4 * Hp, 512, 256), ("bwd", 4 * Hp, Hp, 256, 128)):
                kb = K // 64
                S = L._splits(kb, (N // 64) * mb, target=target)
                assert S >= 1 and kb % S == 0 and K % (64 * S) == 0, (direction, H, B, S)
                assert S == 1 or (kb // S >= 2 and S * (N // 64) * mb <= target), (direction, H, B, S)
                plan = L._step_plan(direction, torch.float32, B, H, CPU)
                assert plan == (("hip", S) if B <= mx else ("blas", 0)), (direction, H, B, plan)
