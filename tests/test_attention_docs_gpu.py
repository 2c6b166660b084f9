"""Document masks of packed sequences in the fused causal attention kernels
(csrc/kernels/attn_docs.hip, attn_f32_docs.hip: the DOC instantiations): query
q sees key k iff start[q] <= k <= q.  bf16 against the fp32 composition, fp32
against fp64 with the kernels' own dropout mask, at the tolerances (and with
the helpers) of test_attention_causal_gpu.py; outputs pre-filled with NaN."""
import math

import pytest
import torch

import test_attention_causal_gpu as causal
from test_attention_causal_gpu import B, HEADS, _check, _dout, _qkv

pytestmark = pytest.mark.gpu
both = lambda f: pytest.mark.parametrize("dtype", causal.DTYPES)(pytest.mark.parametrize("p", causal.PS)(f))   # noqa: E731
# document starts of the two sequences.  0: boundaries on tile edges (row block 1 never visits tiles 0, 1; the wave
# at query 192 skips tile 2).  1: one-token documents at both ends, a boundary inside a wave's 32 rows, row 128
# still in the document from 70 (t_lo = 1).  2: a document over three key blocks (dK/dV: key block 0 stops after
# query tile 4, its wave 0 after tile 1) against two documents.  3: layout 1 under right padding (key bits).
LAYOUTS = [(256, [0, 64, 128, 192], [0, 128], [256, 256]), (256, [0, 1, 70, 129, 255], [0, 33, 200], [256, 256]),
           (384, [0, 100, 300], [0, 383], [384, 384]), (256, [0, 1, 70, 129, 255], [0, 33, 200], [256, 200])]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from gaussiank_sgd_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load(), ops._load_error


def _ids(T, *starts):
    ids = torch.zeros(len(starts), T, dtype=torch.int64, device="cuda")
    for b, st in enumerate(starts):
        for s in st[1:]:
            ids[b, s:] += 1
    return ids


def _seg(T, *starts):
    from gaussiank_sgd_amd.ops import attention
    return attention.pack_segments(_ids(T, *starts))


def _raw(qkv, p, seed, seg, dout, bits=None):
    """The raw ops, causal, on NaN-filled outputs: out, lse [B, heads, T], dqkv."""
    T, f32, ops = qkv.shape[1], qkv.dtype == torch.float32, torch.ops.gksgd
    out = torch.full((B, T, HEADS * 64), float("nan"), dtype=qkv.dtype, device="cuda")
    dqkv = torch.full_like(qkv, float("nan"))
    lse, delta = torch.empty(B * HEADS * T, device="cuda"), torch.empty(B * HEADS * T, device="cuda")
    lo = () if f32 else (torch.empty_like(out),)
    fwd, bwd = (ops.attn_f32_fwd, ops.attn_f32_bwd) if f32 else (ops.attn_fwd, ops.attn_bwd)
    fwd(qkv, out, lse, HEADS, p, seed, None, bits, *lo, True, seg)
    bwd(qkv, out, dout, lse, delta, dqkv, HEADS, p, seed, None, bits, *lo, True, seg)
    return out, lse.view(B, HEADS, T), dqkv


def _reference(qkv, p, seed, seg, dout, m):
    """What test_attention_causal_gpu._reference returns, under the document mask ``seg`` and key mask ``m``: the
    lse bound is that file's, a row's visible keys now being those of its document (q - start[q] + 1)."""
    from gaussiank_sgd_amd.ops import attention
    T, f32 = qkv.shape[1], qkv.dtype == torch.float32
    vis = attention.segments_visible(seg)[:, None] & m[:, None, None, :]
    x = (qkv.double() if f32 else qkv.float()).requires_grad_(True)
    ref = attention.reference_attention(x, HEADS, p, seed, key_mask=m, causal=True, segments=seg)
    ref.backward(dout.to(x.dtype))
    q, k = (x.detach().view(B, T, 3, HEADS, 64)[:, :, i].transpose(1, 2) for i in range(2))
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, float("-inf"))
    lse = (torch.logsumexp(s, dim=-1) / math.log(2.0)).nan_to_num(neginf=0.0)   # 0 for a row that sees nothing
    tol = 2.0 ** -9 * (math.log2(math.e) / 8.0) * (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(~vis, 0.0).amax(-1) + 1e-4
    tol = torch.where((vis.sum(-1) >= 128).expand_as(tol), torch.full_like(tol, 4e-3), tol)
    return ref.detach(), lse, x.grad, torch.full_like(tol, 1e-4) if f32 else tol, None


@both
@pytest.mark.parametrize("T,a,b,lengths", LAYOUTS)
def test_layouts(T, a, b, lengths, p, dtype):
    from gaussiank_sgd_amd.ops import attention
    qkv, dout, seg, m = _qkv(T, 300 + T, dtype), _dout(T, dtype), _seg(T, a, b), causal._lengths_mask(lengths, T)
    got = _raw(qkv, p, 4242, seg, dout, None if min(lengths) == T else attention.pack_key_mask(m))
    _check(got, _reference(qkv, p, 4242, seg, dout, m))
    assert bool((got[2].view(B, T, 3, HEADS, 64)[:, :, 1:][~m] == 0).all())   # dK / dV of masked keys


@pytest.mark.parametrize("dtype", causal.DTYPES)
def test_no_leak_between_documents_bitwise(dtype):
    T, starts = 256, [0, 70, 129, 256]
    qkv, dout, seg = _qkv(T, 7, dtype), _dout(T, dtype), _seg(T, starts[:-1], starts[:-1])
    base = _raw(qkv, 0.0, 1, seg, dout)
    torch.manual_seed(8)
    big = (torch.randint(0, 2, qkv.shape, device="cuda").float() * 2e3 - 1e3).to(dtype)
    for lo, hi in zip(starts, starts[1:]):
        x = big.clone()
        x[:, lo:hi] = qkv[:, lo:hi]
        out, lse, _ = _raw(x, 0.0, 1, seg, dout)
        assert torch.equal(out[:, lo:hi], base[0][:, lo:hi]) and torch.equal(lse[:, :, lo:hi], base[1][:, :, lo:hi])


@both
def test_public_op(p, dtype):
    from gaussiank_sgd_amd.ops import attention
    T, a, b, _ = LAYOUTS[1]
    qkv, dout = _qkv(T, 13, dtype), _dout(T, dtype)
    want = _raw(qkv, p, 4242, _seg(T, a, b), dout)
    x = qkv.clone().requires_grad_(True)
    out = attention.self_attention(x, HEADS, p, True, seed=4242, causal=True, segments=_ids(T, a, b))
    out.backward(dout)
    assert torch.equal(out, want[0]) and torch.equal(x.grad, want[2])
    with pytest.raises(ValueError):
        attention.self_attention(x, HEADS, p, True, segments=_ids(T, a, b))
    # one document per sequence is causal=True without segments, bit for bit
    got, want = _raw(qkv, p, 9, _seg(T, [0], [0]), dout), causal._raw(qkv, p, 9, None, dout)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("dtype", causal.DTYPES)
def test_layout_is_data_in_a_captured_graph(dtype):
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv, dout, seg = _qkv(T, 61, dtype).requires_grad_(True), _dout(T, dtype), _seg(T, [0, 64, 128, 192], [0, 128])

    def step():
        out = attention.self_attention(qkv, HEADS, 0.0, causal=True, segments=seg)
        return out, torch.autograd.grad(out, qkv, dout)[0]

    step()   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, g = step()
    seg.copy_(_seg(T, [0, 1, 70, 129, 255], [0, 33, 200]))
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    want_out, want_g = step()
    assert torch.equal(out, want_out) and torch.equal(g, want_g)


@pytest.mark.parametrize("dtype", causal.DTYPES)
def test_gpt_tiny_matches_sdpa(dtype, monkeypatch):
    from gaussiank_sgd_amd.models import create_net
    from gaussiank_sgd_amd.ops import attention
    torch.manual_seed(0)
    model = create_net(0, "gpt_tiny")[0].cuda().eval()
    T, bf16 = 256, dtype == torch.bfloat16
    ids, labels = torch.randint(0, 1024, (2, B, T), device="cuda")
    docs, calls = _ids(T, [0, 70, 129], [0, 128, 200]), []

    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            logits = model(ids, doc_ids=docs)
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(logits.float().view(-1, 1024), labels.view(-1)).backward()
        return logits.detach().float(), {n: q.grad.float() for n, q in model.named_parameters()}

    for fn in (attention._FlashAttnFn, attention._FlashAttnF32Fn):
        monkeypatch.setattr(fn, "apply", lambda *a, f=fn.apply: (calls.append(a[-1].shape), f(*a))[1])
    fused, gf = run()
    assert calls == [(B, 2, T)] * 2    # both blocks took the fused path
    monkeypatch.setattr(attention, "fused_available", lambda *a: False)
    sdpa, gs = run()
    assert len(calls) == 2
    tol = 5e-2 if bf16 else 1e-4   # test_attention_causal_gpu.py's fused-vs-SDPA bounds
    assert (fused - sdpa).abs().max().item() <= tol
    for n in gf:
        assert (gf[n] - gs[n]).abs().max().item() <= tol * max(1.0, gs[n].abs().max().item()), n
