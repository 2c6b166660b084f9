"""Key-padding masks in the fused attention kernels (csrc/kernels/attn.hip and
attn_f32.hip, MASK instantiations) against PyTorch references with the
kernels' own dropout mask: an all-valid mask is bitwise the unmasked call;
right padding, holes (an empty first tile, a sequence with one valid key), a
whole wave of masked keys, an empty sequence (defined as zeros), the BERT
layer against its SDPA path, and determinism.  bf16 against the fp32
composition at the tolerances of test_attention_gpu.py, fp32 against fp64 at
those of test_attention_f32_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
PS = [0.0, 0.1]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from gaussiank_sgd_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load(), ops._load_error


def _qkv(B, T, heads, seed, dtype):
    torch.manual_seed(seed)
    return torch.randn(B, T, 3 * heads * 64, device="cuda").to(dtype).contiguous()


def _dout(B, T, heads, dtype):
    torch.manual_seed(99)
    return torch.randn(B, T, heads * 64, device="cuda").to(dtype)


def _lengths_mask(lengths, T):
    return torch.arange(T, device="cuda")[None, :] < torch.tensor(lengths, device="cuda")[:, None]


def _raw(qkv, heads, p, seed, bits, dout, fill=None, lo=True):
    """The raw ops: out, lse [B, heads, T], dqkv.  ``fill``: pre-fill of out and dqkv.
    ``lo``: with a mask, the bf16 ops get the out_lo buffer (the output's rounding
    residue, for delta), as ops.attention does."""
    B, T, _ = qkv.shape
    f32 = qkv.dtype == torch.float32
    fwd, bwd = (torch.ops.gksgd.attn_f32_fwd, torch.ops.gksgd.attn_f32_bwd) if f32 else \
        (torch.ops.gksgd.attn_fwd, torch.ops.gksgd.attn_bwd)
    out = torch.empty(B, T, heads * 64, dtype=qkv.dtype, device="cuda")
    dqkv = torch.empty_like(qkv)
    if fill is not None:
        out.fill_(fill)
        dqkv.fill_(fill)
    lse = torch.empty(B * heads * T, device="cuda")
    if f32 or bits is None or not lo:
        fwd(qkv, out, lse, heads, p, seed, None, bits)
        bwd(qkv, out, dout, lse, torch.empty_like(lse), dqkv, heads, p, seed, None, bits)
    else:
        out_lo = torch.full_like(out, float("nan"))
        fwd(qkv, out, lse, heads, p, seed, None, bits, out_lo)
        assert not torch.isnan(out_lo).any()
        assert (out_lo.float().abs() <= 2.0 ** -8 * out.float().abs() + 1e-30).all()   # below half an ulp of out
        bwd(qkv, out, dout, lse, torch.empty_like(lse), dqkv, heads, p, seed, None, bits, out_lo)
    return out, lse.view(B, heads, T), dqkv


def _reference(qkv, heads, p, seed, m, dout):
    """out, lse (log2 units, over valid keys), dqkv, and the bound on the lse
    error: the fp32 composition (ops.attention.reference_attention) for bf16
    inputs, fp64 for fp32 ones.

    The lse bound.  fp32: the 1e-4 of test_attention_f32_gpu.py.  bf16: the
    4e-3 of test_attention_gpu.py for every sequence with at least 128 valid
    keys (the fewest that test has).  That figure relies on the score errors
    averaging out over the keys; a row with one or a few valid keys has nothing
    to average, so shorter sequences get the worst case per row instead: the
    kernels round the pre-scaled query c q (c = log2(e) / 8) to bf16 once more,
    a relative error of at most 2^-9 per element, so a score is off by at most
    2^-9 c sum_d |q_d k_d|, and a log-sum-exp moves by no more than the largest
    score error among its (valid) keys; plus 1e-4 for the fp32 accumulation."""
    from gaussiank_sgd_amd.ops import attention
    B, T, _ = qkv.shape
    if qkv.dtype == torch.float32:
        x = qkv.double().requires_grad_(True)
        v5 = x.view(B, T, 3, heads, 64)
        q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
        s = (torch.matmul(q, k.transpose(-1, -2)) / 8.0).masked_fill(~m[:, None, None, :], float("-inf"))
        a = torch.softmax(s, dim=-1)
        if p > 0:
            a = a * attention.dropout_mask(B, heads, T, p, seed, "cuda").to(a.dtype) * attention.drop_scale(p)
        ref = torch.matmul(a, v).transpose(1, 2).reshape(B, T, heads * 64)
        ref.backward(dout.double())
        lse_tol = 1e-4
    else:
        x = qkv.float().requires_grad_(True)
        ref = attention.reference_attention(x, heads, p, seed, key_mask=m)
        ref.backward(dout.float())
        v5 = x.detach().view(B, T, 3, heads, 64)
        s = (torch.einsum("bqhd,bkhd->bhqk", v5[:, :, 0], v5[:, :, 1]) / 8.0).masked_fill(
            ~m[:, None, None, :], float("-inf"))
        ab = torch.einsum("bqhd,bkhd->bhqk", v5[:, :, 0].abs(), v5[:, :, 1].abs())
        ab = ab.masked_fill(~m[:, None, None, :], 0.0)
        lse_tol = 2.0 ** -9 * (math.log2(math.e) / 8.0) * ab.amax(dim=-1) + 1e-4
        lse_tol = torch.where((m.sum(-1) >= 128)[:, None, None], torch.full_like(lse_tol, 4e-3), lse_tol)
    lse = torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)
    return ref.detach(), lse, x.grad, lse_tol


def _check(got, want, heads):
    """Forward, lse and dQ / dK / dV at the unmasked tests' tolerances (q scale 1)."""
    out, lse, dqkv = got
    ref, lse_ref, gref, lse_tol = want
    f32 = out.dtype == torch.float32
    B, T = out.shape[0], out.shape[1]
    err = (out.to(ref.dtype) - ref).abs().max().item()
    print("fwd err", err, "ref max", ref.abs().max().item())
    assert err <= (2e-5 if f32 else 2e-2) * max(1.0, ref.abs().max().item()), err
    dl = (lse.to(lse_ref.dtype) - lse_ref).abs()
    print("lse err", dl.max().item(), "largest err / bound", (dl / lse_tol).max().item())
    assert bool((dl <= lse_tol).all()), (dl.max().item(), (dl / lse_tol).max().item())
    g = dqkv.to(gref.dtype).view(B, T, 3, heads, 64)
    gr = gref.view(B, T, 3, heads, 64)
    for i, name in enumerate("qkv"):
        e = (g[:, :, i] - gr[:, :, i]).abs().max().item()
        scale = gr[:, :, i].abs().max().item()
        print("d" + name, "err", e, "scale", scale)
        assert e <= ((1e-4 * scale + 1e-5) if f32 else (2.5e-2 * scale + 1e-3)), (name, e, scale)


def _masked_kv_zero(dqkv, m, heads):
    B, T = m.shape
    g = dqkv.view(B, T, 3, heads, 64)
    return bool((g[:, :, 1:][~m] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_key_mask_gpu_matches_cpu(dtype):
    from gaussiank_sgd_amd.ops import attention
    torch.manual_seed(5)
    m = torch.rand(3, 256, device="cuda") < 0.6
    want = attention.pack_key_mask(m.cpu())
    for src in (m, m.to(torch.int64) * 5, m.to(torch.int32), m.to(dtype) * -2.0, m.to(torch.uint8)):
        bits = attention.pack_key_mask(src)
        assert bits.dtype == torch.int32 and bits.is_cuda
        assert torch.equal(bits.cpu(), want)
    assert torch.equal(attention.unpack_key_mask(attention.pack_key_mask(m), 256), m)
    # -0.0 is zero, T = 32 is one word
    z = torch.full((2, 32), -0.0, device="cuda", dtype=dtype)
    z[1, 31] = 1.0
    assert attention.pack_key_mask(z).tolist() == [[0], [-(1 << 31)]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_all_valid_mask_is_the_unmasked_call(dtype, p):
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 2, 256, 2
    qkv, dout = _qkv(B, T, heads, 11, dtype), _dout(B, T, heads, dtype)
    bits = attention.pack_key_mask(torch.ones(B, T, device="cuda"))
    a = _raw(qkv, heads, p, 321, None, dout)
    b = _raw(qkv, heads, p, 321, bits, dout, lo=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # with out_lo the forward is the same; delta, and with it the gradients, only get more exact
    c = _raw(qkv, heads, p, 321, bits, dout)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    want = _reference(qkv, heads, p, 321, torch.ones(B, T, dtype=torch.bool, device="cuda"), dout)
    _check(c, want, heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_right_padding(dtype, p):
    """Lengths 129 (one key into the third tile), 64 (a tile edge; the second
    dK/dV workgroup is all padding), 37 (inside the first tile, across a wave)."""
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 4, 256, 2
    qkv, dout = _qkv(B, T, heads, 21, dtype), _dout(B, T, heads, dtype)
    m = _lengths_mask([256, 129, 64, 37], T)
    want = _reference(qkv, heads, p, 777, m, dout)
    got = _raw(qkv, heads, p, 777, attention.pack_key_mask(m), dout, fill=float("nan"))
    _check(got, want, heads)
    assert _masked_kv_zero(got[2], m, heads)
    # the public op (autograd, a [B, T] mask of another dtype) gives the same bits
    x = qkv.clone().requires_grad_(True)
    out = attention.self_attention(x, heads, p, True, seed=777, key_mask=m.to(torch.int64))
    out.backward(dout)
    assert torch.equal(out, got[0]) and torch.equal(x.grad, got[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_holes(dtype, p):
    """An empty first tile (the ring wraps at 6 tiles) plus a 30% scatter of
    masked keys; the other sequence keeps only its last key.

    The one-key sequence has P = 1, so dS = dP - delta must cancel exactly: its
    true dQ and dK are 0.  With delta = rowsum(dO * O) taken from the bf16
    output alone and p = 0.1, O = bf16(v / (1 - p)) leaves about 2^-9 |dO| |v|
    per query, which the 384 queries add up to 0.089 in dK (scale 0.83, bound
    0.022); the out_lo residue of the forward is what removes it."""
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 2, 384, 1
    qkv, dout = _qkv(B, T, heads, 31, dtype), _dout(B, T, heads, dtype)
    g = torch.Generator(device="cuda").manual_seed(7)
    m = torch.rand(B, T, device="cuda", generator=g) >= 0.3
    m[0, :64] = False
    m[1] = False
    m[1, 383] = True
    want = _reference(qkv, heads, p, 55, m, dout)
    got = _raw(qkv, heads, p, 55, attention.pack_key_mask(m), dout, fill=float("nan"))
    _check(got, want, heads)
    assert _masked_kv_zero(got[2], m, heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,heads", [(1, 2), (2, 2), (2, 4)])
def test_grid_classes(B, heads, dtype):
    """The workgroup -> (batch, head, row block) mapping (attn_common.h) at T = 256, two row blocks per
    (batch, head): a grid of 4 (not a multiple of 8: no XCD remap), of 8 and of 16 (the remap).  A block
    computed twice leaves another one's NaN pre-fill.  Keys 64..127 (a whole tile) masked, the last sequence
    right-padded too; p = 0.1, so the hash index follows the mapping as well.
    test_attention_causal_gpu.py::test_causal_grid_classes is the causal twin."""
    from gaussiank_sgd_amd.ops import attention
    T, p = 256, 0.1
    qkv, dout = _qkv(B, T, heads, 61, dtype), _dout(B, T, heads, dtype)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    m[:, 64:128] = False
    m[-1, 200:] = False
    got = _raw(qkv, heads, p, 91, attention.pack_key_mask(m), dout, fill=float("nan"))
    _check(got, _reference(qkv, heads, p, 91, m, dout), heads)
    assert _masked_kv_zero(got[2], m, heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_masked_keys_dkv_are_written(dtype, p):
    """T = 128: one workgroup per head, keys 32..63 (a whole wave) masked."""
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 1, 128, 2
    qkv, dout = _qkv(B, T, heads, 41, dtype), _dout(B, T, heads, dtype)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    m[:, 32:64] = False
    out, lse, dqkv = _raw(qkv, heads, p, 9, attention.pack_key_mask(m), dout, fill=float("nan"))
    assert not torch.isnan(out).any() and not torch.isnan(dqkv).any()
    assert _masked_kv_zero(dqkv, m, heads)
    _check((out, lse, dqkv), _reference(qkv, heads, p, 9, m, dout), heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_empty_sequence(dtype, p):
    """No valid key: out = 0, finite lse, zero gradients; the other sequence is unaffected."""
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 2, 128, 2
    qkv, dout = _qkv(B, T, heads, 51, dtype), _dout(B, T, heads, dtype)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    m[1] = False
    out, lse, dqkv = _raw(qkv, heads, p, 13, attention.pack_key_mask(m), dout, fill=float("nan"))
    for x in (out, lse, dqkv):
        assert torch.isfinite(x).all()
    assert (out[1] == 0).all() and (dqkv[1] == 0).all()
    # batch element 0 alone (same dropout hashes: bh = b * heads + h) against the reference
    want = _reference(qkv[:1], heads, p, 13, m[:1], dout[:1])
    _check((out[:1], lse[:1], dqkv[:1]), want, heads)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bert_layer_key_mask_matches_sdpa(dtype):
    from gaussiank_sgd_amd.models.bert import BertConfig, BertLayer
    from gaussiank_sgd_amd.ops import attention
    torch.manual_seed(0)
    c = BertConfig(hidden=256, heads=4, intermediate=512, dropout=0.0)
    layer = BertLayer(c).cuda().eval()
    x = torch.randn(2, 256, 256, device="cuda")
    m = _lengths_mask([256, 100], 256)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        assert attention.fused_available(layer.qkv(x), 4)
        y = layer(x, key_mask=m)
        y2 = layer(x, attn_mask=m[:, None, None, :])   # the SDPA path
        y3 = layer(x, key_mask=attention.pack_key_mask(m))
    assert torch.equal(y, y3)
    d = (y.float() - y2.float()).abs()
    tol = 5e-2 if dtype == torch.bfloat16 else 1e-4   # the existing fused-vs-SDPA layer tests' bounds
    print("valid rows", d[m].max().item(), "all rows", d.max().item())
    assert d[m].max().item() <= tol
    assert d.max().item() <= tol   # padded queries are computed too


@pytest.mark.parametrize("dtype", DTYPES)
def test_bert_model_packs_attention_mask(dtype):
    """BertForMaskedLM hands the packed bits to every layer: same logits as the
    layers called with the [B, T] mask, close to the SDPA-mask path."""
    from gaussiank_sgd_amd.models import bert
    torch.manual_seed(0)
    model = bert.BertForMaskedLM(bert.BertConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256,
                                                 max_position=128, dropout=0.0)).cuda().eval()
    ids = torch.randint(0, 512, (2, 128), device="cuda")
    m = _lengths_mask([128, 50], 128).to(torch.int64)
    calls = []
    orig = bert.attention.pack_key_mask
    bert.attention.pack_key_mask = lambda t: calls.append(1) or orig(t)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            out = model(ids, attention_mask=m)
    finally:
        bert.attention.pack_key_mask = orig
    assert len(calls) == 1   # packed once per forward
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        x = model.emb_drop(model.emb_ln(bert.bert_embeddings(
            ids, None, model.word_embeddings, model.position_embeddings, model.token_type_embeddings)))
        for layer in model.encoder:
            x = layer(x, attn_mask=m[:, None, None, :].bool())
        want = bert.vocab_projection(model.mlm_ln(model.mlm_dense(x, act="gelu")), model.word_embeddings.weight,
                                     model.mlm_bias)
    # the layers agree within 5e-2 (bf16) / 1e-4 (fp32), the bounds of the layer tests; the head -- a
    # LayerNorm and a projection on 128 weights of std 0.02 -- does not amplify that, and 1e-3 leaves the
    # fp32 GEMMs a decade of room
    assert (out.float() - want.float()).abs().max().item() <= (5e-2 if dtype == torch.bfloat16 else 1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_masked_deterministic(dtype, p):
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 2, 256, 2
    qkv, dout = _qkv(B, T, heads, 3, dtype), _dout(B, T, heads, dtype)
    g = torch.Generator(device="cuda").manual_seed(1)
    m = torch.rand(B, T, device="cuda", generator=g) < 0.6
    bits = attention.pack_key_mask(m)
    a = _raw(qkv, heads, p, 42, bits, dout)
    b = _raw(qkv, heads, p, 42, bits, dout)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_pack_and_masked_forward_in_graph_capture():
    """pack_key_mask reads nothing back: it records into a graph with the masked
    forward, and a replay sees the mask's new contents."""
    from gaussiank_sgd_amd.ops import attention
    B, T, heads = 2, 128, 1
    qkv = _qkv(B, T, heads, 61, torch.bfloat16)
    mask = torch.ones(B, T, device="cuda")
    attention.self_attention(qkv, heads, 0.0, key_mask=mask)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention.self_attention(qkv, heads, 0.0, key_mask=mask)
    mask[1, 40:] = 0
    graph.replay()
    torch.cuda.synchronize()
    want = attention.reference_attention(qkv, heads, key_mask=mask)
    assert (out.float() - want).abs().max().item() <= 2e-2 * max(1.0, want.abs().max().item())
