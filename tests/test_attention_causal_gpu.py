"""Causal masking in the fused attention kernels (csrc/kernels/attn.hip and
attn_f32.hip, CAUSAL instantiations) against PyTorch references with the
kernels' own dropout mask: causal alone at T = 128 / 256 / 384 (one workgroup
with two diagonal tiles; fully visible tiles and the 2- and 4-tile ring
prologues; the 3-slot ring filled and wrapped, the dK/dV loop starting at
tiles 0, 2 and 4), row 0, no look-ahead (bitwise), causal with key masks
(right padding, all-valid, left padding with rows that see nothing, a hole
over a whole tile), causal=False through the new argument, determinism, graph
capture, and the GPT model against its SDPA path.  bf16 against the fp32
composition, fp32 against fp64, at the tolerances of
test_attention_keymask_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
PS = [0.0, 0.1]
B, HEADS = 2, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from gaussiank_sgd_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert ops.load(), ops._load_error


def _qkv(T, seed, dtype, heads=HEADS):
    torch.manual_seed(seed)
    return torch.randn(B, T, 3 * heads * 64, device="cuda").to(dtype).contiguous()


def _dout(T, dtype, heads=HEADS):
    torch.manual_seed(99)
    return torch.randn(B, T, heads * 64, device="cuda").to(dtype)


def _lengths_mask(lengths, T):
    return torch.arange(T, device="cuda")[None, :] < torch.tensor(lengths, device="cuda")[:, None]


def _raw(qkv, p, seed, bits, dout, causal=True, fill=None, new_arg=True, heads=HEADS):
    """The raw ops: out, lse [B, heads, T], dqkv.  ``fill``: pre-fill of out and
    dqkv.  The bf16 ops get out_lo whenever the kernels take it (a key mask or
    causal), as ops.attention does.  ``new_arg=False``: the call without the
    trailing argument (causal must be False)."""
    Bq, T, _ = qkv.shape
    f32 = qkv.dtype == torch.float32
    fwd, bwd = (torch.ops.gksgd.attn_f32_fwd, torch.ops.gksgd.attn_f32_bwd) if f32 else \
        (torch.ops.gksgd.attn_fwd, torch.ops.gksgd.attn_bwd)
    out = torch.empty(Bq, T, heads * 64, dtype=qkv.dtype, device="cuda")
    dqkv = torch.empty_like(qkv)
    if fill is not None:
        out.fill_(fill)
        dqkv.fill_(fill)
    lse = torch.empty(Bq * heads * T, device="cuda")
    delta = torch.empty_like(lse)
    tail = (causal,) if new_arg else ()
    assert new_arg or not causal
    if f32:
        fwd(qkv, out, lse, heads, p, seed, None, bits, *tail)
        bwd(qkv, out, dout, lse, delta, dqkv, heads, p, seed, None, bits, *tail)
    else:
        out_lo = torch.full_like(out, float("nan")) if (bits is not None or causal) else None
        fwd(qkv, out, lse, heads, p, seed, None, bits, out_lo, *tail)
        if out_lo is not None:
            assert not torch.isnan(out_lo).any()
            assert (out_lo.float().abs() <= 2.0 ** -8 * out.float().abs() + 1e-30).all()   # below half an ulp of out
        bwd(qkv, out, dout, lse, delta, dqkv, heads, p, seed, None, bits, out_lo, *tail)
    return out, lse.view(Bq, heads, T), dqkv


def _reference(qkv, p, seed, m, dout, heads=HEADS):
    """out, lse (log2 units, over the row's visible valid keys; 0 for a row
    without one), dqkv, the per-row bound on the lse error, and ``dark`` [B, T]
    (rows without a visible valid key): the fp32 composition
    (ops.attention.reference_attention) for bf16 inputs, fp64 for fp32 ones.

    The lse bound is the one derived in test_attention_keymask_gpu.py, per
    row: fp32 1e-4; bf16 4e-3 for a row with at least 128 visible valid keys
    (the figure relies on the score errors averaging out over the keys), and
    for earlier rows the worst case 2^-9 c max_k sum_d |q_d k_d| + 1e-4 over
    the row's visible valid keys, c = log2(e) / 8 (the kernels round the
    pre-scaled query to bf16 once more)."""
    from gaussiank_sgd_amd.ops import attention
    Bq, T, _ = qkv.shape
    vis = torch.ones(T, T, dtype=torch.bool, device="cuda").tril_()[None, None] & m[:, None, None, :]   # [B,1,T,T]
    dark = ~vis.any(-1)[:, 0]
    if qkv.dtype == torch.float32:
        x = qkv.double().requires_grad_(True)
        v5 = x.view(Bq, T, 3, heads, 64)
        q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
        s = (torch.matmul(q, k.transpose(-1, -2)) / 8.0).masked_fill(~vis, float("-inf"))
        dk = dark[:, None, :, None]
        a = torch.softmax(s.masked_fill(dk, 0.0), dim=-1).masked_fill(dk, 0.0)
        if p > 0:
            a = a * attention.dropout_mask(Bq, heads, T, p, seed, "cuda").to(a.dtype) * attention.drop_scale(p)
        ref = torch.matmul(a, v).transpose(1, 2).reshape(Bq, T, heads * 64)
        ref.backward(dout.double())
        s = s.detach()
        lse_tol = torch.full((Bq, heads, T), 1e-4, device="cuda", dtype=torch.float64)
    else:
        x = qkv.float().requires_grad_(True)
        ref = attention.reference_attention(x, heads, p, seed, key_mask=m, causal=True)
        ref.backward(dout.float())
        v5 = x.detach().view(Bq, T, 3, heads, 64)
        s = (torch.einsum("bqhd,bkhd->bhqk", v5[:, :, 0], v5[:, :, 1]) / 8.0).masked_fill(~vis, float("-inf"))
        ab = torch.einsum("bqhd,bkhd->bhqk", v5[:, :, 0].abs(), v5[:, :, 1].abs()).masked_fill(~vis, 0.0)
        lse_tol = 2.0 ** -9 * (math.log2(math.e) / 8.0) * ab.amax(dim=-1) + 1e-4
        lse_tol = torch.where((vis.sum(-1) >= 128).expand_as(lse_tol), torch.full_like(lse_tol, 4e-3), lse_tol)
    lse = torch.logsumexp(s, dim=-1) / math.log(2.0)
    lse = lse.masked_fill(dark[:, None, :].expand_as(lse), 0.0)
    return ref.detach(), lse, x.grad, lse_tol, dark


def _check(got, want, heads=HEADS):
    """Forward, lse and dQ / dK / dV at the key-mask tests' tolerances."""
    out, lse, dqkv = got
    ref, lse_ref, gref, lse_tol, _ = want
    f32 = out.dtype == torch.float32
    Bq, T = out.shape[0], out.shape[1]
    err = (out.to(ref.dtype) - ref).abs().max().item()
    print("fwd err", err, "ref max", ref.abs().max().item())
    assert err <= (2e-5 if f32 else 2e-2) * max(1.0, ref.abs().max().item()), err
    dl = (lse.to(lse_ref.dtype) - lse_ref).abs()
    print("lse err", dl.max().item(), "largest err / bound", (dl / lse_tol).max().item())
    assert bool((dl <= lse_tol).all()), (dl.max().item(), (dl / lse_tol).max().item())
    g = dqkv.to(gref.dtype).view(Bq, T, 3, heads, 64)
    gr = gref.view(Bq, T, 3, heads, 64)
    for i, name in enumerate("qkv"):
        e = (g[:, :, i] - gr[:, :, i]).abs().max().item()
        scale = gr[:, :, i].abs().max().item()
        print("d" + name, "err", e, "scale", scale)
        assert e <= ((1e-4 * scale + 1e-5) if f32 else (2.5e-2 * scale + 1e-3)), (name, e, scale)


def _all_valid(T):
    return torch.ones(B, T, dtype=torch.bool, device="cuda")


_REF = {}


def _causal_ref(T, dtype, p):
    """The causal-only inputs and reference of one (T, dtype, p), computed once."""
    key = (T, dtype, p)
    if key not in _REF:
        qkv, dout = _qkv(T, 100 + T, dtype), _dout(T, dtype)
        _REF[key] = (qkv, dout, _reference(qkv, p, 4242, _all_valid(T), dout))
    return _REF[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("T", [128, 256, 384])
def test_causal(T, p, dtype):
    qkv, dout, want = _causal_ref(T, dtype, p)
    got = _raw(qkv, p, 4242, None, dout, fill=float("nan"))
    _check(got, want)
    # the public op (autograd) gives the same bits
    from gaussiank_sgd_amd.ops import attention
    x = qkv.clone().requires_grad_(True)
    out = attention.self_attention(x, HEADS, p, True, seed=4242, causal=True)
    out.backward(dout)
    assert torch.equal(out, got[0]) and torch.equal(x.grad, got[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_row_zero_is_v0(dtype, p):
    """Query 0 sees key 0 only: P = 1, out = v[0] * (dropout scale if kept), and
    dS = dP - delta cancels, so its true dQ is 0 -- with delta from the bf16
    output alone the residue would stay; out_lo removes it."""
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv, dout, want = _causal_ref(T, dtype, p)
    out, lse, dqkv = _raw(qkv, p, 4242, None, dout)
    keep = torch.ones(B, HEADS, dtype=torch.bool, device="cuda")
    if p > 0:
        keep = attention.dropout_mask(B, HEADS, T, p, 4242, "cuda")[:, :, 0, 0]
    v0 = qkv.view(B, T, 3, HEADS, 64)[:, 0, 2].float()                        # [B, heads, 64]
    exp = v0 * (keep.float() * attention.drop_scale(p))[:, :, None]
    got = out.view(B, T, HEADS, 64)[:, 0].float()
    f32 = dtype == torch.float32
    err = (got - exp).abs().max().item()
    print("row 0 err", err)
    assert err <= (2e-5 if f32 else 2e-2) * max(1.0, exp.abs().max().item())
    gref = want[2].view(B, T, 3, HEADS, 64)
    scale = gref[:, :, 0].abs().max().item()
    e = (dqkv.view(B, T, 3, HEADS, 64)[:, 0, 0].to(gref.dtype) - gref[:, 0, 0]).abs().max().item()
    print("row 0 dq err", e, "scale", scale)
    assert e <= ((1e-4 * scale + 1e-5) if f32 else (2.5e-2 * scale + 1e-3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_look_ahead_bitwise(dtype):
    """q, k, v of positions >= j replaced by values of magnitude 1e3: rows < j
    keep out and lse bit for bit (the tile skip, exact zeros on the diagonal
    tiles, and a running max that another row of the wave cannot move)."""
    T = 256
    qkv = _qkv(T, 7, dtype)
    dout = _dout(T, dtype)
    base = _raw(qkv, 0.0, 1, None, dout)
    torch.manual_seed(8)
    big = (torch.randint(0, 2, qkv.shape, device="cuda").float() * 2e3 - 1e3).to(dtype)
    for j in (1, 63, 64, 65, 127, 128, 200):
        x = qkv.clone()
        x[:, j:] = big[:, j:]
        out, lse, _ = _raw(x, 0.0, 1, None, dout)
        assert torch.isfinite(out[:, :j]).all()
        assert torch.equal(out[:, :j], base[0][:, :j]), j
        assert torch.equal(lse[:, :, :j], base[1][:, :, :j]), j


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_causal_right_padding(dtype, p):
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv, dout = _qkv(T, 21, dtype), _dout(T, dtype)
    m = _lengths_mask([T, 70], T)
    want = _reference(qkv, p, 777, m, dout)
    got = _raw(qkv, p, 777, attention.pack_key_mask(m), dout, fill=float("nan"))
    _check(got, want)
    g = got[2].view(B, T, 3, HEADS, 64)
    assert bool((g[:, :, 1:][~m] == 0).all())
    x = qkv.clone().requires_grad_(True)
    out = attention.self_attention(x, HEADS, p, True, seed=777, key_mask=m.to(torch.int64), causal=True)
    out.backward(dout)
    assert torch.equal(out, got[0]) and torch.equal(x.grad, got[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_causal_all_valid_mask_is_causal(dtype, p):
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv, dout, _ = _causal_ref(T, dtype, p)
    a = _raw(qkv, p, 4242, None, dout)
    b = _raw(qkv, p, 4242, attention.pack_key_mask(_all_valid(T)), dout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_causal_left_padding(dtype, p):
    """Keys 0..39 masked: rows 0..39 have no visible valid key -- out, lse and dQ
    exactly 0, where SDPA gives NaN; every element is written."""
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv, dout = _qkv(T, 33, dtype), _dout(T, dtype)
    m = _all_valid(T)
    m[:, :40] = False
    want = _reference(qkv, p, 55, m, dout)
    assert bool((want[4][:, :40]).all()) and not bool(want[4][:, 40:].any())
    out, lse, dqkv = _raw(qkv, p, 55, attention.pack_key_mask(m), dout, fill=float("nan"))
    for x in (out, lse, dqkv):
        assert torch.isfinite(x).all()
    g = dqkv.view(B, T, 3, HEADS, 64)
    assert (out[:, :40] == 0).all() and (lse[:, :, :40] == 0).all() and (g[:, :40, 0] == 0).all()
    assert (g[:, :40, 1:] == 0).all()
    _check((out, lse, dqkv), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_causal_hole_over_a_tile(dtype, p):
    """Keys 64..127 (one whole tile) masked, T = 384: the tile is skipped by the
    key mask in some workgroups and never reached by the causal bound in others."""
    from gaussiank_sgd_amd.ops import attention
    T = 384
    qkv, dout = _qkv(T, 35, dtype), _dout(T, dtype)
    m = _all_valid(T)
    m[:, 64:128] = False
    m[1, :64] = False       # and, in the second sequence, the tile before it: rows 0..127 see nothing
    want = _reference(qkv, p, 56, m, dout)
    got = _raw(qkv, p, 56, attention.pack_key_mask(m), dout, fill=float("nan"))
    _check(got, want)
    g = got[2].view(B, T, 3, HEADS, 64)
    assert bool((g[:, :, 1:][~m] == 0).all())
    assert (got[0][1, :128] == 0).all() and (g[1, :128, 0] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("masked", [False, True])
def test_causal_false_is_the_existing_call(dtype, p, masked):
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv, dout = _qkv(T, 11, dtype), _dout(T, dtype)
    bits = attention.pack_key_mask(_lengths_mask([T, 100], T)) if masked else None
    a = _raw(qkv, p, 321, bits, dout, causal=False, new_arg=False)
    b = _raw(qkv, p, 321, bits, dout, causal=False, new_arg=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bq,heads", [(1, 2), (2, 2), (2, 4)])
def test_causal_grid_classes(Bq, heads, dtype):
    """The workgroup -> (batch, head, row block) mapping (attn_common.h) at T = 256, two row blocks per
    (batch, head): a grid of 4 (not a multiple of 8: no XCD remap), of 8 (the remap, with the causal order
    falling back to one range) and of 16 (whole (batch, head)s per XCD).  A block computed twice leaves
    another one's NaN pre-fill.  Keys 64..127 (a whole tile) masked, the last sequence right-padded too;
    p = 0.1, so the hash index follows the mapping as well."""
    from gaussiank_sgd_amd.ops import attention
    T, p = 256, 0.1
    qkv, dout = _qkv(T, 61, dtype, heads)[:Bq], _dout(T, dtype, heads)[:Bq]
    m = torch.ones(Bq, T, dtype=torch.bool, device="cuda")
    m[:, 64:128] = False
    m[-1, 200:] = False
    want = _reference(qkv, p, 91, m, dout, heads)
    got = _raw(qkv, p, 91, attention.pack_key_mask(m), dout, fill=float("nan"), heads=heads)
    _check(got, want, heads)
    assert bool((got[2].view(Bq, T, 3, heads, 64)[:, :, 1:][~m] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PS)
def test_causal_deterministic(dtype, p):
    from gaussiank_sgd_amd.ops import attention
    T = 384
    qkv, dout = _qkv(T, 3, dtype), _dout(T, dtype)
    g = torch.Generator(device="cuda").manual_seed(1)
    bits = attention.pack_key_mask(torch.rand(B, T, device="cuda", generator=g) < 0.6)
    for kb in (None, bits):
        a = _raw(qkv, p, 42, kb, dout)
        b = _raw(qkv, p, 42, kb, dout)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_in_graph_capture(dtype):
    """The flag is a Python bool: a captured forward and backward replay it, on
    new contents of the same buffers."""
    from gaussiank_sgd_amd.ops import attention
    T = 256
    qkv = _qkv(T, 61, dtype).requires_grad_(True)
    dout = _dout(T, dtype)

    def step():
        out = attention.self_attention(qkv, HEADS, 0.0, causal=True)
        g, = torch.autograd.grad(out, qkv, dout)
        return out, g

    step()   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, g = step()
    with torch.no_grad():
        qkv.copy_(_qkv(T, 62, dtype))
    graph.replay()
    torch.cuda.synchronize()
    want_out, want_g = step()
    assert torch.equal(out, want_out) and torch.equal(g, want_g)
    ref = attention.reference_attention(qkv.detach(), HEADS, causal=True)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert (out.float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [128, 256])
def test_gpt_tiny_matches_sdpa(T, dtype, monkeypatch):
    """gpt_tiny on the fused causal kernels against the same model forced onto
    SDPA: logits and parameter gradients, and no look-ahead on the logits."""
    from gaussiank_sgd_amd.models import create_net
    from gaussiank_sgd_amd.ops import attention
    torch.manual_seed(0)
    model, _ = create_net(0, "gpt_tiny")
    model = model.cuda().eval()     # dropout off: the two paths draw different masks
    ids = torch.randint(0, 1024, (B, T), device="cuda")
    labels = torch.randint(0, 1024, (B, T), device="cuda")
    bf16 = dtype == torch.bfloat16
    calls = []
    orig = attention._FlashAttnFn.apply, attention._FlashAttnF32Fn.apply

    def run(x):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            logits = model(x)
            loss = torch.nn.functional.cross_entropy(logits.float().view(-1, 1024), labels.view(-1))
        model.zero_grad(set_to_none=True)
        loss.backward()
        return logits.detach().float(), {n: p.grad.clone() for n, p in model.named_parameters()}

    def spy(fn):
        def f(*a):
            calls.append(a[-1])
            return fn(*a)
        return f

    monkeypatch.setattr(attention._FlashAttnFn, "apply", spy(orig[0]))
    monkeypatch.setattr(attention._FlashAttnF32Fn, "apply", spy(orig[1]))
    fused, gf = run(ids)
    assert calls == [True, True]    # both blocks took the fused path, causal
    ids2 = ids.clone()
    ids2[:, T // 2 + 5:] = (ids2[:, T // 2 + 5:] + 17) % 1024
    moved, _ = run(ids2)
    assert torch.equal(moved[:, :T // 2 + 5], fused[:, :T // 2 + 5])
    assert not torch.equal(moved[:, T // 2 + 5:], fused[:, T // 2 + 5:])
    calls.clear()
    monkeypatch.setattr(attention, "fused_available", lambda *a: False)
    sdpa, gs = run(ids)
    assert calls == []
    # the fused-vs-SDPA bounds of the BERT layer tests: 5e-2 (bf16), 1e-4 (fp32)
    tol = 5e-2 if bf16 else 1e-4
    d = (fused - sdpa).abs().max().item()
    print("logits diff", d, "scale", sdpa.abs().max().item())
    assert d <= tol
    for n in gf:
        e = (gf[n].float() - gs[n].float()).abs().max().item()
        scale = gs[n].float().abs().max().item()
        print(n, "grad diff", e, "scale", scale)
        assert e <= tol * max(1.0, scale), (n, e, scale)
