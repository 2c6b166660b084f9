"""Key-padding masks of ops.attention on the CPU: the packed bit format
(pack_key_mask / unpack_key_mask), self_attention(key_mask=...) against the
fp32 reference and against SDPA with the boolean mask, and BertForMaskedLM's
attention_mask path against the layers called with the SDPA mask."""
import torch
import torch.nn.functional as F

from gaussiank_sgd_amd.ops import attention


def _mask(B, T, seed, keep=0.7):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, T, generator=g) < keep
    m[:, 0] = True   # no empty sequence: SDPA would return NaN there
    return m


def test_pack_unpack_roundtrip_and_bit_order():
    m = _mask(3, 256, 0)
    bits = attention.pack_key_mask(m)
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (3, 8)
    assert torch.equal(attention.unpack_key_mask(bits, 256), m)
    # any dtype, nonzero = valid
    for dt in (torch.int64, torch.float32, torch.uint8):
        assert torch.equal(attention.pack_key_mask(m.to(dt) * 3), bits)
    # bit j of word w is key 32 w + j: keys 32, 33 and 63 of sequence 1 -> word 1 = 0x80000003
    h = torch.zeros(2, 64, dtype=torch.bool)
    h[1, 32] = h[1, 33] = h[1, 63] = True
    h[0, 5] = True
    hb = attention.pack_key_mask(h)
    assert hb.tolist() == [[1 << 5, 0], [0, 0x80000003 - (1 << 32)]]
    assert torch.equal(attention.unpack_key_mask(hb, 64), h)


def _sdpa_bool(qkv, heads, m):
    B, T, _ = qkv.shape
    x = qkv.view(B, T, 3, heads, -1)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=m[:, None, None, :])
    return o.transpose(1, 2).reshape(B, T, -1)


def test_self_attention_key_mask_cpu_matches_reference_and_sdpa():
    torch.manual_seed(1)
    B, T, heads = 2, 128, 2
    qkv = torch.randn(B, T, 3 * heads * 64)
    m = _mask(B, T, 2)
    ref = attention.reference_attention(qkv, heads, key_mask=m)
    sd = _sdpa_bool(qkv, heads, m)
    assert (ref - sd).abs().max().item() <= 1e-5
    for km in (m, attention.pack_key_mask(m), m.to(torch.int64)):
        out = attention.self_attention(qkv, heads, 0.0, key_mask=km)
        assert (out - ref).abs().max().item() <= 1e-5
        assert (out - sd).abs().max().item() <= 1e-5
    # the packed form is accepted by the reference too
    assert torch.equal(attention.reference_attention(qkv, heads, key_mask=attention.pack_key_mask(m)), ref)
    # masked keys do not matter: changing their k / v rows changes nothing
    q2 = qkv.clone().view(B, T, 3, heads, 64)
    q2[:, :, 1:][~m] = 7.0
    out2 = attention.self_attention(q2.view(B, T, -1), heads, 0.0, key_mask=m)
    assert (out2 - ref).abs().max().item() <= 1e-5
    # with an attn_mask as well, the two are combined
    add = torch.zeros(B, 1, T, T)
    both = attention.self_attention(qkv, heads, 0.0, attn_mask=add, key_mask=m)
    assert (both - ref).abs().max().item() <= 1e-5


def test_bert_attention_mask_cpu_unchanged():
    from gaussiank_sgd_amd.models.bert import bert_tiny
    torch.manual_seed(3)
    model = bert_tiny(dropout=0.0).eval()
    B, T = 2, 64
    ids = torch.randint(0, 1024, (B, T))
    m = torch.ones(B, T, dtype=torch.int64)
    m[0, 40:] = 0
    m[1, 17:] = 0
    with torch.no_grad():
        out = model(ids, attention_mask=m)
        # the same model by hand, its layers on the SDPA mask
        from gaussiank_sgd_amd.ops.embedding import bert_embeddings
        x = bert_embeddings(ids, None, model.word_embeddings, model.position_embeddings, model.token_type_embeddings)
        x = model.emb_drop(model.emb_ln(x))
        for layer in model.encoder:
            x = layer(x, attn_mask=m[:, None, None, :].to(torch.bool))
        from gaussiank_sgd_amd.models.bert import vocab_projection
        h = model.mlm_ln(model.mlm_dense(x, act="gelu"))
        want = vocab_projection(h, model.word_embeddings.weight, model.mlm_bias)
        # and a layer given the key mask directly takes the same SDPA path on the CPU
        y = torch.randn(B, T, 64)
        a = model.encoder[0](y, key_mask=m)
        b = model.encoder[0](y, attn_mask=m[:, None, None, :].to(torch.bool))
    assert torch.equal(out, want)
    assert torch.equal(a, b)
