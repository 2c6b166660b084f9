"""The causal flag of ops.attention on the CPU (the SDPA path and the fp32
reference composition), the GPT model, its dataset kind and its trainer
wiring.  Comparisons with SDPA use torch.testing.assert_close at its fp32
defaults (rtol 1.3e-6, atol 1e-5)."""
import torch
import torch.nn.functional as F

B, T, HEADS = 2, 96, 2


def _qkv(seed=0):
    torch.manual_seed(seed)
    return torch.randn(B, T, 3 * HEADS * 64)


def _sdpa(qkv, **kw):
    v5 = qkv.view(B, T, 3, HEADS, 64)
    q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v, **kw).transpose(1, 2).reshape(B, T, HEADS * 64)


def _with_grad(fn, qkv, dout):
    x = qkv.clone().requires_grad_(True)
    out = fn(x)
    out.backward(dout)
    return out.detach(), x.grad


def test_causal_matches_sdpa_is_causal():
    from gaussiank_sgd_amd.ops import attention
    qkv = _qkv()
    dout = torch.randn(B, T, HEADS * 64)
    want = _with_grad(lambda x: _sdpa(x, is_causal=True), qkv, dout)
    for fn in (lambda x: attention.reference_attention(x, HEADS, causal=True),
               lambda x: attention.self_attention(x, HEADS, 0.0, causal=True)):
        got = _with_grad(fn, qkv, dout)
        torch.testing.assert_close(got[0], want[0])
        torch.testing.assert_close(got[1], want[1])
    # and causal=False is what it was
    torch.testing.assert_close(attention.self_attention(qkv, HEADS, 0.0), _sdpa(qkv))


def test_causal_with_key_mask_matches_merged_mask():
    """Rows with a visible valid key equal SDPA with the merged boolean mask;
    rows without one are zeros in the reference (forward and gradient)."""
    from gaussiank_sgd_amd.ops import attention
    qkv = _qkv(1)
    dout = torch.randn(B, T, HEADS * 64)
    m = torch.ones(B, T, dtype=torch.bool)
    m[0, :7] = False          # left padding: rows 0..6 see nothing
    m[0, 40:50] = False       # a hole
    m[1, 70:] = False         # right padding
    merged = torch.ones(T, T, dtype=torch.bool).tril_()[None, None] & m[:, None, None, :]
    lit = merged.any(-1)[:, 0]                    # [B, T]
    assert not lit[0, :7].any() and lit[0, 7:].all() and lit[1].all()
    dout = dout * lit[:, :, None]                 # dark rows: SDPA's own rows (NaN or not) get no gradient
    for packed in (False, True):
        km = attention.pack_key_mask(m) if packed else m
        ref, gref = _with_grad(lambda x: attention.reference_attention(x, HEADS, key_mask=km, causal=True), qkv, dout)
        assert (ref[~lit] == 0).all() and torch.isfinite(gref).all()
        x = qkv.clone().requires_grad_(True)
        out = attention.self_attention(x, HEADS, 0.0, key_mask=km, causal=True)
        want = _sdpa(qkv, attn_mask=merged)
        torch.testing.assert_close(out[lit], want[lit])
        torch.testing.assert_close(ref[lit], want[lit])
    # the gradient, on a mask without dark rows (SDPA's backward of a fully masked row is NaN)
    m[0, :7] = True
    merged = torch.ones(T, T, dtype=torch.bool).tril_()[None, None] & m[:, None, None, :]
    want = _with_grad(lambda x: _sdpa(x, attn_mask=merged), qkv, dout)
    for fn in (lambda x: attention.reference_attention(x, HEADS, key_mask=m, causal=True),
               lambda x: attention.self_attention(x, HEADS, 0.0, key_mask=m, causal=True),
               lambda x: attention.self_attention(x, HEADS, 0.0, attn_mask=m[:, None, None, :], causal=True)):
        got = _with_grad(fn, qkv, dout)
        torch.testing.assert_close(got[0], want[0])
        torch.testing.assert_close(got[1], want[1])


def test_causal_dataset_labels_are_inputs_shifted():
    from gaussiank_sgd_amd.data import DATASETS, SyntheticData
    assert DATASETS["openwebtext"].kind == "causal_lm"
    for learnable in (False, True):
        d = SyntheticData("openwebtext", 3, seq_len=16, vocab_size=50, learnable=learnable, pool=2)
        for _ in range(2):
            x, y = next(d)
            assert x.shape == (3, 16) and y.shape == (3, 16) and x.dtype == torch.int64
            assert torch.equal(y[:, :-1], x[:, 1:])
            assert int(x.max()) < 50 and int(y.max()) < 50
            if learnable:     # the counting sequences of the "tokens" kind
                assert torch.equal(y, (x + 1) % 50)
    assert SyntheticData("openwebtext", 2).get_batch()[0].shape == (2, 1024)


def test_gpt_tiny_builds_tied_and_causal():
    from gaussiank_sgd_amd import models
    from gaussiank_sgd_amd.models.gpt import GPTForCausalLM
    assert {"gpt2", "gpt_tiny"} <= set(models.available())
    assert models.default_dataset("gpt2") == "openwebtext"
    torch.manual_seed(0)
    net, _ = models.create_net(0, "gpt_tiny")
    assert isinstance(net, GPTForCausalLM) and net.name == "gpt_tiny"
    c = net.config
    assert (c.layers, c.hidden, c.heads, c.vocab_size, c.max_position) == (2, 128, 2, 1024, 256)
    # the head is the token embedding: one [V, hidden] tensor in the state dict, and the logits' gradient reaches it
    sd = net.state_dict()
    assert [k for k, v in sd.items() if tuple(v.shape) == (1024, 128)] == ["word_embeddings.weight"]
    net.eval()
    ids = torch.randint(0, 1024, (2, 48))
    logits = net(ids)
    assert logits.shape == (2, 48, 1024)
    feats = {}
    hook = net.ln_f.register_forward_hook(lambda mod, inp, out: feats.__setitem__("h", out))
    with torch.no_grad():
        net(ids)
    hook.remove()
    torch.testing.assert_close(logits.detach(), feats["h"] @ net.word_embeddings.weight.t())
    net.zero_grad()
    logits.sum().backward()
    assert net.word_embeddings.weight.grad[~torch.isin(torch.arange(1024), ids)].abs().sum() > 0   # through the head
    # no look-ahead: a token change at position j leaves the logits before j alone
    j = 20
    ids2 = ids.clone()
    ids2[:, j] = (ids2[:, j] + 1) % 1024
    with torch.no_grad():
        moved = net(ids2)
    assert torch.equal(moved[:, :j], logits[:, :j])
    assert not torch.equal(moved[:, j], logits[:, j])
    # an all-valid padding mask changes nothing; a padded tail does not reach the rows before it
    with torch.no_grad():
        torch.testing.assert_close(net(ids, attention_mask=torch.ones(2, 48)), logits)
        am = torch.ones(2, 48)
        am[:, 30:] = 0
        torch.testing.assert_close(net(ids, attention_mask=am)[:, :30], logits[:, :30])
    # gpt2's shape, without building its 124M parameters
    from gaussiank_sgd_amd.models.gpt import GPTConfig
    g = GPTConfig()
    assert (g.layers, g.hidden, g.heads, g.vocab_size, g.max_position) == (12, 768, 12, 50304, 1024)
    assert g.vocab_size % 64 == 0 and g.vocab_size >= 50257


def test_gpt_tiny_trainer_adamw_lowers_loss():
    from gaussiank_sgd_amd.train import DLTrainer
    from gaussiank_sgd_amd.train.dist_trainer import build_parser
    args = build_parser().parse_args(["--dnn", "gpt_tiny", "--optimizer", "adamw"])
    assert args.dnn == "gpt_tiny"
    t = DLTrainer(0, 1, dnn="gpt_tiny", dataset="openwebtext", batch_size=4, lr=0.05, device="cpu",
                  learnable_data=True, optimizer="adamw", seq_len=32, data_pool=1, train_samples=16)
    assert isinstance(t.optimizer, torch.optim.AdamW)
    assert t.data.spec.kind == "causal_lm" and t.data.vocab == 1024
    losses = []
    for _ in range(3):
        t.optimizer.zero_grad()
        t.train(1)
        t.update_model()
        losses.append(t.current_loss())
    print(losses)
    assert losses[0] > 6.0          # ln(1024) = 6.93 at the start
    assert losses[2] < losses[0]
    ppl = t.test(0, num_batches=1)  # perplexity = exp(loss), as for the LSTM
    assert 1.0 < ppl < 1024.0 * 1.5
