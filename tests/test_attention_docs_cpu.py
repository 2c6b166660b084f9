"""Document masks of packed sequences on the CPU: the packed form, its visibility, and packing invariance of the
SDPA fallback and of the GPT model (a packed document computes what it computes alone in a row)."""
import pytest
import torch

from gaussiank_sgd_amd.ops import attention


@pytest.mark.parametrize("ids,start,end", [
    ([3, 3, 5, 3], [0, 0, 2, 3], [1, 1, 2, 3]),          # ids repeating non-adjacently: three documents
    ([0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]),          # a boundary at every token
])
def test_pack_segments_and_visibility(ids, start, end):
    seg = attention.pack_segments(torch.tensor([ids, ids[::-1]]))
    assert seg.dtype == torch.int32 and seg[0].tolist() == [start, end]
    assert seg[1].tolist() == [[3 - e for e in end[::-1]], [3 - s for s in start[::-1]]]
    want = [[start[q] <= k <= q for k in range(4)] for q in range(4)]
    assert attention.segments_visible(seg)[0].tolist() == want
    # a query sees a key iff they share a document and the key is not later
    doc = torch.tensor(start)
    assert want == ((doc[:, None] == doc[None, :]) & torch.ones(4, 4, dtype=torch.bool).tril()).tolist()


DOCS = [(0, 5), (5, 6), (6, 16)]


def _doc_ids(B):
    return torch.tensor([[i for i, (lo, hi) in enumerate(DOCS) for _ in range(hi - lo)]] * B)


def test_fallback_packing_invariance():
    torch.manual_seed(0)
    qkv = torch.randn(2, 16, 3 * 2 * 8)
    out = attention.self_attention(qkv, 2, causal=True, segments=_doc_ids(2))
    assert torch.equal(out, attention.self_attention(qkv, 2, causal=True, segments=attention.pack_segments(_doc_ids(2))))
    for lo, hi in DOCS:
        alone = attention.reference_attention(qkv[:, lo:hi], 2, causal=True)
        assert (out[:, lo:hi] - alone).abs().max().item() <= 1e-5
    with pytest.raises(ValueError):
        attention.self_attention(qkv, 2, segments=_doc_ids(2))


def test_gpt_packing_invariance():
    """Positions restart at each document: a packed document gets the logits it gets alone in a row."""
    from gaussiank_sgd_amd.models import create_net
    torch.manual_seed(0)
    model = create_net(0, "gpt_tiny")[0].eval()
    ids = torch.randint(0, 1024, (2, 16))
    with torch.no_grad():
        packed = model(ids, doc_ids=_doc_ids(2))
        for lo, hi in DOCS:
            assert (packed[:, lo:hi] - model(ids[:, lo:hi])).abs().max().item() <= 1e-5
