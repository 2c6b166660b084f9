"""GPT-2-style decoder-only language model (not in the reference).

Learned token and position embeddings, pre-LN blocks, a final LayerNorm and an
LM head tied to the token embedding.  ``gpt2``: 12 layers, 768 hidden, 12
heads, 1024 positions, vocabulary 50,304 (GPT-2's 50,257 padded to a multiple
of 64: even, so the fused cross-entropy takes it, and the GEMMs need no
padding; ~124M parameters).  ``gpt_tiny``: 2 layers, 128 hidden, 2 heads of 64,
vocabulary 1024, 256 positions.

On the GPU, attention is the flash-style HIP kernel of ops/attention.py with
``causal=True`` on the packed QKV projection: no [T, T] mask or score matrix,
no head split / merge copies, and the key tiles above the diagonal are never
visited.  ``attention_mask`` (key padding) is packed to bits once per forward
and honoured inside the same kernels.  On the CPU, or for shapes the kernels
do not take, it is ``F.scaled_dot_product_attention``.  Every block linear is
a ``FastLinear`` (the FFN's first one with the GELU epilogue); the logits go
through ``vocab_projection`` and the loss through ``xent.cross_entropy``.
The pre-LN residual stream uses ``nn.LayerNorm`` (``add_layernorm`` returns
only the normalised sum, which pre-LN cannot use).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import attention, xent
from ..ops.linear import FastLinear
from .bert import vocab_projection


@dataclass
class GPTConfig:
    vocab_size: int = 50304
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    max_position: int = 1024
    dropout: float = 0.1
    ln_eps: float = 1e-5


class GPTBlock(nn.Module):
    def __init__(self, c: GPTConfig):
        super().__init__()
        self.heads = c.heads
        self.ln1 = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.qkv = FastLinear(c.hidden, 3 * c.hidden)
        self.attn_out = FastLinear(c.hidden, c.hidden)
        self.ln2 = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.ffn_in = FastLinear(c.hidden, 4 * c.hidden)
        self.ffn_out = FastLinear(4 * c.hidden, c.hidden)
        self.drop = nn.Dropout(c.dropout)
        self.p = c.dropout

    def forward(self, x, attn_mask=None, key_mask=None):
        """``key_mask``: a key-padding mask ([B, T] or packed bits) for the fused
        kernels; ``attn_mask`` (any SDPA mask) forces the SDPA path.  Both are
        combined with the causal mask."""
        y = self.qkv(self.ln1(x))
        a = attention.self_attention(y, self.heads, self.p, self.training, attn_mask=attn_mask, key_mask=key_mask,
                                     causal=True)
        x = x + self.drop(self.attn_out(a))
        return x + self.drop(self.ffn_out(self.ffn_in(self.ln2(x), act="gelu")))


class GPTForCausalLM(nn.Module):
    def __init__(self, c: GPTConfig = None):
        super().__init__()
        c = c or GPTConfig()
        self.config = c
        self.vocab_size = c.vocab_size
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden)
        self.position_embeddings = nn.Embedding(c.max_position, c.hidden)
        self.emb_drop = nn.Dropout(c.dropout)
        self.blocks = nn.ModuleList([GPTBlock(c) for _ in range(c.layers)])
        self.ln_f = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.name = "gpt2"
        self.apply(self._init)
        # GPT-2: the residual projections start smaller by 1 / sqrt(2 * layers)
        for blk in self.blocks:
            for lin in (blk.attn_out, blk.ffn_out):
                nn.init.normal_(lin.weight, mean=0.0, std=0.02 / (2 * c.layers) ** 0.5)

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, mean=0.0, std=0.02)
        if isinstance(m, nn.Linear) and m.bias is not None:
            nn.init.zeros_(m.bias)

    def forward(self, input_ids, attention_mask=None):
        """Next-token logits [B, T, V].  ``attention_mask``: [B, T] key padding
        (nonzero = real token), on top of the causal mask."""
        B, T = input_ids.shape
        if T > self.config.max_position:
            raise ValueError("sequence length %d exceeds max_position %d" % (T, self.config.max_position))
        pos = torch.arange(T, device=input_ids.device)
        x = self.emb_drop(self.word_embeddings(input_ids) + self.position_embeddings(pos))
        mask = key_bits = None
        if attention_mask is not None:
            if attention.fused_available_for(x, T, self.config.heads, self.config.hidden):
                # the fused kernels take the padding mask as bits: packed once, shared by every block
                key_bits = attention.pack_key_mask(attention_mask)
            else:
                mask = attention_mask[:, None, None, :].to(torch.bool)
        for blk in self.blocks:
            x = blk(x, mask, key_bits)
        # tied head: no bias
        return vocab_projection(self.ln_f(x), self.word_embeddings.weight, None)


class CausalLMLoss(nn.Module):
    """Next-token cross entropy over all positions (labels == -100 ignored)."""

    def forward(self, logits, labels):
        # one fused HIP pass each way on bf16 logits on the GPU (ops/xent.py)
        return xent.cross_entropy(logits, labels, ignore_index=-100)


def gpt2(**kw):
    return GPTForCausalLM(GPTConfig(**kw))


def gpt_tiny(**kw):
    d = dict(vocab_size=1024, hidden=128, layers=2, heads=2, max_position=256)
    d.update(kw)
    m = GPTForCausalLM(GPTConfig(**d))
    m.name = "gpt_tiny"
    return m
