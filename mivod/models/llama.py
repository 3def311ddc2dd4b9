"""A LLaMA-style decoder-only language model on mivod's fused ops.

Per layer: the fused QKV projection (no bias) -> ``rotary`` -> ``grouped_attention(causal=True)``
-> output projection -> ``add_rms_norm`` (residual add + post-attention norm) -> ONE gate / up
projection ``[2 ffn, hidden]`` -> ``swiglu`` -> down projection -> ``add_rms_norm``, which adds
the MLP's output to the residual stream and applies the NEXT layer's input norm (the model's final
norm after the last layer).  The first input norm is ``add_rms_norm(embeddings, None, w)``.  The
residual stream ``v`` and its normed view ``y`` therefore travel together, and every norm's
backward receives the stream's gradient from its later consumers (ops/decoder.py).

Head dim is 128 (the grouped attention kernels'); there is no dropout.  Packed sequences:
``segment_ids [b, s]`` restrict attention to a token's own segment (ops.attention, "Packed
sequences") and restart the rotary positions at every segment's first token; the run bounds and
the positions are computed once per forward.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.attention import decode_attention, grouped_attention, segment_bounds
from ..ops.decoder import add_rms_norm, rotary, rotary_tables, swiglu
from ..ops.linear import end_dgrad_weights, linear, prepare_dgrad_weights
from ..ops.transformer import cross_entropy

HEAD_DIM = 128


@dataclass
class LlamaConfig:
    vocab_size: int = 32000
    hidden_size: int = 4096
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    ffn_size: int = 14336
    max_position: int = 4096
    rope_base: float = 10000.0
    rms_eps: float = 1e-6
    tie_embeddings: bool = False
    initializer_range: float = 0.02

    def __post_init__(self):
        if self.hidden_size != self.num_heads * HEAD_DIM:
            raise ValueError(f"hidden_size must be num_heads * {HEAD_DIM}")
        if self.num_kv_heads < 1 or self.num_heads % self.num_kv_heads:
            raise ValueError("num_heads must be a multiple of num_kv_heads")


def segment_positions(segment_ids: torch.Tensor) -> torch.Tensor:
    """Position of every token within its contiguous run of equal ids, int32 ``[b, s]``."""
    s = segment_ids.shape[1]
    idx = torch.arange(s, device=segment_ids.device).expand_as(segment_ids)
    first = torch.ones_like(segment_ids, dtype=torch.bool)
    first[:, 1:] = segment_ids[:, 1:] != segment_ids[:, :-1]
    start = torch.where(first, idx, torch.zeros_like(idx)).cummax(dim=1).values
    return (idx - start).to(torch.int32)


class LlamaDecoderLayer(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.hq, self.hkv, self.eps = c.num_heads, c.num_kv_heads, c.rms_eps
        self.qkv = nn.Linear(c.hidden_size, (c.num_heads + 2 * c.num_kv_heads) * HEAD_DIM, bias=False)
        self.o = nn.Linear(c.hidden_size, c.hidden_size, bias=False)
        self.post_attention_norm = nn.Parameter(torch.ones(c.hidden_size))
        self.gate_up = nn.Linear(c.hidden_size, 2 * c.ffn_size, bias=False)
        self.down = nn.Linear(c.ffn_size, c.hidden_size, bias=False)

    def projections(self):
        return [self.qkv.weight, self.o.weight, self.gate_up.weight, self.down.weight]

    def forward(self, y, v, next_norm, cos, sin, positions=None, seg=None, kv=None):
        """``y``: the normed input, ``v``: the residual stream, ``next_norm``: the weight of the
        norm that follows this layer -> the next ``(y, v)``.  ``kv``: this layer's tensor of a
        ``KVCache`` being prefilled, which receives the rotated K / V heads of the ``s`` tokens."""
        b, s, _ = y.shape
        qkv = linear(y, self.qkv.weight).view(b, s, self.hq + 2 * self.hkv, HEAD_DIM)
        qkv = rotary(qkv, self.hkv, cos, sin, positions)
        if kv is not None:
            kv[:, :s].copy_(qkv[:, :, self.hq:])
        a = grouped_attention(qkv, self.hkv, causal=True, segment_bounds=seg)
        return self._mlp(a, v, next_norm)

    def _mlp(self, a, v, next_norm):
        y, v = add_rms_norm(linear(a, self.o.weight), v, self.post_attention_norm, self.eps)
        m = linear(swiglu(linear(y, self.gate_up.weight)), self.down.weight)
        return add_rms_norm(m, v, next_norm, self.eps)

    def decode(self, y, v, next_norm, cos, sin, kv, lens):
        """``forward`` for one new token per batch row, ``y`` and ``v`` ``[b, 1, H]``: the token
        sits at position ``lens - 1``, its K / V heads are appended to ``kv`` there and its
        query heads attend keys ``[0, lens)`` of the cache (ops.attention, "Decoding")."""
        b = y.shape[0]
        qkv = linear(y, self.qkv.weight).view(b, 1, self.hq + 2 * self.hkv, HEAD_DIM)
        pos = lens - 1
        qkv = rotary(qkv, self.hkv, cos, sin, pos.view(b, 1))
        kv[torch.arange(b, device=kv.device), pos.long()] = qkv[:, 0, self.hq:]
        a = decode_attention(qkv[:, 0, :self.hq], kv, self.hkv, lens)
        return self._mlp(a.view(b, 1, -1), v, next_norm)


class KVCache:
    """The keys and values of the tokens seen so far: per layer one ``[b, S_max, 2 hkv, 128]``
    tensor (a token's rotated key heads, then its value heads: the tail of its ``qkv`` row) and
    ``lens`` int32 ``[b]``, the number of tokens each batch row holds, shared by the layers."""

    def __init__(self, c: LlamaConfig, batch: int, s_max: int, dtype, device):
        self.s_max = s_max
        self.layers = [torch.zeros(batch, s_max, 2 * c.num_kv_heads, HEAD_DIM, dtype=dtype, device=device)
                       for _ in range(c.num_layers)]
        self.lens = torch.zeros(batch, dtype=torch.int32, device=device)


class LlamaModel(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.config = c
        self.embed = nn.Embedding(c.vocab_size, c.hidden_size)
        self.layers = nn.ModuleList([LlamaDecoderLayer(c) for _ in range(c.num_layers)])
        # input_norms[i] precedes layer i; input_norms[num_layers] is the final norm
        self.input_norms = nn.ParameterList([nn.Parameter(torch.ones(c.hidden_size))
                                             for _ in range(c.num_layers + 1)])
        self._rope = {}         # device -> the fp32 (cos, sin) tables, whatever dtype the module has

    def rope_tables(self, device):
        key = str(device)
        if key not in self._rope:
            self._rope[key] = rotary_tables(self.config.max_position, self.config.rope_base, device)
        return self._rope[key]

    def forward(self, input_ids, segment_ids=None, cache: "KVCache" = None):
        """``cache``: an empty ``KVCache`` to prefill with the K / V of ``input_ids`` (every batch
        row a full prompt of the same length, no segments); without it nothing changes."""
        c = self.config
        if input_ids.shape[1] > c.max_position:
            raise ValueError(f"sequence length {input_ids.shape[1]} exceeds max_position {c.max_position}")
        if cache is not None and (segment_ids is not None or input_ids.shape[1] > cache.s_max):
            raise ValueError("a cache is prefilled with unpacked prompts of at most S_max tokens")
        seg = positions = None
        if segment_ids is not None:
            seg = segment_bounds(segment_ids)
            positions = segment_positions(segment_ids)
        cos, sin = self.rope_tables(input_ids.device)
        y, v = add_rms_norm(self.embed(input_ids), None, self.input_norms[0], c.rms_eps)
        prep = self.training and torch.is_grad_enabled() and y.is_cuda
        if prep:        # W^T of every projection for its data gradient: one launch (ops/linear.py)
            prepare_dgrad_weights([w for lyr in self.layers for w in lyr.projections()])
        try:
            for i, lyr in enumerate(self.layers):
                y, v = lyr(y, v, self.input_norms[i + 1], cos, sin, positions, seg,
                           None if cache is None else cache.layers[i])
        finally:
            if prep:
                end_dgrad_weights()
        if cache is not None:
            cache.lens.fill_(input_ids.shape[1])
        return y

    def decode(self, token_ids, cache: "KVCache"):
        """One further token per batch row, ``token_ids [b]``, appended to ``cache`` (whose rows
        must hold fewer than ``S_max`` tokens) -> the normed final hidden state ``[b, 1, H]``."""
        c = self.config
        cache.lens += 1
        cos, sin = self.rope_tables(token_ids.device)
        y, v = add_rms_norm(self.embed(token_ids[:, None]), None, self.input_norms[0], c.rms_eps)
        for i, lyr in enumerate(self.layers):
            y, v = lyr.decode(y, v, self.input_norms[i + 1], cos, sin, cache.layers[i], cache.lens)
        return y


class LlamaForCausalLM(nn.Module):
    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.config = c
        self.model = LlamaModel(c)
        self.lm_head = None if c.tie_embeddings else nn.Linear(c.hidden_size, c.vocab_size, bias=False)
        self.apply(self._init)

    def _init(self, m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=self.config.initializer_range)

    def logits(self, input_ids, segment_ids=None):
        w = self.model.embed.weight if self.lm_head is None else self.lm_head.weight
        return linear(self.model(input_ids, segment_ids), w)

    def forward(self, input_ids, labels=None, segment_ids=None, ignore_index: int = -100):
        """The logits ``[b, s, vocab]``, or with ``labels [b, s]`` the mean next-token loss:
        position t is scored against ``labels[:, t + 1]`` (``ignore_index`` rows skipped; with
        packed sequences the caller ignores the last token of every segment)."""
        logits = self.logits(input_ids, segment_ids)
        if labels is None:
            return logits
        # shift the labels, not the logits: no copy of [b, s, vocab]; a row's last token has no target
        target = F.pad(labels[:, 1:], (0, 1), value=ignore_index)
        return cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1),
                             ignore_index=ignore_index)

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens: int, eos_token_id=None, return_logits: bool = False):
        """Greedy decoding: ``input_ids [b, s]`` (full prompts of one length) -> ``[b, s + n]``,
        the prompts and up to ``max_new_tokens`` new tokens each.  The prompt runs through the
        training forward once and fills a ``KVCache`` of ``S_max = min(max_position, s +
        max_new_tokens)`` tokens; every further token is one ``decode`` step against it, and
        generation ends early when the cache is full.  A row that has produced ``eos_token_id``
        keeps producing it; when every row has, generation stops.  ``return_logits``: also the
        logits each new token was taken from, ``[b, n, vocab]``."""
        c = self.config
        b, s = input_ids.shape
        if max_new_tokens < 1 or s < 1:
            raise ValueError("generate needs a prompt and max_new_tokens >= 1")
        w = self.model.embed.weight if self.lm_head is None else self.lm_head.weight
        cache = KVCache(c, b, min(c.max_position, s + max_new_tokens), w.dtype, input_ids.device)
        logits = linear(self.model(input_ids, cache=cache)[:, -1:], w)
        tokens, steps = [], []
        done = torch.zeros(b, dtype=torch.bool, device=input_ids.device)
        while True:
            nxt = logits[:, 0].argmax(-1)
            if eos_token_id is not None:
                nxt = torch.where(done, torch.full_like(nxt, eos_token_id), nxt)
                done |= nxt == eos_token_id
            tokens.append(nxt)
            steps.append(logits)
            if (len(tokens) == max_new_tokens or s + len(tokens) > cache.s_max
                    or (eos_token_id is not None and bool(done.all()))):
                break
            logits = linear(self.model.decode(nxt, cache), w)
        out = torch.cat([input_ids, torch.stack(tokens, 1)], 1)
        return (out, torch.cat(steps, 1)) if return_logits else out


def count_params(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters())
