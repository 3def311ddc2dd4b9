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

from ..ops.attention import grouped_attention, segment_bounds
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

    def forward(self, y, v, next_norm, cos, sin, positions=None, seg=None):
        """``y``: the normed input, ``v``: the residual stream, ``next_norm``: the weight of the
        norm that follows this layer -> the next ``(y, v)``."""
        b, s, _ = y.shape
        qkv = linear(y, self.qkv.weight).view(b, s, self.hq + 2 * self.hkv, HEAD_DIM)
        qkv = rotary(qkv, self.hkv, cos, sin, positions)
        a = grouped_attention(qkv, self.hkv, causal=True, segment_bounds=seg)
        y, v = add_rms_norm(linear(a, self.o.weight), v, self.post_attention_norm, self.eps)
        m = linear(swiglu(linear(y, self.gate_up.weight)), self.down.weight)
        return add_rms_norm(m, v, next_norm, self.eps)


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

    def forward(self, input_ids, segment_ids=None):
        c = self.config
        if input_ids.shape[1] > c.max_position:
            raise ValueError(f"sequence length {input_ids.shape[1]} exceeds max_position {c.max_position}")
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
                y, v = lyr(y, v, self.input_norms[i + 1], cos, sin, positions, seg)
        finally:
            if prep:
                end_dgrad_weights()
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


def count_params(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters())
