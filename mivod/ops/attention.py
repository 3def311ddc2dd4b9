"""Multi-head self-attention for the BERT workload.

``attention(qkv, mask_bias, p_drop)`` takes the fused QKV projection
``[b, s, 3, h, d]`` and returns the context ``[b, s, h*d]``.

* GPU, bf16, head dim 64 -> the hand-written MFMA kernels in
  ``csrc/kernels/mv_attn.hip`` (fused QK^T / online softmax / dropout / PV
  forward; FlashAttention-2-style backward with deterministic dQ partials).
* GPU, bf16, head dim 128 -> the kernels of ``csrc/kernels/mv_attn_d128.hip``
  (docs/ATTENTION_D128.md): the same forward at twice the width, and a backward in two
  kernels, a query-block owner that keeps dQ in registers over every key block and a
  key-block owner for dK / dV, with no dQ partials.  Same mask contract, segments, ``causal``
  and dropout hash as below; ``bias_slot`` is accepted and its ``partials`` stay ``None``
  (the projection then sums the columns of dqkv itself).
* anything else -> ``attention_math`` (batched GEMMs + fp32 softmax), which is
  also the numerics reference for the kernels.

The mask contract
-----------------
``mask_bias`` is an additive bias per (batch row, key), in natural-log units like the scores
(the kernels work in the log2 domain and scale it themselves), of any finite value, ``-inf``
or ``finfo(float32).min`` (whose product with log2(e) overflows to ``-inf``).  A key at
``-inf`` has probability exactly 0 and gets zero dK / dV rows.  A batch row whose keys are ALL
at ``-inf`` (a fully padded sequence) has no softmax: the kernels give it ``out = 0`` and
``lse = -inf``, and its backward contributes exactly zero gradients (the row's lse is staged
as ``+inf``, so every recomputed probability is 0).  ``attention_math`` divides 0 by 0 there
and yields NaN for such a row; only the kernels define it.  Other finite values
below about -4e37 are not a supported way to say "masked" (the s <= 128 forward multiplies the
mask by 8 ahead of the common score scale and overflows earlier than the other kernels): use ``-inf``, ``finfo.min``
or a moderate value like -10000.

Packed sequences
----------------
``segment_ids`` is an integer tensor ``[b, s]``: query i and key j of a batch row attend to each
other iff ``segment_ids[i] == segment_ids[j]`` and that id is ``>= 0`` (a block-diagonal mask;
``mask_bias`` still applies on top).  A negative id marks padding: such a token is no key for
anyone, and as a query it is a fully masked row in the sense above (``out = 0``, zero
gradients).  On the kernel path every non-negative id must occupy ONE contiguous run of its row
(padding may sit anywhere); this is the caller's contract and is not checked on the device.
``segment_bounds(segment_ids)`` turns the ids into per-token run bounds in one launch: compute it
once per model forward and pass ``segment_bounds=`` to every layer.  The kernels skip the tiles
outside a run (docs/PACKED_ATTENTION.md).  ``attention_math`` builds the mask from id equality,
so it is correct for any ids, and gives padding queries 0 like the kernels.

Causal attention
----------------
``causal=True``: query i attends key j iff ``j <= i`` and, with segments, j is in i's run;
``mask_bias`` still applies on top.  Everything above holds unchanged: a key at ``-inf`` has
probability exactly 0, a query with no key left (query 0 when key 0 is at ``-inf``) has
``out = 0``, ``lse = -inf`` and zero gradients, padding tokens are exactly 0, and the dropout
hash is the same function of the absolute (b h, query, key).  The kernels are the ``CAUSAL``
instantiations in ``csrc/kernels/mv_attn_causal.hip``: without segments they read no bounds at
all, with ``segment_bounds`` they take the same direction-free bounds and derive the keys of a
query and the queries of a key from them, and they skip the tiles above the diagonal
(docs/CAUSAL_ATTENTION.md).  ``attention_math(..., causal=True)`` puts ``-inf`` above the
diagonal and gives a query with no key 0.

Grouped-query attention
-----------------------
``grouped_attention(qkv, kv_heads, ...)`` takes ``qkv [b, s, hq + 2 * kv_heads, d]`` — within a
token the ``hq`` query heads, then the ``kv_heads`` key heads, then the ``kv_heads`` value heads,
as one fused projection writes them — and returns ``[b, s, hq * d]``.  Query head ``i`` reads
key / value head ``i // G``, ``G = hq // kv_heads``.  Everything above holds with "(b, h)" read
as "(b, query head)", and the dropout hash is that of ``(seed, b_index * hq + query_head)`` over
(query, key): the result EQUALS ``attention`` on the tensor whose K and V heads are each
repeated G times (``repeat_interleave``), with the dK / dV of the G copies summed — the kernels
(GPU, bf16, d = 128: the ``GQA`` forms in ``csrc/kernels/mv_attn_d128.hip``,
docs/ATTENTION_GQA.md) read each shared head in place and do that sum in registers, rounding
once.  Anything else runs ``grouped_attention_math``, which builds the repeated tensor.

Decoding
--------
``decode_attention(q, kv_cache, kv_heads, lens)`` is the attention of ONE new token per batch row
against a cache: ``q [b, hq, d]`` are the token's rotated query heads, ``kv_cache
[b, S_max, 2 * kv_heads, d]`` holds per cached token its ``kv_heads`` key heads, then its
``kv_heads`` value heads — the tail ``qkv[:, :, hq:]`` of the grouped ``qkv`` row, so appending a
token is one slice copy — and ``lens [b]`` (int32) says that batch row ``i`` attends keys
``[0, lens[i])``; the new token's own K / V are appended first, so ``lens`` counts it.  The result
is ``[b, hq * d]``.  No mask, no dropout, no segments, and no autograd: the op is meant for
``torch.no_grad()`` and returns a tensor without a graph.  ``lens[i] == 0`` is a query without a
key (``out = 0``); ``lens[i] <= S_max`` is the caller's contract, and nothing at or past
``lens[i]`` in the cache is read.  GPU, bf16, d = 128 and ``hq / kv_heads <= 16`` run the split-KV
kernels of ``csrc/kernels/mv_attn_decode.hip`` (docs/ATTENTION_DECODE.md), which read ``lens`` on
the device; anything else runs ``decode_attention_math``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..common import fusion
from . import kernels as K


def attention_math(qkv: torch.Tensor, mask_bias=None, p_drop: float = 0.0,
                   keep_mask=None, segment_ids=None, causal: bool = False) -> torch.Tensor:
    """The fallback for devices and dtypes the kernels do not cover.  A row whose keys are all
    masked with ``-inf`` comes out NaN here (softmax of an empty set), where the kernels give
    0: see the mask contract above.  With ``segment_ids`` (any ids, contiguous or not) the
    queries without a key — padding — get 0 instead, and so they do with ``causal``."""
    b, s, _, h, d = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)          # [b, h, s, d]
    scores = torch.matmul(q, k.transpose(-1, -2)).float() * (1.0 / math.sqrt(d))
    if mask_bias is not None:
        scores = scores + mask_bias.float().reshape(b, 1, 1, s)
    if segment_ids is not None:
        ids = segment_ids.reshape(b, s)
        same = (ids[:, :, None] == ids[:, None, :]) & (ids >= 0)[:, None, :]      # [b, q, k]
        scores = scores.masked_fill(~same[:, None], -math.inf)
    if causal:
        above = torch.ones(s, s, dtype=torch.bool, device=scores.device).triu(1)
        scores = scores.masked_fill(above, -math.inf)
    p = torch.softmax(scores, dim=-1)
    if segment_ids is not None or causal:
        p = torch.nan_to_num(p, nan=0.0)                    # a query with no key at all
    if keep_mask is not None:
        p = p * keep_mask.to(p.dtype) / (1.0 - p_drop)
    elif p_drop > 0:
        p = F.dropout(p, p_drop, True)
    ctx = torch.matmul(p.to(v.dtype), v)                    # [b, h, s, d]
    return ctx.permute(0, 2, 1, 3).reshape(b, s, h * d)


class BiasGradSlot:
    """Hand-over of the fused QKV projection's bias gradient from the attention backward
    (which writes dqkv and, for s <= 128, its per-(b, h) column sums in the same kernel)
    to that projection's backward (ops/linear.py), which then skips its column-sum pass
    over dqkv.  One slot per (projection, attention) pair per forward."""
    __slots__ = ("partials",)

    def __init__(self):
        self.partials = None


class _FusedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, mask, p_drop, seed, slot=None, seg=None, causal=False):
        nat = K.native()
        if qkv.shape[-1] == 128:
            out, lse = nat._attn_d128.fwd(qkv, mask, float(p_drop), int(seed), seg, bool(causal))
        elif causal:
            out, lse = nat._attn_causal.fwd(qkv, mask, float(p_drop), int(seed), seg)
        elif seg is None:
            out, lse = nat.attn_fwd(qkv, mask, float(p_drop), int(seed))
        else:
            out, lse = nat._attn_seg.fwd(qkv, mask, float(p_drop), int(seed), seg)
        ctx.save_for_backward(qkv, out, lse, mask, seg)
        ctx.p_drop, ctx.seed = float(p_drop), int(seed)
        ctx.slot, ctx.causal = slot, bool(causal)
        b, s, h, d = out.shape
        return out.view(b, s, h * d)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask, seg = ctx.saved_tensors
        dout = dout.contiguous().view(out.shape)
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        nat = K.native()
        args = (qkv, out, dout, lse, mask, ctx.p_drop, ctx.seed)
        if qkv.shape[-1] == 128:        # no column sums: the slot's partials stay None
            return nat._attn_d128.bwd(*args, seg, ctx.causal), None, None, None, None, None, None
        bsum = ctx.slot is not None and qkv.shape[1] <= 128
        if ctx.causal:
            res = (nat._attn_causal.bwd_bsum if bsum else nat._attn_causal.bwd)(*args, seg)
        elif seg is not None:
            res = (nat._attn_seg.bwd_bsum if bsum else nat._attn_seg.bwd)(*args, seg)
        else:
            res = (nat.attn_bwd_bsum if bsum else nat.attn_bwd)(*args)
        if bsum:
            dqkv, ctx.slot.partials = res
        else:
            dqkv = res
        return dqkv, None, None, None, None, None, None


class _FusedGroupedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, kv_heads, mask, p_drop, seed, seg, causal):
        out, lse = K.native()._attn_gqa.fwd(qkv, kv_heads, mask, float(p_drop), int(seed), seg,
                                            bool(causal))
        ctx.save_for_backward(qkv, out, lse, mask, seg)
        ctx.kv_heads, ctx.p_drop, ctx.seed, ctx.causal = kv_heads, float(p_drop), int(seed), bool(causal)
        b, s, h, d = out.shape
        return out.view(b, s, h * d)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask, seg = ctx.saved_tensors
        dout = dout.contiguous().view(out.shape)
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        dqkv = K.native()._attn_gqa.bwd(qkv, ctx.kv_heads, out, dout, lse, mask, ctx.p_drop, ctx.seed,
                                        seg, ctx.causal)
        return dqkv, None, None, None, None, None, None


def fused_available(qkv: torch.Tensor) -> bool:
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 5 and
            qkv.shape[-1] in (64, 128) and fusion.on("attention"))


def mask_to_key_bias(mask_bias, b, s):
    """[b,1,1,s] additive bias (or None) -> contiguous fp32 [b, s]."""
    if mask_bias is None:
        return None
    return mask_bias.reshape(b, s).float().contiguous()


class SegmentBounds:
    """What ``segment_bounds`` returns: the ids, and on the kernel path their per-token run
    bounds (int32 ``[b, s]``, ``lo | hi << 16``; None where only ``attention_math`` can run)."""
    __slots__ = ("ids", "bounds")

    def __init__(self, ids, bounds):
        self.ids, self.bounds = ids, bounds


def segment_bounds(segment_ids: torch.Tensor) -> SegmentBounds:
    """Prepare ``segment_ids`` ``[b, s]`` for ``attention(..., segment_bounds=)``: one small
    kernel launch on the GPU (no host sync), shared by every layer and both directions."""
    if segment_ids.dim() != 2 or segment_ids.dtype not in (torch.int32, torch.int64):
        raise ValueError("segment_ids must be an int32 or int64 tensor [b, s]")
    bounds = None
    if segment_ids.is_cuda and fusion.on("attention"):
        bounds = K.native()._attn_seg.seg_bounds(segment_ids.contiguous())
    return SegmentBounds(segment_ids, bounds)


_prepare_segments = segment_bounds      # attention() has a keyword of the same name


def attention(qkv: torch.Tensor, mask_bias=None, p_drop: float = 0.0, seed=None,
              bias_slot: "BiasGradSlot" = None, segment_ids=None,
              segment_bounds: "SegmentBounds" = None, causal: bool = False) -> torch.Tensor:
    """``bias_slot``: the slot the projection that produced ``qkv`` was given
    (``ops.linear.linear(..., bias_slot=)``) — its bias gradient then comes out of this
    op's backward kernel.  ``segment_ids`` or (computed once for all layers)
    ``segment_bounds``: packed sequences, see the module docstring.  ``causal``: key j <= query i
    on top of the other masks."""
    if segment_ids is not None and segment_bounds is not None:
        raise ValueError("pass segment_ids or segment_bounds, not both")
    if segment_ids is not None:
        segment_bounds = _prepare_segments(segment_ids)
    b, s = qkv.shape[0], qkv.shape[1]
    if segment_bounds is not None and tuple(segment_bounds.ids.shape) != (b, s):
        raise ValueError(f"segment ids must be [b, s] = [{b}, {s}]")
    if fused_available(qkv):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_drop > 0 else 0
        seg = None
        if segment_bounds is not None:
            if segment_bounds.bounds is None:
                raise RuntimeError("segment_bounds was prepared off the kernel path")
            seg = segment_bounds.bounds
        return _FusedAttention.apply(qkv.contiguous(), mask_to_key_bias(mask_bias, b, s),
                                     p_drop, seed, bias_slot, seg, causal)
    return attention_math(qkv, mask_bias, p_drop,
                          segment_ids=None if segment_bounds is None else segment_bounds.ids,
                          causal=causal)


def _expand_groups(qkv: torch.Tensor, kv_heads: int) -> torch.Tensor:
    """``[b, s, hq + 2 kv_heads, d]`` -> ``[b, s, 3, hq, d]`` with every K / V head repeated G
    times (autograd sums the copies' gradients)."""
    hq = qkv.shape[2] - 2 * kv_heads
    q, k, v = qkv.split([hq, kv_heads, kv_heads], dim=2)
    g = hq // kv_heads
    return torch.stack([q, k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)], dim=2)


def grouped_attention_math(qkv: torch.Tensor, kv_heads: int, mask_bias=None, p_drop: float = 0.0,
                           keep_mask=None, segment_ids=None, causal: bool = False) -> torch.Tensor:
    """``attention_math`` on the expanded tensor: the fallback and the numerics reference of
    ``grouped_attention``."""
    return attention_math(_expand_groups(qkv, kv_heads), mask_bias, p_drop, keep_mask,
                          segment_ids, causal)


def grouped_attention(qkv: torch.Tensor, kv_heads: int, mask_bias=None, p_drop: float = 0.0,
                      seed=None, segment_ids=None, segment_bounds: "SegmentBounds" = None,
                      causal: bool = False) -> torch.Tensor:
    """Grouped-query / multi-query attention on ``qkv [b, s, hq + 2 * kv_heads, d]`` ->
    ``[b, s, hq * d]``, see the module docstring.  ``kv_heads == hq`` is ``attention`` on the
    ``[b, s, 3, hq, d]`` view of the same memory."""
    if qkv.dim() != 4 or kv_heads < 1 or qkv.shape[2] <= 2 * kv_heads:
        raise ValueError("qkv must be [b, s, hq + 2 * kv_heads, d]")
    b, s, d = qkv.shape[0], qkv.shape[1], qkv.shape[3]
    hq = qkv.shape[2] - 2 * kv_heads
    if hq % kv_heads != 0:
        raise ValueError(f"{hq} query heads are no multiple of kv_heads = {kv_heads}")
    if kv_heads == hq:
        return attention(qkv.reshape(b, s, 3, hq, d), mask_bias, p_drop, seed,
                         segment_ids=segment_ids, segment_bounds=segment_bounds, causal=causal)
    if segment_ids is not None and segment_bounds is not None:
        raise ValueError("pass segment_ids or segment_bounds, not both")
    if segment_ids is not None:
        segment_bounds = _prepare_segments(segment_ids)
    if segment_bounds is not None and tuple(segment_bounds.ids.shape) != (b, s):
        raise ValueError(f"segment ids must be [b, s] = [{b}, {s}]")
    if qkv.is_cuda and qkv.dtype == torch.bfloat16 and d == 128 and fusion.on("attention"):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_drop > 0 else 0
        seg = None
        if segment_bounds is not None:
            if segment_bounds.bounds is None:
                raise RuntimeError("segment_bounds was prepared off the kernel path")
            seg = segment_bounds.bounds
        return _FusedGroupedAttention.apply(qkv.contiguous(), int(kv_heads),
                                            mask_to_key_bias(mask_bias, b, s), p_drop, seed, seg, causal)
    return grouped_attention_math(qkv, kv_heads, mask_bias, p_drop,
                                  segment_ids=None if segment_bounds is None else segment_bounds.ids,
                                  causal=causal)


def decode_attention_math(q: torch.Tensor, kv_cache: torch.Tensor, kv_heads: int,
                          lens: torch.Tensor) -> torch.Tensor:
    """The fallback and the numerics reference of ``decode_attention``, for any dtype and device:
    a ``[b, S_max]`` key mask from ``lens``, batched GEMMs and a softmax (fp32 for 16-bit
    inputs).  What the cache holds at or past ``lens`` has no influence here either."""
    b, hq, d = q.shape
    s_max = kv_cache.shape[1]
    k, v = kv_cache.split([kv_heads, kv_heads], dim=2)                   # [b, S_max, hkv, d]
    dead = torch.arange(s_max, device=q.device)[None, :] >= lens.reshape(b, 1)      # [b, S_max]
    scores = torch.einsum("bhgd,bshd->bhgs", q.reshape(b, kv_heads, hq // kv_heads, d), k)
    if scores.dtype in (torch.bfloat16, torch.float16):
        scores = scores.float()
    scores = (scores * (1.0 / math.sqrt(d))).masked_fill(dead[:, None, None], -math.inf)
    p = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0)         # lens == 0: no key at all
    ctx = torch.einsum("bhgs,bshd->bhgd", p.to(v.dtype), v.masked_fill(dead[:, :, None, None], 0))
    return ctx.reshape(b, hq * d)


def decode_attention(q: torch.Tensor, kv_cache: torch.Tensor, kv_heads: int,
                     lens: torch.Tensor) -> torch.Tensor:
    """One new token per batch row against a KV cache: ``q [b, hq, d]``, ``kv_cache
    [b, S_max, 2 * kv_heads, d]``, ``lens [b]`` -> ``[b, hq * d]``, see "Decoding" in the module
    docstring.  Inference only: no autograd, use it under ``torch.no_grad()``."""
    if q.dim() != 3 or kv_cache.dim() != 4 or kv_heads < 1:
        raise ValueError("q must be [b, hq, d] and kv_cache [b, S_max, 2 * kv_heads, d]")
    b, hq, d = q.shape
    if tuple(kv_cache.shape) != (b, kv_cache.shape[1], 2 * kv_heads, d):
        raise ValueError(f"kv_cache must be [{b}, S_max, {2 * kv_heads}, {d}]")
    if hq % kv_heads != 0:
        raise ValueError(f"{hq} query heads are no multiple of kv_heads = {kv_heads}")
    if tuple(lens.shape) != (b,):
        raise ValueError(f"lens must be [b] = [{b}]")
    if (q.is_cuda and q.dtype == torch.bfloat16 and kv_cache.dtype == torch.bfloat16 and d == 128
            and hq // kv_heads <= 16 and fusion.on("attention")):
        out, _ = K.native()._attn_decode.fwd(q.detach().contiguous(), kv_cache.detach().contiguous(),
                                             int(kv_heads), lens.to(torch.int32).contiguous())
        return out.view(b, hq * d)
    return decode_attention_math(q.detach(), kv_cache.detach(), kv_heads, lens)
