"""Multi-head self-attention for the BERT workload.

``attention(qkv, mask_bias, p_drop)`` takes the fused QKV projection
``[b, s, 3, h, d]`` and returns the context ``[b, s, h*d]``.

* GPU, bf16, head dim 64 -> the hand-written MFMA kernels in
  ``csrc/kernels/mv_attn.hip`` (fused QK^T / online softmax / dropout / PV
  forward; FlashAttention-2-style backward with deterministic dQ partials).
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
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..common import fusion
from . import kernels as K


def attention_math(qkv: torch.Tensor, mask_bias=None, p_drop: float = 0.0,
                   keep_mask=None) -> torch.Tensor:
    """The fallback for devices and dtypes the kernels do not cover.  A row whose keys are all
    masked with ``-inf`` comes out NaN here (softmax of an empty set), where the kernels give
    0: see the mask contract above."""
    b, s, _, h, d = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)          # [b, h, s, d]
    scores = torch.matmul(q, k.transpose(-1, -2)).float() * (1.0 / math.sqrt(d))
    if mask_bias is not None:
        scores = scores + mask_bias.float().reshape(b, 1, 1, s)
    p = torch.softmax(scores, dim=-1)
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
    def forward(ctx, qkv, mask, p_drop, seed, slot=None):
        out, lse = K.native().attn_fwd(qkv, mask, float(p_drop), int(seed))
        ctx.save_for_backward(qkv, out, lse, mask)
        ctx.p_drop, ctx.seed = float(p_drop), int(seed)
        ctx.slot = slot
        b, s, h, d = out.shape
        return out.view(b, s, h * d)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask = ctx.saved_tensors
        dout = dout.contiguous().view(out.shape)
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        nat = K.native()
        if ctx.slot is not None and qkv.shape[1] <= 128:
            dqkv, ctx.slot.partials = nat.attn_bwd_bsum(qkv, out, dout, lse, mask, ctx.p_drop,
                                                        ctx.seed)
        else:
            dqkv = nat.attn_bwd(qkv, out, dout, lse, mask, ctx.p_drop, ctx.seed)
        return dqkv, None, None, None, None


def fused_available(qkv: torch.Tensor) -> bool:
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 5 and
            qkv.shape[-1] == 64 and fusion.on("attention"))


def mask_to_key_bias(mask_bias, b, s):
    """[b,1,1,s] additive bias (or None) -> contiguous fp32 [b, s]."""
    if mask_bias is None:
        return None
    return mask_bias.reshape(b, s).float().contiguous()


def attention(qkv: torch.Tensor, mask_bias=None, p_drop: float = 0.0, seed=None,
              bias_slot: "BiasGradSlot" = None) -> torch.Tensor:
    """``bias_slot``: the slot the projection that produced ``qkv`` was given
    (``ops.linear.linear(..., bias_slot=)``) — its bias gradient then comes out of this
    op's backward kernel."""
    if fused_available(qkv):
        b, s = qkv.shape[0], qkv.shape[1]
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_drop > 0 else 0
        return _FusedAttention.apply(qkv.contiguous(), mask_to_key_bias(mask_bias, b, s),
                                     p_drop, seed, bias_slot)
    return attention_math(qkv, mask_bias, p_drop)
