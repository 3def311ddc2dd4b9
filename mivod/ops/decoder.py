"""Fused elementwise ops of a LLaMA-style decoder block (``csrc/kernels/mv_decoder.hip``,
docs/DECODER_BLOCK.md).

* ``add_rms_norm(z, residual, weight, eps)`` -> ``(y, v)``: ``v = residual + z`` (the new residual
  stream; ``z`` itself when ``residual`` is None) and ``y = v * rsqrt(mean(v^2) + eps) * weight``.
  One kernel forward; one backward that takes the gradients of BOTH outputs (either may be
  absent) and writes the one gradient ``z`` and ``residual`` share, plus ``weight``'s.
* ``swiglu(x)`` -> ``silu(x[..., :N]) * x[..., N:]`` for ``x [..., 2 N]``, the output of one fused
  gate / up projection.
* ``rotary(qkv, kv_heads, cos, sin, positions)``: rotary position embedding (half-rotation
  pairing: dim ``i`` with ``i + 64``) of the query and key heads of ``qkv [b, s, hq + 2 kv_heads,
  128]``, the layout ``ops.attention.grouped_attention`` consumes; the value heads pass through.
  ``cos`` / ``sin`` are the fp32 ``[P, 64]`` tables of ``rotary_tables``; ``positions`` is an
  integer ``[b, s]`` (default: the token's index in its row) whose values must be ``< P`` — packed
  sequences restart them per segment.

GPU + bf16 + the ``transformer`` fusion family use the kernels (all arithmetic fp32, every stored
value rounded once); anything else runs the ``*_math`` compositions below, which work in any
floating dtype on any device and are the numerics references of the tests.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ..common import fusion
from . import kernels as K


def _fused_ok(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.bfloat16 and fusion.on("transformer")


def _wide(t: torch.Tensor) -> torch.Tensor:
    """16-bit tensors compute in fp32, as the kernels do."""
    return t.float() if t.dtype in (torch.bfloat16, torch.float16) else t


# --------------------------------------------------------------------------- math
def add_rms_norm_math(z, residual, weight, eps: float = 1e-6):
    v = z if residual is None else residual + z
    x = _wide(v)
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight.to(x.dtype)
    return y.to(v.dtype), v


def swiglu_math(x):
    gate, up = x.chunk(2, dim=-1)
    return F.silu(gate) * up


def rotary_math(qkv, kv_heads: int, cos, sin, positions=None):
    b, s, heads, d = qkv.shape
    if positions is None:
        positions = torch.arange(s, device=qkv.device).expand(b, s)
    x, v = qkv.split([heads - kv_heads, kv_heads], dim=2)
    x = _wide(x)
    c = cos[positions.long()].to(x.dtype)[:, :, None]           # [b, s, 1, d / 2]
    sn = sin[positions.long()].to(x.dtype)[:, :, None]
    lo, hi = x[..., :d // 2], x[..., d // 2:]
    out = torch.cat([lo * c - hi * sn, hi * c + lo * sn], dim=-1)
    return torch.cat([out.to(qkv.dtype), v], dim=2)


def rotary_tables(max_pos: int, base: float = 10000.0, device=None):
    """fp32 ``(cos, sin)`` ``[max_pos, 64]`` of the angles ``pos * base^(-i / 64)`` (head dim 128),
    evaluated in float64."""
    inv = base ** (-torch.arange(64, dtype=torch.float64, device=device) / 64.0)
    ang = torch.arange(max_pos, dtype=torch.float64, device=device)[:, None] * inv
    return ang.cos().float(), ang.sin().float()


# ------------------------------------------------------------------------ kernels
class _AddRmsNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, res, w, eps):
        w16 = w.to(torch.bfloat16).contiguous()
        y, v, rstd = K.native()._decoder.rms_fwd(z, res, w16, float(eps))
        ctx.save_for_backward(v, rstd, w16)
        ctx.has_res, ctx.w_dtype = res is not None, w.dtype
        ctx.set_materialize_grads(False)
        return y, v

    @staticmethod
    def backward(ctx, dy, dv_out):
        v, rstd, w16 = ctx.saved_tensors
        if dy is None and dv_out is None:
            return None, None, None, None
        as16 = lambda g: None if g is None else g.to(torch.bfloat16).contiguous()
        dv, dw = K.native()._decoder.rms_bwd(as16(dy), as16(dv_out), v, rstd, w16)
        return dv, dv if ctx.has_res else None, dw.to(ctx.w_dtype), None


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return K.native()._decoder.swiglu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return K.native()._decoder.swiglu_bwd(dy.to(torch.bfloat16).contiguous(), x)


class _Rotary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, kv_heads, cos, sin, pos):
        ctx.save_for_backward(cos, sin, pos)
        ctx.kv_heads = kv_heads
        return K.native()._decoder.rotary_fwd(qkv, kv_heads, cos, sin, pos)

    @staticmethod
    def backward(ctx, dout):
        cos, sin, pos = ctx.saved_tensors
        dqkv = K.native()._decoder.rotary_bwd(dout.to(torch.bfloat16).contiguous(), ctx.kv_heads,
                                              cos, sin, pos)
        return dqkv, None, None, None, None


# ------------------------------------------------------------------------- public
def add_rms_norm(z: torch.Tensor, residual, weight: torch.Tensor, eps: float = 1e-6):
    """``(y, v)`` with ``v = residual + z`` and ``y = rms_norm(v) * weight``."""
    h = z.shape[-1]
    if weight.shape != (h,) or (residual is not None and residual.shape != z.shape):
        raise ValueError("add_rms_norm: weight must be [H] and residual shaped like z [*, H]")
    if _fused_ok(z) and h % 8 == 0 and 8 <= h <= 8192:
        res = None if residual is None else residual.to(torch.bfloat16).contiguous()
        return _AddRmsNorm.apply(z.contiguous(), res, weight, eps)
    return add_rms_norm_math(z, residual, weight, eps)


def swiglu(x: torch.Tensor) -> torch.Tensor:
    if x.shape[-1] % 2:
        raise ValueError("swiglu: the last dim must hold the gate and the up columns")
    if _fused_ok(x) and x.shape[-1] % 16 == 0 and x.shape[-1] > 0:
        return _SwiGLU.apply(x.contiguous())
    return swiglu_math(x)


def rotary(qkv: torch.Tensor, kv_heads: int, cos: torch.Tensor, sin: torch.Tensor,
           positions=None) -> torch.Tensor:
    if qkv.dim() != 4 or kv_heads < 1 or qkv.shape[2] <= 2 * kv_heads:
        raise ValueError("qkv must be [b, s, hq + 2 * kv_heads, d]")
    b, s, heads, d = qkv.shape
    if (heads - 2 * kv_heads) % kv_heads:
        raise ValueError(f"{heads - 2 * kv_heads} query heads are no multiple of kv_heads = {kv_heads}")
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] * 2 != d:
        raise ValueError(f"cos and sin must be [P, {d // 2}] tables")
    if positions is None and s > cos.shape[0]:
        raise ValueError(f"{s} positions need tables of at least that many rows, not {cos.shape[0]}")
    if positions is not None and tuple(positions.shape) != (b, s):
        raise ValueError(f"positions must be [b, s] = [{b}, {s}]")
    if _fused_ok(qkv) and d == 128:
        pos = None if positions is None else positions.to(torch.int32).contiguous()
        return _Rotary.apply(qkv.contiguous(), int(kv_heads), cos.float().contiguous(),
                             sin.float().contiguous(), pos)
    return rotary_math(qkv, kv_heads, cos, sin, positions)
