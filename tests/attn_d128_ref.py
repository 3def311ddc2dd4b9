"""A plain float64 attention reference, generic in the head dim, for the head-dim-128 kernels
(csrc/kernels/mv_attn_d128.hip).  A helper module, not a test file: tests/test_attn_d128_gpu.py
holds the kernels against it, tests/test_attn_d128_cpu.py ties it to attention_math."""
import math

import torch

import attn_reference as R


def make_inputs(b, s, h, d, kind, seed, dev="cpu"):
    """attn_reference.make_case's recipe at width d: qkv = randn * 1.5 and dout = randn in bf16,
    mask none or frac (randn * 2 per key)."""
    gen = torch.Generator().manual_seed(seed * 7919 + 1000 * b + 10 * s + h + d)
    qkv = (torch.randn(b, s, 3, h, d, generator=gen) * 1.5).to(torch.bfloat16)
    dout = torch.randn(b, s, h, d, generator=gen).to(torch.bfloat16)
    mask = R.make_mask(kind, b, s, gen)
    return {"qkv": qkv.to(dev), "dout": dout.to(dev), "mask": None if mask is None else mask.to(dev)}


def make_ids(b, s, runs, dev="cpu"):
    """runs [(lo, hi), ...] -> int32 [b, s] segment ids, -1 (padding) outside every run."""
    ids = torch.full((b, s), -1, dtype=torch.int32, device=dev)
    for j, (lo, hi) in enumerate(runs):
        ids[:, lo:hi] = j
    return ids


def allowed(b, s, ids, causal, dev="cpu"):
    """bool [b, q, k]: may query q attend key k (diagonal, runs, padding keys)."""
    ok = torch.ones(b, s, s, dtype=torch.bool, device=dev)
    if causal:
        ok = ok.tril()
    if ids is not None:
        ok = ok & (ids[:, :, None] == ids[:, None, :]) & (ids >= 0)[:, None, :]
    return ok


def forward(qkv, mask, ok, keep, p):
    """qkv float64 [b, s, 3, h, d] -> (out [b, s, h, d], lse [b, h, s] in log2 units).  A query
    with no key gets out = 0 and lse = -inf: its scores are taken out of the softmax and its
    probabilities set to 0 (nan_to_num(0) of the softmax, with a finite gradient)."""
    d = qkv.shape[-1]
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)                    # [b, h, s, d]
    sc = q @ k.transpose(-1, -2) / math.sqrt(d)
    if mask is not None:
        sc = sc + mask.double()[:, None, None, :]
    sc = sc.masked_fill(~ok[:, None], -math.inf)
    dead = (sc == -math.inf).all(-1, keepdim=True)
    P = torch.softmax(sc.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    lse = torch.logsumexp(sc.detach(), -1) / math.log(2.0)
    if keep is not None:
        P = P * keep.to(P.device).double() / (1.0 - p)
    return (P @ v).permute(0, 2, 1, 3), lse


def reference(t, p, ok, seed):
    """(out, lse, dq, dk, dv) in float64 from the stored bf16 inputs of ``t``; the gradients by
    float64 autograd on dout; dropout by attn_reference.keep_mask."""
    b, s, _, h, _ = t["qkv"].shape
    keep = R.keep_mask(b, h, s, p, seed) if p > 0 else None
    qkv = t["qkv"].double().requires_grad_()
    out, lse = forward(qkv, t["mask"], ok, keep, p)
    (g,) = torch.autograd.grad(out, qkv, t["dout"].double())
    return (out.detach(), lse) + tuple(g.unbind(2))
