#!/usr/bin/env python
"""The decoder-block kernels (csrc/kernels/mv_decoder.hip) against their eager compositions, and
one LLaMA decoder layer step with and without them.

Per op, forward and backward apart, 65536 tokens, bf16:

    add_rms_norm  [65536, 4096] and [65536, 8192], with a residual; backward with dy and dv_out
    swiglu        x [65536, 2 x 14336]
    rotary        qkv [32, 2048, 32 + 2 x 8, 128], default positions

    kernel  mvk._decoder.*            math  ops.decoder.*_math, backward by autograd

All three are bandwidth-bound, so beside each time stands the rate at which the op moved the bytes
it MUST move (every operand read once, every result written once; computed below from the shapes,
the same count for both variants): the yardstick is HBM bandwidth, not a speed-up.

Then one training step (forward + backward) of a LlamaDecoderLayer at hidden 4096, 32 query heads
over 8 KV heads, ffn 14336, batch 8 x seq 2048: all kernels on, against MIVOD_FUSION_OFF=transformer
(the three ops of this file on their math paths; attention and the GEMMs unchanged).

The variants are timed in turn in one process, REPEATS times over; times are device events around
ITERS calls; one JSON line per measurement with the median and the spread of the repeats.

    python benchmarks/bench_decoder.py [--repeats 5] [--iters 20] [--tokens 65536]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from mivod.common import fusion
    from mivod.models.llama import LlamaConfig, LlamaDecoderLayer
    from mivod.ops import decoder as ops
    from mivod.ops import kernels as K
    if not torch.cuda.is_available():
        sys.exit("bench_decoder: needs a GPU")
    D, dev, T = K.native()._decoder, torch.device("cuda:0"), args.tokens
    gen = torch.Generator(device=dev).manual_seed(5)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=gen).to(torch.bfloat16)

    def timed(fn, iters):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def race(tag, variants, nbytes=None, **info):
        """variants: name -> callable; nbytes: the bytes the op must move (per call)."""
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in variants}
        for _ in range(args.repeats):
            for n, fn in variants.items():
                ms[n].append(timed(fn, args.iters))
        for n in variants:
            med = statistics.median(ms[n])
            rec = dict(bench="decoder", what=tag, variant=n, **info, ms_median=round(med, 4),
                       ms_min_max=[round(min(ms[n]), 4), round(max(ms[n]), 4)],
                       repeats=args.repeats, iters=args.iters)
            if nbytes is not None:
                rec.update(must_move_GB=round(nbytes / 1e9, 3), TB_per_s=round(nbytes / med / 1e9, 3))
            print(json.dumps(rec), flush=True)

    def math_pair(f, xs, couts):
        """(forward, backward) of an eager composition on leaves xs."""
        xs = [x.clone().requires_grad_() for x in xs]
        outs = f(*xs)
        outs = outs if isinstance(outs, tuple) else (outs,)
        return (lambda: f(*xs)), (lambda: torch.autograd.grad(outs, xs, couts, retain_graph=True))

    # ---- add_rms_norm: z, res in, v, y out (+ rstd); dy, dv_out, v in, dv out (+ rstd, partials)
    for H in (4096, 8192):
        z, res, w, dy, dvo = rnd(T, H), rnd(T, H), rnd(H) + 1, rnd(T, H), rnd(T, H)
        y, v, rstd = D.rms_fwd(z, res, w, 1e-6)
        mf, mb = math_pair(lambda z, r, w: ops.add_rms_norm_math(z, r, w, 1e-6), [z, res, w], (dy, dvo))
        row = 2 * H * T
        race("add_rms_norm fwd", {"kernel": lambda: D.rms_fwd(z, res, w, 1e-6), "math": mf},
             4 * row + 4 * T + 2 * H, tokens=T, width=H)
        race("add_rms_norm bwd", {"kernel": lambda: D.rms_bwd(dy, dvo, v, rstd, w), "math": mb},
             4 * row + 4 * T + 4 * H, tokens=T, width=H)
        del z, res, dy, dvo, y, v, mf, mb
        torch.cuda.empty_cache()
    # ---- swiglu: 2 N in, N out; N + 2 N in, 2 N out
    N = 14336
    x, dy = rnd(T, 2 * N), rnd(T, N)
    mf, mb = math_pair(ops.swiglu_math, [x], (dy,))
    race("swiglu fwd", {"kernel": lambda: D.swiglu_fwd(x), "math": mf}, 3 * 2 * N * T, tokens=T, width=N)
    race("swiglu bwd", {"kernel": lambda: D.swiglu_bwd(dy, x), "math": mb}, 5 * 2 * N * T, tokens=T, width=N)
    del x, dy, mf, mb
    torch.cuda.empty_cache()
    # ---- rotary: qkv in, out out, the tables once
    hq, hkv, s = 32, 8, 2048
    b = max(1, T // s)
    cos, sin = ops.rotary_tables(s, device=dev)
    q, dq = rnd(b, s, hq + 2 * hkv, 128), rnd(b, s, hq + 2 * hkv, 128)
    mf, mb = math_pair(lambda t: ops.rotary_math(t, hkv, cos, sin), [q], (dq,))
    nb = 2 * 2 * q.numel() + 2 * 4 * cos.numel()
    race("rotary fwd", {"kernel": lambda: D.rotary_fwd(q, hkv, cos, sin), "math": mf}, nb,
         tokens=b * s, heads=[hq, hkv])
    race("rotary bwd", {"kernel": lambda: D.rotary_bwd(dq, hkv, cos, sin), "math": mb}, nb,
         tokens=b * s, heads=[hq, hkv])
    del q, dq, mf, mb
    torch.cuda.empty_cache()
    # ---- one decoder layer step
    cfg = LlamaConfig(num_layers=1, max_position=s)
    layer = LlamaDecoderLayer(cfg).to(dev, torch.bfloat16)
    norm = torch.ones(cfg.hidden_size, device=dev, dtype=torch.bfloat16, requires_grad=True)
    bl = max(1, min(8, T // s))
    y0, v0, g = (rnd(bl, s, cfg.hidden_size) for _ in range(3))
    y0.requires_grad_(), v0.requires_grad_()

    def step(off):
        def run():
            if off:
                os.environ[fusion.ENV] = off
            try:
                yo, vo = layer(y0, v0, norm, cos, sin)
                torch.autograd.backward((yo, vo), (g, g))
            finally:
                os.environ.pop(fusion.ENV, None)
        return run

    race("decoder layer fwd+bwd", {"fused": step(""), "transformer_off": step("transformer")},
         tokens=bl * s, hidden=cfg.hidden_size, ffn=cfg.ffn_size, heads=[hq, hkv])


if __name__ == "__main__":
    main()
