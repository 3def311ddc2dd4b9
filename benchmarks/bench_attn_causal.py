#!/usr/bin/env python
"""Forward and backward of ONE attention layer (16 heads x 64, bf16, dropout 0.1) on the fused
kernels, causal=True against the unchanged dense call on the same tensors:

    dense         mvk.attn_fwd / attn_bwd(_bsum): the yardstick
    causal        mvk._attn_causal without bounds (lower-triangular)
    seg4          4 equal runs per row, not causal (mvk._attn_seg)       } batch 128 x seq 512
    seg4_causal   the same runs, causal within each (mvk._attn_causal)   } only

at 65536 tokens per call: batch 512 x seq 128 (the one-workgroup-per-(b, h) kernels, with the
bias-gradient column sums as the model runs them), 128 x 512 and 32 x 2048 (fwd_kernel; delta /
bwd_kernel / dq_reduce).  The variants are timed in turn, REPEATS times over, forward and
backward apart (the backward on the variant's own stored out and lse); one JSON line per
(shape, variant) with the medians, the spread of the repeats and the ratios to dense.  Times
are device events around ITERS calls.  The run bounds are computed outside the timed window.

    python benchmarks/bench_attn_causal.py [--repeats 7] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 128), (128, 512), (32, 2048)]
PACKED_SEQ, RUNS = 512, 4
HEADS, P_DROP, SEED = 16, 0.1, 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch
    from mivod.ops import kernels as K
    if not torch.cuda.is_available():
        sys.exit("bench_attn_causal: needs a GPU")
    mvk, dev = K.native(), torch.device("cuda:0")
    for b, s in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        qkv = (torch.randn(b, s, 3, HEADS, 64, device=dev, generator=g) * 1.5).to(torch.bfloat16)
        dout = torch.randn(b, s, HEADS, 64, device=dev, generator=g).to(torch.bfloat16)
        bs = "bwd_bsum" if s <= 128 else "bwd"
        # name -> (forward, backward, trailing operands)
        variants = {"dense": (mvk.attn_fwd, getattr(mvk, "attn_" + bs), ()),
                    "causal": (mvk._attn_causal.fwd, getattr(mvk._attn_causal, bs), ())}
        if s == PACKED_SEQ:
            ids = (torch.arange(s, device=dev, dtype=torch.int32) // (s // RUNS)).expand(b, s)
            seg = (mvk._attn_seg.seg_bounds(ids.contiguous()),)
            variants["seg4"] = (mvk._attn_seg.fwd, getattr(mvk._attn_seg, bs), seg)
            variants["seg4_causal"] = (mvk._attn_causal.fwd, getattr(mvk._attn_causal, bs), seg)
        saved = {}
        for n, (fwd, bwd, tail) in variants.items():          # warm every variant up
            for _ in range(3):
                saved[n] = fwd(qkv, None, P_DROP, SEED, *tail)
                bwd(qkv, *saved[n][:1], dout, saved[n][1], None, P_DROP, SEED, *tail)
        torch.cuda.synchronize()

        def timed(fn):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters

        ms = {n: ([], []) for n in variants}
        for _ in range(args.repeats):
            for n, (fwd, bwd, tail) in variants.items():
                out, lse = saved[n]
                ms[n][0].append(timed(lambda: fwd(qkv, None, P_DROP, SEED, *tail)))
                ms[n][1].append(timed(lambda: bwd(qkv, out, dout, lse, None, P_DROP, SEED, *tail)))
        med = {n: [statistics.median(x) for x in ms[n]] for n in variants}
        for n in variants:
            rec = {"bench": "attn_causal", "batch": b, "seq": s, "variant": n}
            for d, name in enumerate(("fwd", "bwd")):
                rec[f"ms_{name}_median"] = round(med[n][d], 4)
                rec[f"ms_{name}_min_max"] = [round(min(ms[n][d]), 4), round(max(ms[n][d]), 4)]
                rec[f"{name}_vs_dense"] = round(med[n][d] / med["dense"][d], 3)
            rec.update(repeats=args.repeats, iters=args.iters)
            print(json.dumps(rec), flush=True)
        del saved, qkv, dout
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
