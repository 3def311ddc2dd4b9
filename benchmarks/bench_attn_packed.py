#!/usr/bin/env python
"""Forward + backward of ONE BERT-Large attention layer (16 heads x 64, bf16, dropout 0.1) on
the fused kernels, dense against packed rows (block-diagonal attention by segment id):

    dense      no segment ids: the dense kernels
    eq2/4/8    2, 4, 8 equal runs per row
    skew       runs of s/2, s/4, s/8, s/8

at batch 512 x seq 128 (fwd_short_kernel / bwd_short_kernel with the bias-gradient column sums,
as the model runs them) and batch 128 x seq 512 (fwd_kernel / delta / bwd_kernel / dq_reduce).
The layouts are timed in turn, REPEATS times over; one JSON line per (shape, layout) with the
median and the spread of the repeats.  Times are device events around ITERS calls.  The run
bounds are computed outside the timed window (once per model forward, not per layer).

    python benchmarks/bench_attn_packed.py [--layouts dense,eq2,...] [--repeats 7] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 128), (128, 512)]
HEADS, P_DROP, SEED = 16, 0.1, 1234


def layout_ids(name, b, s, dev):
    import torch
    if name == "dense":
        return None
    fr = {"eq2": [1 / 2] * 2, "eq4": [1 / 4] * 4, "eq8": [1 / 8] * 8,
          "skew": [1 / 2, 1 / 4, 1 / 8, 1 / 8]}[name]
    ids, lo = torch.empty(s, dtype=torch.int32), 0
    for j, f in enumerate(fr):
        ids[lo:lo + int(s * f)] = j
        lo += int(s * f)
    assert lo == s
    return ids.expand(b, s).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", default="dense,eq2,eq4,eq8,skew")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch
    from mivod.ops import kernels as K
    if not torch.cuda.is_available():
        sys.exit("bench_attn_packed: needs a GPU")
    mvk, dev = K.native(), torch.device("cuda:0")
    names = args.layouts.split(",")
    for b, s in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        qkv = (torch.randn(b, s, 3, HEADS, 64, device=dev, generator=g) * 1.5).to(torch.bfloat16)
        dout = torch.randn(b, s, HEADS, 64, device=dev, generator=g).to(torch.bfloat16)
        segs = {}
        for n in names:
            ids = layout_ids(n, b, s, dev)
            segs[n] = None if ids is None else mvk._attn_seg.seg_bounds(ids)

        def call(seg):
            tail = () if seg is None else (seg,)
            S = mvk if seg is None else mvk._attn_seg
            fwd = mvk.attn_fwd if seg is None else S.fwd
            if s <= 128:
                bwd = mvk.attn_bwd_bsum if seg is None else S.bwd_bsum
            else:
                bwd = mvk.attn_bwd if seg is None else S.bwd
            out, lse = fwd(qkv, None, P_DROP, SEED, *tail)
            return bwd(qkv, out, dout, lse, None, P_DROP, SEED, *tail)

        for n in names:                                   # warm every layout up
            for _ in range(5):
                call(segs[n])
        torch.cuda.synchronize()
        ms = {n: [] for n in names}
        for _ in range(args.repeats):
            for n in names:
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                for _ in range(args.iters):
                    call(segs[n])
                e1.record()
                e1.synchronize()
                ms[n].append(e0.elapsed_time(e1) / args.iters)
        for n in names:
            med = statistics.median(ms[n])
            print(json.dumps({"bench": "attn_packed", "batch": b, "seq": s, "layout": n,
                              "ms_fwd_bwd_median": round(med, 4),
                              "ms_min": round(min(ms[n]), 4), "ms_max": round(max(ms[n]), 4),
                              "vs_dense": (round(med / statistics.median(ms["dense"]), 3)
                                           if "dense" in ms else None),
                              "repeats": args.repeats, "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
