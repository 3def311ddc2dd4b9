#!/usr/bin/env python
"""Forward and backward of ONE grouped-query attention layer at head dim 128 (8 query heads over
kv_heads = 2 and 1, bf16, dropout 0.1), dense and causal, 65536 tokens per call at batch 512 x
seq 128, 128 x 512 and 32 x 2048:

    gqa     mvk._attn_gqa (the GQA forms of csrc/kernels/mv_attn_d128.hip): the new path
    expand  what the call cost before: repeat_interleave K and V to [b, s, 3, 8, 128], then
            mvk._attn_d128.  The forward time includes the expansion, the backward time the sum
            of the G bf16 dK / dV copies back to the shared heads (what autograd runs)
    math    grouped_attention_math on the same tensor, backward by autograd

The variants are timed in turn in one process, REPEATS times over, forward and backward apart
(the backward on the variant's own stored forward); one JSON line per (kv_heads, shape, mode,
variant) with the medians, the spread of the repeats and the ratios to gqa.  Times are device
events around ITERS calls (MATH_ITERS for the math path, which is tens of milliseconds a call).

    python benchmarks/bench_attn_gqa.py [--repeats 7] [--iters 50] [--math-iters 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 128), (128, 512), (32, 2048)]
HQ, D, P_DROP, SEED = 8, 128, 0.1, 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--math-iters", type=int, default=5)
    args = ap.parse_args()
    import torch
    from mivod.ops import kernels as K
    from mivod.ops.attention import grouped_attention_math
    if not torch.cuda.is_available():
        sys.exit("bench_attn_gqa: needs a GPU")
    mvk, dev = K.native(), torch.device("cuda:0")

    def timed(fn, iters):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for hkv in (2, 1):
        G = HQ // hkv

        def expand(x):          # [b, s, 8 + 2 hkv, 128] -> [b, s, 3, 8, 128]
            q, k, v = x.split([HQ, hkv, hkv], dim=2)
            return torch.stack([q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)], 2)

        def fold(dx):           # the gradient of expand: the group sums, in bf16 like autograd
            b, s = dx.shape[:2]
            dk, dv = (dx[:, :, i].view(b, s, hkv, G, D).sum(3) for i in (1, 2))
            return torch.cat([dx[:, :, 0], dk, dv], 2)

        for b, s in SHAPES:
            g = torch.Generator(device=dev).manual_seed(5)
            x = (torch.randn(b, s, HQ + 2 * hkv, D, device=dev, generator=g) * 1.5).to(torch.bfloat16)
            do = torch.randn(b, s, HQ, D, device=dev, generator=g).to(torch.bfloat16)
            for causal in (False, True):
                a = (None, P_DROP, SEED, None, causal)
                og = mvk._attn_gqa.fwd(x, hkv, *a)
                xe = expand(x)
                oe = mvk._attn_d128.fwd(xe, *a)
                xm = x.clone().requires_grad_()
                ym = grouped_attention_math(xm, hkv, None, P_DROP, causal=causal)
                dym = do.view(b, s, -1)
                # name -> (forward, backward, calls per timing)
                variants = {
                    "gqa": (lambda: mvk._attn_gqa.fwd(x, hkv, *a),
                            lambda: mvk._attn_gqa.bwd(x, hkv, og[0], do, og[1], *a), args.iters),
                    "expand": (lambda: mvk._attn_d128.fwd(expand(x), *a),
                               lambda: fold(mvk._attn_d128.bwd(xe, oe[0], do, oe[1], *a)), args.iters),
                    "math": (lambda: grouped_attention_math(x, hkv, None, P_DROP, causal=causal),
                             lambda: torch.autograd.grad(ym, xm, dym, retain_graph=True), args.math_iters),
                }
                for fwd, bwd, _ in variants.values():          # warm every variant up
                    for _ in range(3):
                        fwd()
                        bwd()
                torch.cuda.synchronize()
                ms = {n: ([], []) for n in variants}
                for _ in range(args.repeats):
                    for n, (fwd, bwd, iters) in variants.items():
                        ms[n][0].append(timed(fwd, iters))
                        ms[n][1].append(timed(bwd, iters))
                med = {n: [statistics.median(v) for v in ms[n]] for n in variants}
                for n in variants:
                    rec = {"bench": "attn_gqa", "kv_heads": hkv, "batch": b, "seq": s, "causal": causal,
                           "variant": n}
                    for i, name in enumerate(("fwd", "bwd")):
                        rec[f"ms_{name}_median"] = round(med[n][i], 4)
                        rec[f"ms_{name}_min_max"] = [round(min(ms[n][i]), 4), round(max(ms[n][i]), 4)]
                        rec[f"{name}_vs_gqa"] = round(med[n][i] / med["gqa"][i], 3)
                    rec.update(repeats=args.repeats, iters=variants[n][2])
                    print(json.dumps(rec), flush=True)
                del ym, xm, xe, oe, variants
                torch.cuda.empty_cache()
            del x, do
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
