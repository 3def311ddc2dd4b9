#!/usr/bin/env python
"""Forward and backward of ONE attention layer at head dim 128 (8 heads x 128, bf16, dropout
0.1), dense and causal, 65536 tokens per call at batch 512 x seq 128, 128 x 512 and 32 x 2048:

    d128    mvk._attn_d128 (csrc/kernels/mv_attn_d128.hip): the new path
    math    attention_math on the same tensors, backward by autograd: what a d = 128 call
            costs without the kernels (batched GEMMs, an fp32 [b, h, s, s] score tensor,
            torch's dropout)
    d64     the d = 64 kernels at 16 heads x 64: the same FLOPs and bytes, for context

The variants are timed in turn in one process, REPEATS times over, forward and backward apart
(the backward on the variant's own stored forward); one JSON line per (shape, mode, variant)
with the medians, the spread of the repeats and the ratios to d128.  Times are device events
around ITERS calls (MATH_ITERS for attention_math, which is tens of milliseconds a call).

    python benchmarks/bench_attn_d128.py [--repeats 7] [--iters 50] [--math-iters 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 128), (128, 512), (32, 2048)]
P_DROP, SEED = 0.1, 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--math-iters", type=int, default=5)
    args = ap.parse_args()
    import torch
    from mivod.ops import kernels as K
    from mivod.ops.attention import attention_math
    if not torch.cuda.is_available():
        sys.exit("bench_attn_d128: needs a GPU")
    mvk, dev = K.native(), torch.device("cuda:0")

    def timed(fn, iters):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for b, s in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        t = {}
        for d, h in ((128, 8), (64, 16)):
            t[d] = ((torch.randn(b, s, 3, h, d, device=dev, generator=g) * 1.5).to(torch.bfloat16),
                    torch.randn(b, s, h, d, device=dev, generator=g).to(torch.bfloat16))
        for causal in (False, True):
            q128, do128 = t[128]
            q64, do64 = t[64]
            f64, b64 = ((mvk._attn_causal.fwd, mvk._attn_causal.bwd) if causal
                        else (mvk.attn_fwd, mvk.attn_bwd))
            o128 = mvk._attn_d128.fwd(q128, None, P_DROP, SEED, None, causal)
            o64 = f64(q64, None, P_DROP, SEED)
            qm = q128.clone().requires_grad_()
            ym = attention_math(qm, None, P_DROP, causal=causal)
            dym = do128.view(b, s, -1)
            # name -> (forward, backward, calls per timing)
            variants = {
                "d128": (lambda: mvk._attn_d128.fwd(q128, None, P_DROP, SEED, None, causal),
                         lambda: mvk._attn_d128.bwd(q128, o128[0], do128, o128[1], None, P_DROP, SEED,
                                                    None, causal), args.iters),
                "math": (lambda: attention_math(q128, None, P_DROP, causal=causal),
                         lambda: torch.autograd.grad(ym, qm, dym, retain_graph=True), args.math_iters),
                "d64": (lambda: f64(q64, None, P_DROP, SEED),
                        lambda: b64(q64, o64[0], do64, o64[1], None, P_DROP, SEED), args.iters),
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
            med = {n: [statistics.median(x) for x in ms[n]] for n in variants}
            for n in variants:
                rec = {"bench": "attn_d128", "batch": b, "seq": s, "causal": causal, "variant": n}
                for i, name in enumerate(("fwd", "bwd")):
                    rec[f"ms_{name}_median"] = round(med[n][i], 4)
                    rec[f"ms_{name}_min_max"] = [round(min(ms[n][i]), 4), round(max(ms[n][i]), 4)]
                    rec[f"{name}_vs_d128"] = round(med[n][i] / med["d128"][i], 3)
                rec.update(repeats=args.repeats, iters=variants[n][2])
                print(json.dumps(rec), flush=True)
            del ym, qm, variants
            torch.cuda.empty_cache()
        del t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
