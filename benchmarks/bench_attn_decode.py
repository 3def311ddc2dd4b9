#!/usr/bin/env python
"""One-token attention against a KV cache at head dim 128 (32 query heads over 8 KV heads, and 8
over 1; bf16), batch 1, 8, 64 x 512, 4096, 32768 cached tokens (every row full: lens = S_max):

    decode  mvk._attn_decode (csrc/kernels/mv_attn_decode.hip), splits chosen by the launcher
    math    decode_attention_math on the same cache
    full    what sampling cost before: grouped_attention(causal=True) over the whole sequence,
            of which the last row is the answer (only where b * len <= 65536; it is O(len^2))

and, with --sweep, the decode kernel at every split count 1, 2, 4, ... 64 (the table the
launcher's rule in mv_attn_decode_splits was read from).

"must move" is the cache itself, b * len * 2 kv_heads * 128 * 2 bytes; TB/s = must move / median
time of a call (both kernels, launch gaps included).  A cache smaller than the last-level cache
would be timed out of that cache, so every variant cycles over enough copies of its operands to
touch COLD_BYTES between two uses of one copy.  The variants are timed in turn in one process,
REPEATS times over; device events around ITERS calls; one JSON line per record.

    python benchmarks/bench_attn_decode.py [--repeats 5] [--iters 40] [--math-iters 5] [--sweep]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS = [(32, 8), (8, 1)]
BATCHES = (1, 8, 64)
LENS = (512, 4096, 32768)
D = 128
COLD_BYTES = 1 << 30
FULL_MAX_TOKENS = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--math-iters", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import torch
    from mivod.ops import kernels as K
    from mivod.ops.attention import decode_attention_math, grouped_attention
    if not torch.cuda.is_available():
        sys.exit("bench_attn_decode: needs a GPU")
    mvk, dev = K.native(), torch.device("cuda:0")

    def timed(fn, iters):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def measure(variants):
        """name -> (fn(i), iters) -> name -> the per-repeat milliseconds, variants in turn."""
        for fn, _ in variants.values():
            for i in range(2):
                fn(i)
        torch.cuda.synchronize()
        ms = {n: [] for n in variants}
        for _ in range(args.repeats):
            for n, (fn, iters) in variants.items():
                ms[n].append(timed(fn, iters))
        return ms

    for hq, hkv in HEADS:
        for b in BATCHES:
            for s in LENS:
                must = b * s * 2 * hkv * D * 2
                copies = max(1, min(args.iters, -(-COLD_BYTES // must)))
                kv = torch.randn(copies, b, s, 2 * hkv, D, device=dev, dtype=torch.bfloat16)
                q = torch.randn(b, hq, D, device=dev, dtype=torch.bfloat16)
                lens = torch.full((b,), s, dtype=torch.int32, device=dev)
                base = {"bench": "attn_decode", "hq": hq, "kv_heads": hkv, "batch": b, "len": s,
                        "must_move_bytes": must, "copies": copies, "repeats": args.repeats}
                variants = {
                    "decode": (lambda i: mvk._attn_decode.fwd(q, kv[i % copies], hkv, lens), args.iters),
                    "math": (lambda i: decode_attention_math(q, kv[i % copies], hkv, lens), args.math_iters),
                }
                if b * s <= FULL_MAX_TOKENS:
                    fc = max(1, min(4, copies))
                    qkv = torch.randn(fc, b, s, hq + 2 * hkv, D, device=dev, dtype=torch.bfloat16)
                    variants["full"] = (lambda i: grouped_attention(qkv[i % fc], hkv, causal=True),
                                        args.math_iters)
                with torch.no_grad():
                    ms = measure(variants)
                    med = {n: statistics.median(v) for n, v in ms.items()}
                    for n in variants:
                        rec = dict(base, variant=n, iters=variants[n][1],
                                   splits=mvk._attn_decode.splits(b * hkv, s) if n == "decode" else None,
                                   ms_median=round(med[n], 5),
                                   ms_min_max=[round(min(ms[n]), 5), round(max(ms[n]), 5)],
                                   vs_decode=round(med[n] / med["decode"], 2))
                        if n != "full":
                            rec["tb_per_s"] = round(must / med[n] / 1e9, 3)
                        print(json.dumps(rec), flush=True)
                    if args.sweep:
                        sw = {sp: ((lambda i, sp=sp: mvk._attn_decode.fwd(q, kv[i % copies], hkv, lens, sp)),
                                   args.iters) for sp in (1, 2, 4, 8, 16, 32, 64)}
                        for sp, v in measure(sw).items():
                            m = statistics.median(v)
                            print(json.dumps(dict(base, variant="sweep", splits=sp, iters=args.iters,
                                                  ms_median=round(m, 5),
                                                  ms_min_max=[round(min(v), 5), round(max(v), 5)],
                                                  tb_per_s=round(must / m / 1e9, 3))), flush=True)
                del kv, q, variants
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
