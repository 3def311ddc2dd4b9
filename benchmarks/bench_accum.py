#!/usr/bin/env python3
"""Local gradient accumulation over backward_passes_per_step = 4 micro-batches on one GPU, on
the parameter lists of BERT-Large and ResNet-50 with bf16 gradients: what autograd does today
(``p.grad += g`` per parameter per pass in bf16, then one ``K.pack`` per bucket onto the fp16
wire) against the fp32 arena of ``accumulation_dtype=torch.float32`` (one ``K.accumulate``
launch per bucket per pass, the last pass fused with the wire cast in ``K.pack_accumulated``;
csrc/kernels/mv_accum.hip).  Only the accumulation work is timed, not the backward passes
between the launches.

    python benchmarks/bench_accum.py                    # both models, one child process each
    python benchmarks/bench_accum.py --only bert_large  # one model in this process

A window is the k passes of one optimizer step:
  autograd: pass 1 keeps the incoming gradient as p.grad (no launch); passes 2..k one add_ per
            parameter (read 2 + 2, write 2 bytes per element); then the pack (read 2, write 2)
  arena:    pass 1 first (read 2, write 4), passes 2..k-1 add (read 2 + 4, write 4), pass k
            last (read 2 + 4, write 2), one launch per bucket each
Both run on the same buffers, alternating round by round in one process; HIP events around
``--iters`` windows, ``--rounds`` rounds after ``--warmup`` windows; the figure is the median
round and ``spread`` is (max - min) / median of the rounds.  Times and bytes are reported per
micro-pass (window / k).  ``flat_cast`` over the whole fp32 accumulator onto the fp16 wire
(read 4, write 2 bytes per element, one launch) is the streaming yardstick of the same script:
``arena_over_flat_cast_rate`` is the arena path's bytes per second over flat_cast's.  Not a
gate: the feature's claim is the numerics and the released gradient memory.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["bert_large", "resnet50"]
ALIGN = 64


def param_sizes(case):
    """element counts of the model's parameters in backward order (built on the meta device)"""
    import torch
    with torch.device("meta"):
        if case == "bert_large":
            from mivod.models.bert import BertConfig, BertForPreTraining
            model = BertForPreTraining(BertConfig.large())
        else:
            from mivod.models.resnet import resnet50
            model = resnet50()
    return [p.numel() for p in reversed(list(model.parameters())) if p.requires_grad]


def layout(sizes, bucket_bytes, wire_bytes=2):
    """64-element-aligned offsets and [(first parameter, one past the last)] per bucket"""
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + ALIGN - 1) // ALIGN * ALIGN
    buckets, i0, cur = [], 0, 0
    for i, n in enumerate(sizes):
        sz = (n + ALIGN - 1) // ALIGN * ALIGN * wire_bytes
        if cur > 0 and cur + sz > bucket_bytes:
            buckets.append((i0, i))
            i0, cur = i, 0
        cur += sz
    buckets.append((i0, len(sizes)))
    return offs, o, buckets


def run_one(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_accum: needs a GPU")
    from mivod.ops import kernels as K
    dev = torch.device("cuda", 0)
    k = args.passes
    sizes = param_sizes(args.only)
    offs, total, buckets = layout(sizes, int(args.bucket_mb * 2 ** 20))
    elements = sum(sizes)
    gen = torch.Generator(device=dev).manual_seed(11)
    gflat = torch.empty(total, dtype=torch.bfloat16, device=dev)
    for lo in range(0, total, 1 << 26):          # filled in pieces: no fp32 copy of the arena
        hi = min(total, lo + (1 << 26))
        gflat[lo:hi] = (torch.randn(hi - lo, device=dev, generator=gen) * 1e-2).to(torch.bfloat16)
    pflat = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    grads = [gflat[o:o + n] for o, n in zip(offs, sizes)]          # a micro-batch's gradients
    pgrads = [pflat[o:o + n] for o, n in zip(offs, sizes)]         # p.grad of the autograd path
    acc = torch.zeros(total, dtype=torch.float32, device=dev)
    wire = torch.zeros(total, dtype=torch.float16, device=dev)
    per_bucket = [(grads[i0:i1], pgrads[i0:i1], offs[i0:i1]) for i0, i1 in buckets]

    def autograd_window():
        for _ in range(k - 1):
            for p, g in zip(pgrads, grads):
                p.add_(g)
        for _, pl, ol in per_bucket:
            K.pack(pl, wire, ol)

    def arena_window():
        for j in range(k - 1):
            for gl, _, ol in per_bucket:
                K.accumulate(gl, acc, ol, j == 0)
        for gl, _, ol in per_bucket:
            K.pack_accumulated(gl, acc, wire, ol)

    def yardstick():
        K.flat_cast(acc, wire)

    fns = {"autograd": autograd_window, "arena": arena_window, "flat_cast": yardstick}

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters               # ms per window

    for fn in fns.values():
        timed(fn, args.warmup)
    rounds = {name: [] for name in fns}
    for _ in range(args.rounds):                          # alternating: one round of each in turn
        for name, fn in fns.items():
            rounds[name].append(timed(fn, args.iters))
    # bytes per window, from the element count (the alignment gaps are not touched)
    window_bytes = {"autograd": elements * (6 * (k - 1) + 4),
                    "arena": elements * (6 + 10 * (k - 2) + 8),
                    "flat_cast": total * 6}
    launches = {"autograd": len(sizes) * (k - 1) + len(buckets), "arena": len(buckets) * k,
                "flat_cast": 1}
    out = {"case": args.only, "passes": k, "parameters": len(sizes), "elements": elements,
           "buckets": len(buckets), "bucket_mb": args.bucket_mb,
           "accumulator_bytes": total * 4}
    for name, t in rounds.items():
        med = statistics.median(t)
        per = 1 if name == "flat_cast" else k
        out[name] = {"us_per_pass": round(med * 1e3 / per, 2),
                     "gb_per_pass": round(window_bytes[name] / per / 1e9, 4),
                     "launches_per_window": launches[name],
                     "gbps": round(window_bytes[name] / (med * 1e-3) / 1e9, 1),
                     "spread": round((max(t) - min(t)) / med, 4)}
    out["arena_over_autograd_time"] = round(out["arena"]["us_per_pass"]
                                            / out["autograd"]["us_per_pass"], 4)
    out["arena_over_flat_cast_rate"] = round(out["arena"]["gbps"] / out["flat_cast"]["gbps"], 4)
    torch.cuda.synchronize()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--bucket-mb", type=float, default=32.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds per case")
    args = ap.parse_args()
    if args.passes < 2:
        raise SystemExit("bench_accum: --passes must be at least 2")
    if args.only:
        run_one(args)
        return
    res = {}
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--only", case, "--passes", str(args.passes), "--bucket-mb", str(args.bucket_mb),
               "--iters", str(args.iters), "--rounds", str(args.rounds),
               "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                  # nothing more starts on the GPU after a failure
            raise SystemExit(f"bench_accum: case {case} ended with status {p.returncode}")
        res[case] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps({"bench": "grad_accumulation", "iters": args.iters, "rounds": args.rounds,
                      **res}))


if __name__ == "__main__":
    main()
