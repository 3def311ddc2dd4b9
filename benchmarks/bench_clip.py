#!/usr/bin/env python3
"""The kernels of global gradient-norm clipping (``max_grad_norm``; csrc/kernels/mv_clip.hip)
on one GPU, on buffers of a BERT-Large's size: the 336M-element gradient arena
(``--elements``) on the fp16 and on the bf16 wire, and one 32 MB bucket.

    python benchmarks/bench_clip.py                  # every case, one child process each
    python benchmarks/bench_clip.py --only fp16      # one case in this process

A case times four read-only variants on the same buffer, alternating round by round in one
process: ``nonfinite_scan`` (the overflow guard's pass, the yardstick), ``grad_sumsq`` with
and without the flag (the same bytes, plus 16 multiply-adds per lane and one partial per
4096 elements), and ``clip_finalize`` at that buffer's partial count.  On the arena it also
times ``adam_step`` (fp32 master and moments, bf16 model copy) with and without the device
clip coefficient.  Each case runs in a process of its own under its own time limit
(``--limit`` seconds), so a case that hangs or runs out of memory costs its own figures only.
Timing: HIP events around ``--iters`` launches, ``--rounds`` rounds after ``--warmup``
launches; the figure is the median round, and ``spread`` is (max - min) / median of the
rounds of ``nonfinite_scan``, the margin a difference between the variants is read against.
GB/s = elements x element size over the measured time.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["fp16", "bf16", "bucket"]
BERT_LARGE_ELEMENTS = 336_226_108        # parameters of mivod.models.bert BertConfig.large()
BUCKET_BYTES = 32 * 2 ** 20


def run_one(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: needs a GPU")
    from mivod.ops import kernels as K
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16 if args.only == "bf16" else torch.float16
    n = BUCKET_BYTES // 2 if args.only == "bucket" else args.elements
    gen = torch.Generator(device=dev).manual_seed(11)
    x = torch.empty(n, dtype=dt, device=dev)
    for lo in range(0, n, 1 << 26):          # filled in pieces: no fp32 copy of the arena
        hi = min(n, lo + (1 << 26))
        x[lo:hi] = (torch.randn(hi - lo, device=dev, generator=gen) * 1e-2).to(dt)
    nc = K.sumsq_chunks(n)
    partial = torch.zeros(nc, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    clip = torch.zeros(2, dtype=torch.float32, device=dev)
    fns = {"nonfinite_scan": lambda: K.nonfinite_scan(x, flag),
           "grad_sumsq_flag": lambda: K.grad_sumsq(x, partial, flag),
           "grad_sumsq": lambda: K.grad_sumsq(x, partial),
           "clip_finalize": lambda: K.clip_finalize(partial, nc, clip, gscale=1.0, max_norm=1.0)}
    if args.only != "bucket":
        w = torch.zeros(n, dtype=torch.float32, device=dev)
        m, v = torch.zeros_like(w), torch.zeros_like(w)
        model = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        hp = dict(lr=1e-4, weight_decay=0.01, adamw=True, step=3)
        fns["adam_step"] = lambda: K.adam_step(x, w, m, v, model, **hp)
        fns["adam_step_clipped"] = lambda: K.adam_step(x, w, m, v, model, gclip=clip, **hp)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters               # ms per launch

    for fn in fns.values():
        timed(fn, args.warmup)
    rounds = {name: [] for name in fns}
    for _ in range(args.rounds):                          # alternating: one round of each in turn
        for name, fn in fns.items():
            rounds[name].append(timed(fn, args.iters))
    out = {"case": args.only, "dtype": str(dt).replace("torch.", ""), "elements": n,
           "bytes": n * x.element_size(), "partials": nc}
    for name, t in rounds.items():
        med = statistics.median(t)
        out[name] = {"ms": round(med, 4), "min_ms": round(min(t), 4),
                     "spread": round((max(t) - min(t)) / med, 4)}
        if name in ("nonfinite_scan", "grad_sumsq_flag", "grad_sumsq"):
            out[name]["gbps"] = round(out["bytes"] / (med * 1e-3) / 1e9, 1)
    scan = out["nonfinite_scan"]["ms"]
    out["sumsq_flag_over_scan"] = round(out["grad_sumsq_flag"]["ms"] / scan, 4)
    out["sumsq_over_scan"] = round(out["grad_sumsq"]["ms"] / scan, 4)
    if "adam_step" in out:
        out["clipped_over_unclipped_adam"] = round(out["adam_step_clipped"]["ms"]
                                                   / out["adam_step"]["ms"], 4)
    torch.cuda.synchronize()
    out["norm"] = round(float(clip[1]), 6)
    out["flag"] = int(flag.item())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--elements", type=int, default=BERT_LARGE_ELEMENTS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per case")
    args = ap.parse_args()
    if args.only:
        run_one(args)
        return
    res = {}
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--only", case, "--elements", str(args.elements), "--iters", str(args.iters),
               "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                  # nothing more starts on the GPU after a failure
            raise SystemExit(f"bench_clip: case {case} ended with status {p.returncode}")
        res[case] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps({"bench": "grad_norm_clip", "iters": args.iters, "rounds": args.rounds,
                      **res}))


if __name__ == "__main__":
    main()
