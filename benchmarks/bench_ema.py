#!/usr/bin/env python3
"""The fp32 weight-average update (``ema_decay`` of the Fused* optimizers) on one GPU, on
arenas of the size of ResNet-50 and BERT-Large: the one streaming pass of
csrc/kernels/mv_ema.hip over the fp32 master arena (read w and e, write e: 12 bytes per
element, one launch) against the same number of elements averaged the
``torch.optim.swa_utils.AveragedModel`` way (one ``lerp_`` launch per parameter tensor on the
bf16 model copy: read 2 + 2, write 2 bytes per element), and against
``torch._foreach_lerp_`` over the same tensors (what AveragedModel's multi_avg_fn does).

    python benchmarks/bench_ema.py                    # both models, one child process each
    python benchmarks/bench_ema.py --only bert_large  # one model in this process

All run on the same buffers, alternating round by round in one process; HIP events around
``--iters`` updates, ``--rounds`` rounds after ``--warmup`` updates; the figure is the median
round and ``spread`` is (max - min) / median of the rounds.  ``copy`` is the copying first
update (decay 0: the same launch, which still reads both streams, storing w).  Not a gate: the
feature's claim is the numerics (a bf16 average at decay 0.999 does not move,
tests/ema_reference.py).

Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["resnet50", "bert_large"]
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


def run_one(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: needs a GPU")
    from mivod.ops import kernels as K
    dev = torch.device("cuda", 0)
    sizes = param_sizes(args.only)
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + ALIGN - 1) // ALIGN * ALIGN
    elements = sum(sizes)
    gen = torch.Generator(device=dev).manual_seed(11)
    master = torch.empty(total, dtype=torch.float32, device=dev)
    for lo in range(0, total, 1 << 26):
        hi = min(total, lo + (1 << 26))
        master[lo:hi] = torch.randn(hi - lo, device=dev, generator=gen) * 1e-2
    ema = master.clone()
    model = master.to(torch.bfloat16)
    avg = model.clone()
    params = [model[o:o + n] for o, n in zip(offs, sizes)]
    avgs = [avg[o:o + n] for o, n in zip(offs, sizes)]
    omd = 1.0 - args.decay

    def arena():
        K.ema_update(master, ema, decay=args.decay)

    def copy():
        K.ema_update(master, ema, decay=0.0)

    def per_tensor():
        for a, p in zip(avgs, params):
            a.lerp_(p, omd)

    def foreach():
        torch._foreach_lerp_(avgs, params, omd)

    fns = {"arena": arena, "copy": copy, "per_tensor_bf16": per_tensor,
           "foreach_bf16": foreach}

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters               # ms per update

    for fn in fns.values():
        timed(fn, args.warmup)
    rounds = {name: [] for name in fns}
    for _ in range(args.rounds):                          # alternating: one round of each in turn
        for name, fn in fns.items():
            rounds[name].append(timed(fn, args.iters))
    nbytes = {"arena": total * 12, "copy": total * 12, "per_tensor_bf16": elements * 6,
              "foreach_bf16": elements * 6}
    launches = {"arena": 1, "copy": 1, "per_tensor_bf16": len(sizes), "foreach_bf16": None}
    out = {"case": args.only, "parameters": len(sizes), "elements": elements,
           "arena_elements": total, "ema_bytes": total * 4, "decay": args.decay}
    for name, t in rounds.items():
        med = statistics.median(t)
        out[name] = {"us": round(med * 1e3, 2), "gb": round(nbytes[name] / 1e9, 4),
                     "launches": launches[name],
                     "gbps": round(nbytes[name] / (med * 1e-3) / 1e9, 1),
                     "spread": round((max(t) - min(t)) / med, 4)}
    out["arena_over_per_tensor_time"] = round(out["arena"]["us"] / out["per_tensor_bf16"]["us"], 4)
    torch.cuda.synchronize()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=CASES)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per case")
    args = ap.parse_args()
    if args.only:
        run_one(args)
        return
    res = {}
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--only", case, "--decay", str(args.decay), "--iters", str(args.iters),
               "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                  # nothing more starts on the GPU after a failure
            raise SystemExit(f"bench_ema: case {case} ended with status {p.returncode}")
        res[case] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps({"bench": "ema_update", "iters": args.iters, "rounds": args.rounds, **res}))


if __name__ == "__main__":
    main()
