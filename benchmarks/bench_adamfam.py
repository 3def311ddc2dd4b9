#!/usr/bin/env python3
"""The fused update of ``FusedAdam(amsgrad=True)``, ``FusedAdamax`` and ``FusedNAdam`` on one
GPU, on flat arenas the size of a ResNet-50 (25.6M elements) and of a BERT-Large (336M
elements): bf16 model, fp32 master and state, fp16 gradient arena (the fp16 wire of
DistributedOptimizer).  Yardsticks in the same process, each on an arena of its own of the same
size, all resident together: ``FusedAdamW`` (adam_flat_kernel, 28 B/element) and
``torch.optim.Adam(amsgrad=True, foreach=True)`` on fp32 copies of the parameters (what a mixed
precision recipe without mivod keeps: fp32 master, fp32 gradients, no bf16 copy).

    python benchmarks/bench_adamfam.py --rounds 15         # both arenas, every variant
    python benchmarks/bench_adamfam.py --arena resnet50 --only adamax adamw

The arenas are synthetic: equal tensors (160 x 160,000 and 384 x 875,000 elements), since one
launch covers the whole arena whatever its tensors are; only the foreach yardstick sees them.

Timing: HIP events around ``iters`` updates (enough of them that a window lasts tens of
milliseconds), ``--rounds`` windows per variant after ``--warmup`` updates, the variants of an
arena taking turns window by window; the figure is the median window (the fastest and the
slowest are printed next to it).  ``update`` is what DistributedOptimizer launches per
bucket: the fused kernel on an already packed gradient arena, here one launch over the arena.

Bytes per element, counted from the kernels (mv_adamfam.hip): g 2, w 4 + 4, bf16 copy 2, and
8 per state buffer: 28 for Adamax and NAdam, as for AdamW; 36 with amsgrad's third stream.  The
TB/s printed are these counts over the measured time, and ``vs_adamw`` stands next to the ratio
the counts predict.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARENAS = {"resnet50": (160, 160_000, 400), "bert_large": (384, 875_000, 40)}   # n, numel, iters
VARIANTS = ["adam_amsgrad", "adamax", "nadam", "adamw", "torch_foreach_adam_amsgrad"]
BYTES = {"adam_amsgrad": 36, "adamax": 28, "nadam": 28, "adamw": 28}


def make_fused(name, params):
    import torch
    from mivod.optim import FusedAdam, FusedAdamax, FusedAdamW, FusedNAdam
    kw = dict(grad_dtype=torch.float16)
    if name == "adam_amsgrad":
        return FusedAdam(params, lr=1e-3, amsgrad=True, **kw)
    if name == "adamax":
        return FusedAdamax(params, lr=1e-3, **kw)
    if name == "nadam":
        return FusedNAdam(params, lr=1e-3, **kw)
    return FusedAdamW(params, lr=1e-3, **kw)


def run_arena(arena, only, args):
    import torch
    dev = torch.device("cuda", 0)
    ntens, numel, iters = ARENAS[arena]
    iters = args.iters or iters
    gen = torch.Generator(device=dev).manual_seed(11)
    out = {"elements": ntens * numel, "tensors": ntens, "iters": iters}

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k               # ms per call

    def fused_update(opt, arenas):
        def update():
            for a in arenas:
                opt._mv_apply(a, 0, len(a.params), 1.0)
        return update

    fns, check, keep = {}, {}, []
    for name in only:
        params = [torch.nn.Parameter((torch.randn(numel, device=dev, generator=gen) * 0.1)
                                     .to(torch.bfloat16)) for _ in range(ntens)]
        if name == "torch_foreach_adam_amsgrad":
            ws = [torch.nn.Parameter(p.detach().float()) for p in params]
            for w in ws:
                w.grad = torch.randn(numel, device=dev, generator=gen) * 1e-2
            opt = torch.optim.Adam(ws, lr=1e-3, amsgrad=True, foreach=True)
            fns[name], check[name] = opt.step, ws[:4]
        else:
            opt = make_fused(name, params)
            arenas = opt._mv_build()
            for a in arenas:
                a.grad.copy_((torch.randn(a.numel, device=dev, generator=gen) * 1e-2))
            opt._mv_begin_step()       # once: the per-step host bookkeeping is not the kernel's
            fns[name], check[name] = fused_update(opt, arenas), params[:4]
        keep.append(opt)
    for fn in fns.values():
        timed(fn, args.warmup)
    # the variants take turns, window by window, so that a drift of the machine (clocks, other
    # people's work on the host) meets all of them alike
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, iters))
    for name, t in times.items():
        rec = {"ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
               "max_ms": round(max(t), 4)}
        if name in BYTES:
            rec["bytes_per_element"] = BYTES[name]
            rec["tbps"] = round(BYTES[name] * out["elements"] / (rec["ms"] * 1e-3) / 1e12, 3)
        rec["finite"] = all(bool(torch.isfinite(p.float()).all()) for p in check[name])
        out[name] = rec
        print(f"# {arena} {name}: {rec}", file=sys.stderr, flush=True)
        if not rec["finite"]:
            raise SystemExit(f"bench_adamfam: non-finite parameters after {name}")
    del fns, check, keep
    torch.cuda.empty_cache()
    if "adamw" in out:
        for name in only:
            if name != "adamw":
                out[name]["vs_adamw"] = round(out[name]["ms"] / out["adamw"]["ms"], 3)
                if name in BYTES:
                    out[name]["vs_adamw_predicted"] = round(BYTES[name] / BYTES["adamw"], 3)
    if "adam_amsgrad" in out and "torch_foreach_adam_amsgrad" in out:
        out["torch_foreach_over_fused_adam_amsgrad"] = round(
            out["torch_foreach_adam_amsgrad"]["ms"] / out["adam_amsgrad"]["ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arena", nargs="+", choices=sorted(ARENAS), default=list(ARENAS))
    ap.add_argument("--only", nargs="+", choices=VARIANTS, default=VARIANTS)
    ap.add_argument("--iters", type=int, default=0, help="updates per window (0: per arena)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_adamfam: needs a GPU")
    rec = {"bench": "fused_adamfam_update", "rounds": args.rounds, "warmup": args.warmup}
    for arena in args.arena:
        rec[arena] = run_arena(arena, args.only, args)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
