#!/usr/bin/env python3
"""The standalone ``step()`` of ``FusedLAMB`` on one GPU, on the flat arena of a BERT-Large
(``mivod.models.bert``, the constructor arguments of ``benchmarks/bench_bert.py --model
large``: bf16 model, fp32 master and moments, bf16 gradients), against two yardsticks on the
same arena: ``FusedAdamW`` (one streaming kernel, 28 B/element) and an unfused LAMB written
here with ``torch._foreach_*`` ops on fp32 copies.

    python benchmarks/bench_lamb.py                 # the three variants, one child process each
    python benchmarks/bench_lamb.py --only lamb     # one variant in this process

Each variant runs in a process of its own under its own time limit (``--limit`` seconds), so
a variant that hangs or runs out of memory costs its own figure only.  Timing: HIP events
around ``--iters`` steps, ``--rounds`` rounds after ``--warmup`` steps; the figure is the
median round (the fastest is printed next to it).  ``step()`` packs the parameters'
gradients into the arena and then runs the fused update; ``update`` is the update alone on
an already packed arena (what DistributedOptimizer launches per bucket).

Bytes, counted from the kernels, per parameter element: LAMB stage 1 reads g (2), w, m, v
(12) and writes m, v (8); stage 2 reads w, m, v (12) and writes w and the bf16 copy (6):
40.  AdamW reads 14 and writes 14: 28.  The GB/s printed are these counts over the measured
update time; the counts predict LAMB at 40/28 = 1.43 of AdamW.

Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ["lamb", "adamw", "foreach"]
BYTES = {"lamb": 40, "adamw": 28}
HP = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
LAMB_EPS = 1e-6


def foreach_lamb_step(w, g, m, v, decay, model, step, lr, b1, b2, eps, wd):
    """One LAMB step with the semantics of mivod.ops.kernels.lamb_step on lists of fp32
    tensors; ``decay[i]`` False: no weight decay and trust 1 (1-D parameters)."""
    import torch
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    torch._foreach_mul_(m, b1)
    torch._foreach_add_(m, g, alpha=1 - b1)
    torch._foreach_mul_(v, b2)
    torch._foreach_addcmul_(v, g, g, value=1 - b2)
    den = torch._foreach_sqrt(v)
    torch._foreach_div_(den, math.sqrt(bc2))
    torch._foreach_add_(den, eps)
    u = torch._foreach_div(m, den)
    torch._foreach_div_(u, bc1)
    ud = [x for x, d in zip(u, decay) if d]
    wdec = [x for x, d in zip(w, decay) if d]
    torch._foreach_add_(ud, wdec, alpha=wd)
    wn = torch.stack(torch._foreach_norm(wdec))
    un = torch.stack(torch._foreach_norm(ud))
    trust = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
    torch._foreach_mul_(ud, list((-lr * trust).unbind()))
    up = [x for x, d in zip(u, decay) if not d]
    torch._foreach_mul_(up, -lr)
    torch._foreach_add_(w, u)
    torch._foreach_copy_(model, w)


def run_one(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lamb: needs a GPU")
    from mivod.models.bert import BertConfig, BertForPreTraining
    from mivod.optim import FusedAdamW, FusedLAMB
    dev = torch.device("cuda", 0)
    cfg = getattr(BertConfig, args.model)()
    torch.manual_seed(7)
    model = BertForPreTraining(cfg).to(dev).to(torch.bfloat16)
    params = [p for p in model.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(11)
    for p in params:
        p.grad = (torch.randn(p.shape, device=dev, generator=gen) * 1e-2).to(p.dtype)
    numel = sum(p.numel() for p in params)
    out = {"variant": args.only, "elements": numel, "tensors": len(params)}

    if args.only == "foreach":
        w = [p.detach().float() for p in params]
        g = [p.grad.float() for p in params]
        m = [torch.zeros_like(x) for x in w]
        v = [torch.zeros_like(x) for x in w]
        decay = [p.dim() > 1 for p in params]
        mod = [p.data for p in params]
        count = [0]

        def step():
            count[0] += 1
            foreach_lamb_step(w, g, m, v, decay, mod, count[0], HP["lr"], *HP["betas"], LAMB_EPS,
                              HP["weight_decay"])
        fns = {"step": step}
    else:
        opt = (FusedLAMB(params, eps=LAMB_EPS, **HP) if args.only == "lamb"
               else FusedAdamW(params, **HP))
        arenas = opt._mv_build()
        out["arena_elements"] = sum(a.numel for a in arenas)

        def update():
            opt._mv_begin_step()
            for a in arenas:
                opt._mv_apply(a, 0, len(a.params), 1.0)
            opt._mv_end_step()
        fns = {"step": opt.step, "update": update}

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters               # ms per call

    for name, fn in fns.items():
        timed(fn, args.warmup)
        t = [timed(fn, args.iters) for _ in range(args.rounds)]
        out[f"{name}_ms"] = round(statistics.median(t), 4)
        out[f"{name}_min_ms"] = round(min(t), 4)
    if args.only in BYTES:
        out["bytes_per_element"] = BYTES[args.only]
        out["update_gbps"] = round(BYTES[args.only] * numel / (out["update_ms"] * 1e-3) / 1e9, 1)
    finite = all(bool(torch.isfinite(p.float()).all()) for p in params[:8])
    out["finite"] = finite
    print(json.dumps(out), flush=True)
    if not finite:
        raise SystemExit("bench_lamb: non-finite parameters")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--model", default="large", choices=["large", "base", "tiny"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per variant")
    args = ap.parse_args()
    if args.only:
        run_one(args)
        return
    res = {}
    for var in VARIANTS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--only", var, "--model", args.model, "--iters", str(args.iters), "--rounds",
               str(args.rounds), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                  # nothing more starts on the GPU after a failure
            raise SystemExit(f"bench_lamb: variant {var} ended with status {p.returncode}")
        res[var] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    rec = {"bench": "fused_lamb_step", "model": f"bert-{args.model}",
           "elements": res["lamb"]["elements"], "iters": args.iters, "rounds": args.rounds,
           **{k: res[k] for k in VARIANTS},
           "lamb_over_adamw_update": round(res["lamb"]["update_ms"] / res["adamw"]["update_ms"], 3),
           "lamb_over_adamw_step": round(res["lamb"]["step_ms"] / res["adamw"]["step_ms"], 3),
           "foreach_over_lamb_step": round(res["foreach"]["step_ms"] / res["lamb"]["step_ms"], 3),
           "predicted_lamb_over_adamw": round(40 / 28, 3)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
