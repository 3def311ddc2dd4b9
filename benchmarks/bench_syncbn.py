#!/usr/bin/env python3
"""Forward + backward of ``hvd.SyncBatchNorm`` against the local fused ``ops.bn.BatchNorm2d``
on the BN shapes of one ResNet-50 step at 32 images per GPU (bf16 NHWC, BN + ReLU), the
regime SyncBatchNorm is for.  What it costs over local BN is two extra launches and one
collective per direction.  Run it at world size 1 with the collectives forced, so mivod's
RCCL communicator really carries the records:

    MIVOD_TRANSPORT=rccl MIVOD_FORCE_COLLECTIVES=1 timeout 300 python benchmarks/bench_syncbn.py

Timing: HIP events around ``--iters`` forward+backward pairs, local and sync alternating in
``--rounds`` rounds of one process; the figure is the median round.  Prints one JSON line:
per shape the microseconds per layer of both, and the 53-layer totals."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mivod.torch as hvd  # noqa: E402
from mivod.ops.bn import BatchNorm2d  # noqa: E402

# (channels, height = width, layers of that shape in ResNet-50): 53 BN layers
SHAPES = [(64, 112, 1), (64, 56, 6), (256, 56, 4), (128, 56, 1), (128, 28, 7), (512, 28, 5),
          (256, 28, 1), (256, 14, 11), (1024, 14, 7), (512, 14, 1), (512, 7, 5), (2048, 7, 4)]


def _time(mod, x, g, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        x.grad = None
        mod(x, relu=True).backward(g)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per forward + backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_syncbn: needs a GPU")
    hvd.init()
    dev = hvd.device()
    from mivod.common import basics
    rows, tot_l, tot_s = [], 0.0, 0.0
    for c, hw, count in SHAPES:
        x = torch.randn(args.batch, c, hw, hw, device=dev).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last).requires_grad_()
        g = torch.randn(args.batch, c, hw, hw, device=dev).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)
        mods = {"local": BatchNorm2d(c).to(dev), "sync": hvd.SyncBatchNorm(c).to(dev)}
        for m in mods.values():
            _time(m, x, g, args.warmup)
        t = {k: [] for k in mods}
        for _ in range(args.rounds):
            for k, m in mods.items():
                t[k].append(_time(m, x, g, args.iters))
        loc, syn = statistics.median(t["local"]), statistics.median(t["sync"])
        rows.append({"C": c, "HW": hw, "layers": count, "local_us": round(loc, 1),
                     "sync_us": round(syn, 1), "local_min_us": round(min(t["local"]), 1),
                     "sync_min_us": round(min(t["sync"]), 1)})
        tot_l += loc * count
        tot_s += syn * count
    st = basics.state()
    print(json.dumps({"bench": "syncbn_fwd_bwd", "batch": args.batch, "world": hvd.size(),
                      "transport": st.gpu.name if st.gpu is not None else "none (no collective)",
                      "iters": args.iters, "rounds": args.rounds, "shapes": rows,
                      "local_us_53_layers": round(tot_l, 1),
                      "sync_us_53_layers": round(tot_s, 1),
                      "sync_over_local": round(tot_s / tot_l, 3)}))
    hvd.shutdown()


if __name__ == "__main__":
    main()
