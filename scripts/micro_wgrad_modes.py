"""mivod's BERT-shape weight gradients (mv_gemm256.hip wgrad256_kernel) alone, for timing
and for PMC passes; --zeros runs zero-filled operands (the DVFS check: the same instruction
stream at the clock the chip holds without data toggling), --blaslt adds hipBLASLt's forward
GEMM of the same FLOPs as a reference.
    python scripts/micro_wgrad_modes.py [--iters 20] [--shape 3072x1024] [--zeros] [--blaslt]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mivod.ops import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--shape", default="")
ap.add_argument("--zeros", action="store_true")
ap.add_argument("--blaslt", action="store_true")
a = ap.parse_args()
nat = K.native()
dev = torch.device("cuda")
T = 65536


def timeit(tag, fn, N, Kd):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.iters * 1000.0
    print(f"{tag:10s} {'zeros' if a.zeros else 'randn'} "
          f"[{N} x {Kd}] over {T}: {us:7.1f} us ({2.0 * T * N * Kd / us / 1e6:5.0f} TF/s)",
          flush=True)


shapes = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]
if a.shape:
    shapes = [tuple(int(v) for v in a.shape.split("x"))]
for N, Kd in shapes:
    x = torch.randn(T, Kd, device=dev).to(torch.bfloat16)
    dy = (torch.randn(T, N, device=dev) * 0.01).to(torch.bfloat16)
    w = (torch.randn(N, Kd, device=dev) * 0.03).to(torch.bfloat16)
    if a.zeros:
        for t in (x, dy, w):
            t.zero_()
    timeit("wgrad", lambda: nat.wgrad1x1(x.view(T, Kd, 1, 1), dy.view(T, N, 1, 1), 1, False,
                                         None), N, Kd)
    if a.blaslt:
        timeit("blaslt-fwd", lambda: torch.nn.functional.linear(x, w), N, Kd)
