"""DistributedOptimizer with max_grad_norm, multi-rank scenarios, run as
`python tests/clip_workers.py <scenario> <device type> [...]` in 2 processes by
tests/test_clip_cpu.py (gloo CPU ranks, the fallbacks) and tests/test_clip_gpu.py (ranks sharing
one GPU over the gloo wire, the HIP kernels).  Every rank rebuilds ALL ranks' batches from
seeds, computes the single-process reference itself, asserts, and prints "OK <rank>"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mivod.torch as hvd  # noqa: E402

LR, MU, MAX_NORM = 0.05, 0.9, 0.5
# FusedSGD with momentum and no weight decay is linear in coef * g: d = coef * g,
# mom = MU * mom + d, w -= LR * mom.  The reference is fed the average of the ranks'
# gradients as the wire carries them (fp16-rounded on the fp16 wire), so what differs is the
# wire's own sum: one rounding to fp16, 2^-11 relative per element; the norm of such a
# gradient, and so the coefficient, is off by at most 2^-11 too.  d is therefore within
# 2 * 2^-11 = 2^-10 of the reference's, per element, and w within 2^-10 * LR * A summed over
# the steps, with A = MU * A + |d| the momentum of the magnitudes (mom itself can cancel).
# Without compression both sums are the same fp32 sum and only fp32 roundings differ (the
# 1/N folded into the kernel's gscale instead of into the gradient, the coefficient's 16 U):
# far inside the same tolerance.  WIRE_TOL doubles the 2^-10 for the second-order terms.
WIRE_TOL = 2 * 2.0 ** -10


def _same_all(rows, what=""):
    odd = [q for q in range(1, rows.shape[0]) if not torch.equal(rows[0], rows[q])]
    assert not odd, f"{what}: ranks {odd} differ from rank 0"


def _mlp(dev):
    torch.manual_seed(0)                       # the same initial model on every rank
    return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(),
                               torch.nn.Linear(32, 4)).to(dev)


def _loss(model, batch, scale):
    x, y = batch
    return scale * ((model(x) - y) ** 2).sum()


# loss scales of the steps: by the reference's own norms the first clips and the second not
SCALES = [1.0, 1e-3, 1.0, 1.0]


def dist_clip(device_type, wire):
    """``wire`` = fp16: fp16 compression with the overflow guard on (the norm and the guard's
    scan are one launch); none: no compression, guard off (the separate norm pass).  Steps 1
    and 2: each rank's parameters equal a single-process FusedSGD(max_grad_norm) fed the
    averaged gradients, within WIRE_TOL.  fp16 only: step 3, where rank 1 injects inf, leaves
    w and the momentum bitwise unchanged; step 4 applies again.  At the end the clip block,
    the parameters and the momentum are bitwise equal across ranks."""
    from mivod.optim import FusedSGD
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    dev = hvd.device()
    assert dev.type == device_type, (dev, device_type)
    fp16 = wire == "fp16"
    m = _mlp(dev)
    inner = FusedSGD(m.parameters(), lr=LR, momentum=MU, max_grad_norm=MAX_NORM)
    opt = hvd.DistributedOptimizer(
        inner, named_parameters=m.named_parameters(),
        compression=hvd.Compression.fp16 if fp16 else hvd.Compression.none,
        overflow_guard=fp16, bucket_mb=0.001, first_bucket_mb=0.0005)
    assert opt.guard_stats()["enabled"] == fp16
    assert len(opt.bucket_plan()) > 1, "the norm must span several buckets"
    ref = _mlp(dev)
    ref_opt = FusedSGD(ref.parameters(), lr=LR, momentum=MU, max_grad_norm=MAX_NORM)
    data = []
    for q in range(n):
        g = torch.Generator().manual_seed(100 + q)
        data.append((torch.randn(8, 16, generator=g).to(dev), torch.randn(8, 4, generator=g).to(dev)))
    inject = [False]

    def poison(gr):
        if inject[0]:
            gr = gr.clone()
            gr.view(-1)[0] = float("inf")
        return gr

    next(iter(m.parameters())).register_hook(poison)

    def step(s):
        opt.zero_grad()
        _loss(m, data[r], SCALES[s]).backward()
        opt.step()

    tol = [torch.zeros_like(p) for p in ref.parameters()]
    amom = [torch.zeros_like(p) for p in ref.parameters()]
    coefs = []
    for s in (0, 1):
        step(s)
        grads = None
        for q in range(n):
            ref.zero_grad()
            _loss(ref, data[q], SCALES[s]).backward()
            gs = [(p.grad.half().float() if fp16 else p.grad.clone()) for p in ref.parameters()]
            grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
        for p, g in zip(ref.parameters(), grads):
            p.grad = g / n
        ref_opt.step()
        coef = float(ref_opt._mv_clip_block[0])
        coefs.append(coef)
        norm, dnorm = float(ref_opt.grad_norm()), float(opt.grad_norm())
        print(f"step {s}: coef {coef:.6g}, norm single {norm:.6g} dist {dnorm:.6g}", flush=True)
        assert abs(dnorm - norm) <= WIRE_TOL * norm, (norm, dnorm)
        amom = [MU * a + coef * p.grad.abs() for a, p in zip(amom, ref.parameters())]
        tol = [t + WIRE_TOL * LR * a for t, a in zip(tol, amom)]
    assert coefs[0] < 0.9 and coefs[1] == 1.0, f"step 1 must clip and step 2 must not: {coefs}"
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for (nm, p), q, t in zip(m.named_parameters(), ref.parameters(), tol):
        err = (p.detach() - q.detach()).abs()
        print(f"{nm}: max |dist - single| {float(err.max()):.3g}, largest tolerance "
              f"{float(t.max()):.3g}", flush=True)
        assert (err <= t).all(), (nm, float((err - t).max()))

    def snapshot():
        return ([p.detach().clone() for p in m.parameters()]
                + [opt.state[p]["momentum_buffer"].clone() for p in m.parameters()])

    if fp16:
        s2 = snapshot()
        inject[0] = r == 1
        step(2)
        inject[0] = False
        s3 = snapshot()
        assert all(torch.equal(a, b) for a, b in zip(s2, s3)), "the overflowing step was not skipped"
        step(3)                                # the flags of the skipped step are read here
        s4 = snapshot()
        assert all(not torch.equal(a, b) for a, b in zip(s3, s4)), "the step after the skip"
        assert opt.guard_stats()["skipped_steps"] == 1, opt.guard_stats()
    flat = torch.cat([t.reshape(-1) for t in snapshot()] + [opt._mv_clip_block.reshape(-1)])
    assert torch.isfinite(flat).all()
    _same_all(hvd.allgather(flat.unsqueeze(0)), "clip block, parameters and momentum")
    hvd.shutdown()
    print("OK", r)


def clip_args(device_type):
    """Run with MIVOD_GUARD_MODE=bucket: wrapping a clipped fused optimizer with the guard on
    raises on every rank; without the guard the mode does not matter, and ranks that disagree
    on max_grad_norm raise through the plan hash."""
    from mivod.optim import FusedSGD
    assert os.environ.get("MIVOD_GUARD_MODE") == "bucket"
    hvd.init()
    r = hvd.rank()
    m = _mlp(hvd.device())
    try:
        hvd.DistributedOptimizer(FusedSGD(m.parameters(), lr=LR, max_grad_norm=1.0),
                                 named_parameters=m.named_parameters(),
                                 compression=hvd.Compression.fp16)
        raise AssertionError("bucket mode with max_grad_norm was accepted")
    except ValueError as e:
        assert "MIVOD_GUARD_MODE=bucket" in str(e), e
    m = _mlp(hvd.device())
    try:
        hvd.DistributedOptimizer(FusedSGD(m.parameters(), lr=LR, max_grad_norm=1.0 + r),
                                 named_parameters=m.named_parameters(),
                                 compression=hvd.Compression.none)
        raise AssertionError("ranks that disagree on max_grad_norm were accepted")
    except ValueError as e:
        assert "differs across ranks" in str(e) and "max_grad_norm" in str(e), e
    m = _mlp(hvd.device())
    hvd.DistributedOptimizer(FusedSGD(m.parameters(), lr=LR, max_grad_norm=1.0),
                             named_parameters=m.named_parameters(),
                             compression=hvd.Compression.none)
    hvd.shutdown()
    print("OK", r)


if __name__ == "__main__":
    # a hung rank prints every thread's stack and exits before the runner's limit
    import faulthandler
    import signal
    _dump = float(os.environ.get("MIVOD_TEST_DUMP_AFTER", "0"))
    if _dump > 0:
        faulthandler.dump_traceback_later(_dump, exit=True)
    faulthandler.register(signal.SIGUSR1, all_threads=True)
    globals()[sys.argv[1]](*sys.argv[2:])
