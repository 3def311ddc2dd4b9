"""DistributedOptimizer(backward_passes_per_step=k, accumulation_dtype=torch.float32),
multi-rank scenarios, run as `python tests/accum_workers.py <scenario> <device type> [...]` in
2 processes by tests/test_accum_cpu.py (gloo CPU ranks, the fallbacks) and
tests/test_accum_gpu.py (ranks sharing one GPU over the gloo wire, the HIP kernels).  Every rank
rebuilds ALL ranks' micro-batches from seeds, computes the float64 reference itself, asserts,
and prints "OK <rank>"."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import accum_reference as R  # noqa: E402
import mivod.torch as hvd  # noqa: E402

K_PASSES = 4


def _same_all(rows, what=""):
    odd = [q for q in range(1, rows.shape[0]) if not torch.equal(rows[0], rows[q])]
    assert not odd, f"{what}: ranks {odd} differ from rank 0"


def _setup(device_type, **kw):
    from mivod.optim import FusedSGD
    hvd.init()
    dev = hvd.device()
    assert dev.type == device_type, (dev, device_type)
    net = R.make_net(dev)                          # the same initial model on every rank
    twin = copy.deepcopy(net)
    opt = hvd.DistributedOptimizer(FusedSGD(net.parameters(), lr=0.1, momentum=0.9),
                                   named_parameters=net.named_parameters(),
                                   backward_passes_per_step=K_PASSES,
                                   accumulation_dtype=torch.float32, bucket_mb=0.002,
                                   first_bucket_mb=0.001, **kw)
    assert len(opt.bucket_plan()) > 1
    return dev, net, twin, opt


def _window(dev, net, twin, opt):
    """One window of per-rank micro-batches; every rank's float64 (sum, magnitudes)."""
    r, n = hvd.rank(), hvd.size()
    data = [R.make_batches(dev, K_PASSES, seed=100 + q) for q in range(n)]
    R.run_passes(opt, net, data[r])
    opt.synchronize()
    R._sync(dev)
    return [R.twin_sums(twin, data[q]) for q in range(n)]


def _same_bits(opt, what):
    flat = torch.cat([a.grad.float().reshape(-1) for a in opt._mvd_arenas]
                     + [a.master.reshape(-1) for a in opt._mvd_arenas])
    assert torch.isfinite(flat).all()
    _same_all(hvd.allgather(flat.unsqueeze(0)), what)


def dist_average(device_type):
    """Average with the fp16 wire and the guard on.  The fused path reduces the SUM over the
    ranks on the wire and folds 1/N into the update, so the averaged gradient is the reduced
    buffer / N.  Its bound: every rank's wire value is within the wire bound of its own sum
    (tests/accum_reference.py) and the errors add; the reduction of N fp16 values rounds at
    most N-1 times to fp16 (an fp32 intermediate adds 2^-24 relative, inside the slack of
    the subnormal term), each rounding relative to a partial sum of at most the sum of the
    stored magnitudes."""
    dev, net, twin, opt = _setup(device_type, compression=hvd.Compression.fp16)
    assert opt.guard_stats()["enabled"]
    sums = _window(dev, net, twin, opt)
    n = hvd.size()
    worst = 0.0
    per_rank = [R.arena_reference(opt, net, *s) for s in sums]
    for ai, a in enumerate(opt._mvd_arenas):
        refs = [per_rank[q][ai][1] for q in range(n)]
        mags = [per_rank[q][ai][2] for q in range(n)]
        ref = sum(refs) / n
        tol = sum(R.wire_tol(rq, mq, K_PASSES, 1.0, R.f16) for rq, mq in zip(refs, mags))
        stored = sum(rq.abs() for rq in refs) + tol
        tol = (tol + (n - 1) * (R.HALF_ULP[R.f16] * stored + 2.0 ** -25)) / n
        err = (R.FR.f64(a.grad) / n - ref).abs()
        assert (err <= tol).all(), f"{int((err > tol).sum())} elements outside the bound"
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
    print(f"average, fp16 wire: worst err/tol {worst:.3f}", flush=True)
    _same_bits(opt, "reduced gradient and master weights")
    assert opt.guard_stats()["skipped_steps"] == 0
    r = hvd.rank()
    hvd.shutdown()
    print("OK", r)


def dist_adasum(device_type):
    """Adasum of the two ranks' sums a and b, per parameter tensor: f = ca*a + cb*b with
    ca = 1 - a.b / (2 |a|^2), cb = 1 - a.b / (2 |b|^2), in float64 from the float64 sums.
    The wire is the parameters' bf16, so e = 2^-8 (half an ulp) governs: the stored a~, b~ are
    within e (1 + small) of a, b element by element (the fp32 part of the wire bound is 2^-16
    of that); then |a~.b~ - a.b| <= (2e + e^2) |a||b| and ||a~|^2 - |a|^2| <= (2e + e^2) |a|^2,
    so ca moves by at most ~2.1 e |b|/|a| (cb: |a|/|b|); the result is rounded to bf16 once
    more.  Element by element
        |f~ - f| <= 1.1 e ((|ca| + 2.1 |b|/|a|) |a_i| + (|cb| + 2.1 |a|/|b|) |b_i| + |f_i|),
    the factor 1.1 covering the second-order terms and the fp32 roundings of the merge; plus
    the fp32 part of the two wire bounds, (k+1) U sum|g|, times |ca| and |cb| (it matters only
    where the passes cancel, so that sum|g| is far above |a_i|)."""
    dev, net, twin, opt = _setup(device_type, compression=hvd.Compression.none, op=hvd.Adasum)
    assert hvd.size() == 2
    sums = _window(dev, net, twin, opt)
    (ra, ma), (rb, mb) = sums
    u5 = (K_PASSES + 1) * R.U
    e = R.HALF_ULP[R.bf16]
    index = {id(p): i for i, p in enumerate(net.parameters())}
    worst = 0.0
    for a in opt._mvd_arenas:
        assert a.grad.dtype == R.bf16
        for i, p in enumerate(a.params):
            x, y = ra[index[id(p)]], rb[index[id(p)]]
            mx, my = ma[index[id(p)]], mb[index[id(p)]]
            dot, nx, ny = float((x * y).sum()), float((x * x).sum()), float((y * y).sum())
            ca, cb = 1 - dot / (2 * nx), 1 - dot / (2 * ny)
            f = ca * x + cb * y
            rx, ry = (ny / nx) ** 0.5, (nx / ny) ** 0.5
            tol = 1.1 * e * ((abs(ca) + 2.1 * rx) * x.abs() + (abs(cb) + 2.1 * ry) * y.abs()
                             + f.abs())
            tol = tol + 1.1 * u5 * (abs(ca) * mx + abs(cb) * my)
            err = (R.FR.f64(a.slot(a.grad, i)) - f).abs()
            assert (err <= tol).all(), (i, float((err / tol).max()))
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
    print(f"adasum, bf16 wire: worst err/tol {worst:.3f}", flush=True)
    _same_bits(opt, "reduced gradient and master weights")
    r = hvd.rank()
    hvd.shutdown()
    print("OK", r)


def accum_args(device_type):
    """Ranks that disagree on accumulation_dtype fail the plan check on every rank; ranks that
    agree pass it."""
    hvd.init()
    r = hvd.rank()
    net = R.make_net(hvd.device())
    try:
        hvd.DistributedOptimizer(torch.optim.SGD(net.parameters(), lr=0.1),
                                 named_parameters=net.named_parameters(),
                                 backward_passes_per_step=2,
                                 accumulation_dtype=torch.float32 if r == 0 else None)
        raise AssertionError("ranks that disagree on accumulation_dtype were accepted")
    except ValueError as e:
        assert "differs across ranks" in str(e) and "accumulation_dtype" in str(e), e
    net = R.make_net(hvd.device())
    hvd.DistributedOptimizer(torch.optim.SGD(net.parameters(), lr=0.1),
                             named_parameters=net.named_parameters(),
                             backward_passes_per_step=2, accumulation_dtype=torch.float32)
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
