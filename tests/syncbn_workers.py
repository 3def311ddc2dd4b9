"""SyncBatchNorm multi-rank scenarios, run as `python tests/syncbn_workers.py <scenario>` in N
processes by tests/test_syncbn_cpu.py (gloo) and tests/test_syncbn_gpu.py (ranks sharing one
GPU over gloo-gpu, or one rank on RCCL).  Every rank rebuilds ALL ranks' inputs from seeds,
computes the single-process reference on the concatenated batch itself, asserts, and prints
"OK <rank>" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import mivod.torch as hvd  # noqa: E402

EPS = 1e-5


def _same_all(rows, what=""):
    """Every rank's row bitwise equal to rank 0's (rows = an allgather result)."""
    odd = [q for q in range(1, rows.shape[0]) if not torch.equal(rows[0], rows[q])]
    assert not odd, f"{what}: ranks {odd} differ from rank 0"


def _ref64(xs, gs, w, b, relu, ress):
    """float64 BatchNorm (+ residual) (+ ReLU) over the concatenation of the ranks' inputs.
    Returns per rank (y, dx, dgamma, dbeta, dres) — dgamma / dbeta from that rank's rows and
    the GLOBAL x-hat — and the global (mean, unbiased variance)."""
    x = torch.cat(xs).double().requires_grad_()
    res = torch.cat(ress).double().requires_grad_() if ress is not None else None
    w64, b64 = w.double(), b.double()
    dims = [0] + list(range(2, x.dim()))
    shape = [1, -1] + [1] * (x.dim() - 2)
    mean = x.detach().mean(dims)
    var = x.detach().var(dims, unbiased=False)
    y = F.batch_norm(x, None, None, w64, b64, True, 0.0, EPS)
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    g = torch.cat(gs).double()
    (y * g).sum().backward()
    xhat = (x.detach() - mean.view(shape)) * torch.rsqrt(var + EPS).view(shape)
    dz = g * (y.detach() > 0) if relu else g
    out, o = [], 0
    for xr in xs:
        k = xr.shape[0]
        sl = slice(o, o + k)
        out.append((y.detach()[sl], x.grad[sl], (dz[sl] * xhat[sl]).sum(dims), dz[sl].sum(dims),
                    res.grad[sl] if res is not None else None))
        o += k
    m = x.numel() // x.shape[1]
    return out, mean, var * m / max(m - 1, 1)


def cpu_fallback():
    """The plain-torch path on gloo CPU ranks: fp32, rank r holds 2 + r rows (4-D) / 3 + r
    rows (2-D), plain / ReLU / add+ReLU, against the float64 reference."""
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    c = 6
    g0 = torch.Generator().manual_seed(5)
    w = torch.rand(c, generator=g0) + 0.5
    b = torch.randn(c, generator=g0) * 0.1
    # fp32 statistics over <= 100 rows of O(1) data: a few roundings of 6e-8 each
    tol = dict(rtol=1e-4, atol=1e-5)
    for shape_of in (lambda q: (2 + q, c, 3, 5), lambda q: (3 + q, c)):
        for relu, use_res in ((False, False), (True, False), (True, True)):
            xs, gs, ress = [], [], []
            for q in range(n):
                g = torch.Generator().manual_seed(100 + q)
                xs.append(torch.randn(shape_of(q), generator=g) * 2 + 3)
                gs.append(torch.randn(shape_of(q), generator=g))
                ress.append(torch.randn(shape_of(q), generator=g))
            ref, mean, unb = _ref64(xs, gs, w, b, relu, ress if use_res else None)
            m = hvd.SyncBatchNorm(c)
            with torch.no_grad():
                m.weight.copy_(w)
                m.bias.copy_(b)
            x = xs[r].clone().requires_grad_()
            res = ress[r].clone().requires_grad_() if use_res else None
            y = m(x, res, relu)
            (y * gs[r]).sum().backward()
            yr, dxr, dgr, dbr, drr = ref[r]
            what = f"{tuple(x.shape)} relu={relu} res={use_res}"
            print(what, flush=True)
            torch.testing.assert_close(y.detach().double(), yr, **tol)
            torch.testing.assert_close(x.grad.double(), dxr, **tol)
            torch.testing.assert_close(m.weight.grad.double(), dgr, **tol)
            torch.testing.assert_close(m.bias.grad.double(), dbr, **tol)
            if use_res:
                torch.testing.assert_close(res.grad.double(), drr, **tol)
            torch.testing.assert_close(m.running_mean.double(), 0.1 * mean, **tol)
            torch.testing.assert_close(m.running_var.double(), 0.9 + 0.1 * unb, **tol)
            stats = torch.cat((m.running_mean, m.running_var))
            _same_all(hvd.allgather(stats.unsqueeze(0)), what)
    hvd.shutdown()
    print("OK", r)


class _Net(torch.nn.Module):
    """conv -> SyncBatchNorm(relu) -> conv -> SyncBatchNorm(residual, relu); ``sync=False``
    builds the single-process reference: the same bf16 convolutions around fp32 torch
    BatchNorm.  With ``sizes`` the reference runs each convolution per rank-sized piece of
    the concatenated batch, as the ranks do: a convolution library may round the last bf16
    bit differently at another batch size, and a BatchNorm turns one such bit of its input
    into |z| / std(z) * 2^-8 of its output, which says nothing about the BatchNorm."""

    def __init__(self, sync: bool, c: int = 16):
        super().__init__()
        bn = hvd.SyncBatchNorm if sync else torch.nn.BatchNorm2d
        self.sync = sync
        self.conv1 = torch.nn.Conv2d(8, c, 3, padding=1, bias=False)
        self.bn1 = bn(c)
        self.conv2 = torch.nn.Conv2d(c, c, 3, padding=1, bias=False)
        self.bn2 = bn(c)

    def _bn(self, bn, z, res, relu):
        if self.sync:
            from mivod.ops.bn import _fusable
            z = z.contiguous(memory_format=torch.channels_last)
            assert _fusable(z, bn.weight), "this scenario is about the fused path"
            return bn(z, res, relu)
        y = bn(z.float())
        if res is not None:
            y = y + res.float()
        return F.relu(y).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def forward(self, x, sizes=None):
        def conv(c, t):
            return c(t) if sizes is None else torch.cat([c(p) for p in t.split(sizes)])
        h = self._bn(self.bn1, conv(self.conv1, x), None, True)
        return self._bn(self.bn2, conv(self.conv2, h), h, True)


def _mixed(net, dev):
    net = net.to(dev).to(memory_format=torch.channels_last)
    net.conv1.to(torch.bfloat16)
    net.conv2.to(torch.bfloat16)
    return net


def gpu_model():
    """A two-BN model on the fused path: rank r holds 2 + r images.  First step: outputs
    and dx against the single-process reference on the concatenated batch (tolerances of
    tests/test_bn_gpu.py); after two DistributedOptimizer steps: running statistics and
    parameters bitwise equal on all ranks.  On a 1-rank RCCL world with every collective
    forced, RCCL carries the records: the transport's call count says so."""
    from mivod.common import basics as B
    from mivod.optim import FusedSGD
    from mivod.parallel import collectives as C
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    dev = hvd.device()
    assert dev.type == "cuda"
    forced = os.environ.get("MIVOD_FORCE_COLLECTIVES") == "1"
    if forced:
        assert B.state().gpu is not None and B.state().gpu.name == "rccl", B.state().backend
    torch.manual_seed(3)                       # the same initial model on every rank
    net = _mixed(_Net(True), dev)
    ref = _mixed(_Net(False), dev)
    ref.load_state_dict(net.state_dict())
    with torch.no_grad():                      # non-trivial affine parameters
        for m in (net, ref):
            for bn in (m.bn1, m.bn2):
                bn.weight.copy_(torch.linspace(0.5, 1.0, bn.num_features))
                bn.bias.copy_(torch.linspace(-0.2, 0.2, bn.num_features))
    xs, gs = [], []
    for q in range(n):
        g = torch.Generator().manual_seed(200 + q)
        xs.append(torch.randn(2 + q, 8, 6, 5, generator=g).to(dev, torch.bfloat16)
                  .contiguous(memory_format=torch.channels_last))
        gs.append(torch.randn(2 + q, 16, 6, 5, generator=g).to(dev))
    opt = hvd.DistributedOptimizer(FusedSGD(net.parameters(), lr=0.05, momentum=0.9),
                                   named_parameters=net.named_parameters())
    for step in range(2):
        x = xs[r].clone().requires_grad_()
        calls0 = C.gpu_stats().get("calls", 0)
        y = net(x)
        if forced:       # one allgather per SyncBatchNorm layer
            assert C.gpu_stats()["calls"] - calls0 >= 2, C.gpu_stats()
        (y.float() * gs[r]).sum().backward()
        if forced:       # + one allreduce per layer (and the gradient buckets)
            assert C.gpu_stats()["calls"] - calls0 >= 4, C.gpu_stats()
        if step == 0:
            xc = torch.cat(xs).contiguous(memory_format=torch.channels_last).requires_grad_()
            yc = ref(xc, [2 + q for q in range(n)])
            (yc.float() * torch.cat(gs)).sum().backward()
            o = sum(2 + q for q in range(r))
            sl = slice(o, o + 2 + r)
            torch.testing.assert_close(y.detach().float(), yc.detach().float()[sl], rtol=2e-2,
                                       atol=2e-2)
            torch.testing.assert_close(x.grad.float(), xc.grad.float()[sl], rtol=3e-2, atol=3e-2)
            # the second BN's inputs agree to a bf16 rounding (2^-9) of a few elements, not
            # bitwise (the first BN's outputs are rounded from values that differ in the last
            # fp32 bits): the statistics to 1e-3 here, to test_bn_gpu's 1e-4 on equal inputs
            # in tests/test_syncbn_kernels_gpu.py
            for a, b in ((net.bn1, ref.bn1), (net.bn2, ref.bn2)):
                torch.testing.assert_close(a.running_mean, b.running_mean, rtol=1e-3, atol=1e-3)
                torch.testing.assert_close(a.running_var, b.running_var, rtol=1e-3, atol=1e-3)
        opt.step()
        opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    flat = torch.cat([t.detach().float().reshape(-1) for t in
                      list(net.parameters()) + [net.bn1.running_mean, net.bn1.running_var,
                                                net.bn2.running_mean, net.bn2.running_var]])
    allf = hvd.allgather(flat.unsqueeze(0))
    assert torch.isfinite(allf).all(), "non-finite parameters or statistics"
    _same_all(allf, "parameters and running statistics")
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
    globals()[sys.argv[1]]()
