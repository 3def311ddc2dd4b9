"""DistributedOptimizer(FusedLAMB) multi-rank scenario, run as
`python tests/lamb_workers.py dist_lamb <device type>` in 2 processes by
tests/test_lamb_cpu.py (gloo CPU ranks, the fallback) and tests/test_lamb_gpu.py (ranks sharing
one GPU over gloo-gpu, the HIP kernels).  Every rank rebuilds ALL ranks' batches from seeds,
computes the single-process reference itself, asserts, and prints "OK <rank>" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mivod.torch as hvd  # noqa: E402

LR, WD = 0.02, 0.05
# Two roundings to fp16 on the wire (each rank's cast, the sum): every gradient the fused
# step sees is within 2^-10, relative, of the one the reference is fed.  Through
# u = m_hat / (sqrt(v_hat) + eps), with |u| of order 1 and the largest |u| of a tensor at
# least 1/2, that moves u by at most 2 * 2^-10 (numerator and denominator) and the trust ratio
# by as much, relative: 6 * 2^-10 of the tensor's largest update per step, and the first
# step's error enters the second through w.  WIRE_TOL of the sum of the two steps' largest
# updates, per tensor, covers it.
WIRE_TOL = 16 * 2.0 ** -10


def _same_all(rows, what=""):
    odd = [q for q in range(1, rows.shape[0]) if not torch.equal(rows[0], rows[q])]
    assert not odd, f"{what}: ranks {odd} differ from rank 0"


def _mlp(dev):
    torch.manual_seed(0)                       # the same initial model on every rank
    return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(),
                               torch.nn.Linear(32, 4)).to(dev)


def _loss(model, batch):
    x, y = batch
    return ((model(x) - y) ** 2).sum()


def dist_lamb(device_type):
    """fp16 wire, overflow guard on.  Steps 1 and 2: each rank's parameters equal a
    single-process FusedLAMB fed the average of the ranks' fp16-rounded gradients, within the
    wire's rounding (WIRE_TOL).  Step 3: rank 1 injects inf; parameters and both moments stay
    bitwise unchanged on every rank.  Step 4 applies again.  Parameters bitwise equal across
    ranks at the end."""
    from mivod.optim import FusedLAMB
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    dev = hvd.device()
    assert dev.type == device_type, (dev, device_type)
    m = _mlp(dev)
    inner = FusedLAMB(m.parameters(), lr=LR, weight_decay=WD)
    opt = hvd.DistributedOptimizer(inner, named_parameters=m.named_parameters(),
                                   compression=hvd.Compression.fp16, overflow_guard=True)
    assert opt.guard_stats()["enabled"]
    ref = _mlp(dev)
    ref_opt = FusedLAMB(ref.parameters(), lr=LR, weight_decay=WD)
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

    def step():
        opt.zero_grad()
        _loss(m, data[r]).backward()
        opt.step()

    moved = [torch.zeros((), device=dev) for _ in ref.parameters()]
    for s in (1, 2):
        step()
        grads = None
        for q in range(n):
            ref.zero_grad()
            _loss(ref, data[q]).backward()
            gs = [p.grad.half().float() for p in ref.parameters()]
            grads = gs if grads is None else [a + b for a, b in zip(grads, gs)]
        before = [p.detach().clone() for p in ref.parameters()]
        for p, g in zip(ref.parameters(), grads):
            p.grad = g / n
        ref_opt.step()
        moved = [mv + (p.detach() - b).abs().max() for mv, p, b in
                 zip(moved, ref.parameters(), before)]
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for (nm, p), q, mv in zip(m.named_parameters(), ref.parameters(), moved):
        err, tol = float((p.detach() - q.detach()).abs().max()), WIRE_TOL * float(mv)
        print(f"{nm}: max |dist - single| {err:.3g}, tolerance {tol:.3g}", flush=True)
        assert float(mv) > 0 and err <= tol, (nm, err, tol)

    def snapshot():
        st = [opt.state[p] for p in m.parameters()]
        return ([p.detach().clone() for p in m.parameters()]
                + [s_["exp_avg"].clone() for s_ in st] + [s_["exp_avg_sq"].clone() for s_ in st])

    s2 = snapshot()
    inject[0] = r == 1
    step()
    inject[0] = False
    s3 = snapshot()
    assert all(torch.equal(a, b) for a, b in zip(s2, s3)), "the overflowing step was not skipped"
    step()                                     # the flags of the skipped step are read here
    s4 = snapshot()
    assert all(not torch.equal(a, b) for a, b in zip(s3, s4)), "the step after the skip"
    assert opt.guard_stats()["skipped_steps"] == 1, opt.guard_stats()
    flat = torch.cat([t.reshape(-1) for t in s4])
    assert torch.isfinite(flat).all()
    _same_all(hvd.allgather(flat.unsqueeze(0)), "parameters and moments")
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
