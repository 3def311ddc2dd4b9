"""DistributedOptimizer(FusedAdamax / FusedAdam(amsgrad=True) / FusedNAdam) scenarios, run as
`python tests/adamfam_workers.py <scenario> <device type>` by tests/test_adamfam_cpu.py (2 gloo
CPU ranks, the fallbacks) and tests/test_adamfam_gpu.py (world size 1 on mivod's RCCL
communicator with every collective forced, the HIP kernels).  Every rank rebuilds ALL ranks'
batches from seeds, computes the float64 reference itself (tests/adamfam_reference.py),
asserts, and prints "OK <rank>" at the end."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import adamfam_reference as R  # noqa: E402
import mivod.torch as hvd  # noqa: E402
from test_adamfam_cpu import check_fused_step  # noqa: E402

HP = dict(lr=0.01, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
MAX_NORM = 0.5


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


def _data(n, dev, seed=100):
    out = []
    for q in range(n):
        g = torch.Generator().manual_seed(seed + q)
        out.append((torch.randn(8, 16, generator=g).to(dev),
                    torch.randn(8, 4, generator=g).to(dev)))
    return out


def _make(kind, params, **kw):
    from mivod.optim import FusedAdam, FusedAdamax, FusedNAdam
    if kind == "adamax":
        return FusedAdamax(params, **HP, **kw)
    if kind == "amsgrad":
        return FusedAdam(params, amsgrad=True, **HP, **kw)
    return FusedNAdam(params, momentum_decay=0.01, **HP, **kw)


def _stored(a):
    """the arena's master, state and model copy, cloned"""
    d = {"w": a.master.clone(), "model": a.model.clone()}
    d.update({n: t.clone() for n, t in a.state.items()})
    return d


def _summed_grads(a, model, twin, data):
    """the sum over ``data`` of the gradients of ``twin`` (a copy of ``model`` before the step),
    in fp32 and in the arena's layout: for 2 ranks exactly what the wire's one addition gives"""
    flat = torch.zeros_like(a.master)
    ids = {id(p): i for i, p in enumerate(a.params)}
    for batch in data:
        twin.zero_grad()
        _loss(twin, batch).backward()
        for p, q in zip(twin.parameters(), model.parameters()):
            a.slot(flat, ids[id(q)]).add_(p.grad.float())
    return flat


def _same_bits(a, what):
    for i, p in enumerate(a.params):
        assert torch.equal(p.detach(), a.slot(a.master, i).to(p.dtype)), "parameters != master"
    flat = torch.cat([a.master] + [a.state[k] for k in sorted(a.state)])
    assert torch.isfinite(flat).all()
    _same_all(hvd.allgather(flat.unsqueeze(0)), what)


def dist_pair(device_type):
    """fp32 wire, 2 ranks, FusedAdamax and then FusedAdam(amsgrad=True, max_grad_norm=0.5).
    Steps 1 and 2: every rank's master weights and state equal, within the counted bound, the
    float64 step on the average of the ranks' gradients (times the clip coefficient the
    optimizer measured, which is checked against the norm of that average) from the state
    stored before the step.  Parameters and state bitwise equal across ranks at the end."""
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    dev = hvd.device()
    assert dev.type == device_type and n == 2, (dev, device_type, n)
    for kind, kw in (("adamax", {}), ("amsgrad", dict(max_grad_norm=MAX_NORM))):
        m = _mlp(dev)
        opt = hvd.DistributedOptimizer(_make(kind, m.parameters(), **kw),
                                       named_parameters=m.named_parameters())
        (a,) = opt._mv_arenas
        data = _data(n, dev)
        for s in (1, 2):
            twin = copy.deepcopy(m)
            before = _stored(a)
            opt.zero_grad()
            _loss(m, data[r]).backward()
            opt.step()
            gsum = _summed_grads(a, m, twin, data)
            gscale = 1.0 / n
            if kw:
                norm = float((gsum.double() / n).norm())
                assert norm > 2 * MAX_NORM, norm
                coef = float(opt._mv_clip_block[0])
                assert abs(coef - MAX_NORM / (norm + 1e-6)) <= 1e-5 * coef, (coef, norm)
                assert abs(float(opt.grad_norm()) - norm) <= 1e-5 * norm
                gscale *= coef              # 1/2 times an fp32 value: the kernel's product is exact
            check_fused_step(opt, a, before, f"{kind} rank {r} step {s}", gscale=gscale, grad=gsum)
            assert not torch.equal(a.master, before["w"]), "nothing moved"
        _same_bits(a, f"{kind}: parameters and state")
    hvd.shutdown()
    print("OK", r)


def dist_options(device_type):
    """2 ranks, FusedNAdam and FusedAdamax on a bf16 model with the fp16 wire, its overflow
    guard and grad_scale, backward_passes_per_step=2 with accumulation_dtype=float32 and
    gradient_predivide_factor=2: the options meet the new steps only through _mv_apply, so the
    gradient scale it is handed is the documented one (predivide / (grad_scale * size)), the
    reduced bucket the arena holds, times that scale, is the mean over the ranks of the summed
    micro-batch gradients within the fp16 wire's rounding, and the step is the float64 step on
    that bucket and scale within the counted bound.  Bitwise equal across ranks at the end."""
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    dev = hvd.device()
    assert dev.type == device_type and n == 2, (dev, device_type, n)
    passes, gs, pre = 2, 8.0, 2.0
    for kind in ("nadam", "adamax"):
        m = _mlp(dev).to(torch.bfloat16)
        opt = hvd.DistributedOptimizer(_make(kind, m.parameters()),
                                       named_parameters=m.named_parameters(),
                                       compression=hvd.Compression.fp16, overflow_guard=True,
                                       grad_scale=gs, backward_passes_per_step=passes,
                                       accumulation_dtype=torch.float32,
                                       gradient_predivide_factor=pre)
        assert opt.guard_stats()["enabled"]
        (a,) = opt._mv_arenas
        assert a.grad.dtype == torch.float16 and a.low_precision
        seen = []
        inner = opt._mv_apply

        def spy(arena, i0, i1, gscale=1.0, inner=inner, seen=seen):
            seen.append(gscale)
            return inner(arena, i0, i1, gscale)

        opt._mv_apply = spy
        for s in (1, 2):
            data = [[(x.to(torch.bfloat16), y.to(torch.bfloat16))
                     for x, y in _data(passes, dev, seed=100 * s + 10 * q)] for q in range(n)]
            twin = copy.deepcopy(m)
            before = _stored(a)
            del seen[:]
            opt.zero_grad()
            for batch in data[r]:
                _loss(m, batch).backward()
            opt.step()
            assert seen and all(abs(g - pre / (gs * n)) <= 1e-12 for g in seen), seen
            mean = _summed_grads(a, m, twin, [b for d in data for b in d]).double() / n
            got = a.grad.double() * seen[0]
            tol = 4 * 2.0 ** -11 * mean.abs() + 1e-4 * float(mean.abs().max())
            assert ((got - mean).abs() <= tol).all(), float(((got - mean).abs() - tol).max())
            check_fused_step(opt, a, before, f"{kind} rank {r} step {s}", gscale=seen[0])
            assert not torch.equal(a.master, before["w"]), "nothing moved"
        assert opt.guard_stats()["skipped_steps"] == 0
        _same_bits(a, f"{kind}: parameters and state")
    hvd.shutdown()
    print("OK", r)


def guard_world1(device_type):
    """World size 1 with the collectives forced, fp16 wire, overflow guard on,
    FusedAdam(amsgrad=True).  Step 1: the master weights and state match float64 on the reduced
    fp16 gradient the arena holds, which is the fp16 rounding of the model's gradient.  Step 2
    carries an injected inf: master, state and model copy stay bitwise unchanged.  Step 3
    applies again and the guard has counted one skipped step."""
    hvd.init()
    dev = hvd.device()
    assert dev.type == device_type and hvd.size() == 1, (dev, device_type)
    m = _mlp(dev).to(torch.bfloat16)
    opt = hvd.DistributedOptimizer(_make("amsgrad", m.parameters()),
                                   named_parameters=m.named_parameters(),
                                   compression=hvd.Compression.fp16, overflow_guard=True)
    assert opt.guard_stats()["enabled"]
    assert opt._mvd_comm or dev.type == "cpu", "the collectives are not forced"
    (a,) = opt._mv_arenas
    assert a.grad.dtype == torch.float16 and a.low_precision
    x, y = _data(1, dev)[0]
    batch = (x.to(torch.bfloat16), y.to(torch.bfloat16))
    inject = [False]

    def poison(gr):
        if inject[0]:
            gr = gr.clone()
            gr.view(-1)[0] = float("inf")
        return gr

    next(iter(m.parameters())).register_hook(poison)

    def step():
        opt.zero_grad()
        _loss(m, batch).backward()
        opt.step()
        if dev.type == "cuda":
            torch.cuda.synchronize()

    twin = copy.deepcopy(m)
    before = _stored(a)
    step()
    want = _summed_grads(a, m, twin, [batch]).to(torch.float16)
    assert torch.equal(a.grad, want), "the reduced bucket is the fp16 rounding of the gradient"
    check_fused_step(opt, a, before, "clean step")
    assert torch.equal(a.model, a.master.to(torch.bfloat16)), "model copy"

    s1 = _stored(a)
    inject[0] = True
    step()
    inject[0] = False
    s2 = _stored(a)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), f"the overflowing step changed {k}"
    step()                                     # the flags of the skipped step are read here
    s3 = _stored(a)
    for k in s2:
        assert not torch.equal(s2[k], s3[k]), f"the step after the skip left {k} unchanged"
        assert torch.isfinite(s3[k].float()).all(), k
    assert opt.guard_stats()["skipped_steps"] == 1, opt.guard_stats()
    hvd.shutdown()
    print("OK", 0)


if __name__ == "__main__":
    # a hung rank prints every thread's stack and exits before the runner's limit
    import faulthandler
    import signal
    _dump = float(os.environ.get("MIVOD_TEST_DUMP_AFTER", "0"))
    if _dump > 0:
        faulthandler.dump_traceback_later(_dump, exit=True)
    faulthandler.register(signal.SIGUSR1, all_threads=True)
    globals()[sys.argv[1]](*sys.argv[2:])
