"""DistributedOptimizer(FusedRMSprop) scenarios, run as
`python tests/adaptive_workers.py <scenario> <device type>` by tests/test_adaptive_cpu.py (2 gloo
CPU ranks, the fallback) and tests/test_adaptive_gpu.py (world size 1 on mivod's RCCL
communicator with every collective forced, the HIP kernel).  Every rank rebuilds ALL ranks'
batches from seeds, computes the float64 reference itself (tests/adaptive_reference.py),
asserts, and prints "OK <rank>" at the end."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import adaptive_reference as R  # noqa: E402
import mivod.torch as hvd  # noqa: E402

HP = dict(lr=0.01, alpha=0.99, eps=1e-8, weight_decay=0.01, momentum=0.9, centered=True)
STATES = ("square_avg", "grad_avg", "momentum_buffer")


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


def _data(n, dev):
    out = []
    for q in range(n):
        g = torch.Generator().manual_seed(100 + q)
        out.append((torch.randn(8, 16, generator=g).to(dev), torch.randn(8, 4, generator=g).to(dev)))
    return out


def _stored(a):
    """the arena's master, state and model copy, cloned"""
    d = {"w": a.master.clone(), "model": a.model.clone()}
    d.update({n: a.state[n].clone() for n in STATES})
    return d


def _check_step(a, before, grad, gscale, label):
    """the arena after a step against rmsprop_ref on the state stored before it"""
    ref = R.rmsprop_ref(grad, before["w"], before["square_avg"], before["grad_avg"],
                        before["momentum_buffer"], gscale=gscale, **HP)
    worst = {"w": R.check(f"{label} w", a.master, ref["w"]),
             "sq": R.check(f"{label} sq", a.state["square_avg"], ref["sq"]),
             "ga": R.check(f"{label} ga", a.state["grad_avg"], ref["ga"]),
             "buf": R.check(f"{label} buf", a.state["momentum_buffer"], ref["buf"])}
    print(f"{label}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF['rmsprop']}", flush=True)
    assert not torch.equal(a.master, before["w"]), f"{label}: nothing moved"


def _summed_grads(a, model, twin, data):
    """the sum over ranks of the gradients of ``twin`` (a copy of ``model`` before the step), in
    fp32 and in the arena's layout: for 2 ranks exactly what the wire's one addition gives"""
    flat = torch.zeros_like(a.master)
    ids = {id(p): i for i, p in enumerate(a.params)}
    for batch in data:
        twin.zero_grad()
        _loss(twin, batch).backward()
        for p, q in zip(twin.parameters(), model.parameters()):
            a.slot(flat, ids[id(q)]).add_(p.grad)
    return flat


def dist_rmsprop(device_type):
    """fp32 wire, 2 ranks.  Steps 1 and 2: every rank's master weights and state equal, within
    the counted bound, the float64 RMSprop step on the average of the ranks' gradients from
    the state stored before the step.  Parameters and state bitwise equal across ranks at the
    end."""
    from mivod.optim import FusedRMSprop
    hvd.init()
    r, n = hvd.rank(), hvd.size()
    dev = hvd.device()
    assert dev.type == device_type and n == 2, (dev, device_type, n)
    m = _mlp(dev)
    opt = hvd.DistributedOptimizer(FusedRMSprop(m.parameters(), **HP),
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
        _check_step(a, before, gsum, 1.0 / n, f"rank {r} step {s}")
    for p, i in zip(a.params, range(len(a.params))):
        assert torch.equal(p.detach(), a.slot(a.master, i)), "parameters are the fp32 master"
    flat = torch.cat([a.master] + [a.state[k] for k in STATES])
    assert torch.isfinite(flat).all()
    _same_all(hvd.allgather(flat.unsqueeze(0)), "parameters and state")
    hvd.shutdown()
    print("OK", r)


def guard_world1(device_type):
    """World size 1 with the collectives forced, fp16 wire, overflow guard on.  Step 1: the
    master weights and state match float64 on the reduced fp16 gradient the arena holds, which
    is the fp16 rounding of the model's gradient.  Step 2 carries an injected inf: master,
    state and model copy stay bitwise unchanged.  Step 3 applies again and the guard has
    counted one skipped step."""
    from mivod.optim import FusedRMSprop
    hvd.init()
    dev = hvd.device()
    assert dev.type == device_type and hvd.size() == 1, (dev, device_type)
    m = _mlp(dev).to(torch.bfloat16)
    opt = hvd.DistributedOptimizer(FusedRMSprop(m.parameters(), **HP),
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
    _check_step(a, before, a.grad, 1.0, "clean step")
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
