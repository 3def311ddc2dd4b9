"""float64 references and counted bounds for local gradient accumulation in an fp32 arena:
the kernels of csrc/kernels/mv_accum.hip, their PyTorch fallbacks (mivod/ops/kernels.py:
accumulate, pack_accumulated) and DistributedOptimizer(backward_passes_per_step=k,
accumulation_dtype=torch.float32).

A helper module, not a test file: tests/test_accum_cpu.py runs the fallbacks and the CPU
hook path through it, tests/test_accum_gpu.py the HIP kernels and the GPU hook path, and
tests/accum_workers.py the rank scenarios, all over the same cases.

Counts (U = 2^-24, one fp32 rounding; as tests/flat_reference.py counts them)
------------------------------------------------------------------------------
accum_kernel, first:  acc = float(g)            the conversion is exact: bit-exact, c = 0
accum_kernel, add:    acc = acc + float(g)      one rounding per launch: after j passes
                      |acc - sum_{i<=j} g_i| <= (j-1) * U * sum_{i<=j} |g_i|
                      (every partial sum is at most the sum of the magnitudes)
accum_kernel, last:   s = acc + float(g)        the (k-1)-th addition
                      p = s * scale             scale reaches the kernel rounded to fp32 (1)
                                                and the product rounds (1)
                      dst = cast_W(p)           half an ulp of the wire dtype
  => |dst - scale * sum g_i| <= (k+1) * U * |scale| * sum |g_i| + HALF_ULP[W] * |ref|
                                + 2^-25 for an fp16 wire (half the spacing of its subnormals)
A slot emitted by flat_cast (no gradient in the last pass; synchronize() on a partial window)
has the same count: the accumulator of k passes carries k-1 additions, then scale and product.

The model-level checks use the same wire bound, with the float64 sum of the micro-batch
gradients of a twin model, one backward at a time, as stored in the parameters' dtype.
"""
from __future__ import annotations

import copy
import warnings

import torch

import flat_reference as FR
from mivod.ops import kernels as K

U = FR.U
HALF_ULP = FR.HALF_ULP
DTYPES = FR.DTYPES
SIZES = FR.SIZES
N_GRID = FR.N_GRID
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32

KS = [2, 4, 16]
SCALES = [1.0, 0.125, 0.37]           # one, a power of two, neither
SENTINEL = 7.0                        # fills everything the launches must not write
TAIL = 70                             # a second tensor in every launch (a scalar tail of 6)


def wire_tol(ref: torch.Tensor, mag: torch.Tensor, k: int, scale: float, wdt) -> torch.Tensor:
    """The bound of a wire value out of k passes (module docstring)."""
    tol = (k + 1) * U * abs(scale) * mag + HALF_ULP[wdt] * ref.abs()
    if wdt == f16:
        tol = tol + 2.0 ** -25
    return tol


def check_wire(name, got, ref, mag, k, scale, wdt) -> float:
    """Assert the wire bound element by element; the worst err / tol."""
    got = FR.f64(got)
    assert torch.isfinite(got).all(), f"{name}: non-finite result"
    err = (got - ref).abs()
    tol = wire_tol(ref, mag, k, scale, wdt)
    bad = err > tol
    worst = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {err.numel()} elements outside the "
                           f"bound, worst err/tol {worst:.3g}")
    return worst


def outside_share(got, ref, mag, k, scale, wdt) -> float:
    """Share of the elements outside the wire bound (no assertion)."""
    err = (FR.f64(got) - ref).abs()
    return float((err > wire_tol(ref, mag, k, scale, wdt)).double().mean())


def make_grads(sizes, gdt, k, dev, seed=0, base_off=0):
    """k passes of N(0,1) gradients, one tensor per size, generated on the CPU (the same bits
    on either device and at either ``base_off``: 0 is a 16-byte-aligned base, 1 is base[1:])."""
    gen = torch.Generator().manual_seed(4000 + seed)
    passes = []
    for _ in range(k):
        ts = []
        for n in sizes:
            base = torch.zeros(n + 8, dtype=gdt)
            base[base_off:base_off + n] = torch.randn(n, generator=gen).to(gdt)
            ts.append(base.to(dev)[base_off:base_off + n])
        passes.append(ts)
    return passes


def run_window(dev, sizes, gdt, wdt, k, scale, base_off=0, seed=0, flag=None):
    """One accumulation window over the tensors ``sizes`` (64-element-aligned offsets): first,
    k-2 adds, last.  Checks the accumulator after every pass and the wire values against
    float64, that ``last`` leaves the accumulator alone, and that nothing outside the segments
    is written.  Returns (worst acc err/(U*mag) over c, worst wire err/tol, acc, dst)."""
    offs, total = FR.layout(sizes)
    passes = make_grads(sizes, gdt, k, dev, seed, base_off)
    acc = torch.full((total,), SENTINEL, dtype=f32, device=dev)
    dst = torch.full((total,), SENTINEL, dtype=wdt, device=dev)
    ref = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    mag = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    worst_acc = 0.0
    for j in range(1, k + 1):
        for t, g in enumerate(passes[j - 1]):
            ref[t] = ref[t] + FR.f64(g)
            mag[t] = mag[t] + FR.f64(g).abs()
        if j == k:
            break
        K.accumulate(passes[j - 1], acc, offs, j == 1)
        for t, (n, o) in enumerate(zip(sizes, offs)):
            if j == 1:
                assert torch.equal(acc[o:o + n], passes[0][t].float()), "first is a plain copy"
            else:
                w = FR.check(f"acc pass {j} n={n} {gdt}", acc[o:o + n],
                             FR.Out(ref[t], mag[t], j - 1))
                worst_acc = max(worst_acc, w / (j - 1))
    held = acc.clone()
    K.pack_accumulated(passes[k - 1], acc, dst, offs, scale, flag)
    assert torch.equal(acc, held), "the last pass wrote the accumulator"
    worst_wire = 0.0
    touched = torch.zeros(total, dtype=torch.bool)
    for t, (n, o) in enumerate(zip(sizes, offs)):
        touched[o:o + n] = True
        worst_wire = max(worst_wire, check_wire(f"wire n={n} {gdt}->{wdt} k={k} scale={scale}",
                                                dst[o:o + n], ref[t] * scale, mag[t], k, scale,
                                                wdt))
    assert (acc.cpu()[~touched] == SENTINEL).all(), "accumulate wrote outside its segments"
    assert (dst.cpu()[~touched].float() == SENTINEL).all(), \
        "pack_accumulated wrote outside its segments"
    return worst_acc, worst_wire, acc.cpu(), dst.cpu()


def run_sizes(dev, gdt, wdt, k=4, scale=0.125):
    """every size around a lane (8), a step (2048) and a chunk (4096), two tensors per launch,
    from an aligned base (load8 / store8) and from base[1:] (one by one): the same bits"""
    wa = ww = 0.0
    for n in SIZES:
        a = run_window(dev, [n, TAIL], gdt, wdt, k, scale, 0, seed=n)
        b = run_window(dev, [n, TAIL], gdt, wdt, k, scale, 1, seed=n)
        assert torch.equal(a[2], b[2]) and torch.equal(a[3].float(), b[3].float()), \
            f"n={n}: an offset source changes the bits"
        wa, ww = max(wa, a[0], b[0]), max(ww, a[1], b[1])
    return wa, ww


MANY = [9] * 70 + [4097, 1]             # more tensors than one kernel-argument table holds


def run_many(dev, gdt=bf16, wdt=f16):
    return run_window(dev, MANY, gdt, wdt, 4, 0.37, seed=99)[:2]


# ---- the flag of the last pass --------------------------------------------------------------------
def run_flag(dev, gdt, wdt, base_off=0):
    """``last`` leaves the flag alone on finite values (0 stays 0, a preset 1 stays), sets it
    for an inf or nan in g at any position and for one left in the accumulator by an earlier
    pass, and, on an fp16 wire, for a finite sum whose cast overflows (not for the same sum
    scaled back into range)."""
    n = N_GRID
    dst = torch.zeros(n, dtype=wdt, device=dev)

    def src(fill=1.0):
        return torch.full((n + 8,), fill, dtype=gdt, device=dev)[base_off:base_off + n]

    acc = torch.zeros(n, dtype=f32, device=dev)
    K.accumulate([src()], acc, [0], True)
    for preset in (0, 1):
        flag = FR.flag_of(dev, preset)
        K.pack_accumulated([src()], acc, dst, [0], 1.0, flag)
        assert flag.item() == preset, "finite values changed the flag"
    for pos in FR.bad_positions(n):
        for bad in FR.BAD_VALUES:
            g = src()
            g[pos] = bad
            flag = FR.flag_of(dev)
            K.pack_accumulated([g], acc, dst, [0], 1.0, flag)
            assert flag.item() == 1, f"missed {bad} in g at {pos}"
    g = src()
    g[n - 1] = float("inf")
    K.accumulate([g], acc, [0], False)
    flag = FR.flag_of(dev)
    K.pack_accumulated([src()], acc, dst, [0], 1.0, flag)
    assert flag.item() == 1, "missed an inf left in the accumulator"
    # 2 * 40000 (39936 in bf16) is finite in fp32 and above fp16's 65504
    big = src()
    big[4095] = 40000.0
    K.accumulate([big], acc, [0], True)
    for scale, want in ((1.0, wdt == f16), (0.125, False)):
        flag = FR.flag_of(dev)
        K.pack_accumulated([big], acc, dst, [0], scale, flag)
        assert bool(flag.item()) == want, f"{wdt} scale {scale}: flag {flag.item()}"
        assert bool(torch.isinf(dst.float()).any()) == want


# ---- today's arithmetic through the same harness ---------------------------------------------------
def run_evidence(dev, k=16, n=N_GRID):
    """k bf16 N(0,1) vectors: (share outside the bound of bf16 ``+=`` followed by K.pack,
    share outside it of the fp32 arena path), fp32 wire, scale 1."""
    passes = make_grads([n], bf16, k, dev, seed=7)
    ref = sum(FR.f64(p[0]) for p in passes)
    mag = sum(FR.f64(p[0]).abs() for p in passes)
    grad = passes[0][0].clone()
    for p in passes[1:]:
        grad += p[0]                      # autograd's accumulation, in the parameter's dtype
    old = torch.zeros(n, dtype=f32, device=dev)
    K.pack([grad], old, [0])
    acc = torch.zeros(n, dtype=f32, device=dev)
    new = torch.zeros(n, dtype=f32, device=dev)
    for j, p in enumerate(passes[:-1]):
        K.accumulate(p, acc, [0], j == 0)
    K.pack_accumulated(passes[-1], acc, new, [0], 1.0)
    return outside_share(old, ref, mag, k, 1.0, f32), outside_share(new, ref, mag, k, 1.0, f32)


# ---- the model level -------------------------------------------------------------------------------
class Net(torch.nn.Module):
    """two linears and a channels_last conv, 2295 parameters, several of odd size"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.lin1 = torch.nn.Linear(8, 129)
        self.lin2 = torch.nn.Linear(129, 7)

    def forward(self, x, head=True):
        h = torch.tanh(self.conv(x)).mean(dim=(2, 3))
        h = torch.tanh(self.lin1(h))
        return self.lin2(h) if head else h[:, :7]


def make_net(dev):
    torch.manual_seed(0)
    return Net().to(bf16).to(dev).to(memory_format=torch.channels_last)


def make_batches(dev, k, seed=0, n=4):
    gen = torch.Generator().manual_seed(500 + seed)
    out = []
    for _ in range(k):
        x = torch.randn(n, 3, 8, 8, generator=gen).to(bf16).to(dev).contiguous(
            memory_format=torch.channels_last)
        out.append((x, torch.randn(n, 7, generator=gen).to(dev)))
    return out


def loss_of(net, batch, scale=1.0, head=True):
    x, y = batch
    return scale * ((net(x, head).float() - y) ** 2).sum()


def twin_sums(twin, batches, heads=None, scales=None):
    """{parameter index: (float64 sum, float64 sum of magnitudes)} of the twin's gradients, one
    backward at a time, each as stored in the parameter's dtype (in its logical shape)."""
    params = list(twin.parameters())
    ref = [torch.zeros(p.shape, dtype=torch.float64) for p in params]
    mag = [torch.zeros(p.shape, dtype=torch.float64) for p in params]
    for j, b in enumerate(batches):
        twin.zero_grad(set_to_none=True)
        loss_of(twin, b, 1.0 if scales is None else scales[j],
                True if heads is None else heads[j]).backward()
        for i, p in enumerate(params):
            if p.grad is not None:
                assert p.grad.dtype == p.dtype
                ref[i] += FR.f64(p.grad)
                mag[i] += FR.f64(p.grad).abs()
    return ref, mag


def arena_reference(opt, net, ref, mag):
    """[(arena, float64 reference, float64 magnitudes)] in the layout of every arena's flat
    gradient buffer (alignment gaps: zeros, to be matched exactly)."""
    index = {id(p): i for i, p in enumerate(net.parameters())}
    out = []
    for a in opt._mvd_arenas:
        r = torch.zeros(a.grad.numel(), dtype=torch.float64)
        m = torch.zeros(a.grad.numel(), dtype=torch.float64)
        for i, p in enumerate(a.params):
            torch.as_strided(r, p.size(), p.stride(), a.offsets[i]).copy_(ref[index[id(p)]])
            torch.as_strided(m, p.size(), p.stride(), a.offsets[i]).copy_(mag[index[id(p)]])
        out.append((a, r, m))
    return out


def check_arenas(label, opt, net, ref, mag, k, scale=1.0, divide=1.0):
    """every arena's gradient buffer / ``divide`` within the wire bound of ref * scale"""
    worst = 0.0
    for a, r, m in arena_reference(opt, net, ref, mag):
        got = FR.f64(a.grad) / divide
        gap = m == 0
        assert (got[gap] == 0).all(), f"{label}: a gap or an unused slot is not zero"
        worst = max(worst, check_wire(label, got, r * scale, m, k, scale, a.grad.dtype))
    return worst


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def wrap(net, kind, k, **kw):
    """DistributedOptimizer over ``kind`` with the arena on; fp16 wire + guard for the fused
    optimizers, no compression for plain SGD"""
    import mivod.torch as hvd
    from mivod.optim import FusedAdam, FusedSGD
    hvd.init()
    if kind == "sgd":
        inner = torch.optim.SGD(net.parameters(), lr=0.1)
        kw.setdefault("compression", hvd.Compression.none)
    else:
        inner = (FusedSGD(net.parameters(), lr=0.1, momentum=0.9) if kind == "fused_sgd"
                 else FusedAdam(net.parameters(), lr=1e-3, weight_decay=1e-2))
        kw.setdefault("compression", hvd.Compression.fp16)
    kw.setdefault("accumulation_dtype", torch.float32)
    return hvd.DistributedOptimizer(inner, named_parameters=net.named_parameters(),
                                    backward_passes_per_step=k, **kw)


def run_passes(opt, net, batches, heads=None, scales=None, released=True):
    """one backward per batch; after every non-final pass of a full window every p.grad is
    released (g)"""
    k = opt._mvd_bpps
    for j, b in enumerate(batches):
        loss_of(net, b, 1.0 if scales is None else scales[j],
                True if heads is None else heads[j]).backward()
        if released and j + 1 < k and (heads is None or all(heads)):
            assert all(p.grad is None for p in net.parameters()), \
                f"p.grad is held after pass {j + 1} of {k}"


def model_plain_sgd(dev, k=4):
    """(a) plain torch.optim.SGD, no compression: p.grad after synchronize() within the wire
    bound (bf16 wire) of the float64 sum; (g) p.grad released after every non-final pass."""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, "sgd", k)
    assert not opt._mvd_acc, "the accumulator is allocated lazily"
    batches = make_batches(dev, k)
    run_passes(opt, net, batches)
    opt.synchronize()
    _sync(dev)
    ref, mag = twin_sums(twin, batches)
    worst = check_arenas("plain SGD", opt, net, ref, mag, k)
    for a in opt._mvd_arenas:
        assert opt._mvd_acc[id(a)].dtype == f32 and opt._mvd_acc[id(a)].numel() == a.grad.numel()
        for i, p in enumerate(a.params):
            assert p.grad is not None and torch.equal(p.grad, a.slot(a.grad, i))
    with opt.skip_synchronize():
        opt.step()
    return worst


def model_fused(dev, kind, k=4):
    """(b) FusedSGD / FusedAdam, fp16 wire, guard on: the arena's gradient buffer within the
    bound; the updated masters match flat_reference's step reference fed that stored
    gradient."""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, kind, k)
    assert opt.guard_stats()["enabled"]
    batches = make_batches(dev, k, seed=1)
    before = [(a.master.clone(), {n: s.clone() for n, s in a.state.items()})
              for a in opt._mvd_arenas]
    run_passes(opt, net, batches)
    opt.step()
    _sync(dev)
    ref, mag = twin_sums(twin, batches)
    worst = {"grad": check_arenas(kind, opt, net, ref, mag, k)}
    for a, (w0, st0) in zip(opt._mvd_arenas, before):
        hp = a.group
        if kind == "fused_sgd":
            want = FR.sgd_ref(a.grad, w0, st0["momentum_buffer"], lr=hp["lr"],
                              momentum=hp["momentum"], gscale=opt._mvd_gscale(), first=True)
            pairs = [("w", a.master), ("mom", a.state["momentum_buffer"])]
        else:
            want = FR.adam_ref(a.grad, w0, st0["exp_avg"], st0["exp_avg_sq"], lr=hp["lr"],
                               beta1=hp["betas"][0], beta2=hp["betas"][1], eps=hp["eps"],
                               weight_decay=hp["weight_decay"], gscale=opt._mvd_gscale(), step=1)
            pairs = [("w", a.master), ("m", a.state["exp_avg"]), ("v", a.state["exp_avg_sq"])]
        for name, got in pairs:
            worst[name] = max(worst.get(name, 0.0), FR.check(f"{kind} {name}", got, want[name]))
        assert not torch.equal(a.master, w0), "no update"
    assert all(p.grad is None for p in net.parameters())
    return worst


def model_partial(dev, k=4, done=2):
    """(c) synchronize() after ``done`` of k passes reduces the sum of ``done``"""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, "fused_sgd", k)
    batches = make_batches(dev, done, seed=2)
    run_passes(opt, net, batches)
    assert all(p.grad is None for p in net.parameters())
    opt.synchronize()
    _sync(dev)
    ref, mag = twin_sums(twin, batches)
    return check_arenas("partial window", opt, net, ref, mag, done)


def model_unused(dev, kind, skip_pass, bucket_mb, k=4):
    """(d) lin2 takes no part in pass ``skip_pass`` (0-based): its hooks fire k-1 times, its
    buckets are launched by synchronize(), and its last gradient or its accumulator slot is
    emitted.  ``bucket_mb`` tiny: every parameter is a bucket of its own."""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, kind, k, bucket_mb=bucket_mb, first_bucket_mb=bucket_mb)
    batches = make_batches(dev, k, seed=3)
    heads = [j != skip_pass for j in range(k)]
    run_passes(opt, net, batches, heads=heads)
    opt.synchronize()
    _sync(dev)
    ref, mag = twin_sums(twin, batches, heads=heads)
    assert float(mag[4].sum()) > 0 and float(mag[5].sum()) > 0
    return check_arenas(f"unused in pass {skip_pass}", opt, net, ref, mag, k), \
        len(opt.bucket_plan())


def model_aliased(dev, k=2):
    """(e) plain SGD: after a step p.grad are views of the arena's gradient buffer, and
    zero_grad(set_to_none=False) keeps them, so the next window's first pass accumulates in
    place in the slots the last pass writes.  Then the rarer order: a gradient that still
    lives in its slot when the window's LAST pass arrives goes through add + flat_cast."""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, "sgd", k)
    run_passes(opt, net, make_batches(dev, k, seed=4))
    opt.step()
    worst = []
    for window, alias_last in ((1, False), (2, True)):
        opt.zero_grad(set_to_none=False)
        a0 = opt._mvd_arenas[0]
        assert all(p.grad.data_ptr() == a.slot(a.grad, i).data_ptr()
                   for a in opt._mvd_arenas for i, p in enumerate(a.params)), "not aliased"
        twin.load_state_dict(net.state_dict())
        batches = make_batches(dev, k, seed=40 + window)
        if alias_last:
            run_passes(opt, net, batches[:-1])
            for a in opt._mvd_arenas:           # as zero_grad(set_to_none=False) leaves them
                for i, p in enumerate(a.params):
                    p.grad = a.slot(a.grad, i).zero_()
            run_passes(opt, net, batches[-1:], released=False)
        else:
            run_passes(opt, net, batches)
        opt.synchronize()
        _sync(dev)
        ref, mag = twin_sums(twin, batches)
        worst.append(check_arenas(f"aliased window {window}", opt, net, ref, mag, k))
        assert a0.grad.dtype == bf16
        with opt.skip_synchronize():
            opt.step()
    return worst


def model_zero_grad(dev, k=4):
    """(f) zero_grad() after 2 of 4 passes drops them: the window reduces passes 3 and 4"""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, "fused_sgd", k)
    batches = make_batches(dev, k, seed=5)
    run_passes(opt, net, batches[:2])
    opt.zero_grad()
    run_passes(opt, net, batches[2:], released=False)
    opt.synchronize()
    _sync(dev)
    ref, mag = twin_sums(twin, batches[2:])
    return check_arenas("zero_grad mid-window", opt, net, ref, mag, 2)


def model_overflow(dev, k=4):
    """(h) window 1 applies; window 2 holds one micro-batch whose gradients are finite in bf16
    and in the fp32 accumulator and overflow the fp16 wire: the step is skipped; window 3 is
    clean again (its gradient within the bound) and applies."""
    net = make_net(dev)
    twin = copy.deepcopy(net)
    opt = wrap(net, "fused_sgd", k)
    batches = make_batches(dev, k, seed=6)

    def window(scales=None):
        opt.zero_grad()
        run_passes(opt, net, batches, scales=scales)
        opt.step()
        _sync(dev)
        return [a.master.clone() for a in opt._mvd_arenas]

    w0 = [a.master.clone() for a in opt._mvd_arenas]
    w1 = window()
    assert all(not torch.equal(a, b) for a, b in zip(w0, w1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w2 = window([1.0, 1e9, 1.0, 1.0])
        assert all(torch.equal(a, b) for a, b in zip(w1, w2)), "the overflowing step was applied"
        twin.load_state_dict(net.state_dict())
        w3 = window()                        # the flags of the skipped step are read here
    assert all(not torch.equal(a, b) for a, b in zip(w2, w3)), "the step after the skip"
    assert opt.guard_stats()["skipped_steps"] == 1, opt.guard_stats()
    ref, mag = twin_sums(twin, batches)
    return check_arenas("window after the skip", opt, net, ref, mag, k)
