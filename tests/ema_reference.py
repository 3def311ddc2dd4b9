"""float64 references and counted bounds for the fp32 exponential moving average of the master
weights: the kernels of csrc/kernels/mv_ema.hip, their PyTorch fallbacks (mivod/ops/kernels.py:
ema_update, ema_swap, ema_overwrite) and ``ema_decay`` of the mivod.optim.Fused* optimizers,
alone and under mivod.torch.DistributedOptimizer.

A helper module, not a test file: tests/test_ema_cpu.py runs the fallbacks and the CPU paths
through it, tests/test_ema_gpu.py the HIP kernels and the GPU paths, and tests/ema_workers.py
the rank scenarios, all over the same cases.

Counts (U = 2^-24, one fp32 rounding; as tests/flat_reference.py counts them)
------------------------------------------------------------------------------
ema_kernel, update:   t = w - e          (1)
                      p = omd * t        omd reaches the kernel rounded to fp32 (1), the
                                         product rounds (1)
                      e = e + p          (1)
  => |e' - (e + (1-d)(w - e))| <= c * U * mag,  c = 4,  mag = |e| + (1-d) (|w| + |e|)
     (every intermediate is at most mag; a contraction of the last two into one fma would
     only remove a rounding)
  omd == 1 (d = 0):   e = w, a copy: bit-exact
ema_kernel, swap / overwrite: copies and one cast to the model dtype: bit-exact against
                      torch's cast

Over k updates an error B already in e is carried on scaled by d (the update is
e' = d e + (1-d) w in exact arithmetic), so with the float64 average as the reference
    B <- d * B + c * U * mag,   B = 0 after the copying first update.
"""
from __future__ import annotations

import copy

import torch

import flat_reference as FR
from mivod.ops import kernels as K

U = FR.U
C_EMA = 4
SIZES = FR.SIZES
MODELS = FR.MODELS
N_GRID = FR.N_GRID
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32

GUARD = 8                              # elements on either side of every range
SENTINEL = 7.0                         # what they hold
DECAY = 0.9973                         # no power of two: omd and the product round


def f64(t):
    return FR.f64(t)


def update_ref(w, e, decay, bound=None):
    """One update in float64 from float64 (or fp32) w and the float64 average e:
    (new e, new accumulated bound)."""
    w, e = f64(w), f64(e)
    omd = 1.0 - float(decay)
    mag = e.abs() + omd * (w.abs() + e.abs())
    new = e + omd * (w - e)
    b = C_EMA * U * mag
    if bound is not None:
        b = float(decay) * bound + b
    return new, b


def sequence_ref(masters, decay, first_copy=True, e0=None):
    """The float64 average of a recorded sequence of fp32 masters and its accumulated bound:
    the first update copies (``first_copy``) or starts from ``e0``."""
    if first_copy:
        e = f64(masters[0])
        rest = masters[1:]
    else:
        e = f64(e0)
        rest = masters
    b = torch.zeros_like(e)
    for w in rest:
        e, b = update_ref(w, e, decay, b)
    return e, b


def worst_ratio(got, ref, bound):
    """max err / bound over the elements with a positive bound; where the bound is zero the
    value must be exact."""
    got = f64(got)
    assert torch.isfinite(got).all(), "non-finite average"
    err = (got - ref).abs()
    pos = bound > 0
    assert (err[~pos] == 0).all(), "an element with a zero bound differs"
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check(name, got, ref, bound) -> float:
    """Assert |got - ref| <= bound element by element; the worst err / (U * mag) in units of
    one rounding (bound / C_EMA is U * mag for a single update)."""
    w = worst_ratio(got, ref, bound)
    err = (f64(got) - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {err.numel()} elements outside the "
                           f"bound, worst err/bound {w:.3g}")
    return w


def outside_share(got, ref, bound) -> float:
    return float(((f64(got) - ref).abs() > bound).double().mean())


# ---- the kernels ------------------------------------------------------------------------------------
def make_streams(n, mdt, dev, base_off=0, seed=0):
    """w, e (fp32) and model (mdt or None): ranges of n elements inside sentinel guards, from a
    16-byte-aligned base (base_off 0) or from base[1:] (1).  The values are generated on the
    CPU: the same bits on either device and at either offset."""
    gen = torch.Generator().manual_seed(7000 + seed)
    lo = GUARD + base_off
    out = []
    for dt, fill in ((f32, lambda: torch.randn(n, generator=gen)),
                     (f32, lambda: torch.randn(n, generator=gen) * 0.5 + 0.25),
                     (mdt, lambda: torch.full((n,), 3.0))):
        if dt is None:
            out.append((None, None))
            continue
        base = torch.full((n + 2 * GUARD + 1,), SENTINEL, dtype=dt)
        base[lo:lo + n] = fill().to(dt)
        base = base.to(dev)
        out.append((base, base[lo:lo + n]))
    return out


def guards_intact(streams, n, base_off):
    lo = GUARD + base_off
    for base, _ in streams:
        if base is None:
            continue
        b = base.cpu().float()
        assert (b[:lo] == SENTINEL).all() and (b[lo + n:] == SENTINEL).all(), \
            "a launch wrote outside its range"


def run_modes(dev, n, mdt, base_off=0, decay=DECAY, seed=0):
    """update, then swap, then overwrite over one range.  Checks the update against float64
    and the two exact modes against copies and torch's cast, and the guards after each.
    Returns (worst update err/(U*mag), e after the update, w, e, model at the end), on the
    CPU."""
    streams = make_streams(n, mdt, dev, base_off, seed)
    (_, w), (_, e), (_, model) = streams
    w0, e0 = w.clone(), e.clone()
    ref, bound = update_ref(w0.cpu(), e0.cpu(), decay)
    K.ema_update(w, e, decay=decay)
    guards_intact(streams, n, base_off)
    assert torch.equal(w, w0), "the update wrote w"
    worst = check(f"update n={n} off={base_off}", e.cpu(), ref, bound) * C_EMA
    e1 = e.clone()
    K.ema_swap(w, e, model)
    guards_intact(streams, n, base_off)
    assert torch.equal(w, e1) and torch.equal(e, w0), "swap is not an exact exchange"
    if model is not None:
        assert torch.equal(model, e1.to(mdt)), "swap: model is not cast(new w)"
    K.ema_overwrite(w, e, model)
    guards_intact(streams, n, base_off)
    assert torch.equal(w, w0) and torch.equal(e, w0), "overwrite: w != e or e changed"
    if model is not None:
        assert torch.equal(model, w0.to(mdt)), "overwrite: model is not cast(e)"
    return worst, e1.cpu(), w.cpu(), e.cpu(), None if model is None else model.cpu()


def run_sizes(dev, mdt):
    """every size around a lane (8), a step (2048) and a chunk (4096), from an aligned base
    (load8 / store8) and from base[1:] (one by one): the same bits either way"""
    worst = 0.0
    for n in SIZES:
        a = run_modes(dev, n, mdt, 0, seed=n)
        b = run_modes(dev, n, mdt, 1, seed=n)
        assert torch.equal(a[1], b[1]), f"n={n}: an offset base changes the update's bits"
        worst = max(worst, a[0], b[0])
    return worst


def run_exact(dev, mdt, n=N_GRID, base_off=0):
    """omd == 1 stores w bit for bit (whatever e held, a NaN included); swap twice is the
    identity on w, e and model"""
    streams = make_streams(n, mdt, dev, base_off, seed=1)
    (_, w), (_, e), (_, model) = streams
    e[n // 2] = float("nan")
    w[0] = 1e-40                      # a subnormal survives a copy
    K.ema_update(w, e, decay=0.0)
    assert torch.equal(e, w), "decay 0 (omd == 1) is not a copy of w"
    e.mul_(0.5).add_(0.125)
    K.ema_swap(w, e, model)           # model := cast(w): the state a second pair returns to
    K.ema_swap(w, e, model)
    held = [t.clone() for t in (w, e)] + ([] if model is None else [model.clone()])
    K.ema_swap(w, e, model)
    K.ema_swap(w, e, model)
    now = [w, e] + ([] if model is None else [model])
    assert all(torch.equal(a, b) for a, b in zip(held, now)), "swap twice is not the identity"
    guards_intact(streams, n, base_off)


def run_skip(dev, mdt, n=N_GRID, base_off=0):
    """skip = 1 leaves every stream untouched in all three modes; skip = 0 does not"""
    streams = make_streams(n, mdt, dev, base_off, seed=2)
    (bw, w), (be, e), (bm, model) = streams
    held = [b.clone() for b in (bw, be)] + ([] if bm is None else [bm.clone()])
    one = FR.flag_of(dev, 1)
    K.ema_update(w, e, decay=DECAY, skip=one)
    K.ema_update(w, e, decay=0.0, skip=one)
    K.ema_swap(w, e, model, skip=one)
    K.ema_overwrite(w, e, model, skip=one)
    now = [bw, be] + ([] if bm is None else [bm])
    assert all(torch.equal(a, b) for a, b in zip(held, now)), "a skipped launch stored something"
    zero = FR.flag_of(dev, 0)
    K.ema_update(w, e, decay=DECAY, skip=zero)
    assert not torch.equal(be, held[1]), "skip = 0 skipped"
    assert one.item() == 1 and zero.item() == 0, "the flag was written"


# ---- bf16 averaging through the same harness ----------------------------------------------------------
EVIDENCE_DECAY = 0.999
EVIDENCE_STEPS = 64


def run_evidence(dev, n=N_GRID, steps=EVIDENCE_STEPS, decay=EVIDENCE_DECAY):
    """seed 0, ``steps`` steps of w -= 1e-2 * randn on an fp32 master: (share of the elements
    outside the accumulated bound of a bf16 ``lerp_`` average of the bf16 model copy, the same
    of the fp32 arena average of the master, the arena's worst err/bound).  Both start from
    the weights; the reference is the float64 average of the fp32 master sequence."""
    torch.manual_seed(0)
    w = torch.randn(n).to(dev)
    steps_ = [(1e-2 * torch.randn(n)).to(dev) for _ in range(steps)]
    e = w.clone()
    eb = w.to(bf16)
    ref, bound = f64(w.cpu()), torch.zeros(n, dtype=torch.float64)
    for d in steps_:
        w -= d
        K.ema_update(w, e, decay=decay)
        eb.lerp_(w.to(bf16), 1.0 - decay)        # AveragedModel / ModelEma on the bf16 model
        ref, bound = update_ref(w.cpu(), ref, decay, bound)
    return (outside_share(eb.cpu(), ref, bound), outside_share(e.cpu(), ref, bound),
            worst_ratio(e.cpu(), ref, bound))


# ---- the optimizers -------------------------------------------------------------------------------------
class MLP(torch.nn.Module):
    """37 -> 64 -> 10: 3082 parameters, odd sizes, four tensors"""

    def __init__(self):
        super().__init__()
        self.lin1 = torch.nn.Linear(37, 64)
        self.lin2 = torch.nn.Linear(64, 10)

    def forward(self, x):
        return self.lin2(torch.tanh(self.lin1(x)))


def make_mlp(dev, dtype):
    torch.manual_seed(0)
    return MLP().to(dtype).to(dev)


def make_batches(dev, dtype, steps, seed=0, n=8):
    gen = torch.Generator().manual_seed(900 + seed)
    return [(torch.randn(n, 37, generator=gen).to(dtype).to(dev),
             torch.randn(n, 10, generator=gen).to(dev)) for _ in range(steps)]


def loss_of(net, batch):
    x, y = batch
    return ((net(x).float() - y) ** 2).mean()


OPTIMIZERS = ["sgd", "adam", "lamb"]


def make_opt(kind, params, ema_decay, **kw):
    from mivod.optim import FusedAdam, FusedLAMB, FusedSGD
    if kind == "sgd":
        return FusedSGD(params, lr=0.1, momentum=0.9, ema_decay=ema_decay, **kw)
    if kind == "adam":
        return FusedAdam(params, lr=1e-2, weight_decay=1e-2, ema_decay=ema_decay, **kw)
    return FusedLAMB(params, lr=1e-2, ema_decay=ema_decay, **kw)


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def train(opt, net, batches, dev, record=True):
    """one step per batch; the masters of every arena after every step"""
    seq = []
    for b in batches:
        loss_of(net, b).backward()
        opt.step()
        opt.zero_grad()
        _sync(dev)
        if record:
            seq.append([a.master.clone().cpu() for a in opt._mv_arenas])
    return seq


def check_arenas(label, opt, seq, decay) -> float:
    """every arena's average against the float64 average of its recorded masters"""
    worst = 0.0
    for i, a in enumerate(opt._mv_arenas):
        assert a.ema is not None and a.ema.dtype == f32 and a.ema.numel() == a.master.numel()
        ref, bound = sequence_ref([s[i] for s in seq], decay)
        worst = max(worst, check(label, a.ema.cpu(), ref, bound))
    return worst


def opt_bits(opt):
    """masters, model copies and state arenas, as CPU tensors"""
    out = []
    for a in opt._mv_arenas:
        out += [a.master.cpu(), a.model.float().cpu()] + [a.state[k].cpu() for k in sorted(a.state)]
    return out


def same_bits(x, y):
    return len(x) == len(y) and all(torch.equal(a, b) for a, b in zip(x, y))


def model_optimizer(dev, kind, dtype, steps=4, decay=0.9):
    """(the average within the accumulated bound, step 1 an exact copy, weights and state the
    bits of a run with ema_decay=None); the worst err/bound"""
    net = make_mlp(dev, dtype)
    twin = copy.deepcopy(net)
    opt = make_opt(kind, net.parameters(), decay)
    plain = make_opt(kind, twin.parameters(), None)
    batches = make_batches(dev, dtype, steps)
    seq = train(opt, net, batches[:1], dev)
    for a in opt._mv_arenas:
        assert a.ema_updates == 1 and torch.equal(a.ema, a.master), "step 1 is not a copy"
    seq += train(opt, net, batches[1:], dev)
    train(plain, twin, batches, dev, record=False)
    assert all(a.ema is None for a in plain._mv_arenas), "ema_decay=None allocated an average"
    assert same_bits(opt_bits(opt), opt_bits(plain)), "the average changed the training"
    assert all(a.ema_updates == steps for a in opt._mv_arenas)
    for a in opt._mv_arenas:
        assert not torch.equal(a.ema, a.master), "the average did not lag"
    return check_arenas(f"{kind} {dtype}", opt, seq, decay), opt, net


def model_swap(dev, dtype):
    """ema_parameters(): inside, the parameters are cast(average); after, parameters and
    masters are back bit for bit; then ema_overwrite() adopts the average"""
    _, opt, net = model_optimizer(dev, "adam", dtype, steps=3)
    before = opt_bits(opt)
    params0 = [p.detach().clone() for p in net.parameters()]
    emas = [a.ema.clone() for a in opt._mv_arenas]
    masters0 = [a.master.clone() for a in opt._mv_arenas]
    with opt.ema_parameters():
        _sync(dev)
        for a, e in zip(opt._mv_arenas, emas):
            for i, p in enumerate(a.params):
                assert torch.equal(p.detach(), a.slot(e, i).to(dtype)), "not cast(average)"
            assert torch.equal(a.master, e), "the master is not the average"
        assert all(torch.equal(a.ema, m) for a, m in zip(opt._mv_arenas, masters0)), \
            "the average's arena does not hold the training weights"
        assert any(not torch.equal(p.detach(), q) for p, q in zip(net.parameters(), params0))
    _sync(dev)
    assert same_bits(opt_bits(opt), before), "the training weights are not restored"
    assert all(torch.equal(p.detach(), q) for p, q in zip(net.parameters(), params0))
    assert all(torch.equal(a.ema, e) for a, e in zip(opt._mv_arenas, emas))
    opt.ema_overwrite()
    _sync(dev)
    for a, e in zip(opt._mv_arenas, emas):
        assert torch.equal(a.master, e) and torch.equal(a.ema, e)
        assert torch.equal(a.model, e.to(dtype))


def model_state_dict(dev, dtype, tmp_path=None):
    """2 steps, state_dict() (or a checkpoint file), a fresh model and optimizer, one more
    step: the bits of the uninterrupted run, the average included"""
    from mivod.utils import checkpoint as CK
    net = make_mlp(dev, dtype)
    opt = make_opt("adam", net.parameters(), 0.9)
    batches = make_batches(dev, dtype, 3, seed=1)
    train(opt, net, batches[:2], dev, record=False)
    sd = opt.state_dict()
    st0 = sd["state"][0]
    assert "ema_param" in st0 and float(st0["ema_updates"]) == 2.0
    assert st0["ema_param"].dtype == f32
    net2 = copy.deepcopy(net)
    opt2 = make_opt("adam", net2.parameters(), 0.9)
    if tmp_path is None:
        opt2.load_state_dict(copy.deepcopy(sd))
    else:
        path = str(tmp_path / "checkpoint-2.safetensors")
        CK.save_checkpoint(path, net, opt, epoch=2)
        torch.manual_seed(5)
        net2 = MLP().to(dtype).to(dev)                 # other weights: the file restores them
        opt2 = make_opt("adam", net2.parameters(), 0.9)
        CK.load_checkpoint(path, net2, opt2)
    assert all(a.ema_updates == 2 for a in opt2._mv_arenas)
    train(opt, net, batches[2:], dev, record=False)
    train(opt2, net2, batches[2:], dev, record=False)

    def bits(o):
        return opt_bits(o) + [a.ema.cpu() for a in o._mv_arenas]
    assert same_bits(bits(opt), bits(opt2)), "the resumed run differs from the uninterrupted one"
    assert all(a.ema_updates == 3 for a in opt2._mv_arenas)
    # a dict without the average: a new one is seeded from the loaded weights
    sd = opt.state_dict()
    for st in sd["state"].values():
        del st["ema_param"], st["ema_updates"]
    opt2.load_state_dict(sd)
    assert all(a.ema is None and a.ema_updates == 0 for a in opt2._mv_arenas)
    assert "ema_param" not in opt2.state_dict()["state"][0]
    train(opt2, net2, batches[2:], dev, record=False)
    assert all(a.ema_updates == 1 and torch.equal(a.ema, a.master) for a in opt2._mv_arenas)


def state_keys(dev, kind, dtype):
    """the per-parameter state_dict() keys of one step with ema_decay=None"""
    net = make_mlp(dev, dtype)
    opt = make_opt(kind, net.parameters(), None)
    train(opt, net, make_batches(dev, dtype, 1), dev, record=False)
    return sorted(opt.state_dict()["state"][0])


# ---- the hook path ----------------------------------------------------------------------------------------
HOOK_MODES = ["overlapped", "guard_step", "guard_bucket", "clipped"]


def wrap(net, mode, ema_decay, kind="sgd"):
    """DistributedOptimizer over a fused optimizer in one of the four scheduling modes, several
    buckets.  MIVOD_GUARD_MODE is read at construction: the caller sets it for guard_bucket."""
    import mivod.torch as hvd
    hvd.init()
    kw = {}
    if mode == "clipped":
        kw["max_grad_norm"] = 0.05
    inner = make_opt(kind, net.parameters(), ema_decay, **kw)
    guard = mode.startswith("guard")
    opt = hvd.DistributedOptimizer(
        inner, named_parameters=net.named_parameters(), bucket_mb=0.002, first_bucket_mb=0.001,
        compression=hvd.Compression.fp16 if guard else hvd.Compression.none)
    assert len(opt.bucket_plan()) > 1
    assert opt.guard_stats()["enabled"] == guard
    if guard:
        assert opt.guard_stats()["mode"] == mode[len("guard_"):]
    return opt


def hook_path(dev, mode, dtype=bf16, steps=4, decay=0.9):
    """one rank: the average rides behind every bucket's step; bounded against the float64
    average of the recorded masters, the training the bits of a run with ema_decay=None"""
    net = make_mlp(dev, dtype)
    twin = copy.deepcopy(net)
    opt = wrap(net, mode, decay)
    plain = wrap(twin, mode, None)
    batches = make_batches(dev, dtype, steps, seed=2)
    seq = train(opt, net, batches, dev)
    train(plain, twin, batches, dev, record=False)
    assert same_bits(opt_bits(opt), opt_bits(plain)), "the average changed the training"
    if mode == "clipped":
        assert float(opt._mv_clip_block[0]) < 1.0, "max_grad_norm is above the norm: not clipped"
    assert all(a.ema_updates == steps for a in opt._mv_arenas)
    return check_arenas(f"hook path {mode}", opt, seq, decay)


def hook_overflow(dev, dtype=bf16, decay=0.9, bad_step=2, steps=4):
    """fp16 wire, guard in step mode, one inf gradient element at step ``bad_step`` (1-based):
    that step changes neither the weights nor the average, the next one proceeds, and the
    average is that of the applied steps"""
    import warnings
    net = make_mlp(dev, dtype)
    opt = wrap(net, "guard_step", decay)
    batches = make_batches(dev, dtype, steps, seed=3)
    seq, emas = [], []
    start = [a.master.clone().cpu() for a in opt._mv_arenas]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j, b in enumerate(batches, 1):
            loss = loss_of(net, b)
            if j == bad_step:
                loss = loss + net.lin2.bias[3].float() * float("inf")
            loss.backward()
            opt.step()
            opt.zero_grad()
            _sync(dev)
            seq.append([a.master.clone().cpu() for a in opt._mv_arenas])
            emas.append([a.ema.clone().cpu() for a in opt._mv_arenas])
        opt.state_dict()                 # resolves the last step's flags
    k = bad_step - 1
    # a skipped first step leaves the average at its seed, the weights it started from
    assert same_bits(seq[k], seq[k - 1] if k else start), "the overflowing step changed the weights"
    assert same_bits(emas[k], emas[k - 1] if k else start), \
        "the overflowing step changed the average"
    assert not same_bits(seq[k + 1], seq[k]) and not same_bits(emas[k + 1], emas[k]), \
        "the step after the skipped one did not proceed"
    assert opt.guard_stats()["skipped_steps"] == 1
    assert all(a.ema_updates == steps - 1 and a.step == steps - 1 for a in opt._mv_arenas)
    applied = [s for j, s in enumerate(seq) if j != k]
    return check_arenas(f"overflow at step {bad_step}", opt, applied, decay)
