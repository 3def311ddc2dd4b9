"""float64 references, counted bounds and shared cases for global gradient-norm clipping
(csrc/kernels/mv_clip.hip: grad_sumsq_kernel, clip_finalize_kernel; the gclip operand of every
K6 step kernel; ``max_grad_norm`` of mivod.optim.Fused*) and their PyTorch fallbacks
(mivod/ops/kernels.py).

A helper module, not a test file: tests/test_clip_cpu.py runs the fallbacks through it and
tests/test_clip_gpu.py the HIP kernels.  The method, ``U`` and ``check`` are those of
tests/flat_reference.py (read its header first): |got - ref| <= c * 2^-24 * mag.

Counts
------
grad_sumsq_kernel: a sum of positive terms, so mag is the sum itself and c the depth of the
  summation.  A lane adds the squares of its 2 x 8 elements in turn: the square 1 (fused
  into the add on the GPU; counted), 16 adds (the first, to 0, is exact; counted); wave_sum
  adds 6 times; block_sum adds the 4 wave results: 4.
  => C_PARTIAL = 1 + 16 + 6 + 4 = 27, for every dtype, size and alignment (the element ->
  lane mapping does not depend on the alignment, so an offset view gives the same bits).
clip_finalize_kernel, from the STORED fp32 partials: the sum, the root, gscale *, + 1e-6 and
  the quotient are float64 (total/256 + 8 + 4 roundings of 2^-53: under 2^-40 of one U for
  any total below 2^20); each result is rounded to fp32 once.  => C_CLIP = 1 + 1 (the second
  covers all of float64).  coef == 1.0 exactly whenever the float64 quotient exceeds 1.
the norm end to end (partials taken by the kernel too): the sum carries 27 U, the root halves
  it (14, rounded up), then C_CLIP.  => C_NORM = 16; the coefficient, where it clips, is
  max_norm / (norm + 1e-6), the same relative error: C_COEF = 16.
a clipped step: gscale' = fp32(gscale) * coef, one more rounding, reaches the step where the
  step's own count has "gscale r" (1): the step's c grows by C_GCLIP = C_COEF + 1 = 17 against
  the same mag (every mag carries |g * gscale| along every path the gradient takes).

Worst err / (2^-24 * mag) measured over all of tests/test_clip_gpu.py on an MI355X (every test
prints its own next to c): partials 1.69 (c 27); clip_finalize coef 0.49, norm 0.51 (c 2); the
model level grad_norm() 1.06 (c 16), w 2.19, exp_avg 3.16, exp_avg_sq 5.59, momentum_buffer 2.46
(c = the step's + 17).
"""
from __future__ import annotations

import math

import torch

import adaptive_reference as AR
import flat_reference as FR
import lamb_reference as LR
from flat_reference import (BAD_VALUES, DTYPES, FINITE_MAX, N_GRID, SIZES, U, Out,  # noqa: F401
                            bad_positions, check, clone_inputs, f64, flag_of)
from mivod.ops import kernels as K

C_PARTIAL = 1 + 16 + 6 + 4
C_CLIP = 2
C_NORM = (C_PARTIAL + 1) // 2 + C_CLIP
C_COEF = C_NORM
C_GCLIP = C_COEF + 1
assert (C_PARTIAL, C_NORM, C_GCLIP) == (27, 16, 17)

f32 = torch.float32
GSCALE = 0.37                     # not a power of two
NAN = float("nan")


# --------------------------------------------------------------------------- A. grad_sumsq
def sumsq_ref(x: torch.Tensor) -> Out:
    """float64 sum of squares of every 4096-element chunk of the stored values"""
    v = f64(x)
    nc = K.sumsq_chunks(v.numel())
    pad = torch.zeros(nc * K.CHUNK, dtype=torch.float64)
    pad[:v.numel()] = v * v
    ref = pad.view(nc, K.CHUNK).sum(dim=1)
    return Out(ref, ref.clone(), C_PARTIAL)


def view_of(vals: torch.Tensor, dev, base_off: int) -> torch.Tensor:
    """``vals`` on ``dev`` as base[base_off : base_off + n]: base_off = 1 is a view no 16-byte
    access may use (the one-by-one path)"""
    base = torch.zeros(vals.numel() + 8, dtype=vals.dtype, device=dev)
    x = base[base_off:base_off + vals.numel()]
    x.copy_(vals)
    assert (x.data_ptr() % 16 == 0) == (base_off == 0)
    return x


def run_sumsq(dev, n, dt, base_off=0, seed=0):
    """One launch against fp64 into a NaN-filled buffer: exactly ceil(n / 4096) entries are
    written; a second launch gives the same bits.  Returns (worst ratio, the partials)."""
    gen = torch.Generator().manual_seed(4000 + seed)
    vals = (torch.randn(n, generator=gen) * 3.0).to(dt)
    x = view_of(vals, dev, base_off)
    ref = sumsq_ref(vals)
    nc = K.sumsq_chunks(n)
    p = torch.full((nc + 3,), NAN, dtype=f32, device=dev)
    K.grad_sumsq(x, p)
    worst = check(f"grad_sumsq n={n} {dt} off={base_off}", p[:nc], ref)
    assert torch.isnan(p[nc:]).all(), "grad_sumsq wrote behind its ceil(n / 4096) partials"
    q = torch.full((nc + 3,), NAN, dtype=f32, device=dev)
    K.grad_sumsq(x, q, None)
    assert torch.equal(p[:nc], q[:nc]), "two launches differ"
    return worst, p[:nc].clone()


def run_sumsq_flag(dev, dt, base_off=0):
    """The flag of grad_sumsq behaves as nonfinite_scan's (flat_reference.run_nonfinite):
    finite extremes leave it (their squares may overflow the partial: that is not the flag's
    business), a preset 1 stays, one bad element at any of ``bad_positions`` sets it; and
    the partials do not depend on whether a flag is given."""
    n = N_GRID
    clean = torch.ones(n, dtype=dt)
    clean[5], clean[6] = FINITE_MAX[dt], -FINITE_MAX[dt]
    x = view_of(clean, dev, base_off)
    nc = K.sumsq_chunks(n)
    p = torch.zeros(nc, dtype=f32, device=dev)
    flag = flag_of(dev)
    K.grad_sumsq(x, p, flag)
    assert flag.item() == 0, "a finite extreme set the flag"
    q = torch.zeros(nc, dtype=f32, device=dev)
    K.grad_sumsq(x, q, None)
    assert torch.equal(p, q), "the flag operand changes the partials"
    flag = flag_of(dev, 1)
    K.grad_sumsq(x, p, flag)
    assert flag.item() == 1, "the flag is OR-ed, a preset 1 stays"
    for pos in bad_positions(n):
        for bad in BAD_VALUES:
            x.copy_(clean)
            x[pos] = bad
            flag = flag_of(dev)
            K.grad_sumsq(x, p, flag)
            assert flag.item() == 1, f"missed {bad} at {pos}"


# --------------------------------------------------------------------------- B. clip_finalize
FINALIZE_COUNTS = [1, 255, 256, 257, 3 * 256 + 5]
FINALIZE_CASES = ["below", "above", "zero", "nan", "inf"]


def clip_ref(partials, gscale, max_norm):
    """(coef, norm) of the float64 formula on the stored partials"""
    s = math.fsum(f64(partials).tolist())
    norm = gscale * math.sqrt(s)
    return min(1.0, max_norm / (norm + 1e-6)), norm


def run_finalize(dev, count, case):
    """clip_finalize on ``count`` stored partials (NaN behind them: only [0, count) is read).
    Returns the worst ratios of (coef, norm), or None where the case asserts exact values."""
    gen = torch.Generator().manual_seed(5000 + count)
    p = torch.rand(count, generator=gen) * 7.0 + 0.01
    if case == "zero":
        p.zero_()
    buf = torch.full((count + 5,), NAN, dtype=f32)
    buf[:count] = p
    _, norm0 = clip_ref(p, GSCALE, 1.0)
    max_norm = {"below": 2.0 * norm0, "above": 0.25 * norm0}.get(case, 1.0)
    if case in ("nan", "inf"):
        buf[count // 2] = NAN if case == "nan" else float("inf")
    buf = buf.to(dev)
    clip = torch.full((4,), 9.0, dtype=f32, device=dev)
    K.clip_finalize(buf, count, clip, gscale=GSCALE, max_norm=max_norm)
    coef, norm = float(clip[0]), float(clip[1])
    assert float(clip[2]) == 9.0 and float(clip[3]) == 9.0, "clip_finalize wrote behind clip[1]"
    if case == "nan":
        assert math.isnan(coef) and math.isnan(norm), (coef, norm)
        return None
    if case == "inf":
        assert not math.isfinite(coef) and norm == math.inf, (coef, norm)
        return None
    rc, rn = clip_ref(p, GSCALE, max_norm)
    wn = check(f"clip norm {case} {count}", clip[1:2], Out(torch.tensor([rn], dtype=torch.float64),
                                                          torch.tensor([abs(rn)], dtype=torch.float64),
                                                          C_CLIP))
    if case in ("below", "zero"):
        assert rc == 1.0 and coef == 1.0, (case, coef)
        if case == "zero":
            assert norm == 0.0
        return 0.0, wn
    assert rc < 0.3
    wc = check(f"clip coef {case} {count}", clip[0:1], Out(torch.tensor([rc], dtype=torch.float64),
                                                          torch.tensor([rc], dtype=torch.float64),
                                                          C_CLIP))
    return wc, wn


# --------------------------------------------------------------------------- C. the step kernels
STEP_KINDS = (["sgd", "adam", "adamw", "adadelta", "lars", "lamb", "adagrad"]
              + [f"rmsprop_c{int(c)}m{int(m != 0)}" for c, m in AR.RMSPROP_FLAGS])
STEP_SIZES = [4097, 3 * 4096 + 5]
CLIP_COEF = 0.3711


def build_step(kind, n, dev, gdt=torch.float16, mdt=torch.bfloat16):
    """(stored inputs, run) of one step kernel on a gradient of ``n`` elements (LARS, LAMB: an
    adapted segment of n and a flagged one of 70); run(t, **kw) does the step in place with
    ``kw`` (gscale, gclip, skip) over the representative hyperparameters."""
    if kind in ("sgd", "adadelta"):
        t = FR.make_inputs(kind, n, gdt, mdt, dev, seed=31)
        return t, lambda t, **kw: FR.call_step(kind, t, dict(FR.HP[kind], **kw))
    if kind in ("adam", "adamw"):
        t = FR.make_inputs("adam", n, gdt, mdt, dev, seed=32)
        hp = dict(FR.HP["adam"], adamw=kind == "adamw")
        return t, lambda t, **kw: FR.call_step("adam", t, dict(hp, **kw))
    if kind == "lars":
        total, lars = FR.lars_case(n)
        t = FR.make_inputs("lars", total, gdt, mdt, dev, seed=33)
        extra = FR.lars_extra(lars, dev)
        return t, lambda t, **kw: FR.call_step("lars", t, dict(FR.HP["lars"], **kw), **extra)
    if kind == "lamb":
        total, layout = LR.pair_layout(n)
        t = LR.lamb_inputs(total, gdt, mdt, dev, layout, seed=34)
        return t, lambda t, **kw: LR.call_lamb(t, dict(LR.HP_LAMB, **kw), layout, dev)
    if kind == "adagrad":
        t = AR.adaptive_inputs("adagrad", n, gdt, mdt, dev, seed=35)
        return t, lambda t, **kw: AR.call_step("adagrad", t, dict(AR.HP["adagrad"], **kw))
    centered, mom = kind[-3] == "1", (0.9 if kind[-1] == "1" else 0.0)
    hp = dict(AR.HP["rmsprop"], centered=centered, momentum=mom)
    t = AR.adaptive_inputs("rmsprop", n, gdt, mdt, dev, seed=36, **AR.flags_of(hp))
    return t, lambda t, **kw: AR.call_step("rmsprop", t, dict(hp, **kw))


def _tensors(t):
    return {k: v for k, v in t.items() if torch.is_tensor(v)}


def _equal(a, b):
    return [k for k, v in _tensors(a).items() if not torch.equal(v, b[k])]


def run_step_clip(kind, n, dev):
    """gclip=[c] equals, bit for bit, the unclipped call with gscale' = fp32(gscale * c), and
    differs from the unclipped call with gscale; gclip=[1] equals no gclip; with skip set a
    clipped call touches nothing."""
    t0, run = build_step(kind, n, dev)
    gs = 0.25
    gs2 = float(torch.tensor(gs, dtype=f32) * torch.tensor(CLIP_COEF, dtype=f32))
    clip = torch.tensor([CLIP_COEF, 123.0], dtype=f32, device=dev)
    one = torch.ones(1, dtype=f32, device=dev)
    a, b, c, d, e = (clone_inputs(t0) for _ in range(5))
    run(a, gscale=gs, gclip=clip)
    run(b, gscale=gs2)
    assert not _equal(a, b), f"{kind}: gclip=[c] differs from gscale*c in {_equal(a, b)}"
    run(c, gscale=gs)
    assert "w" in _equal(a, c), f"{kind}: the clip coefficient changes nothing"
    run(d, gscale=gs, gclip=one)
    assert not _equal(d, c), f"{kind}: gclip=[1] differs from no gclip in {_equal(d, c)}"
    run(e, gscale=gs, gclip=clip, skip=flag_of(dev, 1))
    assert not _equal(e, t0), f"{kind}: a skipped clipped step changed {_equal(e, t0)}"


# --------------------------------------------------------------------------- D. the model level
MAX_NORM = 1.0
GRAD_SCALES = [0.02, 40.0, 0.01, 5.0]        # by the reference's norms: no clip, clip, no, clip


def mlp(mdt, dev):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(70, 64), torch.nn.Tanh(), torch.nn.Linear(64, 10))
    return m.to(dev).to(mdt)


def seeded_grads(model, step):
    """the same gradient bits on either device, in the parameters' dtype"""
    gen = torch.Generator().manual_seed(600 + step)
    return [(torch.randn(p.shape, generator=gen) * GRAD_SCALES[step] / math.sqrt(p.numel()))
            .to(p.dtype).to(p.device) for p in model.parameters()]


OPTIMIZERS = ["adamw", "lamb", "sgd"]
OPT_HP = {"adamw": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
          "lamb": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2),
          "sgd": dict(lr=0.05, momentum=0.9, weight_decay=1e-4)}


def make_opt(name, params, **kw):
    from mivod.optim import FusedAdamW, FusedLAMB, FusedSGD
    cls = {"adamw": FusedAdamW, "lamb": FusedLAMB, "sgd": FusedSGD}[name]
    return cls(params, **OPT_HP[name], **kw)


def _arena_ref(name, a, before, coef, step):
    """the float64 step of the whole arena from its stored state ``before``, with the
    reference's own coefficient as the gradient scale"""
    hp = OPT_HP[name]
    if name == "sgd":
        return FR.sgd_ref(before["g"], before["w"], before["momentum_buffer"], lr=hp["lr"],
                          momentum=hp["momentum"], weight_decay=hp["weight_decay"], gscale=coef,
                          first=step == 1), {"w": "w", "momentum_buffer": "mom"}
    b1, b2 = hp["betas"]
    kw = dict(lr=hp["lr"], beta1=b1, beta2=b2, eps=hp["eps"], weight_decay=hp["weight_decay"],
              gscale=coef, step=step)
    names = {"w": "w", "exp_avg": "m", "exp_avg_sq": "v"}
    if name == "adamw":
        return FR.adam_ref(before["g"], before["w"], before["exp_avg"], before["exp_avg_sq"],
                           adamw=True, **kw), names
    sizes = [p.numel() for p in a.params]
    flags = [1 if p.dim() <= 1 else 0 for p in a.params]
    return LR.lamb_ref(before["g"], before["w"], before["exp_avg"], before["exp_avg_sq"], sizes,
                       a.offsets, flags, **kw), names


def run_model(dev, mdt, name):
    """Four standalone steps of a Fused* optimizer with max_grad_norm on seeded gradients, each
    against the float64 clip followed by the float64 step from the optimizer's stored state
    (bound: the step's c + C_GCLIP); grad_norm() against the float64 norm (C_NORM).  Then
    max_grad_norm = None gives the bits of an optimizer that never had it.  Returns the worst
    ratios and the reference coefficients."""
    model = mlp(mdt, dev)
    opt = make_opt(name, model.parameters(), max_grad_norm=MAX_NORM)
    worst, coefs = {}, []
    for s in range(4):
        grads = seeded_grads(model, s)
        for p, g in zip(model.parameters(), grads):
            p.grad = g
        arenas = opt._mv_build()
        assert len(arenas) == 1
        a = arenas[0]
        a.sync_master_if_modified()
        before = {"w": a.master.clone(), **{k: v.clone() for k, v in a.state.items()}}
        opt.step()
        before["g"] = a.grad.clone()
        norm = math.sqrt(math.fsum((f64(before["g"]) ** 2).tolist()))
        coef = min(1.0, MAX_NORM / (norm + 1e-6))
        coefs.append(coef)
        wn = check(f"{name} grad_norm step {s}", opt.grad_norm().reshape(1),
                   Out(torch.tensor([norm], dtype=torch.float64),
                       torch.tensor([norm], dtype=torch.float64), C_NORM))
        worst["norm"] = max(worst.get("norm", 0.0), wn)
        ref, names = _arena_ref(name, a, before, coef, a.step)
        got = {"w": a.master, **a.state}
        for k, r in names.items():
            out = ref[r]
            c = torch.as_tensor(out.c, dtype=torch.float64) + C_GCLIP
            worst[k] = max(worst.get(k, 0.0), check(f"{name} {k} step {s}", got[k],
                                                    Out(out.ref, out.mag, c)))
        if a.low_precision:
            assert torch.equal(a.model, a.master.to(a.dtype)), "model copy is not RNE(master)"
    assert min(coefs) < 0.5 and max(coefs) == 1.0, \
        f"the reference must clip at least once and not clip at least once: {coefs}"
    # back to None: the bits of an optimizer built without max_grad_norm from the same state
    twin_model = mlp(mdt, dev)
    twin = make_opt(name, twin_model.parameters())
    with torch.no_grad():
        for q, p in zip(twin_model.parameters(), model.parameters()):
            q.copy_(p)
    twin.load_state_dict(opt.state_dict())
    opt.max_grad_norm = None
    for m_, o_ in ((model, opt), (twin_model, twin)):
        for p, g in zip(m_.parameters(), seeded_grads(m_, 1)):
            p.grad = g
        o_.step()
    for p, q in zip(model.parameters(), twin_model.parameters()):
        assert torch.equal(p, q), "max_grad_norm = None does not return to the unclipped bits"
    return worst, coefs
