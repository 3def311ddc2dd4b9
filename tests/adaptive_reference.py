"""float64 references and derived error bounds for the RMSprop and Adagrad steps:
rmsprop_flat_kernel and adagrad_flat_kernel (csrc/kernels/mv_adaptive.hip) and their PyTorch
fallbacks (mivod/ops/kernels.py: rmsprop_step, adagrad_step).

A helper module, not a test file: tests/test_adaptive_cpu.py runs the fallbacks through it and
tests/test_adaptive_gpu.py the HIP kernels.  The method, ``U``, ``check`` and the layouts are
those of tests/flat_reference.py (read its header first): every output must satisfy, per
element,

    |got - ref| <= c * 2^-24 * mag

with ``mag`` the sum of the absolute values of the terms on the way to the output, carried
through a quotient or a square root by first-order sensitivity (for sqrt(x): mag_x / sqrt(x),
without the derivative's factor 1/2), and ``c`` the fp32 roundings on the longest path, counted
from the kernel source.  Where ``mag`` has several sensitivity terms, each path's error is at
most its own count times U times its own term, so ``c`` is the count of the longest path.

Counts (r = rounding of a hyperparameter, * + - / sqrt = one rounding each)
---------------------------------------------------------------------------
rmsprop_flat_kernel
  gr  = g*gscale + wd*w            gscale r, * | wd r, * -> 2, + -> 3
  sq  = alpha*sq + oma*gr*gr       oma = 1-alpha rounded once on the host: r; gr twice = 6;
                                   two * -> 9, + -> 10 (longer than alpha r, * = 2);
                                   mag_sq = alpha*|sq| + (1-alpha)*mag_gr^2
  ga  = alpha*ga + oma*gr          gr 3, oma r, * -> 5, + -> 6 (centered)
                                   mag_ga = alpha*|ga| + (1-alpha)*mag_gr
  x   = max(sq - ga*ga, 0)         mag_x = mag_sq + 2|ga|*mag_ga.  The ga*ga path: ga is off by
                                   at most 6U*mag_ga, so ga^2 by 6U * 2|ga|*mag_ga, and the
                                   product rounds once more, U*ga^2 <= U/2 * 2|ga|*mag_ga
                                   (|ga| <= mag_ga): 7 against its term.  The sq path: 10 against
                                   mag_sq.  The longer, 10, and the subtraction -> 11.  max is
                                   exact.  Not centered: x = sq, 10.
  avg = sqrt(x) + eps              x 11, sqrt 12, (eps r shares), + -> 13 (not centered: 12)
                                   mag_avg = mag_x/sqrt(x) + eps
  q   = gr/avg                     avg path: 13, / -> 14;  gr path: 3, / -> 4
                                   mag_q = mag_gr/avg + |q|/avg * mag_avg
  buf = mu*buf + q                 q 14 (longer than mu r, * = 2), + -> 15 (momentum)
                                   mag_buf = mu*|buf| + mag_q
  w   = w - lr*buf                 buf 15, lr r, * -> 17, - -> 18;  mag_w = |w| + lr*mag_buf
        (no momentum: w - lr*q     14, r, *, - -> 17, the same with mag_q)
  => C_RMSPROP_SQ = 10, C_RMSPROP_GA = 6, C_RMSPROP_BUF = 15, C_RMSPROP_W = 18 (every flag
     combination is a sub-path of these)
  Where x is clamped (the fp64 difference is below zero): avg = eps exactly up to eps's own
  rounding, mag_avg = eps; the dedicated clamp case only.

adagrad_flat_kernel
  gr  3;  sum = sum + gr*gr        gr twice = 6, * -> 7, + -> 8;  mag_sum = |sum| + mag_gr^2
  avg = sqrt(sum) + eps            8, sqrt 9, + -> 10;  mag_avg = mag_sum/sqrt(sum) + eps
  q   = gr/avg                     / -> 11
  w   = w - clr*q                  clr (taken in double on the host) r, * -> 13, - -> 14
  => C_ADAGRAD_SUM = 8, C_ADAGRAD_W = 14

The model copy is the RNE rounding of the stored fp32 master, bit for bit.  The fallbacks do
the same arithmetic in fp32 torch ops, one rounding per op, so the same counts hold for them.

The centered inputs are generated as ga = rho*sqrt(sq) with |rho| <= 0.5, and ``rmsprop_ref``
asserts that the fp64 variance sq' - ga'^2 is at least 0.25 sq' everywhere (by
a x^2 + (1-a) y^2 - (a x + (1-a) y)^2 = a (1-a) (x-y)^2 the update only adds to it): the
root's sensitivity stays bounded and the clamp inactive.  ``clamp_case`` builds the opposite.

Worst err / (2^-24 * mag) measured over all of tests/test_adaptive_gpu.py on an MI355X (every
test prints its own next to c): RMSprop w 1.64, sq 3.13, ga 2.22, buf 1.63 (c 18, 10, 6, 15);
Adagrad w 1.18, sum 2.62 (c 14, 8).  The fallbacks, over all of tests/test_adaptive_cpu.py: w 2.26,
sq 3.34, ga 2.27, buf 2.21; w 1.54, sum 2.57.
"""
from __future__ import annotations

import torch

from flat_reference import (DTYPES, HALF_ULP, MODELS, N_GRID, SIZES, STATE, U,  # noqa: F401
                            UNAL_OFFS, UNAL_SIZES, UNAL_TOTAL, Out, check, check_outputs,
                            clone_inputs, f64, flag_of, fmt, make_inputs, sensitivity)
from mivod.ops import kernels as K

C_RMSPROP_SQ, C_RMSPROP_GA, C_RMSPROP_BUF, C_RMSPROP_W = 10, 6, 15, 18
C_ADAGRAD_SUM, C_ADAGRAD_W = 8, 14
C_OF = {"rmsprop": dict(w=C_RMSPROP_W, sq=C_RMSPROP_SQ, ga=C_RMSPROP_GA, buf=C_RMSPROP_BUF),
        "adagrad": dict(w=C_ADAGRAD_W, sum=C_ADAGRAD_SUM)}

# the state names make_inputs and check_outputs go by (flat_reference.STATE is their table)
STATE.setdefault("rmsprop", ["sq", "ga", "buf"])
STATE.setdefault("adagrad", ["sum"])

HP = {
    "rmsprop": dict(lr=0.01, alpha=0.99, eps=1e-8, weight_decay=1e-4, momentum=0.9, centered=True,
                    gscale=0.25),
    "adagrad": dict(lr=0.01, eps=1e-10, weight_decay=1e-4, gscale=0.25),
}
# the flag cases: a rate, a decay and an eps large enough that each moves w far past a bound
RMSPROP_BASE = dict(lr=0.05, alpha=0.9, eps=1e-2, weight_decay=0.1, momentum=0.9, centered=True,
                    gscale=0.5)
ADAGRAD_BASE = dict(lr=0.05, eps=1e-2, weight_decay=0.1, gscale=0.5)
RMSPROP_FLAGS = [(False, 0.0), (False, 0.9), (True, 0.0), (True, 0.9)]     # (centered, momentum)


# --------------------------------------------------------------------------- references
def rmsprop_ref(g, w, sq, ga, buf, *, lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0,
                centered=False, gscale=1.0, clamp_expected=False):
    """``ga`` is used when ``centered`` and ``buf`` when ``momentum != 0`` (or when given with
    momentum 0, as the kernel does).  Unless ``clamp_expected``, asserts the fp64 variance
    >= 0.25 sq' everywhere; with it, that the variance is below zero everywhere by more than
    100 bounds, so that no fp32 evaluation can see it positive."""
    g, w, sq = f64(g), f64(w), f64(sq)
    gr = g * gscale + weight_decay * w
    mag_gr = (g * gscale).abs() + (weight_decay * w).abs()
    sq_new = alpha * sq + (1 - alpha) * gr * gr
    mag_sq = (alpha * sq).abs() + (1 - alpha) * mag_gr * mag_gr
    out = {"sq": Out(sq_new, mag_sq, C_RMSPROP_SQ)}
    x, mag_x = sq_new, mag_sq
    clamped = torch.zeros_like(x, dtype=torch.bool)
    if centered:
        ga = f64(ga)
        ga_new = alpha * ga + (1 - alpha) * gr
        mag_ga = (alpha * ga).abs() + (1 - alpha) * mag_gr
        out["ga"] = Out(ga_new, mag_ga, C_RMSPROP_GA)
        x = sq_new - ga_new * ga_new
        mag_x = mag_sq + 2 * ga_new.abs() * mag_ga
        if clamp_expected:
            assert (x < -100 * 11 * U * mag_x).all(), "the clamp case must be below zero"
            clamped = x < 0
        else:
            assert (x >= 0.25 * sq_new).all(), \
                f"variance down to {float((x / sq_new).min()):.3g} of sq: inputs outside the design"
        x = x.clamp(min=0)
    root = x.sqrt()
    mag_root = torch.where(root > 0, mag_x / root, mag_x.sqrt())
    mag_root = torch.where(clamped, torch.zeros_like(mag_root), mag_root)
    avg, mag_avg = root + eps, mag_root + eps
    q = gr / avg
    mag_q = mag_gr / avg + q.abs() / avg * mag_avg
    if buf is not None:
        buf = f64(buf)
        b_new, mag_b = momentum * buf + q, (momentum * buf).abs() + mag_q
        out["buf"] = Out(b_new, mag_b, C_RMSPROP_BUF)
        q, mag_q = b_new, mag_b
    out["w"] = Out(w - lr * q, w.abs() + abs(lr) * mag_q, C_RMSPROP_W)
    return out


def adagrad_ref(g, w, sum, *, lr, eps=1e-10, weight_decay=0.0, gscale=1.0):
    """``lr`` is the decayed rate of the step (lr0 / (1 + (step-1) * lr_decay))."""
    g, w, s = f64(g), f64(w), f64(sum)
    gr = g * gscale + weight_decay * w
    mag_gr = (g * gscale).abs() + (weight_decay * w).abs()
    s_new, mag_s = s + gr * gr, s.abs() + mag_gr * mag_gr
    root = s_new.sqrt()
    mag_root = torch.where(root > 0, mag_s / root, mag_s.sqrt())
    avg, mag_avg = root + eps, mag_root + eps
    q = gr / avg
    mag_q = mag_gr / avg + q.abs() / avg * mag_avg
    return {"sum": Out(s_new, mag_s, C_ADAGRAD_SUM),
            "w": Out(w - lr * q, w.abs() + abs(lr) * mag_q, C_ADAGRAD_W)}


# --------------------------------------------------------------------------- inputs and runners
def adaptive_inputs(kind, n, gdt, mdt, dev, seed=0, centered=True, momentum=True, clamp=False):
    """Stored inputs (flat_reference.make_inputs), generated on the CPU: the same bits on
    either device.  rmsprop: sq in [0, 1), ga = rho * sqrt(sq) with |rho| <= 0.5 (``clamp``:
    ga = 2 sqrt(sq) + 3, so that ga^2 > sq after the step too), buf normal; a state the flags
    do not use is None.  adagrad: sum = |normal|."""
    t = make_inputs(kind, n, gdt, mdt, "cpu", seed)
    if kind == "rmsprop":
        root = t["sq"].sqrt()
        t["ga"] = (2.0 * root + 3.0) if clamp else 0.5 * t["ga"].clamp(-1.0, 1.0) * root
        if not centered:
            t["ga"] = None
        if not momentum:
            t["buf"] = None
    else:
        t["sum"] = t["sum"].abs()
    return {k: (x.to(dev) if torch.is_tensor(x) else x) for k, x in t.items()}


def call_step(kind, t, hp, **extra):
    """The step in place on ``t`` through mivod.ops.kernels (the HIP kernel on a GPU, the
    fallback on the CPU)."""
    if kind == "rmsprop":
        K.rmsprop_step(t["g"], t["w"], t["sq"], t["ga"], t["buf"], t["model"], **hp, **extra)
    else:
        K.adagrad_step(t["g"], t["w"], t["sum"], t["model"], **hp, **extra)


def ref_step(kind, t, hp, **extra):
    if kind == "rmsprop":
        return rmsprop_ref(t["g"], t["w"], t["sq"], t["ga"], t["buf"], **hp, **extra)
    return adagrad_ref(t["g"], t["w"], t["sum"], **hp)


def flags_of(hp):
    return dict(centered=bool(hp.get("centered")), momentum=hp.get("momentum", 0.0) != 0)


def run_step(kind, n, gdt, mdt, dev, hp=None, seed=0):
    """One step against fp64: ({output: worst err/(U*mag)}, the reference, the tensors)."""
    hp = dict(HP[kind] if hp is None else hp)
    t = adaptive_inputs(kind, n, gdt, mdt, dev, seed, **flags_of(hp))
    ref = ref_step(kind, t, hp)
    call_step(kind, t, hp)
    return check_outputs(f"{kind} n={n} {gdt}/{mdt}", kind, t, ref), ref, t


def view_inputs(t, off, n):
    return {k: (x[off:off + n] if torch.is_tensor(x) else x) for k, x in t.items()}


def run_unaligned(kind, gdt, mdt, dev, seed=13):
    """One launch per UNAL_* segment on views ``buf[off : off+n]`` that no 16-byte access may
    use (the scalar path of every element); nothing outside the segments may change."""
    hp = dict(HP[kind])
    t = adaptive_inputs(kind, UNAL_TOTAL, gdt, mdt, dev, seed, **flags_of(hp))
    ref = ref_step(kind, t, hp)
    for off, n in zip(UNAL_OFFS, UNAL_SIZES):
        call_step(kind, view_inputs(t, off, n), hp)
    assert UNAL_OFFS[-1] + UNAL_SIZES[-1] == UNAL_TOTAL    # the segments tile the buffer
    return check_outputs(f"{kind} unaligned {gdt}/{mdt}", kind, t, ref)


def run_rmsprop_flags(centered, momentum, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    """One of the four flag combinations on the flag-case hyperparameters; every flag and
    hyperparameter it uses must move w by more than 100 bounds against the reference
    without it.  Returns (worst ratios, {flag: sensitivity})."""
    hp = dict(RMSPROP_BASE, centered=centered, momentum=momentum)
    worst, ref, _ = run_step("rmsprop", n, gdt, mdt, dev, hp=hp, seed=3)
    # every variant is evaluated on the full set of states, the flags choosing among them
    full = adaptive_inputs("rmsprop", n, gdt, mdt, "cpu", 3)

    def variant(**kw):
        v = dict(hp, **kw)
        f = flags_of(v)
        return rmsprop_ref(full["g"], full["w"], full["sq"], full["ga"],
                           full["buf"] if f["momentum"] else None, **v)

    sens = {"centered": sensitivity(ref, variant(centered=not centered)),
            "momentum": sensitivity(ref, variant(momentum=0.9 - momentum)),
            "weight_decay": sensitivity(ref, variant(weight_decay=0.0)),
            "eps": sensitivity(ref, variant(eps=1e-8))}
    for flag, s in sens.items():
        assert s > 100, f"rmsprop centered={centered} momentum={momentum}: {flag} moves w by " \
                        f"only {s:.3g} bounds"
    return worst, sens


def run_adagrad_flags(weight_decay, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    hp = dict(ADAGRAD_BASE, weight_decay=weight_decay)
    worst, ref, _ = run_step("adagrad", n, gdt, mdt, dev, hp=hp, seed=4)
    t0 = adaptive_inputs("adagrad", n, gdt, mdt, "cpu", 4)
    sens = {"weight_decay": sensitivity(ref, ref_step("adagrad", t0, dict(hp, weight_decay=0.1 - weight_decay))),
            "eps": sensitivity(ref, ref_step("adagrad", t0, dict(hp, eps=1e-10)))}
    for flag, s in sens.items():
        assert s > 100, f"adagrad wd={weight_decay}: {flag} moves w by only {s:.3g} bounds"
    return worst, sens


def run_clamp(dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    """ga^2 > sq by construction: the variance is clamped at zero, avg = eps, and w is finite
    and equal to w - lr * gr / eps within the bound (torch's own form gives NaN here)."""
    hp = dict(RMSPROP_BASE, momentum=0.0, eps=1e-2)
    t = adaptive_inputs("rmsprop", n, gdt, mdt, dev, seed=5, momentum=False, clamp=True)
    ref = ref_step("rmsprop", t, hp, clamp_expected=True)
    w0, g0 = f64(t["w"]), f64(t["g"])
    plain = w0 - hp["lr"] * ((g0 * hp["gscale"] + hp["weight_decay"] * w0) / (0.0 + hp["eps"]))
    assert torch.equal(ref["w"].ref, plain), "the clamped reference is the avg = eps formula"
    call_step("rmsprop", t, hp)
    return check_outputs("rmsprop clamp", "rmsprop", t, ref)


def run_skip(kind, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    """skip=[1] leaves w, the state and the model copy bit-identical; skip=[0] equals
    skip=None bit for bit (and does update)."""
    t = adaptive_inputs(kind, n, gdt, mdt, dev, seed=8)
    before = clone_inputs(t)
    call_step(kind, t, HP[kind], skip=flag_of(dev, 1))
    for name, x in before.items():
        assert torch.equal(t[name], x), f"{kind}: skip=[1] changed {name}"
    a, b = clone_inputs(before), clone_inputs(before)
    call_step(kind, a, HP[kind], skip=flag_of(dev, 0))
    call_step(kind, b, HP[kind])
    for name in a:
        assert torch.equal(a[name], b[name]), f"{kind}: skip=[0] differs from skip=None in {name}"
    for name in ["w", "model"] + STATE[kind]:
        assert not torch.equal(a[name], before[name]), f"{kind}: the step left {name} unchanged"
