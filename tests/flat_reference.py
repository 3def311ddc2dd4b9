"""float64 references and derived error bounds for the flat-bucket kernels
(csrc/kernels/mv_kernels.hip) and their PyTorch fallbacks (mivod/ops/kernels.py).

A helper module, not a test file: tests/test_flat_reference_cpu.py runs the fallbacks through
it and tests/test_flat_kernels_gpu.py the HIP kernels, over the same sizes and flag sets.

The check
---------
Every reference takes exactly the stored inputs (the gradient cast up from its storage
dtype, the fp32 master and state) and the caller's hyperparameters as Python doubles, and
computes each output in float64 together with a per-element magnitude ``mag`` and a rounding
count ``c``.  An output passes when, element by element,

    |got - ref| <= c * 2^-24 * mag          (U = 2^-24: one fp32 rounding, relative)

``mag`` is the sum of the absolute values of the terms added or subtracted on the way to the
output, so a rounding anywhere on the way is at most U * mag.  Through a quotient or a square
root ``mag`` is carried by first-order sensitivity: an operand x with magnitude mag_x adds
|d out / d x| * mag_x.  For sqrt(x) we carry mag_x / sqrt(x), without the factor 1/2 of the
derivative: that keeps the carried magnitude >= sqrt(x) itself, so every later rounding of the
root counts once against it.  ``mag == 0`` (elements no segment covers) demands equality.

``c`` is the number of fp32 roundings on the longest path to the output, counted from the
kernel source.  Branches that are *added* share ``mag`` and so count as the longer of the two
plus the addition; factors that are *multiplied* add their counts.  A hyperparameter reaches
the kernel rounded to fp32, which is one rounding at each use (the reference keeps the
double); the complements 1-damp, 1-b1, 1-b2, 1-rho are taken on the host in double and
rounded once (taken in fp32, 1 - 0.999f alone is 216 U off: the first run of these tests
against the kernels found Adam's v that far out, and the launchers were changed).  Compiler FMA contraction only removes roundings.  sqrtf and '/' are correctly
rounded (the build passes no fast-math flag).

Counts (r = rounding of a hyperparameter, * + - / sqrt = one rounding each)
---------------------------------------------------------------------------
sgd_flat_kernel
  d   = g*gscale + wd*w            gscale r, * | wd r, *  -> 2, + -> 3
  mom = mu*mom + (1-damp)*d        d 3, (1-damp) r, * -> 5 (longer than mu r, * = 2), + -> 6
  d'  = d + mu*mom (nesterov)      mom 6, mu r, * -> 8, + -> 9
  w   = w - lr*d'                  lr r, * -> 11, - -> 12
  => C_SGD_MOM = 6, C_SGD_W = 12 (every flag combination is a sub-path of these)

adam_flat_kernel
  gr  = g*gscale (+ wd*w)          3 as above
  m   = b1*m + (1-b1)*gr           gr 3, (1-b1) r, * -> 5, + -> 6
  v   = b2*v + (1-b2)*gr*gr        (1-b2) r; gr twice = 6; two * -> 9, + -> 10
                                   mag_v uses mag_gr^2, not gr^2
  step = lr/bc1                    r, r, / = 3;   rbc2 = 1/sqrt(bc2): r, sqrt, / = 3
  den = sqrt(v)*rbc2 + eps         v 10, sqrt 11, rbc2 3 -> 14, * 15, (eps r shares), + 16
        (keras: (sqrt(v)+eps)*rbc2 the same 16)
  w   = w' - step*m/den            den path: 16, / 17, - 18
                                   m path:   6 + step 3 + * + / + - = 12
                                   w' = w*(1 - lr*wd): r, r, *, -, * = 5, then - 6
  mag_w = |w'| + step*mag_m/den + step*|m|/den^2 * mag_den, where
  mag_m = |b1*m_old| + (1-b1)*mag_gr  (the m update can cancel, so not |m_new|)
  => C_ADAM_M = 6, C_ADAM_V = 10, C_ADAM_W = 18

adadelta_flat_kernel
  gr  3;  sq = rho*sq + (1-rho)*gr*gr  -> 10 (as Adam's v)
  N = sqrt(acc+eps): r, +, sqrt = 3 (all terms positive)
  D = sqrt(sq+eps):  sq 10, + 11, sqrt 12, carried as mag_D = (mag_sq+eps)/D
  delta = N/D*gr     gr path: N 3 + gr 3 + / + * = 8;  D path: 12 + / + * = 14
  mag_delta = N/D*mag_gr + |delta|/D*mag_D
  acc = rho*acc + (1-rho)*delta*delta   (1-rho) r, delta twice 28, two * -> 31, + -> 32
  w   = w - lr*delta                    14, lr r, * -> 16, - -> 17
  => C_ADADELTA_SQ = 10, C_ADADELTA_ACC = 32, C_ADADELTA_W = 17

lars (seg_partial_kernel -> block_sum -> seg_reduce_kernel -> lars_flat_kernel)
  The squared norms are sums of positive terms.  Depth of the summation tree for one segment:
  a lane adds its 4096/256 = 16 products in turn (16), wave_sum adds 6 times, block_sum adds
  the 4 wave results (4), a seg_reduce lane adds its chunks' partials (1 for up to 64 chunks,
  which covers every segment used here, 4 chunks at the most) and the final wave_sum adds 6
  times: LARS_TREE_DEPTH = 33.
  |w|^2: product 1 + 33 = 34 = C_LARS_WN2;  |g*gscale|^2: (r, *) twice + * = 5, + 33 = 38 = C_LARS_GN2
  wn = sqrt: 34/2 + 1 = 18;  gn: 38/2 + 1 = 20
  trust = eta*wn/(gn + wd*wn + eps): numerator 18 + r + * = 20; denominator (positive terms)
          max(20, 18 + r + *) + 1, (eps r shares) + 1 = 22; / -> 43
  slr = lr*trust: r, * -> 45;  b = mu*mom + slr*d: d 3, * -> 49, + -> 50;  w -= b -> 51
  => adapted segments: C_LARS_MOM = 50, C_LARS_W = 51
  trust == 1 (flagged segment, zero norm): slr = lr (r) 1, d 3, * 5, + 6, w 7
  => C_LARS_MOM_PLAIN = 6, C_LARS_W_PLAIN = 7

adasum_merge_kernel (adasum_fcombine): f = cf*f + cr*r, c = 1 - dot/(2n) from fp32 dots
  q = dot/(2n): / (2n is exact); 1 - q: -.  |c_hat - c| <= U*|q| + U*|1-q| <= 2U*k, k = 1+|q|
  cf*f: 2 + * = 3 against k*|f|; + -> 4.  mag = kf*|f| + kr*|r|  =>  C_ADASUM = 4
adasum_combine stores the same sum in the wire dtype: + half an ulp of it.
seg_dot3: products 1 + the tree 33  =>  C_DOT3 = 34 against (sum|xy|, sum x^2, sum y^2).

pack / unpack / flat_cast are exact: (t.float() * scale).to(dst), bit for bit.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from mivod.ops import kernels as K

U = 2.0 ** -24

C_SGD_W, C_SGD_MOM = 12, 6
C_ADAM_W, C_ADAM_M, C_ADAM_V = 18, 6, 10
C_ADADELTA_W, C_ADADELTA_SQ, C_ADADELTA_ACC = 17, 10, 32
LARS_TREE_DEPTH = 33
C_LARS_WN2, C_LARS_GN2 = 1 + LARS_TREE_DEPTH, 5 + LARS_TREE_DEPTH
C_LARS_W, C_LARS_MOM = 51, 50
C_LARS_W_PLAIN, C_LARS_MOM_PLAIN = 7, 6
C_ADASUM = 4
C_DOT3 = 1 + LARS_TREE_DEPTH

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODELS = [None, torch.float32, torch.bfloat16, torch.float16]
# a lane covers 8 elements, a workgroup 4096 in two steps of 2048
SIZES = [1, 7, 8, 9, 2047, 2049, 4095, 4096, 4097, 3 * 4096 + 5]
N_GRID = 3 * 4096 + 5
# unit roundoff of a stored value (normal range): half an ulp <= 2^-p * |x| with p
# significand bits (24, 8, 11)
HALF_ULP = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

STATE = {"sgd": ["mom"], "adam": ["m", "v"], "adadelta": ["sq", "acc"], "lars": ["mom"]}

# the representative flag set of each step (the dtype grid, the size list, skip and dyn)
HP = {
    "sgd": dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=1e-4, gscale=0.125,
                nesterov=True, first=False),
    "adam": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, gscale=0.5, step=7,
                 adamw=True, keras_eps=False),
    "adadelta": dict(lr=1.0, rho=0.95, eps=1e-7, weight_decay=1e-4, gscale=0.25),
    "lars": dict(lr=0.5, momentum=0.9, weight_decay=1e-4, eta=0.001, gscale=0.25, eps=0.0,
                 first=False),
}


class Out(NamedTuple):
    ref: torch.Tensor          # float64
    mag: torch.Tensor          # float64, >= 0
    c: object                  # float, or a float64 tensor per element


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().double()


def ratio(got: torch.Tensor, out: Out) -> torch.Tensor:
    """|got - ref| / (U * mag) per element: compare with ``c``.  Where mag == 0 the
    result is 0 for an exact match and inf otherwise."""
    err = (f64(got) - out.ref).abs()
    r = err / (U * out.mag)
    r = torch.where(out.mag > 0, r, torch.where(err == 0, torch.zeros_like(err),
                                                torch.full_like(err, math.inf)))
    return r


def check(name: str, got: torch.Tensor, out: Out, scale: float = 1.0) -> float:
    """Assert the bound (times ``scale``, the step number of a trajectory); the worst
    |err| / (U * mag), to be printed next to ``c``."""
    assert torch.isfinite(f64(got)).all(), f"{name}: non-finite result"
    r = ratio(got, out)
    if r.numel() == 0:
        return 0.0
    ok = r <= torch.as_tensor(out.c, dtype=torch.float64) * scale
    worst = float(r.max())
    assert ok.all(), (f"{name}: {int((~ok).sum())} of {r.numel()} elements outside the bound, "
                      f"worst err/(U*mag) = {worst:.3g} at {int(r.argmax())}, c = "
                      f"{float(torch.as_tensor(out.c, dtype=torch.float64).max()) * scale:g}")
    return worst


# --------------------------------------------------------------------------- references
def sgd_ref(g, w, mom, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, gscale=1.0,
            nesterov=False, first=False, in_mag=None):
    g, w = f64(g), f64(w)
    aw = in_mag["w"] if in_mag else w.abs()
    d = g * gscale + weight_decay * w
    mag_d = (g * gscale).abs() + abs(weight_decay) * aw
    out = {}
    if mom is not None:
        mom = f64(mom)
        amom = in_mag["mom"] if in_mag else mom.abs()
        if first:
            b, mag_b = d, mag_d
        else:
            b = momentum * mom + (1.0 - dampening) * d
            mag_b = abs(momentum) * amom + abs(1.0 - dampening) * mag_d
        out["mom"] = Out(b, mag_b, C_SGD_MOM)
        if nesterov:
            d, mag_d = d + momentum * b, mag_d + abs(momentum) * mag_b
        else:
            d, mag_d = b, mag_b
    out["w"] = Out(w - lr * d, aw + abs(lr) * mag_d, C_SGD_W)
    return out


def adam_ref(g, w, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0,
             step=1, adamw=False, keras_eps=False, bc1=None, bc2=None, in_mag=None):
    g, w, m, v = f64(g), f64(w), f64(m), f64(v)
    aw, am, av = (in_mag[k] for k in "wmv") if in_mag else (w.abs(), m.abs(), v.abs())
    gr = g * gscale
    mag_gr = gr.abs()
    if not adamw:
        gr = gr + weight_decay * w
        mag_gr = mag_gr + abs(weight_decay) * aw
    m_new = beta1 * m + (1 - beta1) * gr
    mag_m = beta1 * am + (1 - beta1) * mag_gr
    v_new = beta2 * v + (1 - beta2) * gr * gr
    mag_v = beta2 * av + (1 - beta2) * mag_gr * mag_gr
    bc1 = 1 - beta1 ** step if bc1 is None else bc1
    bc2 = 1 - beta2 ** step if bc2 is None else bc2
    wp = w * (1 - lr * weight_decay) if adamw else w
    st, rb = lr / bc1, 1.0 / math.sqrt(bc2)
    sq = v_new.sqrt()
    mag_sq = torch.where(sq > 0, mag_v / sq, mag_v.sqrt())
    if keras_eps:
        den, mag_den = (sq + eps) * rb, (mag_sq + eps) * rb
    else:
        den, mag_den = sq * rb + eps, mag_sq * rb + eps
    w_new = wp - st * m_new / den
    mag_w = aw * (abs(1 - lr * weight_decay) if adamw else 1.0) + st * mag_m / den + st * m_new.abs() / (den * den) * mag_den
    return {"w": Out(w_new, mag_w, C_ADAM_W), "m": Out(m_new, mag_m, C_ADAM_M),
            "v": Out(v_new, mag_v, C_ADAM_V)}


def adadelta_ref(g, w, sq, acc, *, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0, gscale=1.0):
    g, w, sq, acc = f64(g), f64(w), f64(sq), f64(acc)
    gr = g * gscale + weight_decay * w
    mag_gr = (g * gscale).abs() + (weight_decay * w).abs()
    sq_new = rho * sq + (1 - rho) * gr * gr
    mag_sq = (rho * sq).abs() + (1 - rho) * mag_gr * mag_gr
    N, D = (acc + eps).sqrt(), (sq_new + eps).sqrt()
    mag_D = (mag_sq + eps) / D
    delta = N / D * gr
    mag_delta = N / D * mag_gr + delta.abs() / D * mag_D
    acc_new = rho * acc + (1 - rho) * delta * delta
    mag_acc = (rho * acc).abs() + (1 - rho) * mag_delta * mag_delta
    return {"w": Out(w - lr * delta, w.abs() + abs(lr) * mag_delta, C_ADADELTA_W),
            "sq": Out(sq_new, mag_sq, C_ADADELTA_SQ), "acc": Out(acc_new, mag_acc, C_ADADELTA_ACC)}


def lars_ref(g, w, mom, sizes, offsets, flags, *, lr, momentum=0.9, weight_decay=0.0, eta=0.001,
             gscale=1.0, eps=0.0, first=False, zero_norm_guard=True, in_mag=None):
    """Elements outside every segment keep their value with mag 0 (must be untouched).
    ``zero_norm_guard=False`` drops the "trust = 1 when a norm is zero" rule: the variant a
    sensitivity guard compares with.  Also returns the fp64 squared norms and trust ratios."""
    g, w, mom = f64(g), f64(w), f64(mom)
    aw, amom = (in_mag["w"], in_mag["mom"]) if in_mag else (w.abs(), mom.abs())
    w_new, m_new = w.clone(), mom.clone()
    mag_w, mag_m = torch.zeros_like(w), torch.zeros_like(w)
    c_w, c_m = torch.zeros_like(w), torch.zeros_like(w)
    norms, trusts = [], []
    covered = torch.zeros(w.numel(), dtype=torch.bool)
    for off, n, fl in zip(offsets, sizes, flags):
        sl = slice(off, off + n)
        covered[sl] = True
        gi, wi = g[sl] * gscale, w[sl]
        skip = bool(fl & 1)
        wd = 0.0 if skip else weight_decay
        wn2, gn2 = float((wi * wi).sum()), float((gi * gi).sum())
        wn, gn = math.sqrt(wn2), math.sqrt(gn2)
        norms.append([wn2, gn2])
        trust, plain = 1.0, True
        if not skip and ((wn > 0 and gn > 0) or
                         (not zero_norm_guard and gn + wd * wn + eps > 0)):
            trust, plain = eta * wn / (gn + wd * wn + eps), False
        trusts.append(trust)
        slr = lr * trust
        d, mag_d = gi + wd * wi, gi.abs() + abs(wd) * aw[sl]
        if first:
            b, mb = slr * d, slr * mag_d
        else:
            b, mb = momentum * mom[sl] + slr * d, abs(momentum) * amom[sl] + slr * mag_d
        m_new[sl], mag_m[sl], c_m[sl] = b, mb, (C_LARS_MOM_PLAIN if plain else C_LARS_MOM)
        w_new[sl], c_w[sl] = wi - b, (C_LARS_W_PLAIN if plain else C_LARS_W)
        mag_w[sl] = aw[sl] + mb
    nr = torch.tensor(norms, dtype=torch.float64).reshape(-1, 2)
    c_n = torch.tensor([C_LARS_WN2, C_LARS_GN2], dtype=torch.float64).expand_as(nr)
    return {"w": Out(w_new, mag_w, c_w), "mom": Out(m_new, mag_m, c_m),
            "norms": Out(nr, nr.clone(), c_n), "trust": trusts, "covered": covered}


def _coeffs(dots_row):
    dot, na, nb = (float(x) for x in dots_row)
    lim = float(torch.tensor(1e-8, dtype=torch.float32))
    qa = dot / (2 * na) if na >= lim else 0.0
    qb = dot / (2 * nb) if nb >= lim else 0.0
    return 1 - qa, 1 - qb, 1 + abs(qa), 1 + abs(qb)


def adasum_ref(f, r, sizes, offsets, dots, swap, c=C_ADASUM):
    """f <- cf*f + cr*r per segment from the stored fp32 ``dots`` rows (a.b, |a|^2, |b|^2);
    swap: f holds b.  ``adasum_combine`` is swap=False with f = a."""
    f, r, dots = f64(f), f64(r), f64(dots).reshape(-1, 3)
    ref, mag = f.clone(), torch.zeros_like(f)
    for i, (off, n) in enumerate(zip(offsets, sizes)):
        if n <= 0:
            continue
        ca, cb, ka, kb = _coeffs(dots[i])
        (cf, kf), (cr, kr) = ((cb, kb), (ca, ka)) if swap else ((ca, ka), (cb, kb))
        sl = slice(off, off + n)
        ref[sl] = cf * f[sl] + cr * r[sl]
        mag[sl] = kf * f[sl].abs() + kr * r[sl].abs()
    return Out(ref, mag, c)


def dot3_ref(a, b, sizes, offsets):
    a, b = f64(a), f64(b)
    ref, mag = [], []
    for off, n in zip(offsets, sizes):
        x, y = a[off:off + n], b[off:off + n]
        ref.append([float((x * y).sum()), float((x * x).sum()), float((y * y).sum())])
        mag.append([float((x * y).abs().sum()), ref[-1][1], ref[-1][2]])
    return Out(torch.tensor(ref, dtype=torch.float64).reshape(-1, 3),
               torch.tensor(mag, dtype=torch.float64).reshape(-1, 3), C_DOT3)


# --------------------------------------------------------------------------- inputs and runners
def layout(sizes, shift: int = 0):
    """64-element-aligned offsets of consecutive segments (as the arenas lay them out), each
    moved by ``shift`` elements; and the buffer length that holds them."""
    offs, o = [], 0
    for s in sizes:
        offs.append(o + shift)
        o += (s + 63) // 64 * 64
    return offs, o + shift + 64


def make_inputs(kind, n, gdt, mdt, dev, seed=0, zero_state=False):
    """Stored inputs of one step, generated on the CPU (the same bits on either device)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    t = {"g": torch.randn(n, generator=gen).to(gdt), "w": torch.randn(n, generator=gen)}
    for name in STATE[kind]:
        if zero_state:
            t[name] = torch.zeros(n)
        elif name in ("v", "sq", "acc"):
            t[name] = torch.rand(n, generator=gen) * (0.1 if name == "v" else 1.0)
        else:
            t[name] = torch.randn(n, generator=gen) * (0.1 if name == "m" else 1.0)
    t = {k: v.to(dev) for k, v in t.items()}
    # the model copy starts as garbage the step must overwrite
    t["model"] = None if mdt is None else torch.full((n,), MODEL_FILL, dtype=mdt, device=dev)
    return t


MODEL_FILL = 3.0


def clone_inputs(t):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()}


def call_step(kind, t, hp, **extra):
    """Run the step in place on ``t`` through mivod.ops.kernels (HIP kernel on a GPU, the
    fallback on the CPU).  LARS takes ``table`` and ``flags`` in ``extra``."""
    kw = dict(hp, **{k: v for k, v in extra.items() if k not in ("table", "flags")})
    if kind == "sgd":
        K.sgd_step(t["g"], t["w"], t.get("mom"), t["model"], **kw)
    elif kind == "adam":
        K.adam_step(t["g"], t["w"], t["m"], t["v"], t["model"], **kw)
    elif kind == "adadelta":
        K.adadelta_step(t["g"], t["w"], t["sq"], t["acc"], t["model"], **kw)
    else:
        K.lars_step(t["g"], t["w"], t["mom"], t["model"], extra["table"], extra["flags"], **kw)


def ref_step(kind, t, hp, lars=None, **extra):
    """The fp64 reference of ``call_step`` on the (not yet updated) inputs ``t``;
    ``lars`` = (sizes, offsets, flags as a list)."""
    if kind == "sgd":
        return sgd_ref(t["g"], t["w"], t.get("mom"), **hp, **extra)
    if kind == "adam":
        return adam_ref(t["g"], t["w"], t["m"], t["v"], **hp, **extra)
    if kind == "adadelta":
        return adadelta_ref(t["g"], t["w"], t["sq"], t["acc"], **hp)
    return lars_ref(t["g"], t["w"], t["mom"], *lars, **hp, **extra)


def check_outputs(label, kind, t, ref, scale=1.0):
    """w and every state tensor inside the bound; the model copy exactly RNE of the stored
    fp32 master.  Returns {output: worst err/(U*mag)}."""
    worst = {}
    for name in ["w"] + [s for s in STATE[kind] if t.get(s) is not None]:
        worst[name] = check(f"{label} {name}", t[name], ref[name], scale)
    if t["model"] is not None:
        model, want = t["model"].cpu(), t["w"].to(t["model"].dtype).cpu()
        cov = ref.get("covered", torch.ones(model.numel(), dtype=torch.bool))
        assert torch.equal(model[cov], want[cov]), \
            f"{label}: model copy is not the RNE rounding of the fp32 master"
        assert (model[~cov] == MODEL_FILL).all(), f"{label}: model written outside the segments"
    return worst


def run_step(kind, n, gdt, mdt, dev, hp=None, seed=0, drop_state=False, lars=None):
    """One step against fp64.  ``lars`` = (sizes, offsets, flags, zero_grad_segments) for the
    LARS layout (n is then the buffer length)."""
    hp = dict(HP[kind] if hp is None else hp)
    t = make_inputs(kind, n, gdt, mdt, dev, seed)
    if drop_state:
        t["mom"] = None
    extra, lr3 = {}, None
    if kind == "lars":
        sizes, offs, flags, zero = lars
        for i in zero:
            t["g"][offs[i]:offs[i] + sizes[i]] = 0
        extra = dict(table=K.make_chunk_table(sizes, dev, offs),
                     flags=torch.tensor(flags, dtype=torch.int32, device=dev))
        lr3 = (sizes, offs, flags)
    ref = ref_step(kind, t, hp, lars=lr3)
    call_step(kind, t, hp, **extra)
    return check_outputs(f"{kind} n={n} {gdt}/{mdt}", kind, t, ref), ref, t


def fmt(worst: dict) -> str:
    return ", ".join(f"{k} {v:.2f}" for k, v in worst.items())


def sensitivity(ref_with: dict, ref_without: dict, name: str = "w") -> float:
    """max |ref_with - ref_without| / bound_with of one output: how far, in bounds, the
    flag moves the result.  A flag case asserts this > 100, so it cannot pass vacuously."""
    a, b = ref_with[name], ref_without[name]
    bound = torch.as_tensor(a.c, dtype=torch.float64) * U * a.mag
    d = (a.ref - b.ref).abs()
    sel = bound > 0
    return float((d[sel] / bound[sel]).max()) if sel.any() else 0.0


# the LARS layout of the dtype grid: a flagged 1-element segment, short and multi-chunk
# adapted segments, a flagged one, a zero-length one and one whose gradient is all zero
LARS_SIZES = [1, 300, 4096, 9000, 64, 0, 77]
LARS_FLAGS = [1, 0, 0, 0, 1, 0, 0]
LARS_ZERO_GRAD = [6]


def lars_layout(sizes=None, shift=0):
    sizes = LARS_SIZES if sizes is None else sizes
    offs, total = layout(sizes, shift)
    return sizes, offs, total


# flag cases: (name, hp with the flag, hp without it); drop_state marks mom=None
_SGD_BASE = dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=1e-2, gscale=0.125,
                 nesterov=False, first=False)
SGD_FLAG_CASES = {
    "mom_none": (dict(_SGD_BASE), _SGD_BASE),
    "first": (dict(_SGD_BASE, first=True), _SGD_BASE),
    "dampening": (dict(_SGD_BASE, dampening=0.3), _SGD_BASE),
    "nesterov": (dict(_SGD_BASE, nesterov=True), _SGD_BASE),
    "wd0": (dict(_SGD_BASE, weight_decay=0.0), _SGD_BASE),
}
_ADAM_BASE = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-2, weight_decay=0.1, gscale=0.5)
_LARS_BASE = dict(lr=0.5, momentum=0.9, weight_decay=1e-2, eta=0.02, gscale=0.25, eps=0.0,
                  first=False)


def run_sgd_flag(case, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    hp, base = SGD_FLAG_CASES[case]
    drop = case == "mom_none"
    worst, ref, t = run_step("sgd", n, gdt, mdt, dev, hp=hp, seed=3, drop_state=drop)
    t0 = make_inputs("sgd", n, gdt, mdt, "cpu", 3)
    sens = sensitivity(ref, sgd_ref(t0["g"], t0["w"], t0["mom"], **base))
    assert sens > 100, f"sgd {case}: the flag moves w by only {sens:.3g} bounds"
    return worst, sens


def run_adam_flag(adamw, keras_eps, step, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    hp = dict(_ADAM_BASE, adamw=adamw, keras_eps=keras_eps, step=step)
    worst, ref, t = run_step("adam", n, gdt, mdt, dev, hp=hp, seed=4)
    t0 = make_inputs("adam", n, gdt, mdt, "cpu", 4)
    sens = {}
    for flag, other in (("adamw", dict(hp, adamw=not adamw)),
                        ("keras_eps", dict(hp, keras_eps=not keras_eps)),
                        ("step", dict(hp, step=8 - step))):
        sens[flag] = sensitivity(ref, adam_ref(t0["g"], t0["w"], t0["m"], t0["v"], **other))
        assert sens[flag] > 100, f"adam: {flag} moves w by only {sens[flag]:.3g} bounds"
    return worst, sens


# LARS flag cases: (hp, flags, zero-gradient segments, the variant without the flag)
def _lars_cases():
    sizes = LARS_SIZES
    flipped = [1 - f for f in LARS_FLAGS]
    return {
        "first": (dict(_LARS_BASE, first=True), LARS_FLAGS, [], dict(hp=_LARS_BASE)),
        "flags": (_LARS_BASE, LARS_FLAGS, [], dict(flags=flipped)),
        "zero_grad": (_LARS_BASE, LARS_FLAGS, LARS_ZERO_GRAD, dict(zero_norm_guard=False)),
        # a zero-length segment changes nothing by itself: the variant is the layout
        # without it, which must give the same result (no guard applies)
        "zero_len": (_LARS_BASE, LARS_FLAGS, [], None),
        "eps": (dict(_LARS_BASE, eps=1.0), LARS_FLAGS, [], dict(hp=_LARS_BASE)),
    }, sizes


def run_lars_flag(case, dev, gdt=torch.float16, mdt=torch.bfloat16):
    cases, sizes = _lars_cases()
    hp, flags, zero, variant = cases[case]
    sizes, offs, total = lars_layout(sizes)
    worst, ref, t = run_step("lars", total, gdt, mdt, dev, hp=hp, seed=5,
                             lars=(sizes, offs, flags, zero))
    assert ref["trust"][5] == 1.0                       # the zero-length segment
    if zero:
        assert all(ref["trust"][i] == 1.0 for i in zero)
    if variant is None:
        return worst, None
    t0 = make_inputs("lars", total, gdt, mdt, "cpu", 5)
    for i in zero:
        t0["g"][offs[i]:offs[i] + sizes[i]] = 0
    other = lars_ref(t0["g"], t0["w"], t0["mom"], sizes, offs, variant.get("flags", flags),
                     **variant.get("hp", hp),
                     zero_norm_guard=variant.get("zero_norm_guard", True))
    sens = sensitivity(ref, other)
    assert sens > 100, f"lars {case}: the flag moves w by only {sens:.3g} bounds"
    return worst, sens


def run_trajectory(kind, dev, gdt, mdt, n=4097, steps=5):
    """``steps`` steps from a zero state with fresh gradients, against the fp64 trajectory
    that starts from the same stored master; the bound is the step number times c * U * mag,
    with mag carried along the trajectory."""
    hp0 = {"sgd": dict(lr=0.1, momentum=0.9, weight_decay=1e-4, gscale=0.125),
           "adam": dict(lr=1e-3, weight_decay=1e-2, gscale=0.5, adamw=True),
           "lars": dict(_LARS_BASE)}[kind]
    lars, extra = None, {}
    if kind == "lars":
        sizes, offs, n = lars_layout()
        lars = (sizes, offs, LARS_FLAGS)
        extra = dict(table=K.make_chunk_table(sizes, dev, offs),
                     flags=torch.tensor(LARS_FLAGS, dtype=torch.int32, device=dev))
    t = make_inputs(kind, n, gdt, mdt, dev, seed=6, zero_state=True)
    r = {k: f64(v) for k, v in t.items() if torch.is_tensor(v)}       # the fp64 trajectory
    gen = torch.Generator().manual_seed(77)
    # an input that carries the error of earlier steps enters with the magnitude it was
    # computed with, not with its absolute value (a momentum that cancelled is small, the
    # error it carries is not)
    mags = {name: r[name].abs() for name in ["w"] + STATE[kind]}
    worst = {}
    for s in range(1, steps + 1):
        g = torch.randn(n, generator=gen).to(gdt)
        t["g"], r["g"] = g.to(dev), g
        hp = dict(hp0)
        if kind == "adam":
            hp["step"] = s
        else:
            hp["first"] = s == 1
        ref = ref_step(kind, r, hp, lars=lars, in_mag=mags)
        call_step(kind, t, hp, **extra)
        for k, v in check_outputs(f"{kind} step {s}", kind, t, ref, scale=s).items():
            worst[k] = max(worst.get(k, 0.0), v / s)
        for name in ["w"] + STATE[kind]:
            r[name], mags[name] = ref[name].ref, ref[name].mag
    return worst


# ---- Adasum: the layout of tests/test_kernels_gpu.py::test_adasum_merge_vs_fp64 (its
# _ADA_SIZES), segment 5 with zero norms (ca = cb = 1) ----
ADA_SIZES = [1, 63, 4101, 0, 2 * 4096 + 5, 7, 64]


# contiguous segments at offsets no vector access may use (E: the guarded scalar paths);
# the 4101-element one has a second chunk of 5 elements at 4396
UNAL_SIZES = [3, 297, 4101, 70]
UNAL_OFFS = [0, 3, 300, 4401]
UNAL_TOTAL = 4471


def ada_inputs(wire, dev, sizes=None, offs=None, seed=21, fdt=torch.float32):
    """f (fp32, or ``fdt``), r (wire dtype), the fp32 Gram rows (segment 5, if any, with zero
    norms), the offsets and the chunk table"""
    sizes = ADA_SIZES if sizes is None else sizes
    if offs is None:
        offs, total = layout(sizes)
    else:
        total = offs[-1] + sizes[-1]
    gen = torch.Generator().manual_seed(seed)
    f = torch.randn(total, generator=gen).to(fdt)
    r = torch.randn(total, generator=gen).to(wire)
    dots = torch.randn(len(sizes), 3, generator=gen) * 3.0
    dots[:, 1:] = dots[:, 1:].abs() + 0.5
    if len(sizes) > 5:
        dots[5, 1:] = 0.0
    return f.to(dev), r.to(dev), dots.to(dev), offs, K.make_chunk_table(sizes, dev, offs)


def check_stored(name, got, out: Out, dtype) -> float:
    """``check`` for a result stored in ``dtype``: the bound plus half an ulp of the stored
    value (nothing more for fp32, whose last rounding ``c`` already counts)."""
    if dtype == torch.float32:
        return check(name, got, out)
    bound = out.c * U * out.mag
    err = (f64(got) - out.ref).abs()
    tol = bound + HALF_ULP[dtype] * (out.ref.abs() + bound)
    assert (err <= tol).all(), f"{name}: worst err/tol {float((err / tol)[tol > 0].max()):.3g}"
    assert (err[tol == 0] == 0).all(), f"{name}: wrote outside the segments"
    return float((err / tol)[tol > 0].max())


def run_fcombine(dev, wire, swap, sizes=None, offs=None):
    """adasum_fcombine against fp64; elements outside the segments must not change.
    Returns (worst ratio, the merged f, the inputs)."""
    f, r, dots, offs, table = ada_inputs(wire, dev, sizes, offs)
    ref = adasum_ref(f, r, table.seg_sizes, offs, dots, swap)
    f0 = f.clone()
    K.adasum_fcombine(f, r, table, dots, swap)
    return check(f"adasum_fcombine {wire} swap={swap}", f, ref), f, (f0, r, dots, table)


# ---- exact casts and the non-finite flag ----
SCALE = 0.37                      # not a power of two: the product rounds


def cast_ref(src, scale, ddt):
    return (src.float() * scale).to(ddt)


def bad_positions(n=N_GRID):
    """index 0, the last element of a chunk, the first element of the scalar tail, the last"""
    return [0, K.CHUNK - 1, n // K.CHUNK * K.CHUNK if n % K.CHUNK < 8 else n // 8 * 8, n - 1]


BAD_VALUES = [float("nan"), float("inf"), float("-inf")]
FINITE_MAX = {dt: torch.finfo(dt).max for dt in DTYPES}


def flag_of(dev, preset=0):
    return torch.full((1,), preset, dtype=torch.int32, device=dev)


def lars_case(n_seg0=None):
    """(buffer length, (sizes, offsets, flags, zero-gradient segments)): the grid layout, or
    for the size list an adapted segment of ``n_seg0`` elements and a flagged one of 70"""
    sizes = LARS_SIZES if n_seg0 is None else [n_seg0, 70]
    flags = LARS_FLAGS if n_seg0 is None else [0, 1]
    sizes, offs, total = lars_layout(sizes)
    return total, (sizes, offs, flags, LARS_ZERO_GRAD if n_seg0 is None else [])


def lars_extra(lars, dev):
    return dict(table=K.make_chunk_table(lars[0], dev, lars[1]),
                flags=torch.tensor(lars[2], dtype=torch.int32, device=dev))


def run_skip(kind, dev, gdt=torch.float16, mdt=torch.bfloat16):
    """skip=[1] leaves w, the state and the model copy bit-identical; skip=[0] equals
    skip=None bit for bit (and does update)."""
    n, lars = (4097, None) if kind != "lars" else lars_case()
    t = make_inputs(kind, n, gdt, mdt, dev, seed=8)
    extra = lars_extra(lars, dev) if lars else {}
    before = clone_inputs(t)
    call_step(kind, t, HP[kind], skip=flag_of(dev, 1), **extra)
    for name, v in before.items():
        assert torch.equal(t[name], v), f"{kind}: skip=[1] changed {name}"
    a, b = clone_inputs(before), clone_inputs(before)
    call_step(kind, a, HP[kind], skip=flag_of(dev, 0), **extra)
    call_step(kind, b, HP[kind], **extra)
    for name in a:
        assert torch.equal(a[name], b[name]), f"{kind}: skip=[0] differs from skip=None in {name}"
    assert not torch.equal(a["w"], before["w"]) and not torch.equal(a["model"], before["model"])


def run_nonfinite(dev, dt, base_off=0):
    """nonfinite_scan and the nonfinite flag of pack / flat_cast: finite extremes leave the
    flag, a preset 1 stays, one bad element at any of ``bad_positions`` sets it.
    ``base_off`` = 1 scans a view that is not 16-byte aligned."""
    n = N_GRID
    clean = torch.ones(n + base_off, dtype=dt, device=dev)[base_off:]
    clean[5], clean[6] = FINITE_MAX[dt], -FINITE_MAX[dt]
    flat = torch.zeros(n, dtype=dt, device=dev)
    fns = {"nonfinite_scan": lambda x, f: K.nonfinite_scan(x, f),
           "pack": lambda x, f: K.pack([x], flat, [0], nonfinite=f),
           "flat_cast": lambda x, f: K.flat_cast(x, flat, 1.0, f)}
    for name, fn in fns.items():
        flag = flag_of(dev)
        fn(clean, flag)
        assert flag.item() == 0, f"{name}: a finite extreme set the flag"
        flag = flag_of(dev, 1)
        fn(clean, flag)
        assert flag.item() == 1, f"{name}: the flag is OR-ed, a preset 1 stays"
        x = torch.empty(n + base_off, dtype=dt, device=dev)[base_off:]
        for pos in bad_positions(n):
            for bad in BAD_VALUES:
                x.copy_(clean)
                x[pos] = bad
                flag = flag_of(dev)
                fn(x, flag)
                assert flag.item() == 1, f"{name}: missed {bad} at {pos}"


def run_cast_overflow(dev, ddt, val, pos=N_GRID - 1):
    """a finite fp32 source that overflows the destination dtype sets the flag, as
    torch.isfinite of the stored values says"""
    src = torch.ones(N_GRID, device=dev)
    src[pos] = val
    assert not bool(torch.isfinite(cast_ref(src, 1.0, ddt)).all())
    flat = torch.zeros(N_GRID, dtype=ddt, device=dev)
    for fn in (lambda f: K.pack([src], flat, [0], nonfinite=f),
               lambda f: K.flat_cast(src, flat, 1.0, f)):
        flag = flag_of(dev)
        fn(flag)
        assert flag.item() == 1
        assert torch.equal(torch.isfinite(flat.float()), torch.isfinite(cast_ref(src, 1.0, ddt).float()))


CAST_SIZES = [1, 7, 9, 2049, 4097]


def run_cast_exact(dev, sd, dd, aligned=False):
    """pack / unpack / flat_cast between views that are not 16-byte aligned (``base[1:1+n]``
    tensors, flat offsets that are no multiple of 8), with a scale, bit-exact; nothing
    outside the destination ranges is written.  In place (dst is src) when sd == dd.
    ``aligned``: the same from 16-byte-aligned views and offsets (the vector body; the
    scale makes the fp32 product a tie of a 16-bit destination every few hundred elements,
    where rounding the exact product once would differ)."""
    gen = torch.Generator().manual_seed(9)
    b0 = 0 if aligned else 1
    ts = [torch.randn(n + 8, generator=gen).to(sd).to(dev)[b0:b0 + n] for n in CAST_SIZES]
    offs, o = [], 0 if aligned else 3
    for n in CAST_SIZES:
        offs.append(o)
        o += (n + 63) // 64 * 64 if aligned else n + 5
    assert all((x % 8 == 0) == aligned for x in offs)
    flat = torch.full((o,), 9.0, dtype=dd, device=dev)
    K.pack(ts, flat, offs, scale=SCALE)
    touched = torch.zeros(o, dtype=torch.bool)
    for t, off in zip(ts, offs):
        assert torch.equal(flat[off:off + t.numel()], cast_ref(t, SCALE, dd))
        touched[off:off + t.numel()] = True
    assert (flat.cpu()[~touched] == 9.0).all(), "pack wrote outside its ranges"
    bases = [torch.full((n + 8,), 9.0, dtype=sd, device=dev) for n in CAST_SIZES]
    outs = [b[b0:b0 + n] for b, n in zip(bases, CAST_SIZES)]
    K.unpack(outs, flat, offs, scale=2.0)
    for b, out, off in zip(bases, outs, offs):
        assert torch.equal(out, cast_ref(flat[off:off + out.numel()], 2.0, sd))
        assert (b[:b0] == 9.0).all() and (b[b0 + out.numel():] == 9.0).all(), "unpack wrote outside"
    n = N_GRID
    src = torch.randn(n + 8, generator=gen).to(sd).to(dev)[b0:b0 + n]
    other = torch.zeros(n + 8, dtype=dd, device=dev)
    d0 = 0 if aligned else 3
    K.flat_cast(src, other[d0:d0 + n], SCALE)
    assert torch.equal(other[d0:d0 + n], cast_ref(src, SCALE, dd))
    assert (other[:d0] == 0).all() and (other[d0 + n:] == 0).all(), "flat_cast wrote outside"
    if sd == dd:
        want = cast_ref(src, SCALE, dd)
        K.flat_cast(src, src, SCALE)
        assert torch.equal(src, want), "in-place flat_cast"
