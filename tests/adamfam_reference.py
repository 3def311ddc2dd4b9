"""float64 references and derived error bounds for the Adam-family steps of
csrc/kernels/mv_adamfam.hip (adam_amsgrad_flat_kernel, adamax_flat_kernel, nadam_flat_kernel)
and their PyTorch fallbacks (mivod/ops/kernels.py: adam_amsgrad_step, adamax_step, nadam_step).

A helper module, not a test file: tests/test_adamfam_cpu.py runs the fallbacks through it and
tests/test_adamfam_gpu.py the HIP kernels.  The method, ``U``, ``check`` and the layouts are
those of tests/flat_reference.py (read its header first): every output must satisfy, per
element,

    |got - ref| <= c * 2^-24 * mag

with ``mag`` the sum of the absolute values of the terms on the way to the output, carried
through a quotient or a square root by first-order sensitivity, and ``c`` the fp32 roundings on
the longest path, counted from the kernel source.  The kernels spell the one fused product of
every a*b + c*d out (__builtin_fmaf); the counts below take both products and the sum as
rounded, which the fallbacks do, so a fused product only removes a rounding.

``max`` is exact and 1-Lipschitz in each argument: |max(a', b') - max(a, b)| <=
max(|a' - a|, |b' - b|).  The bound of a maximum is therefore the larger of the bounds of its
two arguments, at every element, whichever branch either side takes: no element is excluded
near a tie, and every element of every output is checked.

Counts (r = rounding of a hyperparameter, * + - / sqrt = one rounding each)
---------------------------------------------------------------------------
shared by the three kernels
  gr  = g*gscale (+ wd*w)          gscale r, * | wd r, * -> 2, + -> 3
  m   = b1*m + omb1*gr             gr 3, omb1 = 1-b1 rounded once on the host: r, * -> 5
                                   (longer than b1 r, * = 2), + -> 6
                                   mag_m = b1*|m| + (1-b1)*mag_gr
  v   = b2*v + omb2*gr*gr          omb2 r; gr twice = 6; two * -> 9, + -> 10
                                   mag_v = b2*|v| + (1-b2)*mag_gr^2
  w'  = w*decay (decoupled)        decay = 1 - lr*wd: r, r, *, - = 4, * -> 5

adam_amsgrad_flat_kernel
  vmax = max(vmax, v)              vmax comes in exact (0), v 10: the larger, 10, against mag_v
  step = lr/bc1                    r, r, / = 3;   rbc2 = 1/sqrt(bc2): r, sqrt, / = 3
  den = sqrt(vmax)*rbc2 + eps      vmax 10, sqrt 11, rbc2 3 -> 14, * 15, (eps r shares), + 16
        (keras: (sqrt(vmax)+eps)*rbc2, the same 16)
        mag_root = mag_v/sqrt(vmax); mag_den = mag_root*rb + eps  (keras (mag_root + eps)*rb)
  w   = w' - step*m/den            den path: 16, / 17, - 18
                                   m path: 6 + step 3 + * + / + - = 12;  w' path: 5, - 6
        mag_w = |w'| + step*mag_m/den + step*|m|/den^2 * mag_den
  => C_AMS_M = 6, C_AMS_V = 10, C_AMS_VMAX = 10, C_AMS_W = 18

adamax_flat_kernel
  u   = max(b2*u, |gr| + eps)      first argument: b2 r, * = 2 against b2*|u|;  second: gr 3,
                                   (eps r shares: positive terms), + -> 4 against mag_gr + eps
                                   (keras: |gr| alone, 3 against mag_gr; the + 0.f is exact).
                                   The larger of the two bounds, written as c = 4 (keras 3)
                                   against mag_u = max(2/c * b2*|u|, mag_gr + eps_in)
  d   = u + eps (keras)            u 4, + -> 5 (torch's placement: d = u, 4);
                                   mag_d = max(b2*|u|, mag_gr + eps_in) + eps_out
  step = lr/bc1                    3
  w   = w - step*m/d               m path: 6 + 3 + * + / + - = 12;  d path: 5, / 6, - 7
        mag_w = |w| + step*mag_m/d + step*|m|/d^2 * mag_d
  => C_ADAMAX_M = 6, C_ADAMAX_U = 4 (keras 3), C_ADAMAX_W = 12
  Where d == 0 exactly the kernel leaves w as it is: the reference does the same, with
  mag_w = |w| (the element is then checked for equality up to 12 U |w|, that is, bit for bit).

nadam_flat_kernel
  sg = lr*cg, sm = lr*cm           r, r, * = 3 each (cg, cm, bc2 arrive rounded once from double)
  den = sqrt(v)*rbc2 + eps         v 10, sqrt 11, rbc2 3 -> 14, * 15, + 16
  num = sg*gr + sm*m               sg*gr: 3 + 3 + * = 7;  sm*m: 3 + 6 + * = 10;  + -> 11
                                   mag_num = sg*mag_gr + sm*mag_m
  w   = w' - num/den               den path: 16, / 17, - 18;  num path: 11, / 12, - 13
        mag_w = |w'| + mag_num/den + |num|/den^2 * mag_den
  => C_NADAM_M = 6, C_NADAM_V = 10, C_NADAM_W = 18

The model copy is the RNE rounding of the stored fp32 master, bit for bit.  The fallbacks do
the same arithmetic in fp32 torch ops, one rounding per op, with fewer roundings of the scalar
factors (taken in double, rounded once), so the same counts hold for them.

Inputs (``adamfam_inputs``): v in [0.005, 0.1]; vmax = 1.5 v or 0.5 v, so that each branch of
amsgrad's max is taken about half the time; u = 0.02 + 0.4 |normal|, which b2*u and |gr| + eps
split likewise.  The references assert that each branch is taken on at least a quarter of the
elements (when there are at least 64) and that v, vmax and u stay above 1e-3 of their
magnitude bound, so the sensitivity of the root and of the quotient stays finite.

Worst err / (2^-24 * mag) measured over all of tests/test_adamfam_gpu.py on an MI355X (every
test prints its own next to c): amsgrad w 2.16, m 2.03, v 3.13, vmax 3.13 (c 18, 6, 10, 10);
Adamax w 1.76, m 2.34, u 2.41 (c 12, 6, 4); NAdam w 1.93, m 2.60, v 1.52 (c 18, 6, 10).  The
fallbacks, over all of tests/test_adamfam_cpu.py: amsgrad w 2.16, m 2.34, v 3.58, vmax 3.58;
Adamax w 1.71, m 2.34, u 2.41; NAdam w 1.98, m 2.21, v 3.25.
"""
from __future__ import annotations

import math

import torch

from flat_reference import (DTYPES, HALF_ULP, MODELS, N_GRID, SIZES, STATE, U,  # noqa: F401
                            UNAL_OFFS, UNAL_SIZES, UNAL_TOTAL, Out, adam_ref, check,
                            check_outputs, clone_inputs, f64, flag_of, fmt, make_inputs,
                            sensitivity)
from mivod.ops import kernels as K

C_AMS_W, C_AMS_M, C_AMS_V, C_AMS_VMAX = 18, 6, 10, 10
C_ADAMAX_W, C_ADAMAX_M, C_ADAMAX_U, C_ADAMAX_U_KERAS = 12, 6, 4, 3
C_NADAM_W, C_NADAM_M, C_NADAM_V = 18, 6, 10
C_OF = {"amsgrad": dict(w=C_AMS_W, m=C_AMS_M, v=C_AMS_V, vmax=C_AMS_VMAX),
        "adamax": dict(w=C_ADAMAX_W, m=C_ADAMAX_M, u=C_ADAMAX_U),
        "nadam": dict(w=C_NADAM_W, m=C_NADAM_M, v=C_NADAM_V)}
KINDS = ["amsgrad", "adamax", "nadam"]

# the state names make_inputs and check_outputs go by (flat_reference.STATE is their table)
STATE.setdefault("amsgrad", ["m", "v", "vmax"])
STATE.setdefault("adamax", ["m", "u"])
STATE.setdefault("nadam", ["m", "v"])

FLOOR = 1e-3          # v, vmax and u stay above this share of their magnitude bound
MIN_BRANCH = 0.25     # each branch of a max is taken on at least this share of the elements

HP = {
    "amsgrad": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, gscale=0.5,
                    step=7, adamw=True, keras_eps=False),
    "adamax": dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, gscale=0.25,
                   step=7, keras_eps=False),
    "nadam": dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, gscale=0.5,
                  step=7, momentum_decay=4e-3, decoupled=False),
}
# the flag cases: a rate, a decay and an eps large enough that each moves w far past a bound
AMS_BASE = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-2, weight_decay=0.1, gscale=0.5)
ADAMAX_BASE = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-2, weight_decay=0.1, gscale=0.5, step=3)
NADAM_BASE = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-2, weight_decay=0.1, gscale=0.5, step=7,
                  momentum_decay=0.5)


def _branches(name, first, n):
    """each branch of a max is taken often enough for the case to exercise both"""
    if n >= 64:
        share = float(first.double().mean())
        assert MIN_BRANCH <= share <= 1 - MIN_BRANCH, \
            f"{name}: the first argument of the max wins on {share:.3f} of the elements"


def _floor(name, x, mag):
    assert (x >= FLOOR * mag).all(), \
        f"{name} down to {float((x / mag).min()):.3g} of its magnitude: inputs outside the design"


def _moments(g, w, m, v, beta1, beta2, weight_decay, gscale, coupled):
    gr = g * gscale
    mag_gr = gr.abs()
    if coupled:
        gr = gr + weight_decay * w
        mag_gr = mag_gr + abs(weight_decay) * w.abs()
    m_new = beta1 * m + (1 - beta1) * gr
    mag_m = beta1 * m.abs() + (1 - beta1) * mag_gr
    if v is None:
        return gr, mag_gr, m_new, mag_m, None, None
    v_new = beta2 * v + (1 - beta2) * gr * gr
    mag_v = beta2 * v.abs() + (1 - beta2) * mag_gr * mag_gr
    return gr, mag_gr, m_new, mag_m, v_new, mag_v


# --------------------------------------------------------------------------- references
def adam_amsgrad_ref(g, w, m, v, vmax, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                     gscale=1.0, step=1, adamw=False, keras_eps=False, bc1=None, bc2=None,
                     design=True):
    """``design``: assert the branch shares and the floor, which the generated inputs are laid
    out for; the trajectories from a zero state (vmax == v, and a v that a cancelling
    weight decay can leave far below its magnitude) switch both off."""
    g, w, m, v, vmax = f64(g), f64(w), f64(m), f64(v), f64(vmax)
    gr, mag_gr, m_new, mag_m, v_new, mag_v = _moments(g, w, m, v, beta1, beta2, weight_decay,
                                                      gscale, not adamw)
    x_new = torch.maximum(vmax, v_new)
    if design:
        _branches("amsgrad vmax", vmax > v_new, x_new.numel())
        _floor("v", v_new, mag_v)
        _floor("vmax", x_new, mag_v)
    bc1 = 1 - beta1 ** step if bc1 is None else bc1
    bc2 = 1 - beta2 ** step if bc2 is None else bc2
    wp = w * (1 - lr * weight_decay) if adamw else w
    st, rb = lr / bc1, 1.0 / math.sqrt(bc2)
    root = x_new.sqrt()
    mag_root = torch.where(root > 0, mag_v / root, mag_v.sqrt())
    if keras_eps:
        den, mag_den = (root + eps) * rb, (mag_root + eps) * rb
    else:
        den, mag_den = root * rb + eps, mag_root * rb + eps
    w_new = wp - st * m_new / den
    mag_w = wp.abs() + st * mag_m / den + st * m_new.abs() / (den * den) * mag_den
    return {"w": Out(w_new, mag_w, C_AMS_W), "m": Out(m_new, mag_m, C_AMS_M),
            "v": Out(v_new, mag_v, C_AMS_V), "vmax": Out(x_new, mag_v, C_AMS_VMAX)}


def adamax_ref(g, w, m, u, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0,
               step=1, keras_eps=False, bc1=None, design=True):
    """``design=False`` drops the branch and floor assertions (the zero-divisor case and the
    trajectories from a zero state)."""
    g, w, m, u = f64(g), f64(w), f64(m), f64(u)
    gr, mag_gr, m_new, mag_m, _, _ = _moments(g, w, m, None, beta1, beta2, weight_decay, gscale,
                                              True)
    eps_in, eps_out = (0.0, eps) if keras_eps else (eps, 0.0)
    first, second = beta2 * u, gr.abs() + eps_in
    u_new = torch.maximum(first, second)
    c_u = C_ADAMAX_U_KERAS if keras_eps else C_ADAMAX_U
    mag_u = torch.maximum(2.0 / c_u * first.abs(), mag_gr + eps_in)
    mag_d = torch.maximum(first.abs(), mag_gr + eps_in) + eps_out
    if design:
        _branches("adamax u", first > second, u_new.numel())
        _floor("u", u_new, mag_d)
    bc1 = 1 - beta1 ** step if bc1 is None else bc1
    st = lr / bc1
    d = u_new + eps_out
    live = d != 0
    ds = torch.where(live, d, torch.ones_like(d))
    w_new = torch.where(live, w - st * m_new / ds, w)
    mag_w = w.abs() + torch.where(live, st * mag_m / ds + st * m_new.abs() / (ds * ds) * mag_d,
                                  torch.zeros_like(d))
    return {"w": Out(w_new, mag_w, C_ADAMAX_W), "m": Out(m_new, mag_m, C_ADAMAX_M),
            "u": Out(u_new, mag_u, c_u)}


def nadam_schedule(step, beta1, momentum_decay):
    """(mu_step, mu_{step+1}, P_step = mu_1 ... mu_step) of torch.optim.NAdam, in double"""
    def mu(t):
        return beta1 * (1.0 - 0.5 * 0.96 ** (t * momentum_decay))
    prod = 1.0
    for t in range(1, step + 1):
        prod *= mu(t)
    return mu(step), mu(step + 1), prod


def nadam_ref(g, w, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, gscale=1.0,
              step=1, momentum_decay=4e-3, decoupled=False, cg=None, cm=None, bc2=None,
              design=True):
    """``cg``, ``cm``, ``bc2`` given: the values of a dyn block, instead of those of ``step``.
    ``design=False`` drops the floor assertion (trajectories from a zero state)."""
    g, w, m, v = f64(g), f64(w), f64(m), f64(v)
    gr, mag_gr, m_new, mag_m, v_new, mag_v = _moments(g, w, m, v, beta1, beta2, weight_decay,
                                                      gscale, not decoupled)
    if design:
        _floor("v", v_new, mag_v)
    mu, mu_next, prod = nadam_schedule(step, beta1, momentum_decay)
    cg = (1 - mu) / (1 - prod) if cg is None else cg
    cm = mu_next / (1 - prod * mu_next) if cm is None else cm
    bc2 = 1 - beta2 ** step if bc2 is None else bc2
    wp = w * (1 - lr * weight_decay) if decoupled else w
    root = v_new.sqrt()
    rb = 1.0 / math.sqrt(bc2)
    den = root * rb + eps
    mag_den = torch.where(root > 0, mag_v / root, mag_v.sqrt()) * rb + eps
    num = lr * cg * gr + lr * cm * m_new
    mag_num = abs(lr * cg) * mag_gr + abs(lr * cm) * mag_m
    w_new = wp - num / den
    mag_w = wp.abs() + mag_num / den + num.abs() / (den * den) * mag_den
    return {"w": Out(w_new, mag_w, C_NADAM_W), "m": Out(m_new, mag_m, C_NADAM_M),
            "v": Out(v_new, mag_v, C_NADAM_V), "mu_product": prod}


# --------------------------------------------------------------------------- inputs and runners
def adamfam_inputs(kind, n, gdt, mdt, dev, seed=0):
    """Stored inputs (flat_reference.make_inputs), generated on the CPU: the same bits on
    either device; the module docstring says how v, vmax and u are laid out."""
    t = make_inputs(kind, n, gdt, mdt, "cpu", seed)
    if "v" in t:
        t["v"] = 0.005 + 0.95 * t["v"]
    if kind == "amsgrad":
        t["vmax"] = torch.where(t["vmax"] > 0, 1.5 * t["v"], 0.5 * t["v"])
    if kind == "adamax":
        t["u"] = 0.02 + 0.4 * t["u"].abs()
    return {k: (x.to(dev) if torch.is_tensor(x) else x) for k, x in t.items()}


def nadam_kernel_args(hp):
    """hp of ``nadam_ref`` -> the keyword arguments of K.nadam_step (cg, cm, bc2 through
    mivod.ops.kernels' own schedule functions, not the reference's)"""
    kw = {k: hp[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "gscale") if k in hp}
    b1, md, step = hp.get("beta1", 0.9), hp.get("momentum_decay", 4e-3), hp.get("step", 1)
    prod = 1.0
    for t in range(1, step + 1):
        prod *= K.nadam_mu(t, b1, md)
    cg, cm = K.nadam_coefficients(K.nadam_mu(step, b1, md), K.nadam_mu(step + 1, b1, md), prod)
    return dict(kw, cg=cg, cm=cm, bc2=1 - hp.get("beta2", 0.999) ** step,
                adamw=hp.get("decoupled", False))


def call_step(kind, t, hp, **extra):
    """The step in place on ``t`` through mivod.ops.kernels (the HIP kernel on a GPU, the
    fallback on the CPU)."""
    if kind == "amsgrad":
        K.adam_amsgrad_step(t["g"], t["w"], t["m"], t["v"], t["vmax"], t["model"], **hp, **extra)
    elif kind == "adamax":
        K.adamax_step(t["g"], t["w"], t["m"], t["u"], t["model"], **hp, **extra)
    else:
        K.nadam_step(t["g"], t["w"], t["m"], t["v"], t["model"], **nadam_kernel_args(hp), **extra)


def ref_step(kind, t, hp, **extra):
    if kind == "amsgrad":
        return adam_amsgrad_ref(t["g"], t["w"], t["m"], t["v"], t["vmax"], **hp, **extra)
    if kind == "adamax":
        return adamax_ref(t["g"], t["w"], t["m"], t["u"], **hp, **extra)
    return nadam_ref(t["g"], t["w"], t["m"], t["v"], **hp, **extra)


def run_step(kind, n, gdt, mdt, dev, hp=None, seed=0):
    """One step against fp64: ({output: worst err/(U*mag)}, the reference, the tensors)."""
    hp = dict(HP[kind] if hp is None else hp)
    t = adamfam_inputs(kind, n, gdt, mdt, dev, seed)
    ref = ref_step(kind, t, hp)
    call_step(kind, t, hp)
    return check_outputs(f"{kind} n={n} {gdt}/{mdt}", kind, t, ref), ref, t


def view_inputs(t, off, n):
    return {k: (x[off:off + n] if torch.is_tensor(x) else x) for k, x in t.items()}


def run_unaligned(kind, gdt, mdt, dev, seed=13):
    """One launch per UNAL_* segment on views ``buf[off : off+n]`` that no 16-byte access may
    use (the scalar path of every element); nothing outside the segments may change."""
    hp = dict(HP[kind])
    t = adamfam_inputs(kind, UNAL_TOTAL, gdt, mdt, dev, seed)
    ref = ref_step(kind, t, hp)
    for off, n in zip(UNAL_OFFS, UNAL_SIZES):
        call_step(kind, view_inputs(t, off, n), hp)
    assert UNAL_OFFS[-1] + UNAL_SIZES[-1] == UNAL_TOTAL    # the segments tile the buffer
    return check_outputs(f"{kind} unaligned {gdt}/{mdt}", kind, t, ref)


def _sens(kind, hp, seed, gdt, mdt, n, ref, variants):
    t0 = adamfam_inputs(kind, n, gdt, mdt, "cpu", seed)
    sens = {}
    for flag, other in variants.items():
        sens[flag] = sensitivity(ref, other(t0) if callable(other) else ref_step(kind, t0, other))
        assert sens[flag] > 100, f"{kind} {hp}: {flag} moves w by only {sens[flag]:.3g} bounds"
    return sens


def run_amsgrad_flags(adamw, keras_eps, step, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    """One of the flag combinations on the flag-case hyperparameters.  Every flag must move w
    by more than 100 bounds: amsgrad itself against plain Adam (flat_reference.adam_ref) on the
    same m and v, the decay's coupling, the epsilon placement and the step count."""
    hp = dict(AMS_BASE, adamw=adamw, keras_eps=keras_eps, step=step)
    worst, ref, _ = run_step("amsgrad", n, gdt, mdt, dev, hp=hp, seed=4)
    sens = _sens("amsgrad", hp, 4, gdt, mdt, n, ref, {
        "amsgrad": lambda t0: adam_ref(t0["g"], t0["w"], t0["m"], t0["v"], **hp),
        "adamw": dict(hp, adamw=not adamw),
        "keras_eps": dict(hp, keras_eps=not keras_eps),
        "step": dict(hp, step=8 - step)})
    return worst, sens


def run_adamax_flags(keras_eps, weight_decay, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    hp = dict(ADAMAX_BASE, keras_eps=keras_eps, weight_decay=weight_decay)
    worst, ref, _ = run_step("adamax", n, gdt, mdt, dev, hp=hp, seed=5)
    sens = _sens("adamax", hp, 5, gdt, mdt, n, ref, {
        "keras_eps": dict(hp, keras_eps=not keras_eps),
        "weight_decay": dict(hp, weight_decay=0.1 - weight_decay),
        "step": dict(hp, step=1)})
    return worst, sens


def run_nadam_flags(decoupled, momentum_decay, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    hp = dict(NADAM_BASE, decoupled=decoupled, momentum_decay=momentum_decay)
    worst, ref, _ = run_step("nadam", n, gdt, mdt, dev, hp=hp, seed=6)
    sens = _sens("nadam", hp, 6, gdt, mdt, n, ref, {
        "decoupled_weight_decay": dict(hp, decoupled=not decoupled),
        "momentum_decay": dict(hp, momentum_decay=0.5 - momentum_decay),
        "step": dict(hp, step=8 - hp["step"])})
    return worst, sens


def run_adamax_zero_divisor(dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    """eps = 0, no decay, u = 0 and a zero gradient on every third element: the divisor is
    exactly 0 there and w (with a nonzero m on top, so that torch's form would be inf or NaN)
    stays bit for bit; the other elements update within the bound."""
    hp = dict(HP["adamax"], eps=0.0, weight_decay=0.0)
    t = adamfam_inputs("adamax", n, gdt, mdt, "cpu", seed=9)
    dead = torch.arange(n) % 3 == 0
    t["g"][dead] = 0
    t["u"][dead] = 0
    t = {k: (x.to(dev) if torch.is_tensor(x) else x) for k, x in t.items()}
    w0 = t["w"].clone()
    ref = ref_step("adamax", t, hp, design=False)
    assert torch.equal(ref["w"].ref[dead], f64(w0)[dead])
    call_step("adamax", t, hp)
    worst = check_outputs("adamax zero divisor", "adamax", t, ref)
    dead = dead.to(dev)
    assert torch.equal(t["w"][dead], w0[dead]), "a zero divisor must leave w as it is"
    assert (t["u"][dead] == 0).all() and not torch.equal(t["w"][~dead], w0[~dead])
    return worst


def run_skip(kind, dev, gdt=torch.float16, mdt=torch.bfloat16, n=4097):
    """skip=[1] leaves w, the state and the model copy bit-identical; skip=[0] equals
    skip=None bit for bit (and does update)."""
    t = adamfam_inputs(kind, n, gdt, mdt, dev, seed=8)
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


def run_clip(kind, dev, gdt=torch.float16, mdt=torch.bfloat16, n=N_GRID, coef=0.37):
    """a launch with gclip = [coef] equals the launch of fp32(gscale) * fp32(coef) without it,
    bit for bit, and differs from the unclipped launch"""
    hp = dict(HP[kind])
    t0 = adamfam_inputs(kind, n, gdt, mdt, dev, seed=10)
    a, b, c = clone_inputs(t0), clone_inputs(t0), clone_inputs(t0)
    gclip = torch.tensor([coef], dtype=torch.float32, device=dev)
    call_step(kind, a, hp, gclip=gclip)
    f32 = torch.float32
    prod = float(torch.tensor(hp["gscale"], dtype=f32) * torch.tensor(coef, dtype=f32))
    call_step(kind, b, dict(hp, gscale=prod))
    call_step(kind, c, hp)
    for name in a:
        if torch.is_tensor(a[name]):
            assert torch.equal(a[name], b[name]), f"{kind}: clipped launch differs in {name}"
    assert not torch.equal(a["w"], c["w"]), f"{kind}: the clip coefficient changed nothing"


# the dyn blocks: what each kernel reads from [d0, d1, d2, d3], and the bogus scalars it must
# then ignore
def dyn_case(kind):
    """(hp with the true values, hp with bogus scalars, the dyn block, the reference's extra
    keyword arguments)"""
    hp = dict(HP[kind], lr=0.07)
    if kind in ("amsgrad", "adamax"):
        # [lr, -, bc1, bc2]: bogus lr and step (the step only feeds bc1 and bc2)
        return hp, dict(hp, lr=99.0, step=1), [0.07, 123.0, 0.5, 0.25], \
            (dict(bc1=0.5, bc2=0.25) if kind == "amsgrad" else dict(bc1=0.5))
    # NAdam: [lr, cg, cm, bc2]; a bogus step changes all three scalars
    return hp, dict(hp, lr=99.0, step=1), [0.07, 0.75, 1.5, 0.25], dict(cg=0.75, cm=1.5, bc2=0.25)
