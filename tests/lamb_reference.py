"""float64 reference and derived error bounds for the LAMB step: lamb_moments_kernel ->
seg_reduce_kernel<2> -> lamb_apply_kernel (csrc/kernels/mv_kernels.hip) and the PyTorch
fallback (mivod/ops/kernels.py: lamb_step).

A helper module, not a test file: tests/test_lamb_cpu.py runs the fallback through it and
tests/test_lamb_gpu.py the HIP kernels.  The method, ``U``, ``check`` and the layouts are those
of tests/flat_reference.py (read its header first): every output must satisfy, per element,

    |got - ref| <= c * 2^-24 * mag

with ``mag`` the sum of the absolute values of the terms on the way to the output, carried
through a quotient or a square root by first-order sensitivity, and ``c`` the fp32 roundings
on the longest path, counted from the kernel source.  Where an output has several
sensitivity terms in ``mag`` (a path through the numerator and one through the denominator),
each path's error is at most its own count times U times its own term, so ``c`` is the count
of the longest path against the sum of the terms.

Counts (r = rounding of a hyperparameter, * + - / sqrt = one rounding each)
---------------------------------------------------------------------------
lamb_moments_kernel
  gr  = g*gscale                   gscale r, * -> 2 (no weight-decay term: it is in u)
  m   = b1*m + (1-b1)*gr           gr 2, (1-b1) r, * -> 4 (longer than b1 r, * = 2), + -> 5
  v   = b2*v + (1-b2)*gr*gr        (1-b2) r; gr twice = 4; two * -> 7, + -> 8
                                   mag_v uses mag_gr^2
  => C_LAMB_M = 5, C_LAMB_V = 8
  rbc1 = 1/bc1: r, / = 2;   rbc2 = 1/sqrt(bc2): r, sqrt, / = 3
lamb_u (the one expression both stages evaluate, on the same stored m, v and w, with both
multiply-adds written as fmaf, so stage 2 applies bit for bit the u whose norm stage 1 took)
  den = fma(sqrt(v), rbc2, eps)    v 8, sqrt 9, rbc2 3 -> 12, * 13 (fused: not rounded; counted),
                                   (eps r shares), + 14;  mag_den = mag_sqrt*rbc2 + eps with
                                   mag_sqrt = mag_v / sqrt(v)
  q   = m*rbc1/den                 den path: 14, / 15;  m path: 5 + 2 + * + / = 9
                                   mag_q = mag_m/bc1/den + |q|/den * mag_den
  u   = fma(wd, w, q)              wd r, * = 2 against |wd*w|; q 15; + -> 16
                                   mag_u = mag_q + |wd|*|w|
  => C_LAMB_U = 16
norms (block_sum<2> -> seg_reduce_kernel<2>, the tree of flat_reference's LARS section)
  A lane adds the squares of its 16 elements of the vector body in turn, and lanes 0..6 one
  more from the scalar tail of a chunk whose length is no multiple of 8: 17 terms, of which
  the first is added to 0 exactly, so still 16 roundings; wave_sum 6, block_sum 4, the
  seg_reduce lane 1 (up to 64 chunks), wave_sum 6: LARS_TREE_DEPTH = 33.
  |w|^2: product 1 + 33 = 34 = C_LAMB_WN2 against sum w^2
  |u|^2: u twice 32, * 33, + 33 = 66 = C_LAMB_UN2 against M = sum mag_u^2 (not sum u^2: u
         can cancel between q and wd*w)
lamb_apply_kernel
  wn = sqrt(|w|^2): 34, sqrt 35 against mag_wn = |w|^2/wn = wn
  un = sqrt(|u|^2): 66, sqrt 67 against mag_un = M/un
  trust = wn/un: / -> 68 (the un path; the wn path is 36) against
          mag_trust = mag_wn/un + wn/un^2 * mag_un = trust * (1 + M/|u|^2)
  slr = lr*trust: lr r, * -> 70
  w   = w - slr*u                  trust path: 70, * 71, - 72
                                   u path: 16 + (slr's own rounding is in the trust path) * 17, - 18
  mag_w = |w| + lr*trust*mag_u + lr*|u|*mag_trust
  => C_LAMB_W = 72
  trust == 1 (flagged segment, or a zero norm): slr = lr (r) 1, u 16, * -> 18, - -> 19
  mag_w = |w| + lr*mag_u           => C_LAMB_W_PLAIN = 19
The model copy is the RNE rounding of the stored fp32 master, bit for bit.

The fallback does the same arithmetic in fp32 torch ops with fewer roundings (the norms'
square roots, lr*trust and 1/sqrt(bc2) are taken in double), so the same counts hold for it.
"""
from __future__ import annotations

import math

import torch

from flat_reference import (DTYPES, HALF_ULP, LARS_FLAGS, LARS_SIZES, LARS_TREE_DEPTH,  # noqa: F401
                            MODELS, SIZES, U, UNAL_OFFS, UNAL_SIZES, UNAL_TOTAL, Out, check,
                            check_outputs, clone_inputs, f64, flag_of, fmt, lars_layout,
                            make_inputs, sensitivity)
from mivod.ops import kernels as K

C_LAMB_M, C_LAMB_V, C_LAMB_U = 5, 8, 16
C_LAMB_WN2 = 1 + LARS_TREE_DEPTH
C_LAMB_UN2 = 2 * C_LAMB_U + 1 + LARS_TREE_DEPTH
C_LAMB_W = C_LAMB_UN2 + 1 + 1 + 2 + 1 + 1        # sqrt, /, lr r and *, * u, -
C_LAMB_W_PLAIN = 1 + C_LAMB_U + 1 + 1
assert (C_LAMB_WN2, C_LAMB_UN2, C_LAMB_W, C_LAMB_W_PLAIN) == (34, 66, 72, 19)
C_OF = dict(w=(C_LAMB_W, C_LAMB_W_PLAIN), m=C_LAMB_M, v=C_LAMB_V,
            norms=(C_LAMB_WN2, C_LAMB_UN2))

HP_LAMB = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01, gscale=0.5, step=7)
# the flag cases: a decay and a rate large enough that every flag moves w far past a bound
LAMB_BASE = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.1, gscale=0.5, step=3)
LAMB_ZERO_GRAD = [6]          # of LARS_SIZES: the 77-element adapted segment
LAMB_ZERO_W = [1]             # the 300-element adapted segment


def lamb_ref(g, w, m, v, sizes, offsets, flags, *, lr, beta1=0.9, beta2=0.999, eps=1e-6,
             weight_decay=0.0, gscale=1.0, step=1, bc1=None, bc2=None, zero_norm_guard=True,
             trust_of=None):
    """Elements outside every segment keep their value with mag 0 (must be untouched).
    ``zero_norm_guard=False`` drops the "trust = 1 when a norm is zero" rule and
    ``trust_of`` = {segment: trust} replaces a segment's trust ratio: the variants the
    sensitivity guards compare with.  Also returns the fp64 (|w|^2, |u|^2) and the trust
    ratios."""
    g, w, m, v = f64(g), f64(w), f64(m), f64(v)
    bc1 = 1 - beta1 ** step if bc1 is None else bc1
    bc2 = 1 - beta2 ** step if bc2 is None else bc2
    rb = 1.0 / math.sqrt(bc2)
    out = {k: x.clone() for k, x in (("w", w), ("m", m), ("v", v))}
    mag = {k: torch.zeros_like(w) for k in "wmv"}
    c_w = torch.zeros_like(w)
    norms, nmag, trusts = [], [], []
    covered = torch.zeros(w.numel(), dtype=torch.bool)
    for i, (off, n, fl) in enumerate(zip(offsets, sizes, flags)):
        sl = slice(off, off + n)
        covered[sl] = True
        wi, aw = w[sl], w[sl].abs()
        gr = g[sl] * gscale
        mag_gr = gr.abs()
        flagged = bool(fl & 1)
        wd = 0.0 if flagged else weight_decay
        m_new = beta1 * m[sl] + (1 - beta1) * gr
        mag_m = beta1 * m[sl].abs() + (1 - beta1) * mag_gr
        v_new = beta2 * v[sl] + (1 - beta2) * gr * gr
        mag_v = beta2 * v[sl].abs() + (1 - beta2) * mag_gr * mag_gr
        sq = v_new.sqrt()
        mag_sq = torch.where(sq > 0, mag_v / sq, mag_v.sqrt())
        den, mag_den = sq * rb + eps, mag_sq * rb + eps
        q = (m_new / bc1) / den
        mag_q = (mag_m / bc1) / den + q.abs() / den * mag_den
        u, mag_u = q + wd * wi, mag_q + abs(wd) * aw
        wn2, un2, M = float((wi * wi).sum()), float((u * u).sum()), float((mag_u * mag_u).sum())
        norms.append([wn2, un2])
        nmag.append([wn2, M])
        wn, un = math.sqrt(wn2), math.sqrt(un2)
        trust, plain = 1.0, True
        if not flagged and ((wn > 0 and un > 0) or (not zero_norm_guard and un > 0)):
            trust, plain = wn / un, False
        if trust_of and i in trust_of:
            trust = trust_of[i]
        trusts.append(trust)
        out["m"][sl], mag["m"][sl] = m_new, mag_m
        out["v"][sl], mag["v"][sl] = v_new, mag_v
        out["w"][sl] = wi - lr * trust * u
        if plain:
            mag["w"][sl], c_w[sl] = aw + lr * trust * mag_u, C_LAMB_W_PLAIN
        else:
            mag_trust = trust * (1 + M / un2)
            mag["w"][sl] = aw + lr * trust * mag_u + lr * u.abs() * mag_trust
            c_w[sl] = C_LAMB_W
    nr = torch.tensor(norms, dtype=torch.float64).reshape(-1, 2)
    nm = torch.tensor(nmag, dtype=torch.float64).reshape(-1, 2)
    c_n = torch.tensor([C_LAMB_WN2, C_LAMB_UN2], dtype=torch.float64).expand_as(nr)
    return {"w": Out(out["w"], mag["w"], c_w), "m": Out(out["m"], mag["m"], C_LAMB_M),
            "v": Out(out["v"], mag["v"], C_LAMB_V), "norms": Out(nr, nm, c_n),
            "trust": trusts, "covered": covered}


# --------------------------------------------------------------------------- inputs and runners
def lamb_inputs(total, gdt, mdt, dev, layout, seed=0, zero_grad=(), zero_w=()):
    """Stored inputs (flat_reference.make_inputs: g, w, m, v, model), generated on the CPU.
    ``zero_grad`` segments get a zero gradient AND zero moments (u = wd*w), ``zero_w``
    segments zero weights."""
    sizes, offs = layout[0], layout[1]
    t = make_inputs("adam", total, gdt, mdt, "cpu", seed)
    for i in zero_grad:
        for k in "gmv":
            t[k][offs[i]:offs[i] + sizes[i]] = 0
    for i in zero_w:
        t["w"][offs[i]:offs[i] + sizes[i]] = 0
    return {k: (x.to(dev) if torch.is_tensor(x) else x) for k, x in t.items()}


def lamb_extra(layout, dev):
    return dict(table=K.make_chunk_table(layout[0], dev, layout[1]),
                seg_flags=torch.tensor(layout[2], dtype=torch.int32, device=dev))


def call_lamb(t, hp, layout, dev, **extra):
    """The step in place on ``t`` through mivod.ops.kernels (the HIP kernels on a GPU, the
    fallback on the CPU)."""
    K.lamb_step(t["g"], t["w"], t["m"], t["v"], t["model"], **lamb_extra(layout, dev), **hp,
                **extra)


def ref_lamb(t, hp, layout, **extra):
    return lamb_ref(t["g"], t["w"], t["m"], t["v"], *layout[:3], **hp, **extra)


def run_lamb(total, gdt, mdt, dev, layout, hp=None, seed=0, zero_grad=(), zero_w=(),
             workspace=None):
    """One step against fp64.  ``layout`` = (sizes, offsets, flags)."""
    hp = dict(HP_LAMB if hp is None else hp)
    t = lamb_inputs(total, gdt, mdt, dev, layout, seed, zero_grad, zero_w)
    ref = ref_lamb(t, hp, layout)
    extra = {} if workspace is None else dict(workspace=workspace)
    call_lamb(t, hp, layout, dev, **extra)
    return check_outputs(f"lamb n={total} {gdt}/{mdt}", "adam", t, ref), ref, t


def grid_layout():
    sizes, offs, total = lars_layout()
    return total, (sizes, offs, LARS_FLAGS)


def pair_layout(n):
    """an adapted segment of n elements and a flagged one of 70"""
    sizes, offs, total = lars_layout([n, 70])
    return total, (sizes, offs, [0, 1])


UNAL_LAYOUT = (UNAL_SIZES, UNAL_OFFS, [0, 0, 0, 1])

# flag cases: hp, flags, zero-gradient segments, zero-weight segments, the variant's changes
# to the reference (None: nothing to compare with)
LAMB_FLAG_CASES = {
    "flags": (LAMB_BASE, LARS_FLAGS, [], [], dict(flags=[1 - f for f in LARS_FLAGS])),
    # u = wd*w there, so trust = 1/wd, finite; the variant takes the segment for a zero norm
    "zero_grad": (LAMB_BASE, LARS_FLAGS, LAMB_ZERO_GRAD, [], dict(trust_of={6: 1.0})),
    # |w| = 0: trust 1, the segment moves by lr*u; without the guard trust = 0 and it stays
    "zero_w": (LAMB_BASE, LARS_FLAGS, [], LAMB_ZERO_W, dict(zero_norm_guard=False)),
    # a zero-length segment changes nothing by itself: no variant can differ (trust is 1)
    "zero_len": (LAMB_BASE, LARS_FLAGS, [], [], None),
    "wd0": (dict(LAMB_BASE, weight_decay=0.0), LARS_FLAGS, [], [], dict(hp=LAMB_BASE)),
}


def run_lamb_flag(case, dev, gdt=torch.float16, mdt=torch.bfloat16):
    hp, flags, zg, zw, variant = LAMB_FLAG_CASES[case]
    sizes, offs, total = lars_layout()
    layout = (sizes, offs, flags)
    worst, ref, _ = run_lamb(total, gdt, mdt, dev, layout, hp=hp, seed=5, zero_grad=zg, zero_w=zw)
    assert ref["trust"][5] == 1.0                       # the zero-length segment
    assert all(math.isfinite(x) for x in ref["trust"])
    for i in zg:
        assert abs(ref["trust"][i] * hp["weight_decay"] - 1.0) < 1e-9
    for i in zw:
        assert ref["trust"][i] == 1.0
    if variant is None:
        return worst, None
    t0 = lamb_inputs(total, gdt, mdt, "cpu", layout, 5, zg, zw)
    other = lamb_ref(t0["g"], t0["w"], t0["m"], t0["v"], sizes, offs,
                     variant.get("flags", flags), **variant.get("hp", hp),
                     zero_norm_guard=variant.get("zero_norm_guard", True),
                     trust_of=variant.get("trust_of"))
    sens = sensitivity(ref, other)
    assert sens > 100, f"lamb {case}: the variant moves w by only {sens:.3g} bounds"
    return worst, sens


def run_lamb_skip(dev, gdt=torch.float16, mdt=torch.bfloat16):
    """skip=[1] leaves w, m, v and the model copy bit-identical; skip=[0] equals skip=None
    bit for bit (and does update)."""
    total, layout = grid_layout()
    t = lamb_inputs(total, gdt, mdt, dev, layout, seed=8)
    before = clone_inputs(t)
    call_lamb(t, HP_LAMB, layout, dev, skip=flag_of(dev, 1))
    for name, x in before.items():
        assert torch.equal(t[name], x), f"lamb: skip=[1] changed {name}"
    a, b = clone_inputs(before), clone_inputs(before)
    call_lamb(a, HP_LAMB, layout, dev, skip=flag_of(dev, 0))
    call_lamb(b, HP_LAMB, layout, dev)
    for name in a:
        assert torch.equal(a[name], b[name]), f"lamb: skip=[0] differs from skip=None in {name}"
    for name in ("w", "m", "v", "model"):
        assert not torch.equal(a[name], before[name]), f"lamb: the step left {name} unchanged"
