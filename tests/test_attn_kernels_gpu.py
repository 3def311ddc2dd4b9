"""The fused attention kernels (csrc/kernels/mv_attn.hip: fwd_kernel, fwd_short_kernel,
bwd_kernel with delta_kernel and dq_reduce_kernel, bwd_short_kernel) through their bindings in
mivod._mvk against the float64 references and counted bounds of tests/attn_reference.py: every
sequence edge of both kernel families, both head layouts and b > h, with and without dropout,
without a mask, with -10000 on front and middle keys (the key s - 1 stays live) and with a
fractional mask that differs per batch row; out AND lse; the backward fed the kernel's own out
and lse; the bias-gradient column sums; -inf masks.  The dropout keep mask of the references is
the Python port, which the kernels' own mask must equal bit for bit.  The float64 references
run on the GPU (plain torch)."""
import math

import pytest
import torch

import attn_reference as R

mvk = pytest.importorskip("mivod._mvk")

pytestmark = pytest.mark.gpu


def _run(cuda, t, p, label, keep=None, twice=False):
    """One forward and backward through the bindings against the references.  Returns (worst
    ratios, forward reference, backward reference, (out, lse, dqkv))."""
    qkv, dout, mask = t["qkv"], t["dout"], t["mask"]
    b, s, _, h, _ = qkv.shape
    if p > 0 and keep is None:
        keep = R.keep_mask(b, h, s, p, R.SEED).to(cuda)
    if p > 0:
        own = mvk.attn_dropout_mask(b, h, s, p, R.SEED, cuda).bool()
        assert torch.equal(own, keep), f"{label}: attn_dropout_mask differs from the Python port"
    out, lse = mvk.attn_fwd(qkv, mask, p, R.SEED)
    assert out.shape == (b, s, h, R.D) and out.dtype == torch.bfloat16
    assert lse.shape == (b, h, s) and lse.dtype == torch.float32
    fref = R.fwd_ref(qkv, mask, keep, p)
    worst = R.check_fwd(label, out, lse, fref)
    dqkv = mvk.attn_bwd(qkv, out, dout, lse, mask, p, R.SEED)
    assert dqkv.shape == qkv.shape and dqkv.dtype == torch.bfloat16
    bref = R.bwd_ref(qkv, out, lse, dout, mask, keep, p)
    bsum = None
    if R.is_short(s):
        dqkv2, bsum = mvk.attn_bwd_bsum(qkv, out, dout, lse, mask, p, R.SEED)
        assert torch.equal(dqkv2, dqkv), f"{label}: attn_bwd_bsum changes dqkv"
        assert bsum.shape == (b, 3 * h * R.D) and bsum.dtype == torch.float32
    worst.update(R.check_bwd(label, dqkv, bsum, bref))
    if twice:
        out2, lse2 = mvk.attn_fwd(qkv, mask, p, R.SEED)
        assert torch.equal(out2, out) and torch.equal(lse2, lse), f"{label}: two forwards differ"
        assert torch.equal(mvk.attn_bwd(qkv, out, dout, lse, mask, p, R.SEED), dqkv), \
            f"{label}: two backwards differ"
        if bsum is not None:
            assert torch.equal(mvk.attn_bwd_bsum(qkv, out, dout, lse, mask, p, R.SEED)[1], bsum), \
                f"{label}: two column sums differ"
    return worst, fref, bref, (out, lse, dqkv)


@pytest.mark.parametrize("b,s,h", R.SHAPES)
def test_kernels_inside_every_bound(cuda, b, s, h):
    """Every mask kind with and without dropout at one (b, s, h); the calls repeat bit for bit
    (checked on one short and one long shape)."""
    for kind in R.MASK_KINDS:
        t = R.to_dev(R.make_case(b, s, h, kind), cuda)
        for p in R.P_DROPS:
            tag = f"b={b} s={s} h={h} {kind} p={p}"
            w, _, _, _ = _run(cuda, t, p, tag, twice=(b, s, h) in ((3, 127, 2), (2, 193, 3)))
            print(f"{tag}: {R.fmt(w)}")


@pytest.mark.parametrize("s", [17, 128, 129, 193])
def test_some_keys_at_minus_inf(cuda, s):
    """Keys masked with -inf: P and every gradient are what the reference gives without those
    keys (its P is exactly 0 there: tests/test_attn_reference_cpu.py), and their dK and dV rows
    are exactly 0."""
    b, h = 2, 3
    t = R.make_case(b, s, h, "frac")
    dead = torch.tensor(sorted({0, 7, 8, s // 2, s - 1}))
    t["mask"][0, dead] = -math.inf
    t["mask"][1, dead[:-1] + 1] = -math.inf                # row 1: the key s - 1 stays live
    t = R.to_dev(t, cuda)
    for p in R.P_DROPS:
        w, fref, bref, (out, lse, dqkv) = _run(cuda, t, p, f"inf keys s={s} p={p}")
        assert torch.isfinite(dqkv.float()).all()
        assert (dqkv[0, dead, 1:] == 0).all() and (dqkv[1, dead[:-1] + 1, 1:] == 0).all()
        print(f"s={s} p={p}: {R.fmt(w)}")


@pytest.mark.parametrize("s", [128, 129])
@pytest.mark.parametrize("value", [-math.inf, torch.finfo(torch.float32).min])
def test_fully_masked_batch_row(cuda, s, value):
    """One batch row with every key at -inf (or finfo.min, whose product with log2(e)
    overflows to -inf): out = 0 and lse = -inf for it, every gradient finite, its own gradient
    exactly 0, and the other batch rows inside their ordinary bounds."""
    b, h = 3, 2
    t = R.make_case(b, s, h, "frac")
    t["mask"][1] = value
    t = R.to_dev(t, cuda)
    for p in R.P_DROPS:
        w, fref, bref, (out, lse, dqkv) = _run(cuda, t, p, f"masked row s={s} p={p}")
        assert (out[1] == 0).all() and (lse[1] == -math.inf).all()
        assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
        assert (dqkv[1] == 0).all()
        assert torch.isfinite(lse[0]).all() and torch.isfinite(lse[2]).all()
        print(f"s={s} p={p}: {R.fmt(w)}")


def test_zz_report_worst_ratios(mivod_report):
    """Not a check: the worst err / bound per output over this module's run, for the table in
    attn_reference's docstring."""
    if R.WORST:
        mivod_report("attention kernels, worst err / bound: " + R.fmt(dict(sorted(R.WORST.items()))))
