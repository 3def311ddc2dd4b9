"""Head-dim-128 attention (csrc/kernels/mv_attn_d128.hip) through mivod._mvk._attn_d128 against
the plain float64 reference of tests/attn_d128_ref.py.

Per tensor of out, lse, dq, dk, dv: err = max |got - ref| / max |ref| over ALL elements (lse:
max of |got - ref| / max(1, |ref|) over the finite ones; -inf must match).  The yardstick is
the shipped d = 64 kernels on a case of the same s, mode, mask, p and seed against the same
reference function: err128 <= max(4 err64, floor), floor = 2^-8 (bf16 tensors: one store
rounding 2^-9, doubled) or 2^-20 (lse: a handful of fp32 operations); 4 = twice the terms in
every d-contraction and another summation order (x 2), doubled for a maximum over few samples.
A tensor whose reference is exactly zero (dq and dk at s = 1: the softmax of one key has no
gradient, dS = P (dZ - delta) cancels) has max |ref| = 0 and no scale of its own; what the
kernels store there is the rounding of the stored bf16 out inside delta = rowsum(dO out), at
most 2^-9 sum_d |dO_d out_d| per query, times |q| or |k| / sqrt(d).  Its err is therefore taken
against max_q sum_d |dO_d out_d| max |qkv| / sqrt(d), the size of the terms that cancel: a
correct kernel stays below 2^-9 of it, a lost 1 / (1 - p) on either term is 0.1 of a typical one.
The worst err128 / err64 per tensor on an MI355X are in docs/ATTENTION_D128.md."""
import math

import pytest
import torch

import attn_d128_ref as A
from mivod import _mvk as mvk

pytestmark = pytest.mark.gpu

B, H, SEED = 2, 3, 1234
RUNS = {100: [(0, 30), (50, 90)], 193: [(0, 40), (40, 128), (128, 129), (129, 193)]}
CASES = ([(s, m) for s in (1, 17, 64, 65, 129, 193) for m in ("dense", "causal")]
         + [(s, m) for s in RUNS for m in ("seg", "seg+causal")])
NAMES = ("out", "lse", "dq", "dk", "dv")


def run(t, p, seg, causal):
    """(out, lse, dqkv) of the kernels of the width of t["qkv"]."""
    qkv, a = t["qkv"], (t["mask"], p, SEED)
    if qkv.shape[-1] == 128:
        out, lse = mvk._attn_d128.fwd(qkv, *a, seg, causal)
        return out, lse, mvk._attn_d128.bwd(qkv, out, t["dout"], lse, *a, seg, causal)
    if causal:
        out, lse = mvk._attn_causal.fwd(qkv, *a, seg)
        return out, lse, mvk._attn_causal.bwd(qkv, out, t["dout"], lse, *a, seg)
    if seg is not None:
        out, lse = mvk._attn_seg.fwd(qkv, *a, seg)
        return out, lse, mvk._attn_seg.bwd(qkv, out, t["dout"], lse, *a, seg)
    out, lse = mvk.attn_fwd(qkv, *a)
    return out, lse, mvk.attn_bwd(qkv, out, t["dout"], lse, *a)


def errors(t, p, ok, got):
    out, lse, dqkv = got
    want, e = A.reference(t, p, ok, SEED), {}
    for name, g, r in zip(NAMES, (out, lse) + dqkv.unbind(2), want):
        g = g.double()
        if name == "lse":
            fin = torch.isfinite(r)
            assert torch.equal(g[~fin], r[~fin]), "lse of the queries without a key"
            e[name] = float(((g - r).abs() / r.abs().clamp(min=1.0))[fin].max()) if fin.any() else 0.0
        else:
            scale = float(r.abs().max())
            if scale == 0:       # dq, dk at s = 1: the size of the terms that cancel
                scale = (float((t["dout"].double() * want[0]).abs().sum(-1).max())
                         * float(t["qkv"].double().abs().max()) / math.sqrt(r.shape[-1]))
            e[name] = float((g - r).abs().max()) / scale
    return e


def check(tag, d128, d64, p, seg, ok, causal):
    """The d = 128 case inside max(4 err64, floor) on every tensor -> its kernel results."""
    got = run(d128, p, seg, causal)
    e128, e64 = errors(d128, p, ok, got), errors(d64, p, ok, run(d64, p, seg, causal))
    print(f"{tag}: " + ", ".join(f"{n} {e128[n]:.3g} / {e64[n]:.3g} = {e128[n] / max(e64[n], 1e-300):.2f}"
                                 for n in NAMES))
    for n in NAMES:
        assert e128[n] <= max(4 * e64[n], 2.0 ** -20 if n == "lse" else 2.0 ** -8), (tag, n, e128[n], e64[n])
    return got


def setup(s, mode, dev):
    causal, runs = "causal" in mode, RUNS[s] if "seg" in mode else None
    ids = None if runs is None else A.make_ids(B, s, runs, dev)
    seg = None if ids is None else mvk._attn_seg.seg_bounds(ids)
    return causal, ids, seg, A.allowed(B, s, ids, causal, dev)


@pytest.mark.parametrize("s,mode", CASES)
def test_d128_against_float64(cuda, s, mode):
    causal, ids, seg, ok = setup(s, mode, cuda)
    for kind in ("none", "frac"):
        d128, d64 = (A.make_inputs(B, s, H, d, kind, 0, cuda) for d in (128, 64))
        for p in (0.0, 0.1):
            out, lse, dqkv = check(f"s={s} {mode} {kind} p={p}", d128, d64, p, seg, ok, causal)
            if ids is not None:
                assert (out[ids < 0] == 0).all() and (dqkv[ids < 0] == 0).all()
                assert (lse.transpose(1, 2)[ids < 0] == -math.inf).all()


def test_key0_masked_leaves_query0_dead(cuda):
    causal, _, seg, ok = setup(65, "causal", cuda)
    d128, d64 = (A.make_inputs(B, 65, H, d, "frac", 0, cuda) for d in (128, 64))
    for t in (d128, d64):
        t["mask"][:, 0] = -math.inf
    out, lse, dqkv = check("dead query", d128, d64, 0.1, seg, ok, causal)
    assert (out[:, 0] == 0).all() and (lse[..., 0] == -math.inf).all() and (dqkv[:, 0] == 0).all()


def test_no_look_ahead_bit_for_bit(cuda):
    s, cut = 129, 70
    t = A.make_inputs(B, s, H, 128, "frac", 0, cuda)
    u = dict(t, qkv=t["qkv"].clone())
    u["qkv"][:, cut:] = A.make_inputs(B, s, H, 128, "none", 1, cuda)["qkv"][:, cut:]
    (o1, l1), (o2, l2) = (mvk._attn_d128.fwd(x["qkv"], x["mask"], 0.1, SEED, None, True) for x in (t, u))
    assert torch.equal(o1[:, :cut], o2[:, :cut]) and torch.equal(l1[..., :cut], l2[..., :cut])


@pytest.mark.parametrize("mode", ["dense", "seg+causal"])
def test_two_runs_are_bit_identical(cuda, mode):
    causal, _, seg, _ = setup(193, mode, cuda)
    t = A.make_inputs(B, 193, H, 128, "frac", 0, cuda)
    first = run(t, 0.1, seg, causal)
    torch.empty(1 << 24, device=cuda).fill_(math.nan)       # dirty the freed memory (delta)
    assert all(map(torch.equal, run(t, 0.1, seg, causal), first))


def test_attention_op_d128(cuda):
    from mivod.ops.attention import BiasGradSlot, attention, attention_math
    s, ids = 100, A.make_ids(B, 100, RUNS[100], cuda)
    t = A.make_inputs(B, s, H, 128, "none", 0, cuda)
    seg = mvk._attn_seg.seg_bounds(ids)
    out, _, dqkv = run(t, 0.1, seg, True)
    qkv, slot = t["qkv"].clone().requires_grad_(), BiasGradSlot()
    y = attention(qkv, p_drop=0.1, seed=SEED, causal=True, segment_ids=ids, bias_slot=slot)
    y.backward(t["dout"].view(B, s, -1))
    assert torch.equal(y.view(out.shape), out) and torch.equal(qkv.grad, dqkv) and slot.partials is None
    y0 = attention(t["qkv"], causal=True, segment_ids=ids)
    torch.testing.assert_close(y0.float(), attention_math(t["qkv"].float(), segment_ids=ids, causal=True),
                               atol=2e-2, rtol=2e-2)


def test_binding_checks_name_the_operand(cuda):
    t = A.make_inputs(B, 17, H, 128, "none", 0, cuda)
    with pytest.raises(RuntimeError, match=r"_attn_d128\.fwd: qkv must be \[b, s, 3, h, 128\]"):
        mvk._attn_d128.fwd(A.make_inputs(B, 17, H, 64, "none", 0, cuda)["qkv"], None, 0.0, SEED)
    out, lse = mvk._attn_d128.fwd(t["qkv"], None, 0.0, SEED)
    with pytest.raises(RuntimeError, match=r"_attn_d128\.bwd: lse must hold"):
        mvk._attn_d128.bwd(t["qkv"], out, t["dout"], lse[:, :, :16].contiguous(), None, 0.0, SEED)
