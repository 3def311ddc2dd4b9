"""Grouped-query attention at head dim 128 (the GQA forms of csrc/kernels/mv_attn_d128.hip)
through mivod._mvk._attn_gqa against the plain float64 reference of tests/attn_d128_ref.py.

The grouped op equals multi-head attention on the tensor whose K / V heads are repeated G times,
with dK / dV summed over each group, so the reference is A.reference on that expansion with its
dk, dv group-summed in float64.  Per tensor of out, lse, dq, dk, dv the error is the one of
tests/test_attn_d128_gpu.py: max |got - ref| / max |ref| over all elements (lse: |got - ref| /
max(1, |ref|) over the finite ones, -inf must match; a reference that is exactly zero — dq, dk at
s = 1 — is measured against max_q sum_d |dO_d out_d| max |qkv| / sqrt(d)).  The yardstick is the
shipped _attn_d128 kernels on the expansion against the same reference, their bf16 dk / dv
group-summed in float64: err_gqa <= max(4 err_d128, floor), floor 2^-8 (bf16 tensors) or 2^-20
(lse).  The contractions have the same length; dK / dV take another summation order (x 2),
doubled for a maximum over few samples.  A wrong head mapping gives errors of order 1.  The
worst ratios per tensor on an MI355X are in docs/ATTENTION_GQA.md."""
import math

import pytest
import torch

import attn_d128_ref as A
from mivod import _mvk as mvk

pytestmark = pytest.mark.gpu

B, SEED, D = 2, 1234, 128
HEADS = [(4, 2), (6, 2), (8, 2), (8, 1)]       # G = 2, 3, 4, 8: HW = 2, 1, 4, 4 in two chunks
RUNS = {100: [(0, 30), (50, 90)], 193: [(0, 40), (40, 128), (128, 129), (129, 193)]}
CASES = ([(s, m) for s in (1, 17, 33, 65, 129) for m in ("dense", "causal")]
         + [(s, m) for s in RUNS for m in ("seg", "seg+causal")])
NAMES = ("out", "lse", "dq", "dk", "dv")


def make(s, hq, hkv, kind, dev):
    """(grouped qkv [b, s, hq + 2 hkv, 128], the case on its expansion [b, s, 3, hq, 128])."""
    t = A.make_inputs(B, s, hq, D, kind, 0, dev)
    q, k, v = t["qkv"].unbind(2)
    k, v, G = k[:, :, ::hq // hkv], v[:, :, ::hq // hkv], hq // hkv
    expanded = torch.stack([q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)], 2).contiguous()
    return torch.cat([q, k, v], 2).contiguous(), dict(t, qkv=expanded)


def setup(s, mode, dev):
    causal, runs = "causal" in mode, RUNS[s] if "seg" in mode else None
    ids = None if runs is None else A.make_ids(B, s, runs, dev)
    seg = None if ids is None else mvk._attn_seg.seg_bounds(ids)
    return causal, ids, seg, A.allowed(B, s, ids, causal, dev)


def run_gqa(qkv, hkv, t, p, seg, causal):
    a = (t["mask"], p, SEED, seg, causal)
    out, lse = mvk._attn_gqa.fwd(qkv, hkv, *a)
    return out, lse, mvk._attn_gqa.bwd(qkv, hkv, out, t["dout"], lse, *a)


def run_d128(t, p, seg, causal):
    a = (t["mask"], p, SEED, seg, causal)
    out, lse = mvk._attn_d128.fwd(t["qkv"], *a)
    return out, lse, mvk._attn_d128.bwd(t["qkv"], out, t["dout"], lse, *a)


def group_sum(x, hkv):
    b, s, h, d = x.shape
    return x.double().view(b, s, hkv, h // hkv, d).sum(3)


def errors(t, want, got):
    """got, want: (out, lse, dq, dk, dv), dk / dv already over the KV heads."""
    e = {}
    for name, g, r in zip(NAMES, got, want):
        g = g.double()
        if name == "lse":
            fin = torch.isfinite(r)
            assert torch.equal(g[~fin], r[~fin]), "lse of the queries without a key"
            e[name] = float(((g - r).abs() / r.abs().clamp(min=1.0))[fin].max()) if fin.any() else 0.0
        else:
            scale = float(r.abs().max())
            if scale == 0:       # dq, dk at s = 1: the size of the terms that cancel
                scale = (float((t["dout"].double() * want[0]).abs().sum(-1).max())
                         * float(t["qkv"].double().abs().max()) / math.sqrt(D))
            e[name] = float((g - r).abs().max()) / scale
    return e


def check(tag, qkv, t, hq, hkv, p, seg, ok, causal):
    out, lse, dqkv = run_gqa(qkv, hkv, t, p, seg, causal)
    o2, l2, d2 = run_d128(t, p, seg, causal)
    ref = A.reference(t, p, ok, SEED)
    want = ref[:3] + (group_sum(ref[3], hkv), group_sum(ref[4], hkv))
    e = errors(t, want, (out, lse) + dqkv.split([hq, hkv, hkv], 2))
    y = errors(t, want, (o2, l2, d2[:, :, 0], group_sum(d2[:, :, 1], hkv), group_sum(d2[:, :, 2], hkv)))
    print(f"{tag}: " + ", ".join(f"{n} {e[n]:.3g} / {y[n]:.3g} = {e[n] / y[n] if y[n] else math.inf:.2f}"
                                 for n in NAMES))
    for n in NAMES:
        assert e[n] <= max(4 * y[n], 2.0 ** -20 if n == "lse" else 2.0 ** -8), (tag, n, e[n], y[n])
    return out, lse, dqkv


@pytest.mark.parametrize("hq,hkv", HEADS)
@pytest.mark.parametrize("s,mode", CASES)
def test_gqa_against_float64(cuda, s, mode, hq, hkv):
    causal, ids, seg, ok = setup(s, mode, cuda)
    for kind in ("none", "frac"):
        qkv, t = make(s, hq, hkv, kind, cuda)
        for p in (0.0, 0.1):
            out, lse, dqkv = check(f"h={hq}/{hkv} s={s} {mode} {kind} p={p}", qkv, t, hq, hkv, p, seg, ok, causal)
            if ids is not None:
                assert (out[ids < 0] == 0).all() and (dqkv[ids < 0] == 0).all()
                assert (lse.transpose(1, 2)[ids < 0] == -math.inf).all()


@pytest.mark.parametrize("mode", ["dense", "seg+causal"])
def test_one_head_per_group_is_d128_bit_for_bit(cuda, mode):
    causal, _, seg, _ = setup(193, mode, cuda)
    t = A.make_inputs(B, 193, 3, D, "frac", 0, cuda)
    got = run_gqa(t["qkv"].view(B, 193, 9, D), 3, t, 0.1, seg, causal)
    out, lse, dqkv = run_d128(t, 0.1, seg, causal)
    assert torch.equal(got[0], out) and torch.equal(got[1], lse) and torch.equal(got[2].view_as(dqkv), dqkv)


def test_two_runs_are_bit_identical(cuda):
    causal, _, seg, _ = setup(193, "seg+causal", cuda)
    qkv, t = make(193, 8, 2, "frac", cuda)
    first = run_gqa(qkv, 2, t, 0.1, seg, causal)
    torch.empty(1 << 24, device=cuda).fill_(math.nan)       # dirty the freed memory (delta)
    assert all(map(torch.equal, run_gqa(qkv, 2, t, 0.1, seg, causal), first))


def test_key0_masked_leaves_query0_dead(cuda):
    causal, _, seg, ok = setup(65, "causal", cuda)
    qkv, t = make(65, 4, 2, "frac", cuda)
    t["mask"][:, 0] = -math.inf
    out, lse, dqkv = check("dead query", qkv, t, 4, 2, 0.1, seg, ok, causal)
    assert (out[:, 0] == 0).all() and (lse[..., 0] == -math.inf).all() and (dqkv[:, 0] == 0).all()


def test_grouped_attention_op(cuda):
    from mivod.ops.attention import attention, grouped_attention, grouped_attention_math
    s, ids = 100, A.make_ids(B, 100, RUNS[100], cuda)
    g, t = make(s, 8, 2, "none", cuda)
    out, _, dqkv = run_gqa(g, 2, t, 0.1, mvk._attn_seg.seg_bounds(ids), True)
    qkv = g.clone().requires_grad_()
    y = grouped_attention(qkv, 2, p_drop=0.1, seed=SEED, causal=True, segment_ids=ids)
    y.backward(t["dout"].view(B, s, -1))
    assert torch.equal(y.view(out.shape), out) and torch.equal(qkv.grad, dqkv)
    y0 = grouped_attention(g, 2, causal=True, segment_ids=ids)
    torch.testing.assert_close(y0.float(), grouped_attention_math(g.float(), 2, segment_ids=ids, causal=True),
                               atol=2e-2, rtol=2e-2)
    full = t["qkv"]       # kv_heads == hq: attention() on the 5-D view of the same memory
    assert torch.equal(grouped_attention(full.view(B, s, 24, D), 8, p_drop=0.1, seed=SEED, causal=True),
                       attention(full, p_drop=0.1, seed=SEED, causal=True))


def test_binding_checks_name_the_operand(cuda):
    qkv, t = make(17, 4, 2, "none", cuda)
    with pytest.raises(RuntimeError, match=r"_attn_gqa\.fwd: qkv's 8 heads must be hq \+ 2 kv_heads"):
        mvk._attn_gqa.fwd(qkv, 3, None, 0.0, SEED)
    with pytest.raises(RuntimeError, match=r"_attn_gqa\.fwd: qkv must be \[b, s, hq \+ 2 kv_heads, 128\]"):
        mvk._attn_gqa.fwd(qkv[..., :64].contiguous(), 2, None, 0.0, SEED)
    out, lse = mvk._attn_gqa.fwd(qkv, 2, None, 0.0, SEED)
    with pytest.raises(RuntimeError, match=r"_attn_gqa\.bwd: lse must hold"):
        mvk._attn_gqa.bwd(qkv, 2, out, t["dout"], lse[:, :, :16].contiguous(), None, 0.0, SEED)
