"""Block-diagonal attention for packed sequences (csrc/kernels/mv_attn_seg.hip: the segmented
fwd_kernel, fwd_short_kernel, bwd_kernel + dq_reduce_kernel and bwd_short_kernel, and
seg_bounds_kernel) through mivod._mvk._attn_seg against the float64 references and counted
bounds of tests/attn_reference.py, used unchanged with one call per run: the full row with -inf
on every key outside the run (and, backward, dout = 0 and lse = +inf on the queries outside it).
The bounds count roundings at the full s; a kernel that skips tiles performs fewer.

Worst err / bound on an MI355X over this module: see docs/PACKED_ATTENTION.md."""
import math

import pytest
import torch

import attn_reference as R

mvk = pytest.importorskip("mivod._mvk")

pytestmark = pytest.mark.gpu

# name -> (s, per batch row (cycled): [(lo, hi), ...] runs; tokens outside every run are padding)
CASES = {
    "short128": (128, [[(0, 5), (5, 70), (70, 128)]]),             # edges off every tile and wave
    "short64": (64, [[(0, 1), (1, 64)], [(0, 63), (63, 64)]]),
    "short17": (17, [[(0, 16), (16, 17)]]),
    "short100pad": (100, [[(0, 30), (50, 90)], [(3, 100)]]),        # keys 32..47: a padding wave
    "long193": (193, [[(0, 63), (63, 130), (130, 193)]]),
    "long257": (257, [[(0, 40), (40, 128), (128, 129), (129, 257)]]),   # 1 token; three 64-blocks
    "long129pad": (129, [[(0, 60), (60, 109)], [(0, 50), (70, 129)]]),  # padded tail; padded gap
}


def make_ids(name, b, dtype=torch.int32):
    s, rows = CASES[name]
    ids = torch.full((b, s), -1, dtype=dtype)
    for i in range(b):
        for j, (lo, hi) in enumerate(rows[i % len(rows)]):
            ids[i, lo:hi] = j
    return ids


def seg_refs(t, ids, keep, p, out=None, lse=None):
    """(Fwd, None) or, given the stored out and lse, (None, Bwd): attn_reference's results
    assembled over the runs.  Token rows come from the run that owns the token; bsum is the
    sum over the runs, tolerances summed.  Padding tokens: reference 0 (lse -inf), bound 0."""
    qkv, dout, mask = t["qkv"], t["dout"], t["mask"]
    b, s, _, h, _ = qkv.shape
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=qkv.device)
    o_ref, o_del = z(b, s, h, R.D), z(b, s, h, R.D)
    l_ref, l_tol = z(b, h, s) - math.inf, z(b, h, s)
    g_ref, g_del = z(b, s, 3, h, R.D), z(b, s, 3, h, R.D)
    bs_ref, bs_tol = z(b, 3, h, R.D), z(b, 3, h, R.D)
    for j in range(int(ids.max()) + 1):
        own = ids == j                                                   # [b, s]
        kmask = (torch.zeros(b, s, device=qkv.device) if mask is None else mask.clone())
        kmask[~own] = -math.inf
        if out is None:
            f = R.fwd_ref(qkv, kmask, keep, p)
            o_ref[own], o_del[own] = f.out.ref[own], f.out.delta[own]
            oq = own[:, None, :].expand(b, h, s)
            l_ref[oq], l_tol[oq] = f.lse.ref[oq], f.lse.tol[oq]
        else:
            lse_j = torch.where(own[:, None, :], lse, torch.full_like(lse, math.inf))
            g = R.bwd_ref(qkv, out, lse_j, dout * own[:, :, None, None], kmask, keep, p)
            g_ref[own], g_del[own] = g.dqkv.ref[own], g.dqkv.delta[own]
            bs_ref += g.bsum.ref
            bs_tol += g.bsum.tol
    if out is None:
        return R.Fwd(R.Stored(o_ref, o_del), R.Bound(l_ref, l_tol), None, o_ref), None
    return None, R.Bwd(R.Stored(g_ref, g_del), R.Bound(bs_ref, bs_tol), None)


def run_seg(t, ids, p, seg=None):
    """(out, lse, dqkv, bsum or None) of the segmented bindings (``seg`` None: the dense ones)."""
    qkv, dout, mask = t["qkv"], t["dout"], t["mask"]
    S = mvk._attn_seg
    tail = () if seg is None else (seg,)
    out, lse = (mvk.attn_fwd if seg is None else S.fwd)(qkv, mask, p, R.SEED, *tail)
    dqkv = (mvk.attn_bwd if seg is None else S.bwd)(qkv, out, dout, lse, mask, p, R.SEED, *tail)
    bsum = None
    if R.is_short(qkv.shape[1]):
        d2, bsum = (mvk.attn_bwd_bsum if seg is None else S.bwd_bsum)(qkv, out, dout, lse, mask, p,
                                                                     R.SEED, *tail)
        assert torch.equal(d2, dqkv)
    return out, lse, dqkv, bsum


@pytest.mark.parametrize("b,h", [(2, 3), (3, 2)])
@pytest.mark.parametrize("name", list(CASES))
def test_segments_inside_every_bound(cuda, name, b, h):
    """Every case with and without a fractional mask and dropout; padding tokens exactly 0;
    two runs bit-identical on one short and one long case (stale dQ partials would differ)."""
    s = CASES[name][0]
    ids = make_ids(name, b, torch.int64 if b == 2 else torch.int32).to(cuda)
    seg = mvk._attn_seg.seg_bounds(ids)
    pad = ids < 0
    for kind in ("none", "frac"):
        t = R.to_dev(R.make_case(b, s, h, kind), cuda)
        for p in R.P_DROPS:
            tag = f"{name} b={b} h={h} {kind} p={p}"
            keep = R.keep_mask(b, h, s, p, R.SEED).to(cuda) if p > 0 else None
            out, lse, dqkv, bsum = run_seg(t, ids, p, seg)
            fref, _ = seg_refs(t, ids, keep, p)
            w = R.check_fwd(tag, out, lse, fref)
            _, bref = seg_refs(t, ids, keep, p, out, lse)
            w.update(R.check_bwd(tag, dqkv, bsum, bref))
            print(f"{tag}: {R.fmt(w)}")
            assert (out[pad] == 0).all() and (dqkv[pad] == 0).all()
            assert (lse.transpose(1, 2)[pad] == -math.inf).all()
            assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
            assert torch.isfinite(lse.transpose(1, 2)[~pad]).all()
            if name in ("short128", "long257"):
                for a, c in zip(run_seg(t, ids, p, seg), (out, lse, dqkv, bsum)):
                    assert c is None or torch.equal(a, c), f"{tag}: two runs differ"


@pytest.mark.parametrize("s", [17, 128, 129, 257])
def test_one_segment_equals_the_dense_call(cuda, s):
    """All ids equal: nothing is skipped and the arithmetic is the dense kernels', bit for bit."""
    t = R.to_dev(R.make_case(2, s, 3, "frac"), cuda)
    ids = torch.full((2, s), 7, dtype=torch.int32, device=cuda)
    got = run_seg(t, ids, 0.1, mvk._attn_seg.seg_bounds(ids))
    for a, c in zip(got, run_seg(t, ids, 0.1)):
        assert c is None or torch.equal(a, c)


def test_seg_bounds(cuda):
    """Run bounds lo | hi << 16, 0 for padding; a row longer than one 256-token scan chunk."""
    ids = torch.tensor([[4] * 300 + [-1] * 3 + [2] * 297, [-1] + [9] * 255 + [0] * 343 + [-2]],
                       device=cuda)
    word = lambda lo, hi: lo | hi << 16
    want = torch.tensor([[word(0, 300)] * 300 + [0] * 3 + [word(303, 600)] * 297,
                         [0] + [word(1, 256)] * 255 + [word(256, 599)] * 343 + [0]], device=cuda)
    for dt in (torch.int32, torch.int64):
        assert torch.equal(mvk._attn_seg.seg_bounds(ids.to(dt)).long(), want)
    with pytest.raises(RuntimeError, match="65535"):
        mvk._attn_seg.seg_bounds(torch.zeros(1, 65536, dtype=torch.int32, device=cuda))


def test_attention_op_with_segments_and_bias_slot(cuda):
    """ops.attention.attention(segment_ids=) runs the segmented kernels in both directions and
    hands the bias-gradient partials over (s <= 128); segment_ids and segment_bounds exclude
    each other."""
    from mivod.ops.attention import BiasGradSlot, attention, attention_math, segment_bounds
    b, h = 2, 3
    ids = make_ids("short128", b).to(cuda)
    t = R.to_dev(R.make_case(b, 128, h, "none"), cuda)
    out, lse, dqkv, bsum = run_seg(t, ids, 0.0, mvk._attn_seg.seg_bounds(ids))
    qkv = t["qkv"].clone().requires_grad_()
    slot = BiasGradSlot()
    y = attention(qkv, segment_bounds=segment_bounds(ids), bias_slot=slot)
    y.backward(t["dout"].view(b, 128, -1))
    assert torch.equal(y.view(out.shape), out) and torch.equal(qkv.grad, dqkv)
    assert torch.equal(slot.partials, bsum)
    torch.testing.assert_close(y.float(), attention_math(t["qkv"].float(), segment_ids=ids),
                               atol=2e-2, rtol=2e-2)
    with pytest.raises(ValueError, match="not both"):
        attention(qkv, segment_ids=ids, segment_bounds=segment_bounds(ids))


def test_bert_model_runs_do_not_see_each_other(cuda):
    """BertModel(segment_ids=) in eval(): the hidden states of run 0's tokens do not change
    when run 1's tokens are replaced; without segment_ids they do."""
    from mivod.models.bert import BertConfig, BertModel
    torch.manual_seed(3)
    c = BertConfig.tiny(hidden_size=128, num_attention_heads=2)       # head dim 64: the kernels
    model = BertModel(c).to(cuda).to(torch.bfloat16).eval()
    b, s, cut = 2, 48, 20
    ids_a = torch.randint(0, c.vocab_size, (b, s), device=cuda)
    ids_b = ids_a.clone()
    ids_b[:, cut:] = torch.randint(0, c.vocab_size, (b, s - cut), device=cuda)
    tt = torch.zeros(b, s, dtype=torch.long, device=cuda)
    seg = (torch.arange(s, device=cuda) >= cut).int().expand(b, s).contiguous()
    with torch.no_grad():
        xa, _ = model(ids_a, tt, segment_ids=seg)
        xb, _ = model(ids_b, tt, segment_ids=seg)
        da, _ = model(ids_a, tt)
        db, _ = model(ids_b, tt)
    assert torch.isfinite(xa.float()).all()
    assert torch.equal(xa[:, :cut], xb[:, :cut])
    assert not torch.equal(da[:, :cut], db[:, :cut])
