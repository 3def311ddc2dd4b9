"""Causal attention (csrc/kernels/mv_attn_causal.hip) through mivod._mvk._attn_causal against
the float64 references and counted bounds of tests/attn_reference.py, used unchanged: R.scores
is wrapped to return S2 = -inf, cA = inf at every disallowed (query, key) pair, as it does for
a -inf key.  Worst err / bound on an MI355X: docs/CAUSAL_ATTENTION.md."""
import math

import pytest
import torch

import attn_reference as R

mvk = pytest.importorskip("mivod._mvk")
pytestmark = pytest.mark.gpu

# s -> runs [(lo, hi), ...] (tokens outside every run are padding), or None: dense causal
SEGS = {128: [(0, 5), (5, 70), (70, 128)], 257: [(0, 40), (40, 128), (128, 129), (129, 257)],
        100: [(0, 30), (50, 90)]}
CASES = [(s, None) for s in (1, 17, 64, 65, 128, 129, 193, 257)] + list(SEGS.items())
B, H = 2, 3


def make_ids(s, runs, dev):
    if runs is None:
        return None
    ids = torch.full((B, s), -1, dtype=torch.int32, device=dev)
    for j, (lo, hi) in enumerate(runs):
        ids[:, lo:hi] = j
    return ids


def wrap_scores(monkeypatch, s, ids, dev):
    """Disallowed: above the diagonal, in different runs or on a padding key."""
    ok = torch.ones(s, s, dtype=torch.bool, device=dev).tril().expand(B, s, s)
    if ids is not None:
        ok = ok & (ids[:, :, None] == ids[:, None, :]) & (ids >= 0)[:, None, :]
    base = R.scores

    def scores(qkv, mask):
        S2, cA = base(qkv, mask)
        no = ~ok[:, None].to(S2.device)
        return S2.masked_fill(no, -math.inf), cA.masked_fill(no, math.inf)
    monkeypatch.setattr(R, "scores", scores)
    return ok


def run(t, p, seg=None):
    C, a = mvk._attn_causal, (t["mask"], p, R.SEED, seg)
    out, lse = C.fwd(t["qkv"], *a)
    dqkv = C.bwd(t["qkv"], out, t["dout"], lse, *a)
    bsum = None
    if R.is_short(t["qkv"].shape[1]):
        d2, bsum = C.bwd_bsum(t["qkv"], out, t["dout"], lse, *a)
        assert torch.equal(d2, dqkv)
    return out, lse, dqkv, bsum


def check(tag, t, p, got, cuda):
    out, lse, dqkv, bsum = got
    b, s, _, h, _ = t["qkv"].shape
    keep = R.keep_mask(b, h, s, p, R.SEED).to(cuda) if p > 0 else None
    w = R.check_fwd(tag, out, lse, R.fwd_ref(t["qkv"], t["mask"], keep, p))
    w.update(R.check_bwd(tag, dqkv, bsum, R.bwd_ref(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)))
    print(f"{tag}: {R.fmt(w)}")
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()


def test_wrapped_reference_is_a_masked_softmax(monkeypatch):
    """On the CPU at s = 17: fwd_ref over the wrapped scores against a plain float64 softmax."""
    s, t = 17, R.make_case(B, 17, H, "frac")
    ids = make_ids(s, [(0, 6), (8, 17)], "cpu")
    ok = wrap_scores(monkeypatch, s, ids, "cpu")
    q, k, v = R.f64(t["qkv"]).permute(2, 0, 3, 1, 4).unbind(0)
    sc = R.SC * (q @ k.transpose(-1, -2)) + R.LOG2E * R.f64(t["mask"])[:, None, None, :]     # log2 units
    want = torch.softmax(sc.masked_fill(~ok[:, None], -math.inf) * math.log(2), -1).nan_to_num(0.0) @ v
    f = R.fwd_ref(t["qkv"], t["mask"], None, 0.0)
    torch.testing.assert_close(f.out64, want.permute(0, 2, 1, 3), atol=1e-9, rtol=1e-9)
    assert (f.out64[:, 6:8] == 0).all() and (f.lse.ref[..., 6:8] == -math.inf).all()


@pytest.mark.parametrize("s,runs", CASES)
def test_causal_inside_every_bound(cuda, monkeypatch, s, runs):
    ids = make_ids(s, runs, cuda)
    seg = None if ids is None else mvk._attn_seg.seg_bounds(ids)
    wrap_scores(monkeypatch, s, ids, cuda)
    for kind in ("none", "frac"):
        t = R.to_dev(R.make_case(B, s, H, kind), cuda)
        for p in R.P_DROPS:
            got = run(t, p, seg)
            check(f"causal s={s} seg={runs is not None} {kind} p={p}", t, p, got, cuda)
            if ids is not None:
                assert (got[0][ids < 0] == 0).all() and (got[2][ids < 0] == 0).all()
                assert (got[1].transpose(1, 2)[ids < 0] == -math.inf).all()


@pytest.mark.parametrize("s", [65, 193])
def test_key0_masked_leaves_query0_dead(cuda, monkeypatch, s):
    wrap_scores(monkeypatch, s, None, cuda)
    t = R.to_dev(R.make_case(B, s, H, "frac"), cuda)
    t["mask"][:, 0] = -math.inf
    out, lse, dqkv, _ = got = run(t, 0.1)
    check(f"dead row s={s}", t, 0.1, got, cuda)
    assert (out[:, 0] == 0).all() and (lse[..., 0] == -math.inf).all() and (dqkv[:, 0] == 0).all()


@pytest.mark.parametrize("s,cut", [(128, 37), (257, 130)])
def test_no_look_ahead_bit_for_bit(cuda, s, cut):
    t = R.to_dev(R.make_case(B, s, H, "frac"), cuda)
    u = dict(t, qkv=t["qkv"].clone())
    u["qkv"][:, cut:] = R.to_dev(R.make_case(B, s, H, "none", seed=1), cuda)["qkv"][:, cut:]
    (o1, l1), (o2, l2) = (mvk._attn_causal.fwd(x["qkv"], x["mask"], 0.1, R.SEED) for x in (t, u))
    assert torch.equal(o1[:, :cut], o2[:, :cut]) and torch.equal(l1[..., :cut], l2[..., :cut])


@pytest.mark.parametrize("s", [128, 257])
def test_two_runs_are_bit_identical(cuda, s):
    t = R.to_dev(R.make_case(B, s, H, "frac"), cuda)
    for seg in (None, mvk._attn_seg.seg_bounds(make_ids(s, SEGS[s], cuda))):
        first = run(t, 0.1, seg)
        torch.empty(1 << 24, device=cuda).fill_(math.nan)       # dirty freed memory (dQ partials)
        for a, c in zip(run(t, 0.1, seg), first):
            assert c is None or torch.equal(a, c)


@pytest.mark.parametrize("segments", [False, True])
def test_attention_op_causal(cuda, segments):
    from mivod.ops.attention import BiasGradSlot, attention, attention_math
    ids = make_ids(128, SEGS[128], cuda) if segments else None
    t = R.to_dev(R.make_case(B, 128, H, "none"), cuda)
    out, _, dqkv, bsum = run(t, 0.0, None if ids is None else mvk._attn_seg.seg_bounds(ids))
    qkv, slot = t["qkv"].clone().requires_grad_(), BiasGradSlot()
    y = attention(qkv, causal=True, bias_slot=slot, segment_ids=ids)
    y.backward(t["dout"].view(B, 128, -1))
    assert all(map(torch.equal, (y.view(out.shape), qkv.grad, slot.partials), (out, dqkv, bsum)))
    torch.testing.assert_close(y.float(), attention_math(t["qkv"].float(), segment_ids=ids, causal=True),
                               atol=2e-2, rtol=2e-2)
