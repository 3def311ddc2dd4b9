"""One-token attention against a KV cache (csrc/kernels/mv_attn_decode.hip) through
mivod._mvk._attn_decode against the float64 formula of tests/attn_decode_ref.py on the same bf16
inputs; err = max |got - ref| / max |ref| per tensor.  Yardstick: the shipped
_attn_gqa.fwd(causal=True) on a qkv whose K / V are the cache and whose last query row is q; its
row len - 1 is measured against the same reference.  Required: err_decode <= max(2 err_yard,
floor), floor 2^-8 (out) or 2^-20 (lse).  The worst ratios on an MI355X are in
docs/ATTENTION_DECODE.md."""
import functools
import math

import pytest
import torch

import attn_decode_ref as R
from mivod import _mvk as mvk

pytestmark = pytest.mark.gpu

B, S_MAX, D = 3, 320, 128
HEADS = [(4, 2), (8, 1), (16, 1), (3, 3)]          # G = 2, 8, 16 (no dead column), 1 (15 dead)
LENS = [(1, 64, 257), (63, 65, 200)]


@functools.lru_cache(maxsize=None)
def case(hq, hkv, lens):
    """Inputs (zeros at and past lens), the float64 reference and the yardstick's errors."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(hq * 1000 + hkv * 100 + lens[0])
    q = (torch.randn(B, hq, D, device=dev, generator=g) * 1.5).to(torch.bfloat16)
    kv = (torch.randn(B, S_MAX, 2 * hkv, D, device=dev, generator=g) * 1.5).to(torch.bfloat16)
    for i, n in enumerate(lens):
        kv[i, n:] = 0
    ref = R.reference(q, kv, hkv, lens)
    yo, yl = torch.zeros_like(ref[0]), torch.zeros_like(ref[1])
    for i, n in enumerate(lens):
        qkv = torch.cat([q[i].expand(n, hq, D), kv[i, :n]], 1)[None].contiguous()
        o, l = mvk._attn_gqa.fwd(qkv, hkv, None, 0.0, 0, None, True)
        yo[i], yl[i] = o[0, n - 1].double().cpu(), l[0, :, n - 1].double().cpu()
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    return q, kv, lens_t, ref, (err(yo, ref[0]), err(yl, ref[1]))


def err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def filled(kv, lens, value):
    kv = kv.clone()
    for i, n in enumerate(lens):
        kv[i, n:] = value
    return kv


@pytest.mark.parametrize("splits", [1, 3, 5, 0])
@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_decode_against_float64(cuda, hq, hkv, lens, splits):
    q, kv, lens_t, ref, yard = case(hq, hkv, lens)
    got = mvk._attn_decode.fwd(q, kv, hkv, lens_t, splits)
    for name, g, r, y, floor in zip(("out", "lse"), got, ref, yard, (2.0 ** -8, 2.0 ** -20)):
        e, bound = err(g, r), max(2 * y, floor)
        print(f"h={hq}/{hkv} lens={lens} splits={splits} {name}: {e:.3g} / {y:.3g}, to bound {e / bound:.3f}")
        assert e <= bound, (name, e, y)


@pytest.mark.parametrize("value", [math.nan, 1e30])
def test_cache_past_lens_is_never_read(cuda, value):
    q, kv, lens_t, _, _ = case(8, 1, LENS[1])
    want = mvk._attn_decode.fwd(q, kv, 1, lens_t, 3)
    got = mvk._attn_decode.fwd(q, filled(kv, LENS[1], value), 1, lens_t, 3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_empty_row_is_dead_and_alone(cuda):
    q, kv, lens_t, _, _ = case(4, 2, LENS[0])
    want = mvk._attn_decode.fwd(q, kv, 2, lens_t)
    lens0 = lens_t.clone()
    lens0[0] = 0
    out, lse = mvk._attn_decode.fwd(q, filled(kv, (0,), math.nan), 2, lens0)
    assert (out[0] == 0).all() and (lse[0] == -math.inf).all()
    assert torch.equal(out[1:], want[0][1:]) and torch.equal(lse[1:], want[1][1:])


def test_two_runs_are_bit_identical(cuda):
    q, kv, lens_t, _, _ = case(16, 1, LENS[0])
    first = mvk._attn_decode.fwd(q, kv, 1, lens_t, 5)
    torch.empty(1 << 24, device=cuda).fill_(math.nan)       # dirty the freed memory (partials)
    assert all(map(torch.equal, mvk._attn_decode.fwd(q, kv, 1, lens_t, 5), first))


def test_decode_attention_op_is_the_binding(cuda):
    from mivod.ops.attention import decode_attention
    q, kv, lens_t, _, _ = case(4, 2, LENS[1])
    y = decode_attention(q, kv, 2, lens_t)
    assert y.shape == (B, 4 * D) and torch.equal(y, mvk._attn_decode.fwd(q, kv, 2, lens_t)[0].view(B, -1))


def test_binding_checks_name_the_operand(cuda):
    q, kv, lens_t, _, _ = case(4, 2, LENS[0])
    with pytest.raises(RuntimeError, match=r"_attn_decode\.fwd: at most 16 query heads per KV head, not 32"):
        mvk._attn_decode.fwd(q.repeat(1, 8, 1), kv[:, :, :2].contiguous(), 1, lens_t)
    with pytest.raises(RuntimeError, match=r"_attn_decode\.fwd: kv_cache's 4 heads must be 2 kv_heads = 2"):
        mvk._attn_decode.fwd(q, kv, 1, lens_t)
    with pytest.raises(RuntimeError, match=r"_attn_decode\.fwd: lens must be a Int GPU tensor"):
        mvk._attn_decode.fwd(q, kv, 2, lens_t.long())
