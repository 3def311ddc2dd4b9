"""Causal attention off the kernel path: attention_math(causal=True), with and without
segment_ids, against an explicit float64 masked softmax; a padding query and a query whose
only visible key is at -inf come out exactly 0, never NaN."""
import math

import pytest
import torch

from mivod.ops.attention import attention, attention_math

B, S, H, D = 2, 9, 2, 8


def masked_softmax_ref(qkv, bias, allowed):
    """float64: softmax over the allowed [b, q, k] pairs only, 0 for a query with none."""
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4).unbind(0)                       # [b, h, s, d]
    sc = q @ k.transpose(-1, -2) / math.sqrt(D) + bias.double().reshape(B, 1, 1, S)
    live = allowed[:, None] & torch.isfinite(sc)
    e = torch.where(live, torch.exp(sc - sc.masked_fill(~live, -1e300).amax(-1, keepdim=True)),
                    torch.zeros_like(sc))
    p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    return (p @ v).permute(0, 2, 1, 3)                                            # [b, s, h, d]


@pytest.mark.parametrize("ids", [None, [0, 0, 0, 1, 1, 1, 1, -1, 2]], ids=["dense", "segments"])
def test_attention_math_causal(ids):
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3, H, D)
    bias = torch.randn(B, 1, 1, S)
    bias[1, ..., 0] = -math.inf                      # row 1: query 0 has no key left
    seg = None if ids is None else torch.tensor([ids, ids])
    allowed = torch.ones(S, S, dtype=torch.bool).tril().expand(B, S, S)
    if seg is not None:
        allowed = allowed & (seg[:, :, None] == seg[:, None, :]) & (seg >= 0)[:, None, :]
    got = attention_math(qkv, bias, segment_ids=seg, causal=True).view(B, S, H, D)
    torch.testing.assert_close(got.double(), masked_softmax_ref(qkv, bias, allowed),
                               atol=1e-5, rtol=1e-5)
    assert (got[1, 0] == 0).all()                    # the empty row
    if seg is not None:
        assert (got[:, 7] == 0).all()                # the padding query
    assert torch.equal(attention(qkv, bias, segment_ids=seg, causal=True).view(B, S, H, D), got)
