"""Packed sequences off the kernel path: attention_math's segment mask (any ids, padding
queries 0), the arguments of ops.attention.attention, BertModel(segment_ids=) and
synthetic_batch(segments=)."""
import math

import pytest
import torch

from mivod.models.bert import BertConfig, BertModel, synthetic_batch
from mivod.ops.attention import attention, attention_math, segment_bounds


@pytest.mark.parametrize("ids", [[0, 0, 0, 1, 1, 1, 1, 1, 2], [5, 5, -1, -1, 3, 3, 3, -7, 3],
                                 [1, 0, 1, 0, 1, 0, -1, 0, 1]], ids=["runs", "padding", "interleaved"])
def test_attention_math_masks_by_id_equality(ids):
    """Against float64 attention of each id's tokens alone (gathered, so no mask is involved);
    tokens with a negative id come out exactly 0, never NaN."""
    torch.manual_seed(0)
    b, h, d = 2, 3, 8
    seg = torch.tensor([ids, ids[::-1]])
    s = seg.shape[1]
    qkv = torch.randn(b, s, 3, h, d)
    bias = torch.randn(b, 1, 1, s)
    got = attention_math(qkv, bias, segment_ids=seg).view(b, s, h, d)
    for i in range(b):
        for j in set(seg[i].tolist()):
            idx = (seg[i] == j).nonzero().flatten()
            if j < 0:
                assert (got[i, idx] == 0).all()
                continue
            q, k, v = qkv[i, idx].double().permute(1, 2, 0, 3)                   # [h, n, d]
            sc = q @ k.transpose(-1, -2) / math.sqrt(d) + bias[i, 0, 0, idx].double()
            want = (torch.softmax(sc, -1) @ v).permute(1, 0, 2)
            torch.testing.assert_close(got[i, idx].double(), want, atol=1e-5, rtol=1e-5)


def test_attention_arguments():
    qkv = torch.randn(2, 6, 3, 1, 8)
    seg = torch.tensor([[0, 0, 1, 1, 1, -1]] * 2)
    sb = segment_bounds(seg)
    assert sb.bounds is None                     # no kernels off the GPU: attention_math runs
    assert torch.equal(attention(qkv, segment_bounds=sb), attention_math(qkv, segment_ids=seg))
    assert torch.equal(attention(qkv, segment_ids=seg), attention_math(qkv, segment_ids=seg))
    with pytest.raises(ValueError, match="not both"):
        attention(qkv, segment_ids=seg, segment_bounds=sb)
    with pytest.raises(ValueError, match=r"\[b, s\]"):
        attention(qkv, segment_ids=seg[:, :5])
    with pytest.raises(ValueError, match="int32 or int64"):
        segment_bounds(seg.float())


def test_bert_model_runs_do_not_see_each_other():
    """Run 0's hidden states do not depend on run 1's tokens; without segment_ids they do."""
    torch.manual_seed(1)
    c = BertConfig.tiny()
    model = BertModel(c).eval()
    b, s, cut = 2, 24, 10
    ids_a = torch.randint(0, c.vocab_size, (b, s))
    ids_b = ids_a.clone()
    ids_b[:, cut:] = torch.randint(0, c.vocab_size, (b, s - cut))
    tt = torch.zeros(b, s, dtype=torch.long)
    seg = (torch.arange(s) >= cut).long().expand(b, s)
    with torch.no_grad():
        xa, xb = model(ids_a, tt, segment_ids=seg)[0], model(ids_b, tt, segment_ids=seg)[0]
        da, db = model(ids_a, tt)[0], model(ids_b, tt)[0]
    torch.testing.assert_close(xa[:, :cut], xb[:, :cut], atol=1e-6, rtol=0)
    assert (da[:, :cut] - db[:, :cut]).abs().max() > 1e-3


def test_synthetic_batch_segments():
    c = BertConfig.tiny()
    batch = synthetic_batch(c, 5, 32, "cpu", generator=torch.Generator().manual_seed(0), segments=4)
    assert len(batch) == 7
    seg = batch[-1]
    assert seg.shape == (5, 32) and seg.dtype == torch.int32
    assert (seg[:, 0] == 0).all() and (seg[:, -1] == 3).all()          # 4 runs, each >= 1 token
    assert ((seg[:, 1:] - seg[:, :-1]) >= 0).all() and ((seg[:, 1:] - seg[:, :-1]) <= 1).all()
    assert len(synthetic_batch(c, 5, 32, "cpu", generator=torch.Generator().manual_seed(0))) == 6
