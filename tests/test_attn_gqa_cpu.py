"""grouped_attention off the kernel path (CPU, fp32): it equals attention_math on the tensor whose
K / V heads are repeated G times, and its autograd dK / dV are that tensor's, summed per group."""
import pytest
import torch

import attn_d128_ref as A
from mivod.ops.attention import attention_math, grouped_attention

B, S, HQ, HKV, D = 2, 17, 6, 2, 16
G = HQ // HKV


@pytest.mark.parametrize("mode", ["dense", "seg+causal"])
def test_grouped_attention_is_attention_on_the_expansion(mode):
    t = A.make_inputs(B, S, HQ, D, "frac", 0)
    kw = {} if mode == "dense" else {"causal": True, "segment_ids": A.make_ids(B, S, [(0, 7), (9, 17)])}
    q, k, v = t["qkv"].float().unbind(2)
    k, v = k[:, :, ::G], v[:, :, ::G]
    grouped = torch.cat([q, k, v], 2).requires_grad_()
    expanded = torch.stack([q, k.repeat_interleave(G, 2), v.repeat_interleave(G, 2)], 2).requires_grad_()
    y = grouped_attention(grouped, HKV, t["mask"], **kw)
    want = attention_math(expanded, t["mask"], **kw)
    torch.testing.assert_close(y, want, atol=1e-6, rtol=1e-6)
    dout = t["dout"].float().view(B, S, -1)
    y.backward(dout)
    want.backward(dout)
    dq, dk, dv = expanded.grad.unbind(2)
    sums = [dq] + [x.view(B, S, HKV, G, D).sum(3) for x in (dk, dv)]
    torch.testing.assert_close(grouped.grad, torch.cat(sums, 2), atol=1e-5, rtol=1e-5)


def test_heads_must_divide():
    with pytest.raises(ValueError, match="no multiple of kv_heads"):
        grouped_attention(torch.zeros(1, 4, 5 + 4, 16), 2)
