"""The float64 reference of tests/attn_d128_ref.py against attention_math, the project's
documented numerics reference, so that a wrong reference cannot widen the d = 64 yardstick of
tests/test_attn_d128_gpu.py.  attention_math computes its softmax in fp32: 1e-5."""
import torch

import attn_d128_ref as A
from mivod.ops.attention import attention_math


def test_reference_matches_attention_math():
    b, s, h = 2, 17, 3
    t = A.make_inputs(b, s, h, 128, "frac", 0)
    ids = A.make_ids(b, s, [(0, 6), (8, 17)])
    out, lse = A.forward(t["qkv"].double(), t["mask"], A.allowed(b, s, ids, True), None, 0.0)
    want = attention_math(t["qkv"].double(), t["mask"].double(), segment_ids=ids, causal=True)
    torch.testing.assert_close(out.reshape(b, s, -1), want, atol=1e-5, rtol=1e-5)
    assert (out[:, 6:8] == 0).all() and (lse[..., 6:8] == -float("inf")).all()
