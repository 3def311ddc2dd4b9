"""CPU tier of KV-cache decoding: decode_attention_math against the float64 formula, and
LlamaForCausalLM.generate on the math paths against a loop of full forwards."""
import math

import pytest
import torch

import attn_decode_ref as R
from mivod.models.llama import LlamaConfig, LlamaForCausalLM
from mivod.ops.attention import decode_attention, decode_attention_math

TOL = 1e-4          # fp32 logits, decode step against full forward


@pytest.mark.parametrize("hq,hkv", [(4, 2), (8, 1), (3, 3)])
def test_decode_attention_math_is_the_formula(hq, hkv):
    g = torch.Generator().manual_seed(hq)
    q = torch.randn(3, hq, 32, dtype=torch.float64, generator=g)
    kv = torch.randn(3, 70, 2 * hkv, 32, dtype=torch.float64, generator=g)
    lens = torch.tensor([1, 0, 70], dtype=torch.int32)
    kv[0, 1:] = math.nan                      # nothing at or past lens has any influence
    out, _ = R.reference(q, kv, hkv, lens)
    got = decode_attention_math(q, kv, hkv, lens)
    assert float((got.view_as(out) - out).abs().max()) <= 1e-12
    assert torch.equal(decode_attention(q, kv, hkv, lens), got)          # off the kernel path


def test_generate_is_a_loop_of_full_forwards():
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1,
                      ffn_size=264, max_position=16)
    model = LlamaForCausalLM(cfg)
    ids = torch.randint(0, 64, (2, 5))
    seq, logits = model.generate(ids, 6, return_logits=True)
    want = ids
    with torch.no_grad():
        for t in range(6):
            full = model.logits(want)[:, -1]
            top = full.topk(2, dim=-1).values
            # the argmax is no coin flip: both candidates would have to move by more than TOL
            assert float((top[:, 0] - top[:, 1]).min()) > 2 * TOL
            assert float((logits[:, t] - full).abs().max()) <= TOL
            want = torch.cat([want, full.argmax(-1, keepdim=True)], 1)
    assert torch.equal(seq, want)
    # a full cache ends generation: max_position 16 holds the prompt and 11 more tokens, and the
    # token taken from the last cached position is still returned
    assert model.generate(ids, 20).shape == (2, 17)
    assert torch.equal(model.generate(ids, 20, eos_token_id=int(seq[0, 5]))[0, 5:].unique(), seq[0, 5:6])
