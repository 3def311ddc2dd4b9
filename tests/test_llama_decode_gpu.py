"""LlamaForCausalLM.generate in bf16 on the kernel path: the logits every new token is taken from
against the float64 CPU full forward on the extended sequence.  Yardstick: the bf16 kernel-path
full forward on the same sequence; err_decode <= max(2 err_full, 2^-8), err = max |got - ref| /
max |ref|.  Prompt 62 + 4 tokens: the first comes from the prefill, the 3 decode steps see 63, 64
and 65 keys, across a 64-key block.  The ratio measured on an MI355X is in
docs/ATTENTION_DECODE.md."""
import copy

import pytest
import torch

from mivod import _mvk as mvk
from mivod.models.llama import LlamaConfig, LlamaForCausalLM

pytestmark = pytest.mark.gpu

B, S, NEW = 2, 62, 4


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1,
                      ffn_size=264, max_position=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    return copy.deepcopy(model).cuda(), copy.deepcopy(model).double(), torch.randint(0, 64, (B, S))


def test_decode_logits_match_float64(models):
    gpu, cpu, ids = models
    seq, logits = gpu.generate(ids.cuda(), NEW, return_logits=True)
    assert seq.shape == (B, S + NEW) and torch.equal(seq[:, S:], logits.argmax(-1))
    with torch.no_grad():
        ref = cpu.logits(seq.cpu())[:, S - 1:S + NEW - 1]
        full = gpu.logits(seq)[:, S - 1:S + NEW - 1]
    e, y = (float((x.double().cpu() - ref).abs().max() / ref.abs().max()) for x in (logits, full))
    bound = max(2 * y, 2.0 ** -8)
    print(f"llama decode logits: err {e:.3e} full forward {y:.3e} ratio to bound {e / bound:.3f}")
    assert e <= bound


def test_generate_runs_the_decode_kernel(models, monkeypatch):
    gpu, _, ids = models
    calls, real = {}, mvk._attn_decode

    class Counting:
        def __getattr__(self, name):
            def f(*a, **kw):
                calls[name] = calls.get(name, 0) + 1
                return getattr(real, name)(*a, **kw)
            return f

    monkeypatch.setattr(mvk, "_attn_decode", Counting())
    gpu.generate(ids.cuda(), NEW)
    assert calls == {"fwd": 2 * (NEW - 1)}          # per layer and decode step
