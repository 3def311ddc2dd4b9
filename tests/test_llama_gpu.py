"""mivod.models.llama in bf16 on the kernel path against the same weights in float64 on the CPU
(the *_math paths).  Yardstick: the same bf16 model with MIVOD_FUSION_OFF=all; per quantity
err_fused <= max(2 err_unfused, 2^-8), err = max |got - ref| / max |ref|.  The ratios measured on
an MI355X are in docs/DECODER_BLOCK.md."""
import copy

import pytest
import torch

from mivod import _mvk as mvk
from mivod.models.llama import LlamaConfig, LlamaForCausalLM

pytestmark = pytest.mark.gpu

B, S = 2, 67
WATCH = {"embedding": lambda m: m.model.embed.weight, "qkv": lambda m: m.model.layers[1].qkv.weight,
         "norm": lambda m: m.model.input_norms[1]}


def step(model, ids):
    model.zero_grad()
    loss = model(ids, labels=ids)
    loss.backward()
    out = {"loss": loss.detach().double().cpu()}
    out.update({k: f(model).grad.detach().double().cpu() for k, f in WATCH.items()})
    return out


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=64, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1,
                      ffn_size=264, max_position=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ids = torch.randint(0, 64, (B, S))
    return copy.deepcopy(model).cuda(), ids, step(copy.deepcopy(model).double(), ids)


def test_llama_step_matches_float64(models, monkeypatch):
    gpu, ids, ref = models
    fused = step(gpu, ids.cuda())
    monkeypatch.setenv("MIVOD_FUSION_OFF", "all")
    unfused = step(gpu, ids.cuda())
    for k, r in ref.items():
        e, u = (float((x[k] - r).abs().max() / r.abs().max()) for x in (fused, unfused))
        bound = max(2 * u, 2.0 ** -8)
        print(f"llama {k}: err fused {e:.3e} unfused {u:.3e} ratio to bound {e / bound:.3f}")
        assert e <= bound, k


def test_llama_step_runs_every_decoder_kernel(models, monkeypatch):
    gpu, ids, _ = models
    calls, real = {}, mvk._decoder

    class Counting:
        def __getattr__(self, name):
            def f(*a, **kw):
                calls[name] = calls.get(name, 0) + 1
                return getattr(real, name)(*a, **kw)
            return f

    monkeypatch.setattr(mvk, "_decoder", Counting())
    step(gpu, ids.cuda())
    # 2 layers: 5 norms (dy and dv_out both reach every backward but the last), 2 MLPs, 2 rotaries
    assert calls == {"rms_fwd": 5, "rms_bwd": 5, "swiglu_fwd": 2, "swiglu_bwd": 2,
                     "rotary_fwd": 2, "rotary_bwd": 2}
