"""The decoder-block ops off the kernel path (ops/decoder.py *_math) against the float64 formulas of
tests/decoder_reference.py, and mivod.models.llama on the CPU."""
import pytest
import torch

import decoder_reference as R
from mivod.models.llama import LlamaConfig, LlamaForCausalLM
from mivod.ops.decoder import (add_rms_norm, add_rms_norm_math, rotary, rotary_math, rotary_tables,
                               swiglu_math)

TINY = dict(vocab_size=64, hidden_size=256, num_layers=2, num_heads=2, num_kv_heads=1, ffn_size=264,
            max_position=32)


def rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def close(got, want):
    torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12)


def both(f_math, f_ref, inputs, couts):
    """Outputs and autograd gradients (cotangents ``couts``) of the two functions."""
    res = []
    for f in (f_math, f_ref):
        xs = [x.clone().requires_grad_() for x in inputs]
        outs = f(*xs)
        outs = outs if isinstance(outs, tuple) else (outs,)
        res.append(list(outs) + list(torch.autograd.grad(outs, xs, couts)))
    for a, b in zip(*res):
        close(a, b)


@pytest.mark.parametrize("with_res", [True, False])
def test_add_rms_norm_math(with_res):
    z, r, w = rand(5, 24), rand(5, 24, seed=1), rand(24, seed=2)
    couts = (rand(5, 24, seed=3), rand(5, 24, seed=4))
    if with_res:
        both(lambda z, r, w: add_rms_norm_math(z, r, w, 1e-5), lambda z, r, w: R.add_rms_norm(z, r, w, 1e-5),
             [z, r, w], couts)
    else:
        both(lambda z, w: add_rms_norm_math(z, None, w, 1e-5), lambda z, w: R.add_rms_norm(z, None, w, 1e-5),
             [z, w], couts)


def test_swiglu_math():
    both(swiglu_math, R.swiglu, [rand(5, 48) * 3], (rand(5, 24, seed=1),))


@pytest.mark.parametrize("given_pos", [False, True])
def test_rotary_math(given_pos):
    cos, sin = rotary_tables(16)
    pos = torch.tensor([[0, 1, 2, 0, 1, 0, 15], [3, 4, 0, 1, 2, 3, 4]]) if given_pos else None
    x, y = rand(2, 7, 5, 128), rand(2, 7, 5, 128, seed=1)
    both(lambda t: rotary_math(t, 1, cos, sin, pos), lambda t: R.rotary(t, 1, cos, sin, pos), [x], (y,))
    rx = rotary(x, 1, cos, sin, pos)
    # a rotation of every (i, i + 64) pair: the pair's norm is kept (as far as cos^2 + sin^2 of the
    # fp32 tables is 1: 4 roundings of 2^-24), the value head untouched
    torch.testing.assert_close(rx[:, :, :4, :64] ** 2 + rx[:, :, :4, 64:] ** 2,
                               x[:, :, :4, :64] ** 2 + x[:, :, :4, 64:] ** 2, atol=0, rtol=2.0 ** -22)
    assert torch.equal(rx[:, :, 4], x[:, :, 4])
    # the backward is the adjoint: <R x, y> == <x, R^T y>
    xg = x.clone().requires_grad_()
    (rty,) = torch.autograd.grad(rotary(xg, 1, cos, sin, pos), xg, y)
    close((rx * y).sum(), (x * rty).sum())


def test_rotary_rejects():
    cos, sin = rotary_tables(4)
    with pytest.raises(ValueError, match="no multiple of kv_heads"):
        rotary(torch.zeros(1, 2, 3 + 4, 128), 2, cos, sin)
    with pytest.raises(ValueError, match="positions need tables"):
        rotary(torch.zeros(1, 5, 3, 128), 1, cos, sin)


def test_add_rms_norm_one_sided_gradients():
    z, r, w = (t.requires_grad_() for t in (rand(3, 16), rand(3, 16, seed=1), rand(16, seed=2)))
    y, v = add_rms_norm(z, r, w)
    (dz,) = torch.autograd.grad(v.sum(), z, retain_graph=True)       # y unused
    close(dz, torch.ones_like(z))
    assert torch.autograd.grad(y.sum(), w)[0].abs().sum() > 0         # v unused


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig(**TINY)), torch.randint(0, 64, (2, 19))


def test_llama_forward_backward(tiny):
    model, ids = tiny
    loss = model(ids, labels=ids)
    loss.backward()
    assert abs(loss.item() - 4.16) < 0.3                                # ln(64) at initialisation
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
    model.zero_grad()


def test_llama_packed_segment_equals_alone(tiny):
    """The second of two packed segments sees neither the first one nor its positions."""
    model, ids = tiny
    seg = torch.zeros(2, 19, dtype=torch.int64)
    seg[:, 8:] = 1
    with torch.no_grad():
        packed, alone, unsegmented = model(ids, segment_ids=seg), model(ids[:, 8:]), model(ids)
    torch.testing.assert_close(packed[:, 8:], alone, atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(packed[:, :8], unsegmented[:, :8], atol=2e-5, rtol=1e-4)    # causal
    assert (unsegmented[:, 8:] - alone).abs().max() > 1e-3
