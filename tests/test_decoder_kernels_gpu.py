"""The decoder-block kernels (csrc/kernels/mv_decoder.hip) through mivod._mvk._decoder against the
float64 formulas of tests/decoder_reference.py on the same bf16 inputs.

err = max |got - ref| / max |ref| per tensor.  y, v, swiglu's y / dx and rotary's outputs are one
bf16 rounding of an fp32-accurate value: err <= 2^-8 (twice the rounding bound 2^-9, the floor of
the attention tests).  add_rms_norm's dv and dw depend on the stored, rounded v, so they are held
against add_rms_norm_math run in bf16 on the same inputs: err_kernel <= max(2 err_math, 2^-8) —
the kernel rounds strictly less often than the eager composition, and the maxima over elements of
two like-distributed errors rarely differ by more than 2.  The worst ratios measured on an MI355X
are in docs/DECODER_BLOCK.md."""
import pytest
import torch

import decoder_reference as R
from mivod import _mvk as mvk
from mivod.ops import decoder as ops

pytestmark = pytest.mark.gpu

D = mvk._decoder
FLOOR = 2.0 ** -8
EPS = 1e-6


def bf16(*shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(torch.bfloat16)


def err(got, ref):
    if ref is None:                  # an unused input: the gradient must be exactly zero
        return float(got.double().abs().max())
    ref = ref.detach()
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-300))


def grads(f, xs, couts, dtype):
    xs = [x.detach().clone().to(dtype).requires_grad_() for x in xs]
    outs = f(*xs)
    outs, couts = zip(*[(o, c.to(dtype)) for o, c in zip(outs, couts) if c is not None])
    return torch.autograd.grad(outs, xs, couts, allow_unused=True)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M", [1, 67])
@pytest.mark.parametrize("H", [8, 520, 4096, 8192])
def test_add_rms_norm(H, M, with_res):
    z, w = bf16(M, H, seed=1, scale=2.0), bf16(H, seed=3) + 1
    res = bf16(M, H, seed=2, scale=2.0) if with_res else None
    y, v, rstd = D.rms_fwd(z, res, w, EPS)
    ry, rv = R.add_rms_norm(z, res, w, EPS)
    assert with_res or v.data_ptr() == z.data_ptr()
    for name, got, ref in (("y", y, ry), ("v", v, rv)):
        e = err(got, ref)
        print(f"rms H={H} M={M} res={with_res} {name}: err {e:.3e} = {e / FLOOR:.3f} floor")
        assert e <= FLOOR, name
    assert err(rstd, torch.rsqrt((rv * rv).mean(-1) + EPS)) <= 2.0 ** -20
    xs = [z, w] + ([res] if with_res else [])
    f = lambda fn: lambda z, w, r=None: fn(z, r, w, EPS)
    for mode, dy, dvo in (("both", bf16(M, H, seed=4), bf16(M, H, seed=5)),
                          ("dy", bf16(M, H, seed=4), None), ("dv_out", None, bf16(M, H, seed=5))):
        dv, dw = D.rms_bwd(dy, dvo, v, rstd, w)
        ref = grads(f(R.add_rms_norm), xs, (dy, dvo), torch.float64)
        math = grads(f(ops.add_rms_norm_math), xs, (dy, dvo), torch.bfloat16)
        if with_res:                 # z and res share one gradient
            assert torch.equal(ref[0], ref[2])
        for name, got, i in (("dv", dv, 0), ("dw", dw, 1)):
            e = err(got, ref[i])
            bound = max(2 * err(math[i], ref[i]), FLOOR) if ref[i] is not None else 0.0
            print(f"rms H={H} M={M} res={with_res} {mode} {name}: err {e:.3e} bound {bound:.3e} "
                  f"ratio {e / bound if bound else 0:.3f}")
            assert e <= bound, (mode, name)


@pytest.mark.parametrize("M", [1, 67])
@pytest.mark.parametrize("N", [8, 264, 2056])
def test_swiglu(N, M):
    x, dy = bf16(M, 2 * N, seed=1, scale=3.0), bf16(M, N, seed=2)
    xr = x.double().requires_grad_()
    ry = R.swiglu(xr)
    (rdx,) = torch.autograd.grad(ry, xr, dy.double())
    for name, got, ref in (("y", D.swiglu_fwd(x), ry), ("dx", D.swiglu_bwd(dy, x), rdx)):
        e = err(got, ref)
        print(f"swiglu N={N} M={M} {name}: err {e:.3e} = {e / FLOOR:.3f} floor")
        assert e <= FLOOR, name


@pytest.mark.parametrize("given_pos", [False, True])
@pytest.mark.parametrize("hq,hkv", [(4, 2), (3, 1), (2, 2)])
@pytest.mark.parametrize("s", [1, 67])
def test_rotary(s, hq, hkv, given_pos):
    P = 80
    cos, sin = ops.rotary_tables(P, device="cuda")
    pos = None
    if given_pos:                    # row 0 restarts mid-row, row 1 ends at the last table row
        t = torch.arange(s, device="cuda")
        pos = torch.stack([t % 29, t + (P - s)]).to(torch.int32)
    x, dout = bf16(2, s, hq + 2 * hkv, 128, seed=1, scale=2.0), bf16(2, s, hq + 2 * hkv, 128, seed=2)
    xr = x.double().requires_grad_()
    rout = R.rotary(xr, hkv, cos, sin, pos)
    (rdx,) = torch.autograd.grad(rout, xr, dout.double())
    out, dx = D.rotary_fwd(x, hkv, cos, sin, pos), D.rotary_bwd(dout, hkv, cos, sin, pos)
    for name, got, ref, src in (("out", out, rout, x), ("dqkv", dx, rdx, dout)):
        e = err(got, ref)
        print(f"rotary s={s} hq={hq} hkv={hkv} pos={given_pos} {name}: err {e:.3e} = {e / FLOOR:.3f} floor")
        assert e <= FLOOR, name
        assert torch.equal(got[:, :, hq + hkv:], src[:, :, hq + hkv:]), name + ": value heads"


@pytest.mark.parametrize("H", [520, 8192])
def test_rms_bwd_is_deterministic(H):
    M = 67
    z, res, w = bf16(M, H, seed=1), bf16(M, H, seed=2), bf16(H, seed=3)
    dy, dvo = bf16(M, H, seed=4), bf16(M, H, seed=5)
    y, v, rstd = D.rms_fwd(z, res, w, EPS)
    first = D.rms_bwd(dy, dvo, v, rstd, w)
    junk = [torch.full((n,), float("nan"), device="cuda") for n in (M * H, 3 * H, 7 * H)]
    del junk                         # the next partial rows land in dirtied blocks
    again = D.rms_bwd(dy, dvo, v, rstd, w)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_public_ops_equal_the_bindings():
    M, H, N = 67, 520, 264
    z, res, w = (t.requires_grad_() for t in (bf16(M, H, seed=1), bf16(M, H, seed=2), bf16(H, seed=3)))
    dy, dvo = bf16(M, H, seed=4), bf16(M, H, seed=5)
    y, v, rstd = D.rms_fwd(z, res, w, EPS)
    dv, dw = D.rms_bwd(dy, dvo, v, rstd, w)
    got = ops.add_rms_norm(z, res, w, EPS)
    want = (y, v, dv, dv, dw)
    for a, b in zip(got + torch.autograd.grad(got, (z, res, w), (dy, dvo)), want):
        assert torch.equal(a, b)
    x, dyn = bf16(M, 2 * N, seed=6).requires_grad_(), bf16(M, N, seed=7)
    ys = ops.swiglu(x)
    assert torch.equal(ys, D.swiglu_fwd(x))
    assert torch.equal(torch.autograd.grad(ys, x, dyn)[0], D.swiglu_bwd(dyn, x))
    cos, sin = ops.rotary_tables(80, device="cuda")
    pos = (torch.arange(67, device="cuda") % 13).expand(2, 67)
    q, dq = bf16(2, 67, 5, 128, seed=8).requires_grad_(), bf16(2, 67, 5, 128, seed=9)
    out = ops.rotary(q, 1, cos, sin, pos)
    assert torch.equal(out, D.rotary_fwd(q, 1, cos, sin, pos.int().contiguous()))
    assert torch.equal(torch.autograd.grad(out, q, dq)[0],
                       D.rotary_bwd(dq, 1, cos, sin, pos.int().contiguous()))


def _tables(width=64, rows=8):
    return torch.zeros(rows, width, device="cuda"), torch.zeros(rows, width, device="cuda")


@pytest.mark.parametrize("call, match", [
    (lambda: D.rms_fwd(bf16(2, 8200, seed=0), None, bf16(8200, seed=0), EPS), "rms_fwd: hidden size"),
    (lambda: D.rms_fwd(bf16(2, 12, seed=0), None, bf16(12, seed=0), EPS), "rms_fwd: hidden size"),
    (lambda: D.rms_bwd(bf16(2, 12, seed=0), None, bf16(2, 12, seed=0), torch.ones(2, device="cuda"),
                       bf16(12, seed=0)), "rms_bwd: hidden size"),
    (lambda: D.swiglu_fwd(bf16(2, 24, seed=0)), "swiglu_fwd: x must be"),
    (lambda: D.swiglu_bwd(bf16(2, 12, seed=0), bf16(2, 24, seed=0)), "swiglu_bwd: x must be"),
    (lambda: D.rotary_fwd(bf16(1, 2, 3, 64, seed=0), 1, *_tables()), "rotary_fwd: qkv must be"),
    (lambda: D.rotary_fwd(bf16(1, 2, 7, 128, seed=0), 2, *_tables()), "rotary_fwd: qkv's 7 heads"),
    (lambda: D.rotary_bwd(bf16(1, 2, 3, 128, seed=0), 1, *_tables(width=32)), "rotary_bwd: cos and sin"),
    (lambda: D.rotary_fwd(bf16(1, 9, 3, 128, seed=0), 1, *_tables()), "rotary_fwd: 9 positions"),
])
def test_binding_checks(call, match):
    with pytest.raises(RuntimeError, match=match):
        call()
