"""mivod.ops.linear (BERT's linear layers: hipBLASLt forward and NT data gradient
over the prepared W^T, mivod MFMA weight gradient) against an fp32 PyTorch reference of the same op."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T,nin,nout,bias", [(4096 + 17, 1024, 3072, True),
                                              (2048, 1024, 1024, False),
                                              (1000, 4096, 1024, False),
                                              (333, 1024, 4096, False)])
def test_linear_backward_matches_fp32(cuda, T, nin, nout, bias):
    from mivod.ops import kernels as K
    from mivod.ops.linear import MV_DGRAD, linear
    K.native()
    g = torch.Generator(device=cuda).manual_seed(T + nin + nout)
    x = (torch.rand(1, T, nin, device=cuda, generator=g) * 2 - 1).to(
        torch.bfloat16).requires_grad_()
    w = ((torch.rand(nout, nin, device=cuda, generator=g) * 2 - 1) / nin ** 0.5).to(
        torch.bfloat16).requires_grad_()
    b = (torch.rand(nout, device=cuda, generator=g) * 0.1).to(torch.bfloat16).requires_grad_() \
        if bias else None
    dy = (torch.rand(1, T, nout, device=cuda, generator=g) * 2 - 1).to(torch.bfloat16)
    y = linear(x, w, b)
    y.backward(dy)
    xr, wr = x.detach().float().requires_grad_(), w.detach().float().requires_grad_()
    br = b.detach().float().requires_grad_() if bias else None
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(dy.float())
    rel = lambda a, r: float((a.float() - r).norm() / r.norm())   # noqa: E731
    assert rel(y, yr) < 1e-2
    assert rel(w.grad, wr.grad) < 1e-2, rel(w.grad, wr.grad)
    assert rel(x.grad, xr.grad) < 1e-2, rel(x.grad, xr.grad)
    if bias:
        assert rel(b.grad, br.grad) < 1e-2
    assert not MV_DGRAD     # round 6: every data gradient on hipBLASLt NT over W^T


def test_bert_layer_uses_mivod_weight_gradient(cuda, monkeypatch):
    """The encoder's weight gradients run on mivod's wgrad1x1 (not a silent fallback)."""
    from mivod.models.bert import BertConfig, BertLayer
    from mivod.ops import kernels as K
    nat = K.native()
    calls = []
    real = nat.wgrad1x1

    class Spy:
        def __getattr__(self, n):
            return getattr(nat, n)

        def wgrad1x1(self, *a):
            calls.append(tuple(a[0].shape))
            return real(*a)
    monkeypatch.setattr(K, "native", lambda: Spy())
    c = BertConfig(hidden_size=256, num_attention_heads=4, intermediate_size=1024)
    layer = BertLayer(c).to(cuda).to(torch.bfloat16)
    x = torch.randn(2, 128, 256, device=cuda, dtype=torch.bfloat16, requires_grad=True)
    mask = torch.zeros(2, 1, 1, 128, device=cuda, dtype=torch.bfloat16)
    layer(x, mask).float().sum().backward()
    assert len(calls) == 4, calls            # qkv, attention-out, FFN up, FFN down
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.parameters())


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("T,nin,nout", [(4096 + 17, 4096, 1024), (333, 1024, 256), (2048, 256, 64),
                                        (448, 256, 64)])   # nin 256, T % 224 == 0: 224-row tiles
def test_gelu_linear_fused_backward_matches_fp32(cuda, monkeypatch, T, nin, nout, split):
    """BERT's FFN tail y = gelu(pre + b) W^T: the down projection's data gradient with the
    bias-GELU backward in the GEMM epilogue (mv_gemm256.hip EPI 7; split=True: hipBLASLt's
    dh + the bias_gelu_bwd pass, the round-6 default) — d pre, d b, d W and y against fp32
    PyTorch, and the chosen kernel really ran."""
    from mivod.ops import kernels as K
    from mivod.ops import linear as L
    from mivod.ops.linear import gelu_linear
    monkeypatch.setattr(L, "_GELU_BWD_SPLIT", split)
    nat = K.native()
    calls = []
    name = "bias_gelu_bwd" if split else "gemm_gelu_bwd"
    real = getattr(nat, name)

    class Spy:
        def __getattr__(self, n):
            if n == name:
                def f(*a):
                    calls.append(tuple(a[1].shape if split else a[2].shape))
                    return real(*a)
                return f
            return getattr(nat, n)
    monkeypatch.setattr(K, "native", lambda: Spy())
    g = torch.Generator(device=cuda).manual_seed(T + nin)
    pre = (torch.randn(1, T, nin, device=cuda, generator=g) * 1.5).to(torch.bfloat16).requires_grad_()
    b = (torch.randn(nin, device=cuda, generator=g) * 0.5).to(torch.bfloat16).requires_grad_()
    w = ((torch.rand(nout, nin, device=cuda, generator=g) * 2 - 1) / nin ** 0.5).to(
        torch.bfloat16).requires_grad_()
    dy = (torch.rand(1, T, nout, device=cuda, generator=g) * 2 - 1).to(torch.bfloat16)
    y = gelu_linear(pre, b, w)
    y.backward(dy)
    assert calls == [(T, nin)], calls
    pr, br, wr = (t.detach().float().requires_grad_() for t in (pre, b, w))
    yr = torch.nn.functional.linear(torch.nn.functional.gelu(pr + br), wr)
    yr.backward(dy.float())
    rel = lambda a, r: float((a.float() - r).norm() / r.norm())   # noqa: E731
    assert rel(y, yr) < 1e-2
    assert rel(pre.grad, pr.grad) < 1e-2, rel(pre.grad, pr.grad)
    assert rel(b.grad, br.grad) < 1e-2, rel(b.grad, br.grad)
    assert rel(w.grad, wr.grad) < 1e-2, rel(w.grad, wr.grad)


@pytest.mark.parametrize("M,N", [(65536 + 3, 3072), (5, 1024), (1000, 8),
                                 (9728, 30522), (7, 2), (3, 1030)])
def test_bias_grad_column_sum_vs_fp32(cuda, M, N):
    """Native bias-gradient column sum (mv_bert.hip rowsum_partial + colsum, fixed order;
    rowsum_partial2 for even N not a multiple of 8, e.g. the 30,522-word MLM decoder)
    against a float64 column sum of the same bf16 values; bitwise reproducible."""
    from mivod.ops import kernels as K
    nat = K.native()
    g = torch.Generator(device=cuda).manual_seed(M + N)
    dy = (torch.randn(M, N, device=cuda, generator=g)).to(torch.bfloat16)
    db = nat.bias_grad(dy)
    ref = dy.double().sum(0)
    assert db.dtype == torch.bfloat16 and db.shape == (N,)
    # one bf16 rounding of the result (fp32 accumulation error is far below it)
    torch.testing.assert_close(db.double(), ref, rtol=8e-3, atol=1e-2 * M ** 0.5)
    assert torch.equal(db, nat.bias_grad(dy))


def test_bert_dgrad_weights_prepared_in_one_launch(cuda, monkeypatch):
    """A training forward of BertModel makes the W^T of every encoder projection (QKV,
    attention output, FFN up / down) in ONE transpose launch and the backward uses them:
    gradients bitwise equal to the per-layer transpose-copy path."""
    import mivod.models.bert as B
    from mivod.ops import kernels as K
    nat = K.native()
    launches = []
    real = nat.transpose_filters

    class Spy:
        def __getattr__(self, n):
            return getattr(nat, n)

        def transpose_filters(self, ws):
            launches.append(len(ws))
            return real(ws)
    monkeypatch.setattr(K, "native", lambda: Spy())
    c = B.BertConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                     intermediate_size=1024, max_position_embeddings=128)
    torch.manual_seed(0)
    model = B.BertModel(c).to(cuda).to(torch.bfloat16).train()
    ids = torch.randint(0, c.vocab_size, (2, 128), device=cuda)
    tt = torch.zeros_like(ids)

    def grads():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)                       # same dropout seeds in both runs
        x, pooled = model(ids, tt)
        (x.float().square().mean() + pooled.float().sum()).backward()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    g1 = grads()
    assert launches == [4 * c.num_hidden_layers], launches
    monkeypatch.setattr(B, "prepare_dgrad_weights", lambda ws: None)
    g0 = grads()
    assert launches == [4 * c.num_hidden_layers]
    assert g1.keys() == g0.keys()
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


def test_mlm_decoder_linear_bias_grad_native(cuda):
    """linear() on a width that is not a multiple of 64 (the tied MLM decoder): hipBLASLt
    GEMMs as autograd issues them, the bias gradient from the native column sum — all three
    gradients vs fp32."""
    from mivod.ops.linear import linear
    g = torch.Generator(device=cuda).manual_seed(30522)
    x = (torch.randn(300, 256, device=cuda, generator=g)).to(torch.bfloat16).requires_grad_()
    w = (torch.randn(1030, 256, device=cuda, generator=g) / 16).to(torch.bfloat16).requires_grad_()
    b = (torch.randn(1030, device=cuda, generator=g) * 0.1).to(torch.bfloat16).requires_grad_()
    dy = torch.randn(300, 1030, device=cuda, generator=g).to(torch.bfloat16)
    linear(x, w, b).backward(dy)
    xr, wr, br = (t.detach().float().requires_grad_() for t in (x, w, b))
    torch.nn.functional.linear(xr, wr, br).backward(dy.float())
    for t, r in ((x, xr), (w, wr), (b, br)):
        rel = float((t.grad.float() - r.grad).norm() / r.grad.norm())
        assert rel < 1e-2, rel


@pytest.mark.parametrize("N", [1024, 30522])
def test_bias_grad_misaligned_view(cuda, N):
    """A dy view at a 2-byte offset (not 16- / 4-byte aligned for the vector loads) is
    summed from an aligned copy: same result as the aligned tensor."""
    from mivod.ops import kernels as K
    nat = K.native()
    M = 37
    g = torch.Generator(device=cuda).manual_seed(N)
    base = torch.randn(M * N + 1, device=cuda, generator=g).to(torch.bfloat16)
    dy = base[1:].view(M, N)
    assert dy.data_ptr() % 4 != 0
    assert torch.equal(nat.bias_grad(dy), nat.bias_grad(dy.clone()))
