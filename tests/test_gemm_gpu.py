"""mivod's MFMA NT GEMM (csrc/kernels/mv_gemm.hip) for NHWC 1x1 convolutions and
its fused BN-statistics epilogue, against fp32 PyTorch references; and the fused
conv1x1 -> BN path (ops.bn.conv_bn) against the unfused composition."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _nat():
    from mivod.ops import kernels as K
    return K.native()


@pytest.mark.parametrize("K,N", [(64, 64), (64, 256), (128, 512), (256, 64), (256, 128),
                                 (512, 128), (512, 256), (1024, 512)])
@pytest.mark.parametrize("M", [1, 63, 64 * 7 + 5, 4096 + 17])
def test_gemm_nt_matches_fp32(cuda, M, K, N):
    nat = _nat()
    g = torch.Generator(device=cuda).manual_seed(M * 7 + K + N)
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    c = torch.full((M, N), float("nan"), device=cuda).to(torch.bfloat16)
    shift = torch.randn(N, device=cuda, generator=g) * 0.1
    P = nat.gemm_partials(M, N, K)
    part = torch.full((P, 2, N), float("nan"), device=cuda)
    nat.gemm_nt(a, b, c, shift, part)
    ref = a.float() @ b.float().t()
    torch.testing.assert_close(c.float(), ref, rtol=1e-2, atol=1e-2 * ref.abs().max().item())
    # statistics of the bf16-ROUNDED output around shift, every partial row written
    d = c.float() - shift
    s = part.sum(0)
    assert torch.isfinite(part).all()
    torch.testing.assert_close(s[0], d.sum(0), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(s[1], (d * d).sum(0), rtol=1e-4, atol=1e-3)
    # plain variant writes the same C
    c2 = torch.empty_like(c)
    nat.gemm_nt(a, b, c2, None, None)
    assert torch.equal(c, c2)


@pytest.mark.parametrize("M,K,N", [(256 * 700 + 37, 64, 256), (153637, 512, 512),
                                   (300000, 256, 1024), (4096, 2048, 2048), (255, 128, 256),
                                   # M % 224 == 0: 224-row blocks (MT = 7)
                                   (224 * 300, 1024, 256), (224 * 5, 256, 1024),
                                   (224 * 1000, 512, 512)])
def test_gemm256_persistent_matches_fp32(cuda, M, K, N):
    """mv_gemm256.hip: several output tiles per persistent workgroup (the next tile's
    first K tile staged during the previous epilogue), a ragged last row block, a single
    K tile (K = 64); via gemm_nt (with statistics) where gemm_nt routes to it."""
    nat = _nat()
    g = torch.Generator(device=cuda).manual_seed(M + K + N)
    a = (torch.rand(M, K, device=cuda, generator=g) * 2 - 1).to(torch.bfloat16)
    b = ((torch.rand(N, K, device=cuda, generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
    c = torch.full((M, N), float("nan"), device=cuda).to(torch.bfloat16)
    nat.gemm256_nt(a, b, c)
    ref = a.float() @ b.float().t()
    torch.testing.assert_close(c.float(), ref, rtol=1e-2, atol=1e-2 * ref.abs().max().item())
    c2 = torch.empty_like(c)
    nat.gemm256_nt(a, b, c2)
    assert torch.equal(c, c2)
    if K >= 512 or (K == 256 and N >= 1024):
        shift = torch.randn(N, device=cuda, generator=g) * 0.1
        part = torch.full((nat.gemm_partials(M, N, K), 2, N), float("nan"), device=cuda)
        c3 = torch.empty_like(c)
        nat.gemm_nt(a, b, c3, shift, part)
        assert torch.equal(c3, c)
        d = c.float() - shift
        s = part.sum(0)
        torch.testing.assert_close(s[0], d.sum(0), rtol=1e-4, atol=1e-2)
        torch.testing.assert_close(s[1], (d * d).sum(0), rtol=1e-4, atol=1e-2)
        if K == 256:                 # statistics only (C = None): the same partials
            part2 = torch.full_like(part, float("nan"))
            nat.gemm_nt(a, b, None, shift, part2)
            assert torch.equal(part2, part)


def test_gemm_nt_rejects_bad_shapes(cuda):
    nat = _nat()
    a = torch.zeros(8, 96, device=cuda, dtype=torch.bfloat16)
    b = torch.zeros(64, 96, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        nat.gemm_nt(a, b, torch.zeros(8, 64, device=cuda, dtype=torch.bfloat16), None, None)


def test_conv_bn_fused_matches_unfused(cuda, monkeypatch):
    """conv1x1 -> BN(+residual)(+ReLU) with GEMM-epilogue statistics: same forward
    output, running statistics and gradients as the unfused path (to bf16 rounding)."""
    import copy

    from mivod.ops.bn import BatchNorm2d, conv_bn
    from mivod.ops.conv import Conv2d
    torch.manual_seed(0)
    for cin, cout, res in ((64, 256, True), (256, 64, False), (128, 512, True)):
        conv = Conv2d(cin, cout, 1, bias=False).to(cuda).to(torch.bfloat16).to(
            memory_format=torch.channels_last)
        bn = BatchNorm2d(cout).to(cuda)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2)
        x0 = torch.randn(4, cin, 14, 14, device=cuda).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)
        r0 = torch.randn(4, cout, 14, 14, device=cuda).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last) if res else None
        outs = []
        for fuse in ("1", "0"):
            monkeypatch.setenv("MIVOD_FUSION_OFF", "" if fuse == "1" else "gemm")
            c2, b2 = copy.deepcopy(conv), copy.deepcopy(bn)
            x = x0.clone().requires_grad_()
            y = conv_bn(c2, b2, x, relu=True, residual=r0)
            y.float().square().mean().backward()
            outs.append((y.detach().float(), x.grad.float(), c2.weight.grad.float(),
                         b2.weight.grad, b2.running_mean.clone(), b2.running_var.clone()))
        (yf, dxf, dwf, dgf, rmf, rvf), (yu, dxu, dwu, dgu, rmu, rvu) = outs
        torch.testing.assert_close(rmf, rmu, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(rvf, rvu, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(yf, yu, rtol=2e-2, atol=2e-2)
        for a, b in ((dxf, dxu), (dwf, dwu), (dgf, dgu)):
            torch.testing.assert_close(a, b, rtol=5e-2, atol=5e-2 * float(b.abs().max()))
    os.environ.pop("MIVOD_FUSION_OFF", None)


def test_resnet_uses_gemm_stats_path(cuda):
    """The bottleneck's qualifying 1x1 convs run through _Conv1x1BN."""
    from mivod.models.resnet import ResNet, to_mixed_bf16
    m = to_mixed_bf16(ResNet((1, 1, 1, 1), num_classes=10)).to(cuda)
    x = torch.rand(2, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    out = m(x)
    names, seen, stack = set(), set(), [out.grad_fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        stack.extend(nf for nf, _ in f.next_functions)
    assert any("Conv1x1BN" in n for n in names), names


def _unpack_mask(mask, N):
    bits = torch.arange(8, device=mask.device)
    return ((mask.long().unsqueeze(-1) >> bits) & 1).reshape(mask.shape[0], N).bool()


@pytest.mark.parametrize("K,N", [(64, 64), (64, 256), (128, 128), (128, 512), (256, 64),
                                 (256, 1024)])
@pytest.mark.parametrize("M", [1, 64 * 3 + 5, 4096 + 17])
@pytest.mark.parametrize("with_dy2", [True, False])
def test_gemm_nt_bn_bwd_matches_fp32(cuda, M, K, N, with_dy2):
    """dz = mask ? bf16(a . b^T) + dy2 : 0 and the (sum dz, sum dz (x - mean)) partials."""
    nat = _nat()
    g = torch.Generator(device=cuda).manual_seed(M + 3 * K + N)
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    x = torch.randn(M, N, device=cuda, generator=g).to(torch.bfloat16)
    vec = torch.randn(4, N, device=cuda, generator=g)
    mask = torch.randint(0, 256, (M, N // 8), device=cuda, generator=g, dtype=torch.int32).to(
        torch.uint8)
    dy2 = (torch.randn(M, N, device=cuda, generator=g).to(torch.bfloat16)
           if with_dy2 else None)
    dz = torch.full((M, N), float("nan"), device=cuda).to(torch.bfloat16)
    part = nat.gemm_nt_bn_bwd(a, b, dz, dy2, mask, x, vec)
    assert part.shape == (nat.gemm_bwd_partials(M, N, K), 2, N)
    dyb = (a.float() @ b.float().t()).to(torch.bfloat16).float()
    d = dyb + (dy2.float() if with_dy2 else 0.0)
    d = torch.where(_unpack_mask(mask, N), d, torch.zeros_like(d))
    torch.testing.assert_close(dz.float(), d, rtol=2e-2, atol=2e-2)
    assert torch.isfinite(part).all()
    s = part.sum(0)
    torch.testing.assert_close(s[0], d.sum(0), rtol=1e-2, atol=1e-2 * (M ** 0.5))
    torch.testing.assert_close(s[1], (d * (x.float() - vec[0])).sum(0), rtol=1e-2,
                               atol=3e-2 * (M ** 0.5))
    assert (dz.float()[~_unpack_mask(mask, N)] == 0).all()


@pytest.mark.parametrize("H,W,ds", [(8, 8, 2), (7, 9, 2), (5, 5, 3)])
def test_gemm_nt_bn_bwd_strided_dy2(cuda, H, W, ds):
    """dy2 on the stride-ds grid is added at rows whose (h, w) are multiples of ds."""
    nat = _nat()
    n, K, N = 3, 128, 256
    M = n * H * W
    g = torch.Generator(device=cuda).manual_seed(H * 100 + W + ds)
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    x = torch.randn(M, N, device=cuda, generator=g).to(torch.bfloat16)
    vec = torch.randn(4, N, device=cuda, generator=g)
    mask = torch.randint(0, 256, (M, N // 8), device=cuda, generator=g, dtype=torch.int32).to(
        torch.uint8)
    hs, ws = (H + ds - 1) // ds, (W + ds - 1) // ds
    dy2 = torch.randn(n, N, hs, ws, device=cuda, generator=g).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    dz = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
    part = nat.gemm_nt_bn_bwd(a, b, dz, dy2, mask, x, vec, 0, ds, H, W)
    full = torch.zeros(n, N, H, W, device=cuda)
    full[:, :, ::ds, ::ds] = dy2.float()
    d = (a.float() @ b.float().t()).to(torch.bfloat16).float() + full.permute(0, 2, 3, 1).reshape(M, N)
    d = torch.where(_unpack_mask(mask, N), d, torch.zeros_like(d))
    torch.testing.assert_close(dz.float(), d, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(part.sum(0)[0], d.sum(0), rtol=1e-2, atol=1e-1)


def test_gemm_nt_bn_bwd_rejects_unsupported(cuda):
    nat = _nat()
    M, K, N = 64, 512, 128          # K = 512: no streaming kernel
    z = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        nat.gemm_nt_bn_bwd(z(M, K), z(N, K), z(M, N), None,
                           torch.zeros(M, N // 8, device=cuda, dtype=torch.uint8), z(M, N),
                           torch.zeros(4, N, device=cuda))
    with pytest.raises(RuntimeError):   # mask of the wrong size
        nat.gemm_nt_bn_bwd(z(M, 64), z(N, 64), z(M, N), None,
                           torch.zeros(M, N // 16, device=cuda, dtype=torch.uint8), z(M, N),
                           torch.zeros(4, N, device=cuda))


def test_bn_bwd_from_partials_matches_bn_bwd(cuda):
    """finalize + dx from GEMM-epilogue partials == the mode-3 BN backward on the same dy."""
    from mivod.ops.bn import BatchNorm2d
    nat = _nat()
    torch.manual_seed(1)
    n, c, h, w, k = 8, 256, 14, 14, 64
    bn = BatchNorm2d(c).to(cuda)
    xin = torch.randn(n, c, h, w, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    res = torch.randn_like(xin)
    _, vec, mask = nat.bn_fwd_train_mask(xin, bn.weight, bn.bias, bn.running_mean,
                                         bn.running_var, 0.1, 1e-5, res)
    m = n * h * w
    a = torch.randn(m, k, device=cuda).to(torch.bfloat16)
    wt = (torch.randn(c, k, device=cuda) / 8).to(torch.bfloat16)
    dy2 = torch.randn_like(xin)
    dz = torch.empty_like(xin)
    x2 = xin.permute(0, 2, 3, 1).reshape(m, c)
    part = nat.gemm_nt_bn_bwd(a, wt, dz.permute(0, 2, 3, 1).reshape(m, c), dy2, mask, x2, vec)
    dx, dg, db = nat.bn_bwd_from_partials(dz, xin, vec, bn.weight, True, part)
    dy = (a.float() @ wt.float().t()).to(torch.bfloat16).view(n, h, w, c).permute(0, 3, 1, 2)
    dy = dy.contiguous(memory_format=torch.channels_last)
    rdx, rdg, rdb, rdz = nat.bn_bwd(3, dy, xin, mask, vec, bn.weight, True, dy2, 1)
    torch.testing.assert_close(dz.float(), rdz.float(), rtol=2e-2, atol=2e-2)
    for u, v in ((dx, rdx), (dg, rdg), (db, rdb)):
        torch.testing.assert_close(u.float(), v.float(), rtol=3e-2,
                                   atol=3e-2 * float(v.float().abs().max()))


def test_resnet_bwd_fusion_matches_unfused(cuda, monkeypatch):
    """A ResNet whose layers have >1 block: conv1's dgrad GEMM runs the previous
    block's BN backward reduce (gemm_nt_bn_bwd is called) and every parameter
    gradient is as close to an fp32 eager reference of the same weights as the
    unfused bf16 path's (bf16 + small-batch BN backward is far from fp32 at random
    init for BOTH paths, measured in round 2: ~0.5 relative L2, so the
    fused path is judged against the unfused path's own error)."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    nat = _nat()
    calls = []
    real = nat.gemm_nt_bn_bwd

    def counted(*args, **kw):
        calls.append(args[0].shape)
        return real(*args, **kw)

    monkeypatch.setattr(nat, "gemm_nt_bn_bwd", counted)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return {k: p.grad.float() for k, p in m.named_parameters()}

    ref = grads(copy.deepcopy(base).float(), x.float())
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("MIVOD_FUSION_OFF", "" if fuse == "1" else "fold")
        out[fuse] = grads(copy.deepcopy(base), x)
        if fuse == "1":
            # layer1.1, layer2.0 (strided shortcut grad), layer2.1, layer3.0 (strided), layer3.1
            assert len(calls) == 5, calls
    for k, r in ref.items():
        n = float(r.norm()) + 1e-12
        ef = float((out["1"][k] - r).norm()) / n
        eu = float((out["0"][k] - r).norm()) / n
        assert ef <= 1.25 * eu + 2e-3, (k, ef, eu)


def test_resnet_bn_fold_matches_unfolded(cuda, monkeypatch):
    """ops.bn._Conv1x1BNFold: conv3 + BN3's backward as GEMMs on dz and x (BN dx never
    materialised) — every parameter gradient as close to the fp32 eager reference as the
    unfolded bf16 path's, and the folded branch really runs (bn_bwd_coeffs calls: the
    blocks whose output feeds a fused conv1 data gradient)."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    nat = _nat()
    calls = []
    real = nat.bn_bwd_coeffs

    def counted(*args, **kw):
        calls.append(args[2].shape)
        return real(*args, **kw)

    real_fc = nat.fold_coeffs

    def counted_fc(*args):           # the fused coefficient kernel (ops.bn._FOLD_MATH)
        calls.append(args[0].shape)
        return real_fc(*args)

    monkeypatch.setattr(nat, "bn_bwd_coeffs", counted)
    monkeypatch.setattr(nat, "fold_coeffs", counted_fc)
    from mivod.ops import bn as B
    monkeypatch.setattr(B, "_SHORTCUT_FOLD", False)     # counted separately (shortcut test)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return {k: p.grad.float() for k, p in m.named_parameters()}

    ref = grads(copy.deepcopy(base).float(), x.float())
    out = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("MIVOD_FUSION_OFF", "" if fold == "1" else "fold")
        calls.clear()
        out[fold] = grads(copy.deepcopy(base), x)
        assert len(calls) == (5 if fold == "1" else 0), calls
    for k, r in ref.items():
        n = float(r.norm()) + 1e-12
        ef = float((out["1"][k] - r).norm()) / n
        eu = float((out["0"][k] - r).norm()) / n
        assert ef <= 1.25 * eu + 2e-3, (k, ef, eu)


def test_gemm_nt_bn_bwd_without_x(cuda):
    """x = None: same dz and sum dz, second partial exactly 0 (the folded producer's path)."""
    nat = _nat()
    g = torch.Generator(device=cuda).manual_seed(5)
    M, K, N = 1000, 256, 64
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    x = torch.randn(M, N, device=cuda, generator=g).to(torch.bfloat16)
    vec = torch.randn(4, N, device=cuda, generator=g)
    mask = torch.randint(0, 256, (M, N // 8), device=cuda, generator=g, dtype=torch.int32).to(
        torch.uint8)
    dz1, dz2 = torch.empty(M, N, device=cuda, dtype=torch.bfloat16), torch.empty(
        M, N, device=cuda, dtype=torch.bfloat16)
    p1 = nat.gemm_nt_bn_bwd(a, b, dz1, None, mask, x, vec)
    p2 = nat.gemm_nt_bn_bwd(a, b, dz2, None, mask, None, vec)
    assert torch.equal(dz1, dz2)
    assert torch.equal(p1[:, 0], p2[:, 0])
    assert not p2[:, 1].any()


@pytest.mark.parametrize("K,N", [(64, 256), (128, 512), (256, 1024), (64, 128), (256, 128)])
@pytest.mark.parametrize("M", [1, 64 * 3 + 5, 4096 + 17])
def test_gemm_nt_apply_matches_two_pass(cuda, M, K, N):
    """Recompute forward of the BN3 fold: statistics-only GEMM + finalize + GEMM with the
    BN+add+ReLU apply and bitmask in its epilogue == gemm_nt's z + the BN apply pass,
    bit for bit (y, mask, statistics, running statistics)."""
    nat = _nat()
    assert nat.gemm_apply_supported(N, K)
    g = torch.Generator(device=cuda).manual_seed(M + K + N)
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    res = torch.randn(M, N, device=cuda, generator=g).to(torch.bfloat16)
    gamma = torch.rand(N, device=cuda, generator=g) + 0.5
    beta = torch.randn(N, device=cuda, generator=g) * 0.1
    P = nat.gemm_partials(M, N, K)
    rm1, rv1 = torch.randn(N, device=cuda, generator=g) * 0.1, torch.rand(N, device=cuda) + 0.5
    rm2, rv2 = rm1.clone(), rv1.clone()
    # two-pass reference: z materialised, then the fused BN apply (mode 3 mask)
    z = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
    p1 = torch.empty(P, 2, N, device=cuda)
    nat.gemm_nt(a, b, z, rm1, p1)
    z4 = z.view(1, 1, M, N).permute(0, 3, 1, 2)
    r4 = res.view(1, 1, M, N).permute(0, 3, 1, 2)
    y1, vec1, mask1 = nat.bn_fwd_train_stats(z4, p1, gamma, beta, rm1, rv1, 0.1, 1e-5, True, r4,
                                             True)
    # recompute path
    p2 = torch.full((P, 2, N), float("nan"), device=cuda)
    nat.gemm_nt(a, b, None, rm2, p2)
    assert torch.equal(p1, p2)
    vec2 = nat.bn_finalize(p2, gamma, beta, rm2, rv2, 0.1, 1e-5, M)
    y2, mask2 = nat.gemm_nt_apply(a, b, res, vec2[2], vec2[3])
    assert torch.equal(vec1, vec2) and torch.equal(rm1, rm2) and torch.equal(rv1, rv2)
    assert torch.equal(y1.permute(0, 2, 3, 1).reshape(M, N), y2)
    assert torch.equal(mask1.view(M, N // 8), mask2)
    # and against fp32 math (to bf16 rounding)
    ref = torch.relu(z.float() * vec2[2] + vec2[3] + res.float())
    torch.testing.assert_close(y2.float(), ref, rtol=1e-2, atol=1e-2)
    # affine residual (a projection shortcut's BN applied in the epilogue) == that BN's
    # apply pass materialising the identity first
    rsc = torch.rand(N, device=cuda, generator=g) + 0.5
    rbi = torch.randn(N, device=cuda, generator=g) * 0.1
    ident = nat.bn_apply(r4, rsc, rbi, False, None).permute(0, 2, 3, 1).reshape(M, N)
    y3, mask3 = nat.gemm_nt_apply(a, b, ident, vec2[2], vec2[3])
    y4, mask4 = nat.gemm_nt_apply(a, b, res, vec2[2], vec2[3], rsc, rbi)
    assert torch.equal(y3, y4) and torch.equal(mask3, mask4)


def test_gemm_nt_apply_rejects_unsupported(cuda):
    nat = _nat()
    assert not nat.gemm_apply_supported(64, 64)       # 64-wide tiles: half mask bytes
    assert not nat.gemm_apply_supported(512, 512)     # K > 256: not a streamed shape
    a = torch.zeros(8, 512, device=cuda, dtype=torch.bfloat16)
    b = torch.zeros(512, 512, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        nat.gemm_nt(a, b, None, None, torch.zeros(16, 2, 512, device=cuda))
    with pytest.raises(RuntimeError):
        nat.gemm_nt_apply(a, b, torch.zeros(8, 512, device=cuda, dtype=torch.bfloat16),
                          torch.ones(512, device=cuda), torch.zeros(512, device=cuda))


def test_resnet_bn_recompute_matches_materialised(cuda, monkeypatch):
    """The fold's recompute forward (z never written; ops.bn._RECOMPUTE) runs, and every
    parameter gradient is as close to the fp32 eager reference as the materialised-z
    path's (the model-level comparison is against fp32: MIOpen / hipBLASLt backward
    kernels are not run-to-run deterministic, ~6% gradient spread on this tiny net; the
    bit-exactness of the recompute itself is pinned by test_gemm_nt_apply_matches_two_pass)."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    from mivod.ops import bn as B
    nat = _nat()
    calls = []
    real = nat.gemm_nt_apply

    def counted(*args):
        calls.append(args[0].shape)
        return real(*args)

    monkeypatch.setattr(nat, "gemm_nt_apply", counted)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return {k: p.grad.float() for k, p in m.named_parameters()}

    ref = grads(copy.deepcopy(base).float(), x.float())
    out = {}
    for rc in (True, False):
        monkeypatch.setattr(B, "_RECOMPUTE", rc)
        calls.clear()
        out[rc] = grads(copy.deepcopy(base), x)
        assert (len(calls) > 0) == rc, calls
    for k, r in ref.items():
        n = float(r.norm()) + 1e-12
        er = float((out[True][k] - r).norm()) / n
        em = float((out[False][k] - r).norm()) / n
        assert er <= 1.25 * em + 2e-2, (k, er, em)


@pytest.mark.parametrize("K1,K2", [(256, 64), (512, 128), (1024, 256), (2048, 512)])
# M = 448 with K2 = 256: mv_gemm256.hip's 224-row blocks (MT = 7)
@pytest.mark.parametrize("M", [1, 64 * 3 + 5, 448, 4096 + 17, 70000])
def test_gemm_fold_dx_matches_fp32(cuda, M, K1, K2):
    """Dual-source fold data gradient + BN2 ReLU-backward reduce epilogue vs fp32 math."""
    nat = _nat()
    assert nat.gemm_fold_dx_partials(M, K1, K2) > 0
    g = torch.Generator(device=cuda).manual_seed(M + K1)
    a1 = torch.randn(M, K1, device=cuda, generator=g).to(torch.bfloat16)
    a2 = torch.randn(M, K2, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(K2, K1 + K2, device=cuda, generator=g) / (K1 + K2) ** 0.5).to(torch.bfloat16)
    badd = torch.randn(K2, device=cuda, generator=g) * 0.1
    xb = torch.randn(M, K2, device=cuda, generator=g).to(torch.bfloat16)
    vec = torch.stack((torch.randn(K2, device=cuda, generator=g) * 0.1,
                       torch.rand(K2, device=cuda, generator=g) + 0.5,
                       torch.randn(K2, device=cuda, generator=g),
                       torch.randn(K2, device=cuda, generator=g) * 0.1)).contiguous()
    d = torch.full((M, K2), float("nan"), device=cuda).to(torch.bfloat16)
    part = nat.gemm_fold_dx(a1, a2, b, badd, d, xb, vec)
    dx = a1.float() @ b[:, :K1].float().t() + a2.float() @ b[:, K1:].float().t() + badd
    keep = (xb.float() * vec[2] + vec[3]) > 0
    ref = torch.where(keep, dx.to(torch.bfloat16).float(), torch.zeros_like(dx))
    torch.testing.assert_close(d.float(), ref, rtol=1e-2, atol=1e-2 * float(ref.abs().max()))
    s = part.sum(0)
    df = d.float()
    torch.testing.assert_close(s[0], df.sum(0), rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(s[1], (df * (xb.float() - vec[0])).sum(0), rtol=1e-4, atol=1e-2)
    assert nat.gemm_fold_dx_partials(M, 1024, 128) == -1      # not a covered shape


def test_resnet_fold_dx_matches_hipblaslt(cuda, monkeypatch):
    """The fold's fused data gradient (+ BN2 reduce) runs on the 64/128-channel bottlenecks
    and every parameter gradient is as close to the fp32 reference as the hipBLASLt path's."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    from mivod.ops import bn as B
    nat = _nat()
    calls = []
    real = nat.gemm_fold_dx

    def counted(*args):
        calls.append(args[0].shape)
        return real(*args)

    monkeypatch.setattr(nat, "gemm_fold_dx", counted)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return {k: p.grad.float() for k, p in m.named_parameters()}

    ref = grads(copy.deepcopy(base).float(), x.float())
    out = {}
    for on in (True, False):
        monkeypatch.setattr(B, "_FOLD_DX", on)
        calls.clear()
        out[on] = grads(copy.deepcopy(base), x)
        assert (len(calls) > 0) == on, calls
    for k, r in ref.items():
        n = float(r.norm()) + 1e-12
        e1 = float((out[True][k] - r).norm()) / n
        e0 = float((out[False][k] - r).norm()) / n
        assert e1 <= 1.25 * e0 + 2e-2, (k, e1, e0)


def test_resnet_shortcut_bn_in_epilogue(cuda, monkeypatch):
    """Projection-shortcut BNs applied inside conv3's recomputing GEMM (ops.bn._SHORTCUT):
    the fused path runs for the stride-1 and strided shortcuts it covers, the running
    statistics match the materialised path, and every parameter gradient is as close to
    the fp32 reference as the materialised path's."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    from mivod.ops import bn as B
    nat = _nat()
    calls = []
    real = nat.gemm_nt_apply

    def counted(*args):
        calls.append(len(args) > 5 and args[5] is not None)
        return real(*args)

    real_dual = nat.gemm_nt_apply_dual

    def counted_dual(*args):          # the stride-1 shortcut, recomputed in the kernel
        calls.append(True)
        return real_dual(*args)

    monkeypatch.setattr(nat, "gemm_nt_apply", counted)
    monkeypatch.setattr(nat, "gemm_nt_apply_dual", counted_dual)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return ({k: p.grad.float() for k, p in m.named_parameters()},
                {k: v.float() for k, v in m.state_dict().items() if "running" in k})

    ref, _ = grads(copy.deepcopy(base).float(), x.float())
    out, stats = {}, {}
    for on in (True, False):
        monkeypatch.setattr(B, "_SHORTCUT", on)
        calls.clear()
        out[on], stats[on] = grads(copy.deepcopy(base), x)
        # layer1.0 (stride 1), layer2.0, layer3.0 (strided); layer4's conv3 (K 512) is not
        # a recomputed GEMM
        assert sum(calls) == (3 if on else 0), calls
    for k, r in ref.items():
        n = float(r.norm()) + 1e-12
        e1 = float((out[True][k] - r).norm()) / n
        e0 = float((out[False][k] - r).norm()) / n
        assert e1 <= 1.25 * e0 + 2e-2, (k, e1, e0)
    for k, r in stats[False].items():     # (MIOpen may pick another solution on a first call)
        torch.testing.assert_close(stats[True][k], r, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("M", [1, 64 * 3 + 5, 4096 + 17])
def test_gemm_dual_bias_matches_fp32(cuda, M):
    """EPI 6: [a1 | a2] . b^T + badd with a plain bf16 store (the shortcut fold's dx0)."""
    nat = _nat()
    K1, K2 = 256, 64
    assert nat.gemm_dual_supported(K1, K2) and not nat.gemm_dual_supported(512, 128)
    g = torch.Generator(device=cuda).manual_seed(M + 11)
    a1 = torch.randn(M, K1, device=cuda, generator=g).to(torch.bfloat16)
    a2 = torch.randn(M, K2, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(K2, K1 + K2, device=cuda, generator=g) / (K1 + K2) ** 0.5).to(torch.bfloat16)
    badd = torch.randn(K2, device=cuda, generator=g) * 0.1
    d = torch.full((M, K2), float("nan"), device=cuda).to(torch.bfloat16)
    nat.gemm_dual_bias(a1, a2, b, badd, d)
    ref = a1.float() @ b[:, :K1].float().t() + a2.float() @ b[:, K1:].float().t() + badd
    torch.testing.assert_close(d.float(), ref, rtol=1e-2, atol=1e-2 * float(ref.abs().max()))


def test_resnet_shortcut_fold_matches_unfolded(cuda, monkeypatch):
    """Projection shortcut conv + BN folded into the block's fused backward
    (ops.bn._SHORTCUT_FOLD): runs on the stride-1 (dual GEMM kernel) and strided shortcuts,
    and every parameter gradient and running statistic is as close to the fp32 / unfolded
    results as the unfolded path's."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    from mivod.ops import bn as B
    nat = _nat()
    calls = []
    real = nat.bn_bwd_coeffs

    def counted(*args):
        calls.append(args[2].shape)
        return real(*args)

    real_fc = nat.fold_coeffs

    def counted_fc(*args):
        calls.append(args[0].shape)
        return real_fc(*args)

    monkeypatch.setattr(nat, "bn_bwd_coeffs", counted)
    monkeypatch.setattr(nat, "fold_coeffs", counted_fc)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return ({k: p.grad.float() for k, p in m.named_parameters()},
                {k: v.float() for k, v in m.state_dict().items() if "running" in k})

    ref, _ = grads(copy.deepcopy(base).float(), x.float())
    out, stats, n = {}, {}, {}
    for on in (True, False):
        monkeypatch.setattr(B, "_SHORTCUT_FOLD", on)
        calls.clear()
        out[on], stats[on] = grads(copy.deepcopy(base), x)
        n[on] = len(calls)
    assert n[True] == n[False] + 3, n          # layer1.0 / 2.0 / 3.0 shortcut BNs folded
    for k, r in ref.items():
        nr = float(r.norm()) + 1e-12
        e1 = float((out[True][k] - r).norm()) / nr
        e0 = float((out[False][k] - r).norm()) / nr
        assert e1 <= 1.25 * e0 + 2e-2, (k, e1, e0)
    for k, r in stats[False].items():     # (MIOpen may pick another solution on a first call)
        torch.testing.assert_close(stats[True][k], r, rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("M,C", [(1, 64), (3000, 64), (50000, 128), (777, 256), (4096, 512)])
def test_bn_apply_colsum(cuda, M, C):
    """BN+ReLU apply with column-sum partials == the plain apply (bitwise) + fp32 colsum."""
    nat = _nat()
    g = torch.Generator(device=cuda).manual_seed(M + C)
    x = torch.randn(M, C, device=cuda, generator=g).to(torch.bfloat16)
    x4 = x.view(1, 1, M, C).permute(0, 3, 1, 2)
    sc = torch.rand(C, device=cuda, generator=g) + 0.5
    bi = torch.randn(C, device=cuda, generator=g) * 0.2
    y1 = nat.bn_apply(x4, sc, bi, True, None)
    y2, part = nat.bn_apply_colsum(x4, sc, bi)
    assert torch.equal(y1, y2)
    assert part.dim() == 2 and part.shape[1] == C and torch.isfinite(part).all()
    ref = y1.permute(0, 2, 3, 1).reshape(M, C).float().sum(0)
    torch.testing.assert_close(part.sum(0), ref, rtol=1e-4, atol=1e-2)


def test_resnet_colsum_from_bn2_apply(cuda, monkeypatch):
    """conv3's folded weight gradient takes colsum(x) from BN2's apply pass
    (ops.bn._COLSUM) — same gradients (to fp32-reference closeness) and no statistics pass."""
    import copy

    from mivod.models.resnet import ResNet, to_mixed_bf16
    from mivod.ops import bn as B
    nat = _nat()
    calls = []
    real = nat.bn_apply_colsum

    def counted(*args):
        calls.append(args[0].shape)
        return real(*args)

    monkeypatch.setattr(nat, "bn_apply_colsum", counted)
    torch.manual_seed(0)
    base = to_mixed_bf16(ResNet((2, 2, 2, 1), num_classes=10)).to(cuda)
    x = torch.rand(16, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (16,), device=cuda)

    def grads(m, inp):
        F.cross_entropy(m(inp).float(), tgt).backward()
        return {k: p.grad.float() for k, p in m.named_parameters()}

    ref = grads(copy.deepcopy(base).float(), x.float())
    out = {}
    for on in (True, False):
        monkeypatch.setattr(B, "_COLSUM", on)
        calls.clear()
        out[on] = grads(copy.deepcopy(base), x)
        assert (len(calls) > 0) == on, calls
    for k, r in ref.items():
        nr = float(r.norm()) + 1e-12
        e1 = float((out[True][k] - r).norm()) / nr
        e0 = float((out[False][k] - r).norm()) / nr
        assert e1 <= 1.25 * e0 + 2e-2, (k, e1, e0)


@pytest.mark.parametrize("N", [256, 128])
@pytest.mark.parametrize("M", [1, 64 * 3 + 5, 4096 + 17])
def test_gemm_nt_apply_dual_matches_materialised(cuda, M, N):
    """EPI 7 (shortcut conv recomputed inside the apply GEMM) == writing the shortcut conv's
    output and applying it as an affine residual (EPI 5), bit for bit."""
    nat = _nat()
    K = 64
    assert nat.gemm_apply_dual_supported(N, K) and not nat.gemm_apply_dual_supported(512, 128)
    g = torch.Generator(device=cuda).manual_seed(M + N + 3)
    a = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    a2 = torch.randn(M, K, device=cuda, generator=g).to(torch.bfloat16)
    b2 = (torch.randn(N, K, device=cuda, generator=g) / K ** 0.5).to(torch.bfloat16)
    sc, rsc = torch.rand(N, device=cuda, generator=g) + 0.5, torch.rand(N, device=cuda) + 0.5
    bi, rbi = torch.randn(N, device=cuda, generator=g) * 0.1, torch.randn(N, device=cuda) * 0.1
    z2 = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
    nat.gemm_nt(a2, b2, z2, None, None)
    y1, m1 = nat.gemm_nt_apply(a, b, z2, sc, bi, rsc, rbi)
    y2, m2 = nat.gemm_nt_apply_dual(a, b, a2, b2, sc, bi, rsc, rbi)
    assert torch.equal(y1, y2) and torch.equal(m1, m2)


@pytest.mark.parametrize("cout,cin", [(256, 64), (512, 128), (1024, 256), (2048, 512), (256, 512)])
@pytest.mark.parametrize("colsum", [True, False])
def test_fold_math_kernels_match_eager(cuda, monkeypatch, cout, cin, colsum):
    """mv_fold.hip's two kernels == the eager PyTorch composition of the fold's small math."""
    from mivod.ops import bn as B
    nat = _nat()
    g0 = torch.Generator(device=cuda).manual_seed(cout + cin)
    m = 50000
    wb = (torch.randn(cout, cin, device=cuda, generator=g0) / cin ** 0.5).to(torch.bfloat16)
    g = torch.randn(cout, cin, device=cuda, generator=g0) * 10
    x = torch.randn(m, cin, device=cuda, generator=g0)
    gram = (x.t() @ x).contiguous()
    vec = torch.stack((torch.randn(cout, device=cuda, generator=g0) * 0.1,
                       torch.rand(cout, device=cuda, generator=g0) + 0.5,
                       torch.randn(cout, device=cuda, generator=g0),
                       torch.randn(cout, device=cuda, generator=g0))).contiguous()
    gamma = torch.rand(cout, device=cuda, generator=g0) + 0.5
    part = torch.randn(37, 2, cout, device=cuda, generator=g0)
    cs = torch.randn(29, cin, device=cuda, generator=g0) * 5 if colsum else None
    xs = torch.randn(cin, device=cuda, generator=g0) * 50
    out = {}
    for on in (True, False):
        monkeypatch.setattr(B, "_FOLD_MATH", on)
        out[on] = B._fold_math(nat, wb, g, gram, vec, gamma, m, part, None, cs, lambda: xs, True)
    for a, b, name in zip(out[True], out[False], ("dg", "db", "dw", "bcat", "badd")):
        torch.testing.assert_close(a.float(), b.float(), rtol=2e-2, atol=2e-2 * float(b.abs().max()),
                                   msg=name)


@pytest.mark.parametrize("M,K1,K2", [(1, 512, 256), (64 * 3 + 5, 1024, 512), (70000, 2048, 1024)])
def test_gemm_dual_bias_256(cuda, M, K1, K2):
    """[a1 | a2] . b^T + badd on mv_gemm256.hip's dual-source mode (K2 % 256 == 0)."""
    nat = _nat()
    assert nat.gemm_dual_supported(K1, K2)
    g = torch.Generator(device=cuda).manual_seed(M + K1)
    a1 = torch.randn(M, K1, device=cuda, generator=g).to(torch.bfloat16)
    a2 = torch.randn(M, K2, device=cuda, generator=g).to(torch.bfloat16)
    b = (torch.randn(K2, K1 + K2, device=cuda, generator=g) / (K1 + K2) ** 0.5).to(torch.bfloat16)
    badd = torch.randn(K2, device=cuda, generator=g) * 0.1
    d = torch.full((M, K2), float("nan"), device=cuda).to(torch.bfloat16)
    nat.gemm_dual_bias(a1, a2, b, badd, d)
    ref = a1.float() @ b[:, :K1].float().t() + a2.float() @ b[:, K1:].float().t() + badd
    torch.testing.assert_close(d.float(), ref, rtol=1e-2, atol=1e-2 * float(ref.abs().max()))


@pytest.mark.parametrize("n,c,h,k,s", [(2, 256, 9, 512, 2), (8, 512, 28, 1024, 2),
                                       (3, 1024, 14, 2048, 2), (2, 512, 7, 256, 1),
                                       (1, 64, 5, 256, 3),
                                       # M = 28 x 4 x 4 = 448, N = 256: 224-row blocks (MT = 7)
                                       (28, 64, 7, 256, 2)])
def test_conv1x1_strided_stats(cuda, n, c, h, k, s):
    """Strided 1x1 conv (rows gathered at the stride) + BN statistics on mv_gemm256.hip."""
    nat = _nat()
    g = torch.Generator(device=cuda).manual_seed(n + c + h + k)
    x = torch.randn(n, c, h, h + 1, device=cuda, generator=g).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    w = (torch.randn(k, c, 1, 1, device=cuda, generator=g) / c ** 0.5).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    shift = torch.randn(k, device=cuda, generator=g) * 0.1
    r = nat.conv1x1_strided_stats(x, w, s, shift)
    assert r is not None
    y, part = r
    ref = F.conv2d(x.float(), w.float(), None, s)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    torch.testing.assert_close(y.float(), ref, rtol=1e-2, atol=1e-2 * float(ref.abs().max()))
    d = (y.float() - shift.view(1, -1, 1, 1)).permute(1, 0, 2, 3).reshape(k, -1)
    sp = part.sum(0)
    torch.testing.assert_close(sp[0], d.sum(1), rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(sp[1], (d * d).sum(1), rtol=1e-4, atol=1e-2)
    y2 = nat.conv1x1_strided_stats(x, w, s)[0]
    assert torch.equal(y, y2)
