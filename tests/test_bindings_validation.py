"""The host side of mivod._mvk: the exported surface, and the operand checks every binding
runs before a launch (csrc/kernels/mv_checks.h).

* the surface (names, argument names, types, defaults) equals tests/mvk_api.json;
* CPU tier: every tensor-taking binding, called with well-shaped CPU tensors, raises
  "<binding>: <first operand> must ...";
* GPU tier: a bad *secondary* operand (non-contiguous, wrong dtype, wrong size, other
  device) of an otherwise valid call raises.  Non-contiguous operands are ``base[::2]``
  views and wrong sizes are too large, so every pointer stays inside a live allocation.
  The flat SGD / Adam / Adadelta steps, which the arenas hand 16-byte-aligned slices only,
  reject a ``base[1:]`` view of any operand before they launch (their kernels have a
  one-by-one path for it; the binding keeps the arenas' contract).
"""
import json
import os

import pytest
import torch

mvk = pytest.importorskip("mivod._mvk")

with open(os.path.join(os.path.dirname(__file__), "mvk_api.json")) as f:
    API = json.load(f)

bf16, f32, i32, i64, u8 = torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8


def t(*shape, dtype=bf16, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def cl(n, c, h, w, device="cpu"):
    return t(n, c, h, w, device=device).contiguous(memory_format=torch.channels_last)


def surface(mod):
    return {n: (getattr(mod, n).__doc__ or "").splitlines()[0]
            for n in dir(mod) if not n.startswith("_")}


def test_surface_matches_snapshot():
    assert surface(mvk) == API


def _tables():
    return t(1, dtype=i64), t(1, dtype=i32), t(1, dtype=i32), t(1, dtype=i32), t(1, dtype=i32)


def _attn():
    return t(1, 64, 3, 1, 64), t(1, 64, 1, 64), t(1, 64, 1, 64), t(1, 1, 64, dtype=f32)


def _stem():
    # x, dy, idx, y, z, vec of the ResNet stem at batch 1
    return (cl(1, 4, 224, 224), cl(1, 64, 56, 56), t(1, 56, 56, 64, dtype=u8), cl(1, 64, 56, 56),
            cl(1, 64, 112, 112), t(4, 64, dtype=f32))


G, W, V64 = t(64), t(64, dtype=f32), t(64, dtype=f32)   # flat grad, fp32 master, fp32 [64]
X = cl(1, 64, 8, 8)                                     # a BN / conv activation
A = t(128, 64)                                          # a GEMM operand [M, K] / [N, K]

# binding -> (first tensor operand's name, the call on CPU tensors)
CPU_CALLS = {
    "mt_copy": ("tensors", lambda: mvk.mt_copy([G], t(64), [0], True, 1.0, None)),
    "flat_cast": ("src", lambda: mvk.flat_cast(G, W, 1.0, None)),
    "nonfinite_scan": ("x", lambda: mvk.nonfinite_scan(G, t(1, dtype=i32))),
    "sgd_step": ("grad", lambda: mvk.sgd_step(G, W, W.clone(), None, 0.1, 0.9, 0.0, 0.0, 1.0,
                                              False, True, None, None)),
    "adam_step": ("grad", lambda: mvk.adam_step(G, W, W.clone(), W.clone(), None, 1e-3, 0.9, 0.999,
                                                1e-8, 0.0, 1.0, 1, False, False, None, None)),
    "adadelta_step": ("grad", lambda: mvk.adadelta_step(G, W, W.clone(), W.clone(), None, 1.0, 0.9,
                                                        1e-6, 0.0, 1.0, None, None)),
    "lars_step": ("grad", lambda: mvk.lars_step(G, W, W.clone(), None, *_tables(),
                                                t(1, dtype=i32), t(2, dtype=f32), t(2, dtype=f32),
                                                0.1, 0.9, 0.0, 1e-3, 1.0, 1e-8, True, None, None)),
    "seg_dot3": ("a", lambda: mvk.seg_dot3(G, t(64), *_tables(), t(3, dtype=f32), t(3, dtype=f32),
                                           False)),
    "adasum_merge": ("fin", lambda: mvk.adasum_merge(G, W, t(64), *_tables(), t(3, dtype=f32), 1,
                                                     False, None, 0, 0)),
    "adasum_combine": ("a", lambda: mvk.adasum_combine(G, t(64), *_tables(), t(3, dtype=f32))),
    "adasum_fcombine": ("f", lambda: mvk.adasum_fcombine(W, G, *_tables(), t(3, dtype=f32), False)),
    "attn_fwd": ("qkv", lambda: mvk.attn_fwd(_attn()[0], None, 0.0, 0)),
    "attn_bwd": ("qkv", lambda: mvk.attn_bwd(*_attn(), None, 0.0, 0)),
    "attn_bwd_bsum": ("qkv", lambda: mvk.attn_bwd_bsum(*_attn(), None, 0.0, 0)),
    "bias_gelu_fwd": ("x", lambda: mvk.bias_gelu_fwd(t(4, 8), t(8))),
    "bias_gelu_bwd": ("dy", lambda: mvk.bias_gelu_bwd(t(4, 8), t(4, 8), t(8))),
    "ce_fwd": ("x", lambda: mvk.ce_fwd(t(4, 8), t(4, dtype=i64), -100)),
    "ce_bwd": ("x", lambda: mvk.ce_bwd(t(4, 8), t(4, dtype=i64), t(4, dtype=f32),
                                       t(1, dtype=f32), -100)),
    "bias_grad": ("dy", lambda: mvk.bias_grad(t(4, 8))),
    "colsum_partials": ("partial", lambda: mvk.colsum_partials(t(2, 8, dtype=f32))),
    "embedding_bwd": ("ids", lambda: mvk.embedding_bwd(t(4, dtype=i64), t(4, 8), 16)),
    "bert_emb_fwd": ("ids", lambda: mvk.bert_emb_fwd(t(2, 4, dtype=i64), t(2, 4, dtype=i64),
                                                     t(16, 8), t(4, 8), t(2, 8))),
    "bert_emb_pt_bwd": ("dy", lambda: mvk.bert_emb_pt_bwd(t(2, 4, 8), t(2, 4, dtype=i64), 4)),
    "gemm_gelu_bwd": ("dy", lambda: mvk.gemm_gelu_bwd(t(128, 64), t(256, 64), t(128, 256),
                                                      t(256))),
    "ln_fwd": ("z", lambda: mvk.ln_fwd(t(4, 8), None, None, t(8), t(8), 1e-5, 0.0, 0, True)),
    "ln_bwd": ("dy", lambda: mvk.ln_bwd(t(4, 8), t(4, 8), t(4, dtype=f32), t(4, dtype=f32), t(8),
                                        0.0, 0, False, None)),
    "bn_fwd_train": ("x", lambda: mvk.bn_fwd_train(X, V64, V64, None, None, 0.1, 1e-5, True, None)),
    "bn_fwd_train_mask": ("x", lambda: mvk.bn_fwd_train_mask(X, V64, V64, None, None, 0.1, 1e-5,
                                                             X.clone())),
    "bn_fwd_train_stats": ("x", lambda: mvk.bn_fwd_train_stats(X, t(1, 2, 64, dtype=f32), V64, V64,
                                                               None, None, 0.1, 1e-5, True, None,
                                                               False)),
    "bn_apply": ("x", lambda: mvk.bn_apply(X, V64, V64, True, None)),
    "bn_apply_colsum": ("x", lambda: mvk.bn_apply_colsum(X, V64, V64)),
    "bn_stats": ("x", lambda: mvk.bn_stats(X, V64, V64, None, None, 0.1, 1e-5)),
    "bn_stats_strided": ("x", lambda: mvk.bn_stats_strided(X, 2)),
    "bn_bwd": ("dy", lambda: mvk.bn_bwd(1, X, X.clone(), None, t(4, 64, dtype=f32), V64, True,
                                        None, 1)),
    "bn_finalize": ("stats", lambda: mvk.bn_finalize(t(1, 2, 64, dtype=f32), V64, V64, None, None,
                                                     0.1, 1e-5, 64)),
    "bn_bwd_coeffs": ("vec", lambda: mvk.bn_bwd_coeffs(t(4, 64, dtype=f32), V64,
                                                       t(1, 2, 64, dtype=f32), 64)),
    "bn_bwd_from_partials": ("dz", lambda: mvk.bn_bwd_from_partials(
        X, X.clone(), t(4, 64, dtype=f32), V64, True, t(1, 2, 64, dtype=f32))),
    "maxpool_fwd": ("x", lambda: mvk.maxpool_fwd(X, None, None, False, 3, 2, 1)),
    "maxpool_bwd": ("dy", lambda: mvk.maxpool_bwd(cl(1, 64, 4, 4), None, t(1, 4, 4, 64, dtype=u8),
                                                  8, 8, 3, 2, 1)),
    "maxpool_bn_bwd": ("dy", lambda: mvk.maxpool_bn_bwd(
        cl(1, 64, 4, 4), None, t(1, 4, 4, 64, dtype=u8), cl(1, 64, 4, 4), X,
        t(4, 64, dtype=f32), V64)),
    "gap_fwd": ("x", lambda: mvk.gap_fwd(X)),
    "gap_bwd": ("dy", lambda: mvk.gap_bwd(t(1, 64), 8, 8)),
    "pad_channels": ("x", lambda: mvk.pad_channels(cl(1, 3, 8, 8), 4)),
    "stem_fwd": ("x", lambda: mvk.stem_fwd(_stem()[0], cl(64, 4, 7, 7), V64, 0)),
    "stem_wgrad": ("x", lambda: mvk.stem_wgrad(_stem()[0], _stem()[4])),
    "stem_wgrad_pool_bn": ("x", lambda: (lambda x, dy, idx, y, z, vec: mvk.stem_wgrad_pool_bn(
        x, dy, None, idx, y, z, vec, V64))(*_stem())),
    "gemm_nt": ("a", lambda: mvk.gemm_nt(A, t(64, 64), t(128, 64), None, None)),
    "gemm256_nt": ("a", lambda: mvk.gemm256_nt(A, t(256, 64), t(128, 256))),
    "conv1x1_strided_stats": ("x", lambda: mvk.conv1x1_strided_stats(X, t(256, 64, 1, 1), 2,
                                                                     t(256, dtype=f32))),
    "gemm_fold_dx": ("a1", lambda: mvk.gemm_fold_dx(A, t(128, 64), t(64, 128), V64, t(128, 64),
                                                    t(128, 64), t(4, 64, dtype=f32))),
    "gemm_dual_bias_strided": ("a1", lambda: mvk.gemm_dual_bias_strided(
        t(16, 64), X, 2, t(256, 128), t(256, dtype=f32), t(16, 256))),
    "gemm_dual_bias": ("a1", lambda: mvk.gemm_dual_bias(A, t(128, 64), t(64, 128), V64,
                                                        t(128, 64))),
    "gram_stats": ("w", lambda: mvk.gram_stats(t(64, 64), t(64, 64, dtype=f32), V64, None, 1)),
    "fold_coeffs": ("part", lambda: mvk.fold_coeffs(t(1, 2, 64, dtype=f32), t(64, 64),
                                                    t(64, 64, dtype=f32), t(4, 64, dtype=f32), V64,
                                                    128, None)),
    "fold_products": ("w", lambda: mvk.fold_products(t(64, 64), t(64, 64, dtype=f32), None,
                                                     t(5, 64, dtype=f32), V64, False)),
    "gemm_nt_apply": ("a", lambda: mvk.gemm_nt_apply(A, t(64, 64), t(128, 64), V64, V64)),
    "gemm_nt_apply_dual": ("a", lambda: mvk.gemm_nt_apply_dual(A, t(64, 64), t(128, 64), t(64, 64),
                                                               V64, V64, V64, V64)),
    "gemm_nt_bn_bwd": ("a", lambda: mvk.gemm_nt_bn_bwd(A, t(64, 64), t(128, 64), None,
                                                       t(128, 8, dtype=u8), None,
                                                       t(4, 64, dtype=f32))),
    "conv3x3": ("x", lambda: mvk.conv3x3(X, cl(64, 64, 3, 3))),
    "conv1x1": ("x", lambda: mvk.conv1x1(X, cl(64, 64, 1, 1))),
    "conv3x3_bn_bwd": ("dy", lambda: mvk.conv3x3_bn_bwd(X, cl(64, 64, 3, 3), X.clone(),
                                                        t(4, 64, dtype=f32))),
    "conv3x3_s2_dgrad": ("dy", lambda: mvk.conv3x3_s2_dgrad(cl(1, 64, 4, 4), cl(64, 64, 3, 3),
                                                            8, 8)),
    "transpose_filters": ("ws", lambda: mvk.transpose_filters([cl(64, 64, 3, 3)])),
    "wgrad3x3": ("x", lambda: mvk.wgrad3x3(X, X.clone())),
    "wgrad1x1": ("x", lambda: mvk.wgrad1x1(X, X.clone())),
}


def test_cpu_table_covers_every_tensor_binding():
    # a binding takes tensors when its argument list (left of "->") names one
    takes = {n for n, sig in API.items() if "Tensor" in sig.split("->")[0]}
    assert set(CPU_CALLS) == takes


@pytest.mark.parametrize("name", sorted(CPU_CALLS))
def test_cpu_operand_is_rejected_by_name(name):
    operand, call = CPU_CALLS[name]
    with pytest.raises(RuntimeError) as ei:
        call()
    assert f"{name}: {operand} must" in str(ei.value)


# --------------------------------------------------------------------------- GPU tier
def _strided(n, dev):
    """fp32 [n] with stride 2 over a base of 2 n elements."""
    v = torch.zeros(2 * n, dtype=f32, device=dev)[::2]
    assert v.numel() == n and not v.is_contiguous()
    return v


def _gemm_nt_args(dev):
    a, b, c = t(128, 64, device=dev), t(64, 64, device=dev), t(128, 64, device=dev)
    part = t(mvk.gemm_partials(128, 64, 64) * 2 * 64, dtype=f32, device=dev)
    return a, b, c, part


@pytest.mark.gpu
def test_gemm_nt_rejects_strided_shift(cuda):
    a, b, c, part = _gemm_nt_args(cuda)
    mvk.gemm_nt(a, b, c, t(64, dtype=f32, device=cuda), part)
    with pytest.raises(RuntimeError, match="gemm_nt: shift must"):
        mvk.gemm_nt(a, b, c, _strided(64, cuda), part)


@pytest.mark.gpu
def test_conv1x1_strided_stats_rejects_strided_shift(cuda):
    x, w = cl(1, 64, 8, 8, device=cuda), t(256, 64, 1, 1, device=cuda)
    mvk.conv1x1_strided_stats(x, w, 2, t(256, dtype=f32, device=cuda))
    with pytest.raises(RuntimeError, match="conv1x1_strided_stats: shift must"):
        mvk.conv1x1_strided_stats(x, w, 2, _strided(256, cuda))


@pytest.mark.gpu
def test_bias_gelu_fwd_rejects_fp16_bias(cuda):
    x = t(4, 8, device=cuda)
    mvk.bias_gelu_fwd(x, t(8, device=cuda))
    with pytest.raises(RuntimeError, match="bias_gelu_fwd: b must"):
        mvk.bias_gelu_fwd(x, t(8, dtype=torch.float16, device=cuda))


@pytest.mark.gpu
def test_maxpool_bwd_rejects_oversized_idx(cuda):
    dy = cl(1, 8, 4, 4, device=cuda)
    mvk.maxpool_bwd(dy, None, t(1, 4, 4, 8, dtype=u8, device=cuda), 8, 8, 3, 2, 1)
    with pytest.raises(RuntimeError, match="maxpool_bwd: idx must"):
        mvk.maxpool_bwd(dy, None, t(2, 4, 4, 8, dtype=u8, device=cuda), 8, 8, 3, 2, 1)


@pytest.mark.gpu
def test_bn_apply_rejects_strided_scale(cuda):
    x, bias = cl(1, 64, 8, 8, device=cuda), t(64, dtype=f32, device=cuda)
    mvk.bn_apply(x, t(64, dtype=f32, device=cuda), bias, True, None)
    with pytest.raises(RuntimeError, match="bn_apply: scale must"):
        mvk.bn_apply(x, _strided(64, cuda), bias, True, None)


@pytest.mark.gpu
def test_bn_activation_without_channels_is_rejected(cuda):
    """[M, 0] passes C % 8 == 0; the row count M = numel / C must not be computed from it."""
    with pytest.raises(RuntimeError, match="bn_stats: x must have a channel count"):
        mvk.bn_stats(t(4, 0, device=cuda), None, None, None, None, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match="bn_apply: x must have a channel count"):
        mvk.bn_apply(t(4, 0, device=cuda), t(0, dtype=f32, device=cuda),
                     t(0, dtype=f32, device=cuda), True, None)


@pytest.mark.gpu
def test_bn_apply_returns_an_empty_batch(cuda):
    """No launch for zero rows: the empty y, as stock PyTorch's eval BatchNorm returns."""
    from mivod.ops.bn import batch_norm_act
    sc, bi = t(64, dtype=f32, device=cuda), t(64, dtype=f32, device=cuda)
    for x in (t(0, 64, device=cuda), cl(0, 64, 8, 8, device=cuda)):
        y = mvk.bn_apply(x, sc, bi, True, None)
        assert y.shape == x.shape and y.dtype == bf16 and y.numel() == 0
    x = cl(0, 64, 8, 8, device=cuda)
    with torch.no_grad():
        y = batch_norm_act(x, sc + 1, bi, bi.clone(), sc + 1, False, 0.1, 1e-5, True, None)
    assert y.shape == x.shape and y.numel() == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_bn_bwd_rejects_an_empty_batch(cuda):
    x = t(0, 64, device=cuda)
    with pytest.raises(RuntimeError, match="bn_bwd: empty input"):
        mvk.bn_bwd(0, x, x.clone(), None, t(4, 64, dtype=f32, device=cuda), None, True, None, 1)


@pytest.mark.gpu
def test_secondary_operand_on_another_gpu_is_rejected(cuda):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = torch.device("cuda", 1)
    with pytest.raises(RuntimeError, match="bias_gelu_fwd: b must be on"):
        mvk.bias_gelu_fwd(t(4, 8, device=cuda), t(8, device=other))
    a, b, c, part = _gemm_nt_args(cuda)
    with pytest.raises(RuntimeError, match="gemm_nt: shift must be on"):
        mvk.gemm_nt(a, b, c, t(64, dtype=f32, device=other), part)


# binding -> (the call on a dict of operands, the operands that must be 16-byte aligned)
_STEP_CALLS = {
    "sgd_step": (lambda o: mvk.sgd_step(o["grad"], o["master"], o["momentum"], o["model"], 0.1, 0.9,
                                        0.0, 0.0, 1.0, False, False, None, None),
                 ["grad", "master", "momentum", "model"]),
    "adam_step": (lambda o: mvk.adam_step(o["grad"], o["master"], o["exp_avg"], o["exp_avg_sq"],
                                          o["model"], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, False,
                                          False, None, None),
                  ["grad", "master", "exp_avg", "exp_avg_sq", "model"]),
    "adadelta_step": (lambda o: mvk.adadelta_step(o["grad"], o["master"], o["square_avg"],
                                                  o["acc_delta"], o["model"], 1.0, 0.9, 1e-6, 0.0,
                                                  1.0, None, None),
                      ["grad", "master", "square_avg", "acc_delta", "model"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_STEP_CALLS))
def test_flat_steps_reject_unaligned_operands(cuda, name):
    """A view one element into its allocation is contiguous and of the right size but not
    16-byte aligned: the error fires before any launch, so no unaligned vector access runs."""
    call, operands = _STEP_CALLS[name]

    def ops():
        return {k: t(64, dtype=bf16 if k in ("grad", "model") else f32, device=cuda)
                for k in operands}

    call(ops())
    for bad in operands:
        o = ops()
        o[bad] = t(65, dtype=o[bad].dtype, device=cuda)[1:]
        assert o[bad].is_contiguous() and o[bad].numel() == 64 and o[bad].data_ptr() % 16
        with pytest.raises(RuntimeError, match=f"{name}: {bad} must be 16-byte aligned"):
            call(o)
