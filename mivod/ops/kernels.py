"""Python entry points for the hand-written gfx950 kernels (``mivod._mvk``).

GPU tensors always go to the HIP kernels; if the extension is missing on a GPU
process this module raises instead of silently falling back.  CPU tensors (the
gloo test tier) use the plain-PyTorch reference implementations below, which
are also the fp32 references the numerics tests compare the kernels against.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import torch

try:
    from .. import _mvk  # type: ignore
    _IMPORT_ERROR = None
except Exception as e:  # pragma: no cover - exercised when not built
    _mvk = None
    _IMPORT_ERROR = e

CHUNK = 4096


def available() -> bool:
    return _mvk is not None


def native():
    """Return the native module or raise loudly (GPU path must be native)."""
    if _mvk is None:
        raise RuntimeError(
            "mivod HIP kernels (mivod/_mvk*.so) are not built/loadable: "
            f"{_IMPORT_ERROR!r}. Run `python -m mivod._build`.")
    return _mvk


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# ---------------------------------------------------------------------------
# K1/K2 pack / unpack
# ---------------------------------------------------------------------------
def pack(tensors: Sequence[torch.Tensor], flat: torch.Tensor, offsets: Sequence[int],
         scale: float = 1.0, nonfinite: Optional[torch.Tensor] = None) -> None:
    """flat[off_i : off_i+n_i] = cast(t_i * scale) for every tensor (raw memory
    order of t_i).  Tensors of one call must share a dtype."""
    if not tensors:
        return
    if _on_gpu(flat):
        native().mt_copy(list(tensors), flat, [int(o) for o in offsets], True, float(scale),
                         nonfinite)
        return
    for t, o in zip(tensors, offsets):
        src = _raw_flat(t)
        dst = flat[o:o + src.numel()]
        v = src.float() * scale if scale != 1.0 else src
        dst.copy_(v)
        # the stored values (an overflow of the cast to a 16-bit wire counts)
        if nonfinite is not None and not bool(torch.isfinite(dst.float()).all()):
            nonfinite.fill_(1)


def unpack(tensors: Sequence[torch.Tensor], flat: torch.Tensor, offsets: Sequence[int],
           scale: float = 1.0) -> None:
    """t_i (raw memory order) = cast(flat[off_i : off_i+n_i] * scale)."""
    if not tensors:
        return
    if _on_gpu(flat):
        native().mt_copy(list(tensors), flat, [int(o) for o in offsets], False, float(scale), None)
        return
    for t, o in zip(tensors, offsets):
        dst = _raw_flat(t)
        src = flat[o:o + dst.numel()]
        dst.copy_(src.float() * scale if scale != 1.0 else src)


def is_dense(t: torch.Tensor) -> bool:
    """True when ``t`` covers exactly numel() contiguous elements in some dim
    order (contiguous, channels_last, any permutation)."""
    if t.is_contiguous():
        return True
    dims = sorted((d for d in range(t.dim()) if t.size(d) != 1), key=lambda d: t.stride(d))
    expect = 1
    for d in dims:
        if t.stride(d) != expect:
            return False
        expect *= t.size(d)
    return True


def _raw_flat(t: torch.Tensor) -> torch.Tensor:
    """1-D view of a dense tensor in its memory order (channels_last aware)."""
    if t.is_contiguous():
        return t.view(-1)
    if not is_dense(t):
        raise ValueError("mivod pack/unpack needs dense tensors")
    # permute to memory order, which is contiguous
    perm = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))
    return t.permute(*perm).reshape(-1)


def flat_cast(src: torch.Tensor, dst: torch.Tensor, scale: float = 1.0,
              nonfinite: Optional[torch.Tensor] = None) -> None:
    """dst = cast(src * scale); src and dst may alias (in-place scale)."""
    if _on_gpu(src):
        native().flat_cast(src, dst, float(scale), nonfinite)
        return
    dst.copy_(src.float() * scale)
    # the stored values, as in the kernel and in pack (an overflow of the cast counts)
    if nonfinite is not None and not bool(torch.isfinite(dst.float()).all()):
        nonfinite.fill_(1)


def nonfinite_scan(x: torch.Tensor, flag: torch.Tensor) -> None:
    """flag |= any non-finite element of ``x`` (read-only; the overflow guard's
    per-bucket check of the REDUCED gradient)."""
    if _on_gpu(x):
        native().nonfinite_scan(x, flag)
        return
    if not bool(torch.isfinite(x.float()).all()):
        flag.fill_(1)


# ---------------------------------------------------------------------------
# Local gradient accumulation in an fp32 arena (backward_passes_per_step > 1)
# ---------------------------------------------------------------------------
def _check_accum(tensors, acc, offsets) -> None:
    if len(tensors) != len(offsets):
        raise ValueError("accumulate: tensors/offsets length mismatch")
    if acc.dtype != torch.float32 or not acc.is_contiguous():
        raise ValueError("accumulate: acc must be a contiguous fp32 tensor")


def accumulate(tensors: Sequence[torch.Tensor], acc: torch.Tensor, offsets: Sequence[int],
               first: bool) -> None:
    """acc[off_i : off_i+n_i] = float(t_i) (``first``: a write, so the accumulator needs no
    zeroing) or += float(t_i), in the raw memory order of t_i: one multi-tensor launch.  The
    conversion is exact and each add rounds once to fp32.  Tensors of one call share a dtype;
    nothing outside the ranges is touched."""
    if not tensors:
        return
    _check_accum(tensors, acc, offsets)
    if _on_gpu(acc):
        native()._accum.accumulate(list(tensors), acc, [int(o) for o in offsets], bool(first))
        return
    for t, o in zip(tensors, offsets):
        src = _raw_flat(t).float()
        dst = acc[o:o + src.numel()]
        if first:
            dst.copy_(src)
        else:
            dst.add_(src)


def pack_accumulated(tensors: Sequence[torch.Tensor], acc: torch.Tensor, dst: torch.Tensor,
                     offsets: Sequence[int], scale: float = 1.0,
                     nonfinite: Optional[torch.Tensor] = None) -> None:
    """dst[off_i : off_i+n_i] = cast((acc[off_i : off_i+n_i] + float(t_i)) * scale): the last
    pass of an accumulation window fused with the wire cast of ``pack``.  The fp32 sum and the
    fp32 product are each rounded before the cast; ``acc`` is only read.  ``nonfinite``
    (optional) |= any stored value that is not finite, as in ``pack``."""
    if not tensors:
        return
    _check_accum(tensors, acc, offsets)
    if _on_gpu(dst):
        native()._accum.pack_accumulated(list(tensors), acc, dst, [int(o) for o in offsets],
                                         float(scale), nonfinite)
        return
    for t, o in zip(tensors, offsets):
        src = _raw_flat(t).float()
        out = dst[o:o + src.numel()]
        out.copy_((acc[o:o + src.numel()] + src) * scale)
        if nonfinite is not None and not bool(torch.isfinite(out.float()).all()):
            nonfinite.fill_(1)


# ---------------------------------------------------------------------------
# fp32 exponential moving average of the master weights (ema_decay of the Fused* optimizers)
# ---------------------------------------------------------------------------
def ema_omd(decay: float) -> float:
    """1 - decay taken in float64 and rounded once to fp32: the factor of ``ema_update``."""
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_update: decay must be in [0, 1), not {decay}")
    return float(torch.tensor(1.0 - decay, dtype=torch.float64).to(torch.float32))


def _check_ema(fn, w, e, model=None) -> None:
    for what, t in (("master", w), ("ema", e)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{fn}: {what} must be a contiguous fp32 tensor")
    if e.numel() != w.numel() or (model is not None and model.numel() != w.numel()):
        raise ValueError(f"{fn}: every stream must hold exactly {w.numel()} elements")


def ema_update(w: torch.Tensor, e: torch.Tensor, *, decay: float,
               skip: Optional[torch.Tensor] = None) -> None:
    """e = e + omd * (w - e) over two flat fp32 ranges of equal length, omd = fp32(1 - decay):
    a difference, a product and a sum, each rounded to fp32.  Where omd == 1 (decay 0) ``e``
    receives ``w`` itself, the copying first update.  ``w`` is only read.  ``skip``: device
    int32 flag; nonzero => nothing is stored (the overflow guard's)."""
    omd = ema_omd(decay)
    if _on_gpu(w):
        native()._ema.ema_update(w, e, float(decay), skip)
        return
    _check_ema("ema_update", w, e)
    if _skipped(skip):
        return
    if omd == 1.0:
        e.copy_(w)
        return
    d = w - e
    d.mul_(omd)
    e.add_(d)


def ema_swap(w: torch.Tensor, e: torch.Tensor, model: Optional[torch.Tensor], *,
             skip: Optional[torch.Tensor] = None) -> None:
    """(w, e) = (e, w) exactly, and model = cast(new w) where a model copy is given."""
    if _on_gpu(w):
        native()._ema.ema_swap(w, e, model, skip)
        return
    _check_ema("ema_swap", w, e, model)
    if _skipped(skip):
        return
    t = w.clone()
    w.copy_(e)
    e.copy_(t)
    if model is not None:
        model.copy_(w)


def ema_overwrite(w: torch.Tensor, e: torch.Tensor, model: Optional[torch.Tensor], *,
                  skip: Optional[torch.Tensor] = None) -> None:
    """w = e and model = cast(e); ``e`` is only read."""
    if _on_gpu(w):
        native()._ema.ema_overwrite(w, e, model, skip)
        return
    _check_ema("ema_overwrite", w, e, model)
    if _skipped(skip):
        return
    w.copy_(e)
    if model is not None:
        model.copy_(e)


# ---------------------------------------------------------------------------
# Global gradient-norm clipping (max_grad_norm of the Fused* optimizers)
# ---------------------------------------------------------------------------
def sumsq_chunks(n: int) -> int:
    """Entries of ``partial`` that ``grad_sumsq`` writes for ``n`` elements."""
    return (int(n) + CHUNK - 1) // CHUNK


def grad_sumsq(x: torch.Tensor, partial: torch.Tensor, flag: Optional[torch.Tensor] = None) -> None:
    """partial[b] = fp32 sum of squares of x[b*4096 : (b+1)*4096] for every chunk b of the
    flat bucket ``x`` (written, not accumulated; entries past the last chunk stay), reduced in
    a fixed order so that equal inputs give equal bits.  ``flag`` (optional) |= any non-finite
    element of ``x``, as ``nonfinite_scan``: the overflow guard's scan and the norm share one
    read-only pass."""
    n, nc = x.numel(), sumsq_chunks(x.numel())
    if _on_gpu(x):
        native()._clip.grad_sumsq(x, partial, flag)
        return
    if partial.dtype != torch.float32 or partial.numel() < nc:
        raise ValueError(f"grad_sumsq: partial must hold at least {nc} fp32 entries")
    if n == 0:
        return
    # the kernel's summation structure (csrc/kernels/mv_clip.hip): lane t of 256 adds its 8
    # consecutive elements of step 0, then of step 1; the 64-lane butterfly; the 4 waves in
    # order.  Zeros pad the last chunk (adding them is exact).
    v = torch.zeros(nc * CHUNK, dtype=torch.float32)
    v[:n] = x.reshape(-1).float()
    if flag is not None and not bool(torch.isfinite(v).all()):
        flag.fill_(1)
    sq = (v * v).view(nc, 2, 256, 8)
    acc = torch.zeros(nc, 256, dtype=torch.float32)
    for s in range(2):
        for j in range(8):
            acc = acc + sq[:, s, :, j]
    acc = acc.view(nc, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    tot = torch.zeros(nc, dtype=torch.float32)
    for w in range(4):
        tot = tot + acc[:, w, 0]
    partial[:nc].copy_(tot)


def clip_finalize(partial: torch.Tensor, total: int, clip: torch.Tensor, *, gscale: float,
                  max_norm: float) -> None:
    """clip[0] = min(1, max_norm / (norm + 1e-6)) and clip[1] = norm = gscale *
    sqrt(sum(partial[:total])) (torch.nn.utils.clip_grad_norm_'s coefficient), the sum, the
    root and the quotient in float64 and in a fixed order, each result rounded to fp32 once.
    A non-finite sum gives clip[0] = NaN (never a finite coefficient from a norm that is
    not)."""
    total = int(total)
    if _on_gpu(partial):
        native()._clip.clip_finalize(partial, total, float(gscale), float(max_norm), clip)
        return
    if total < 0 or partial.numel() < total or clip.numel() < 2:
        raise ValueError("clip_finalize: partial must hold total entries and clip 2")
    rows = max((total + 255) // 256, 1)
    p = torch.zeros(rows * 256, dtype=torch.float64)
    p[:total] = partial[:total].double()
    s = torch.zeros(256, dtype=torch.float64)
    for r in p.view(rows, 256):            # lane t adds partial[t], partial[t + 256], ..
        s = s + r
    h = 128
    while h:                               # the binary tree over the 256 lanes
        s = s[:h] + s[h:2 * h]
        h //= 2
    tot = float(s[0])
    norm = float(gscale) * math.sqrt(tot) if tot == tot else tot
    if math.isfinite(tot):
        q = float(max_norm) / (norm + 1e-6)
        coef = 1.0 if q > 1.0 else q
    else:
        coef = math.nan
    clip[0] = coef
    clip[1] = norm


def _clipped(gscale: float, gclip) -> float:
    """The fallbacks' gscale under a clip coefficient: fp32(gscale) * fp32(gclip[0]) rounded to
    fp32, the one product the kernels take."""
    if gclip is None:
        return gscale
    return float(torch.tensor(float(gscale), dtype=torch.float32) * gclip.reshape(-1)[0].float())


# ---------------------------------------------------------------------------
# K6 fused optimizers (flat)
# ---------------------------------------------------------------------------
def _skipped(skip) -> bool:
    return skip is not None and int(skip.reshape(-1)[0]) != 0


def sgd_step(g, w, mom, model, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
             gscale=1.0, nesterov=False, first=False, dyn=None, skip=None, gclip=None):
    """``dyn`` (GPU only): device fp32 [lr, first, bc1, bc2] read by the kernel in
    place of ``lr`` / ``first`` — the HIP-graph replay path (mivod.torch.graphs).
    ``skip``: device int32 flag; nonzero => no update (fp16-wire overflow guard).
    ``gclip`` (every step takes it): device fp32 clip coefficient (``clip_finalize``); the
    step runs with gscale * gclip[0], one fp32 product."""
    if _on_gpu(g):
        args = (g, w, mom, model, float(lr), float(momentum), float(dampening),
                float(weight_decay), float(gscale), bool(nesterov), bool(first), dyn, skip)
        if gclip is None:
            native().sgd_step(*args)
        else:
            native()._clip.sgd_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    d = g.float() * gscale + weight_decay * w
    if mom is not None:
        if first:
            mom.copy_(d)
        else:
            mom.mul_(momentum).add_(d, alpha=1.0 - dampening)
        d = d + momentum * mom if nesterov else mom
    w.sub_(lr * d)
    if model is not None:
        model.copy_(w)


def adam_step(g, w, m, v, model, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
              gscale=1.0, step=1, adamw=False, keras_eps=False, dyn=None, skip=None, gclip=None):
    if _on_gpu(g):
        args = (g, w, m, v, model, float(lr), float(beta1), float(beta2), float(eps),
                float(weight_decay), float(gscale), int(step), bool(adamw), bool(keras_eps), dyn,
                skip)
        if gclip is None:
            native().adam_step(*args)
        else:
            native()._clip.adam_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    gr = g.float() * gscale
    if not adamw and weight_decay:
        gr = gr + weight_decay * w
    m.mul_(beta1).add_(gr, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gr, gr, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    if adamw and weight_decay:
        w.mul_(1 - lr * weight_decay)
    if keras_eps:
        denom = (v.sqrt() + eps) / math.sqrt(bc2)
    else:
        denom = v.sqrt() / math.sqrt(bc2) + eps
    w.addcdiv_(m, denom, value=-lr / bc1)
    if model is not None:
        model.copy_(w)


def adadelta_step(g, w, sq, acc, model, *, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0,
                  gscale=1.0, dyn=None, skip=None, gclip=None):
    if _on_gpu(g):
        args = (g, w, sq, acc, model, float(lr), float(rho), float(eps), float(weight_decay),
                float(gscale), dyn, skip)
        if gclip is None:
            native().adadelta_step(*args)
        else:
            native()._clip.adadelta_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    gr = g.float() * gscale + weight_decay * w
    sq.mul_(rho).addcmul_(gr, gr, value=1 - rho)
    delta = (acc + eps).sqrt() / (sq + eps).sqrt() * gr
    acc.mul_(rho).addcmul_(delta, delta, value=1 - rho)
    w.sub_(lr * delta)
    if model is not None:
        model.copy_(w)


def rmsprop_step(g, w, sq, ga, buf, model, *, lr, alpha=0.99, eps=1e-8, weight_decay=0.0,
                 momentum=0.0, centered=False, gscale=1.0, dyn=None, skip=None, gclip=None):
    """RMSprop with torch.optim.RMSprop's semantics (eps outside the root, lr outside the
    momentum buffer).  With gr = g * gscale + wd * w: sq = alpha sq + (1-alpha) gr^2;
    centered: ga = alpha ga + (1-alpha) gr and avg = sqrt(max(sq - ga^2, 0)) + eps, else
    avg = sqrt(sq) + eps; with a momentum buffer buf = momentum buf + gr / avg and
    w -= lr buf, else w -= lr gr / avg.  The clamp at zero is the one deviation from torch,
    whose root of a difference that rounded below zero is NaN.  ``ga`` (``buf``) is the state
    of ``centered`` (``momentum``) and may be None without it; ``dyn[0]`` replaces ``lr``."""
    if centered and ga is None:
        raise ValueError("rmsprop_step: centered needs the grad_avg buffer")
    if momentum != 0 and buf is None:
        raise ValueError("rmsprop_step: momentum needs the momentum buffer")
    if not centered:
        ga = None
    if _on_gpu(g):
        args = (g, w, sq, ga, buf, model, float(lr), float(alpha), float(eps),
                float(weight_decay), float(momentum), float(gscale), dyn, skip)
        if gclip is None:
            native()._adaptive.rmsprop_step(*args)
        else:
            native()._clip.rmsprop_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    gr = g.float() * gscale + weight_decay * w
    sq.mul_(alpha).addcmul_(gr, gr, value=1 - alpha)
    if ga is not None:
        ga.mul_(alpha).add_(gr, alpha=1 - alpha)
        avg = (sq - ga * ga).clamp_(min=0).sqrt_().add_(eps)
    else:
        avg = sq.sqrt().add_(eps)
    q = gr / avg
    if buf is not None:
        buf.mul_(momentum).add_(q)
        q = buf
    w.sub_(lr * q)
    if model is not None:
        model.copy_(w)


def adagrad_step(g, w, sum, model, *, lr, eps=1e-10, weight_decay=0.0, gscale=1.0, dyn=None,
                 skip=None, gclip=None):
    """Adagrad with torch.optim.Adagrad's semantics: gr = g * gscale + wd * w, sum += gr^2,
    w -= lr gr / (sqrt(sum) + eps).  ``lr`` is the decayed rate lr0 / (1 + (step-1) lr_decay)
    of this step, taken by the caller; ``dyn[0]`` replaces it."""
    if _on_gpu(g):
        args = (g, w, sum, model, float(lr), float(eps), float(weight_decay), float(gscale), dyn,
                skip)
        if gclip is None:
            native()._adaptive.adagrad_step(*args)
        else:
            native()._clip.adagrad_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    gr = g.float() * gscale + weight_decay * w
    sum.addcmul_(gr, gr)
    w.sub_(lr * (gr / sum.sqrt().add_(eps)))
    if model is not None:
        model.copy_(w)


# ---- the rest of the Adam family (csrc/kernels/mv_adamfam.hip): amsgrad, Adamax, NAdam ----
def _adam_moments(g, w, m, v, beta1, beta2, weight_decay, gscale, coupled):
    """gr = g * gscale (+ wd * w), m = b1 m + (1-b1) gr and, with ``v``, v = b2 v + (1-b2) gr^2
    in place, in the kernels' order; returns gr."""
    gr = g.float() * gscale
    if coupled and weight_decay:
        gr = gr + weight_decay * w
    m.mul_(beta1).add_(gr, alpha=1 - beta1)
    if v is not None:
        v.mul_(beta2).addcmul_(gr, gr, value=1 - beta2)
    return gr


def adam_amsgrad_step(g, w, m, v, vmax, model, *, lr, beta1=0.9, beta2=0.999, eps=1e-8,
                      weight_decay=0.0, gscale=1.0, step=1, adamw=False, keras_eps=False,
                      dyn=None, skip=None, gclip=None):
    """``adam_step`` with amsgrad: vmax = max(vmax, v), taken on the uncorrected v as torch and
    Keras take it, replaces v in the denominator (either epsilon placement).  ``dyn`` (GPU
    only) = [lr, -, bc1, bc2]."""
    if _on_gpu(g):
        native()._adamfam.adam_amsgrad_step(
            g, w, m, v, vmax, model, float(lr), float(beta1), float(beta2), float(eps),
            float(weight_decay), float(gscale), int(step), bool(adamw), bool(keras_eps), dyn, skip,
            gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    _adam_moments(g, w, m, v, beta1, beta2, weight_decay, gscale, not adamw)
    torch.maximum(vmax, v, out=vmax)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    if adamw and weight_decay:
        w.mul_(1 - lr * weight_decay)
    if keras_eps:
        denom = (vmax.sqrt() + eps) / math.sqrt(bc2)
    else:
        denom = vmax.sqrt() / math.sqrt(bc2) + eps
    w.addcdiv_(m, denom, value=-lr / bc1)
    if model is not None:
        model.copy_(w)


def adamax_step(g, w, m, u, model, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                gscale=1.0, step=1, keras_eps=False, dyn=None, skip=None, gclip=None):
    """Adamax with torch.optim.Adamax's semantics: gr = g * gscale + wd * w,
    m = b1 m + (1-b1) gr, u = max(b2 u, |gr| + eps), w -= lr / (1 - b1^step) * m / u.
    ``keras_eps``: Keras' placement, u = max(b2 u, |gr|) and the divisor u + eps.  One deviation
    from torch: an element whose divisor is exactly 0 (eps = 0 and an all-zero history) takes no
    update, where torch's 0/0 is NaN.  ``dyn`` (GPU only) = [lr, -, bc1, -]."""
    if _on_gpu(g):
        native()._adamfam.adamax_step(
            g, w, m, u, model, float(lr), float(beta1), float(beta2), float(eps),
            float(weight_decay), float(gscale), int(step), bool(keras_eps), dyn, skip, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    gr = _adam_moments(g, w, m, None, beta1, beta2, weight_decay, gscale, True)
    a = gr.abs()
    torch.maximum(u.mul_(beta2), a if keras_eps else a.add_(eps), out=u)
    d = u + eps if keras_eps else u
    q = (lr / (1 - beta1 ** step)) * m / d
    w.sub_(torch.where(d != 0, q, torch.zeros_like(q)))
    if model is not None:
        model.copy_(w)


def nadam_coefficients(mu, mu_next, mu_product):
    """(cg, cm) of a NAdam step from mu_t, mu_{t+1} and P_t = mu_1 ... mu_t, in double: the
    weight of the gradient, (1 - mu_t) / (1 - P_t), and of the first moment,
    mu_{t+1} / (1 - P_t mu_{t+1})."""
    return (1.0 - mu) / (1.0 - mu_product), mu_next / (1.0 - mu_product * mu_next)


def nadam_mu(step, beta1, momentum_decay):
    """mu_step = beta1 (1 - 0.5 * 0.96^(step * momentum_decay)) of torch.optim.NAdam."""
    return beta1 * (1.0 - 0.5 * (0.96 ** (step * momentum_decay)))


def nadam_step(g, w, m, v, model, *, lr, cg, cm, bc2, beta1=0.9, beta2=0.999, eps=1e-8,
               weight_decay=0.0, gscale=1.0, adamw=False, dyn=None, skip=None, gclip=None):
    """NAdam with torch.optim.NAdam's semantics: m and v as in Adam,
    denom = sqrt(v / bc2) + eps, w -= lr cg gr / denom + lr cm m / denom with ``cg``, ``cm``
    (``nadam_coefficients``) and ``bc2`` = 1 - b2^step taken by the caller in double.
    ``adamw``: decoupled weight decay, w *= 1 - lr wd, instead of the coupled + wd w.
    ``dyn`` (GPU only) = [lr, cg, cm, bc2]."""
    if _on_gpu(g):
        native()._adamfam.nadam_step(
            g, w, m, v, model, float(lr), float(beta1), float(beta2), float(eps),
            float(weight_decay), float(gscale), float(cg), float(cm), float(bc2), bool(adamw), dyn,
            skip, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    gr = _adam_moments(g, w, m, v, beta1, beta2, weight_decay, gscale, not adamw)
    if adamw and weight_decay:
        w.mul_(1 - lr * weight_decay)
    denom = v.sqrt() / math.sqrt(bc2) + eps
    w.sub_(((lr * cg) * gr + (lr * cm) * m) / denom)
    if model is not None:
        model.copy_(w)


# ---------------------------------------------------------------------------
# Segment / chunk tables (LARS, Adasum)
# ---------------------------------------------------------------------------
@dataclass
class ChunkTable:
    seg_sizes: list
    begin: torch.Tensor
    len: torch.Tensor
    seg: torch.Tensor
    seg_c0: torch.Tensor
    seg_nc: torch.Tensor
    seg_offsets: list
    total: int
    # derived tables (e.g. Adasum's per-level clipped ranges), owned by this
    # table so they can never outlive it or be served to another table
    derived: dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def nchunks(self) -> int:
        return self.begin.numel()

    @property
    def nseg(self) -> int:
        return len(self.seg_sizes)


def make_chunk_table(seg_sizes: Sequence[int], device, seg_offsets: Optional[Sequence[int]] = None,
                     chunk: int = CHUNK) -> ChunkTable:
    """Chunk table of a flat buffer made of consecutive segments (optionally at
    explicit offsets, e.g. 64-element-aligned arena slots)."""
    if seg_offsets is None:
        seg_offsets, o = [], 0
        for s in seg_sizes:
            seg_offsets.append(o)
            o += s
    begin, ln, sg, c0, nc = [], [], [], [], []
    for i, (s, off) in enumerate(zip(seg_sizes, seg_offsets)):
        c0.append(len(begin))
        n = 0
        for b in range(0, max(int(s), 1), chunk):
            begin.append(int(off) + b)
            ln.append(int(min(chunk, s - b)) if s > 0 else 0)
            sg.append(i)
            n += 1
        nc.append(n)
    total = max((o + s for o, s in zip(seg_offsets, seg_sizes)), default=0)
    dev = torch.device(device)
    return ChunkTable(list(map(int, seg_sizes)),
                      torch.tensor(begin, dtype=torch.int64, device=dev),
                      torch.tensor(ln, dtype=torch.int32, device=dev),
                      torch.tensor(sg, dtype=torch.int32, device=dev),
                      torch.tensor(c0, dtype=torch.int32, device=dev),
                      torch.tensor(nc, dtype=torch.int32, device=dev),
                      list(map(int, seg_offsets)), int(total))


def _check_table(table: ChunkTable, numel: int) -> None:
    """Host-side bound check before a segmented launch: every chunk of the
    table must lie inside the buffers the kernel will index."""
    if table.total > numel:
        raise ValueError(f"mivod: chunk table covers {table.total} elements but the buffer "
                         f"has {numel}")


def lars_step(g, w, mom, model, table: ChunkTable, seg_flags: torch.Tensor, *, lr, momentum=0.9,
              weight_decay=0.0, eta=0.001, gscale=1.0, eps=0.0, first=False,
              workspace: Optional[dict] = None, dyn=None, skip=None, gclip=None):
    """Segmented LARS (You et al. 2017): per segment trust = eta*|w|/(|g|+wd*|w|);
    flagged segments (bit0) get trust 1 and no weight decay.  With ``gclip`` the norm |g| is
    that of the clipped gradient."""
    _check_table(table, g.numel())
    if _on_gpu(g):
        ws = workspace if workspace is not None else {}
        partial = ws.get("partial")
        if partial is None or partial.numel() < 2 * table.nchunks:
            partial = ws["partial"] = torch.empty(2 * table.nchunks, dtype=torch.float32,
                                                  device=g.device)
        norms = ws.get("norms")
        if norms is None or norms.numel() < 2 * table.nseg:
            norms = ws["norms"] = torch.empty(2 * table.nseg, dtype=torch.float32, device=g.device)
        args = (g, w, mom, model, table.begin, table.len, table.seg, table.seg_c0, table.seg_nc,
                seg_flags, partial, norms, float(lr), float(momentum), float(weight_decay),
                float(eta), float(gscale), float(eps), bool(first), dyn, skip)
        if gclip is None:
            native().lars_step(*args)
        else:
            native()._clip.lars_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    flags = seg_flags.tolist()
    for i, (off, n) in enumerate(zip(table.seg_offsets, table.seg_sizes)):
        sl = slice(off, off + n)
        wi, gi = w[sl], g[sl].float() * gscale
        skip = flags[i] & 1
        wd = 0.0 if skip else weight_decay
        wn, gn = float(wi.norm()), float(gi.norm())
        trust = 1.0
        if not skip and wn > 0 and gn > 0:
            trust = eta * wn / (gn + wd * wn + eps)
        d = lr * trust * (gi + wd * wi)
        if first:
            mom[sl].copy_(d)
        else:
            mom[sl].mul_(momentum).add_(d)
        wi.sub_(mom[sl])
        if model is not None:
            model[sl].copy_(wi)


def lamb_step(g, w, m, v, model, table: ChunkTable, seg_flags: torch.Tensor, *, lr, beta1=0.9,
              beta2=0.999, eps=1e-6, weight_decay=0.0, gscale=1.0, step=1,
              workspace: Optional[dict] = None, dyn=None, skip=None, gclip=None):
    """Segmented LAMB (You et al. 2019).  Per segment, with gr = g * gscale:
    m = b1 m + (1-b1) gr, v = b2 v + (1-b2) gr^2, u = (m/bc1) / (sqrt(v/bc2) + eps) + wd w,
    trust = |w| / |u| when both norms are positive (else 1), w -= lr trust u.  Flagged
    segments (bit0) get trust 1 and no weight decay.  ``dyn`` overrides lr, bc1 and bc2;
    ``skip`` leaves w, m, v and the model copy untouched.  On the GPU the workspace keeps
    ``norms`` = (|w|^2, |u|^2) per segment of the last call."""
    _check_table(table, g.numel())
    if _on_gpu(g):
        ws = workspace if workspace is not None else {}
        partial = ws.get("partial")
        if partial is None or partial.numel() < 2 * table.nchunks:
            partial = ws["partial"] = torch.empty(2 * table.nchunks, dtype=torch.float32,
                                                  device=g.device)
        norms = ws.get("norms")
        if norms is None or norms.numel() < 2 * table.nseg:
            norms = ws["norms"] = torch.empty(2 * table.nseg, dtype=torch.float32, device=g.device)
        args = (g, w, m, v, model, table.begin, table.len, table.seg, table.seg_c0, table.seg_nc,
                seg_flags, partial, norms, float(lr), float(beta1), float(beta2), float(eps),
                float(weight_decay), float(gscale), int(step), dyn, skip)
        if gclip is None:
            native()._lamb.lamb_step(*args)
        else:
            native()._clip.lamb_step(*args, gclip)
        return
    if _skipped(skip):
        return
    gscale = _clipped(gscale, gclip)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    flags = seg_flags.tolist()
    for i, (off, n) in enumerate(zip(table.seg_offsets, table.seg_sizes)):
        sl = slice(off, off + n)
        wi, mi, vi = w[sl], m[sl], v[sl]
        gr = g[sl].float() * gscale
        plain = flags[i] & 1
        wd = 0.0 if plain else weight_decay
        mi.mul_(beta1).add_(gr, alpha=1 - beta1)
        vi.mul_(beta2).addcmul_(gr, gr, value=1 - beta2)
        u = (mi / bc1) / (vi.sqrt() / math.sqrt(bc2) + eps) + wd * wi
        wn, un = math.sqrt(float((wi * wi).sum())), math.sqrt(float((u * u).sum()))
        trust = wn / un if (not plain and wn > 0 and un > 0) else 1.0
        wi.sub_(u, alpha=lr * trust)
        if model is not None:
            model[sl].copy_(wi)


def seg_dot3(a: torch.Tensor, b: torch.Tensor, table: ChunkTable,
             workspace: Optional[dict] = None) -> torch.Tensor:
    """Per segment (a.b, |a|^2, |b|^2) as a [nseg, 3] fp32 tensor (deterministic).
    ``a`` may be fp32 while ``b`` is the (fp16/bf16) wire copy."""
    _check_table(table, min(a.numel(), b.numel()))
    if _on_gpu(a):
        ws = workspace if workspace is not None else {}
        partial = ws.get("partial3")
        if partial is None or partial.numel() < 3 * table.nchunks:
            partial = ws["partial3"] = torch.empty(3 * table.nchunks, dtype=torch.float32,
                                                   device=a.device)
        out = torch.empty(3 * table.nseg, dtype=torch.float32, device=a.device)
        native().seg_dot3(a, b, table.begin, table.len, table.seg, table.seg_c0, table.seg_nc,
                          partial, out, False)
        return out.view(-1, 3)
    rows = []
    for off, n in zip(table.seg_offsets, table.seg_sizes):
        x, y = a[off:off + n].float(), b[off:off + n].float()
        rows.append(torch.stack([(x * y).sum(), (x * x).sum(), (y * y).sum()]))
    return torch.stack(rows) if rows else torch.zeros(0, 3)


def seg_dot3_into(a: torch.Tensor, b: torch.Tensor, table: ChunkTable, out: torch.Tensor,
                  swap: bool = False, workspace: Optional[dict] = None) -> None:
    """``seg_dot3`` written into ``out`` (a contiguous [nseg * 3] fp32 view, e.g.
    this rank's row of the Adasum Gram exchange buffer); ``swap`` stores
    (a.b, |b|^2, |a|^2) — a vector-halving level where ``a`` holds the upper
    group's vector — so no permute pass is needed."""
    _check_table(table, min(a.numel(), b.numel()))
    if out.numel() != 3 * table.nseg or not out.is_contiguous():
        raise ValueError("seg_dot3_into: out must be a contiguous [nseg * 3] buffer")
    if _on_gpu(a):
        ws = workspace if workspace is not None else _WS_DOT
        key = ("partial3", a.device)
        partial = ws.get(key)
        if partial is None or partial.numel() < 3 * table.nchunks:
            partial = ws[key] = torch.empty(max(3 * table.nchunks, 3 * 1024),
                                            dtype=torch.float32, device=a.device)
        native().seg_dot3(a, b, table.begin, table.len, table.seg, table.seg_c0, table.seg_nc,
                          partial, out, bool(swap))
        return
    d = seg_dot3(a, b, table)
    if swap:
        d = d[:, [0, 2, 1]]
    out.copy_(d.reshape(-1))


_WS_DOT: dict = {}


def adasum_merge(fin: torch.Tensor, f: torch.Tensor, r: torch.Tensor, table: ChunkTable,
                 rows: torch.Tensor, nrows: int, swap: bool,
                 emit: Optional[torch.Tensor] = None, elo: int = 0, ehi: int = 0) -> None:
    """One vector-halving Adasum level over ``table``'s chunks:
    f <- cf * fin + cr * r with (a.b, |a|^2, |b|^2) = the fixed-order sum of the
    ``nrows`` rows of ``rows`` ([nrows * nseg * 3]); ``fin`` is ``f`` or the wire
    bucket (level 0).  ``emit`` (wire dtype, full length) additionally gets
    cast(f) on the covered elements of [elo, ehi)."""
    _check_table(table, min(f.numel(), r.numel()))
    if _on_gpu(f):
        native().adasum_merge(fin, f, r, table.begin, table.len, table.seg, table.seg_c0,
                              table.seg_nc, rows, int(nrows), bool(swap), emit, int(elo), int(ehi))
        return
    R = rows.reshape(int(nrows), -1, 3)
    tot = R[0].clone()
    for g in range(1, int(nrows)):
        tot = tot + R[g]
    d = tot.tolist()
    for i, (off, n) in enumerate(zip(table.seg_offsets, table.seg_sizes)):
        if n <= 0:
            continue
        dot, na, nb = d[i]
        ca = 1.0 - dot / (2 * na) if na >= 1e-8 else 1.0
        cb = 1.0 - dot / (2 * nb) if nb >= 1e-8 else 1.0
        cf, cr = (cb, ca) if swap else (ca, cb)
        v = cf * fin[off:off + n].float() + cr * r[off:off + n].float()
        f[off:off + n].copy_(v)
        if emit is not None:
            a, b = max(off, elo), min(off + n, ehi)
            if b > a:
                emit[a:b].copy_(v[a - off:b - off])


def adasum_combine(a: torch.Tensor, b: torch.Tensor, table: ChunkTable, dots: torch.Tensor) -> None:
    """a <- (1 - d/(2|a|^2)) a + (1 - d/(2|b|^2)) b per segment."""
    _check_table(table, min(a.numel(), b.numel()))
    if _on_gpu(a):
        native().adasum_combine(a, b, table.begin, table.len, table.seg, table.seg_c0,
                                table.seg_nc, dots.reshape(-1).contiguous())
        return
    d = dots.reshape(-1, 3).tolist()
    for i, (off, n) in enumerate(zip(table.seg_offsets, table.seg_sizes)):
        dot, na, nb = d[i]
        ca = 1.0 - dot / (2 * na) if na >= 1e-8 else 1.0
        cb = 1.0 - dot / (2 * nb) if nb >= 1e-8 else 1.0
        x = a[off:off + n]
        x.copy_(ca * x.float() + cb * b[off:off + n].float())


def adasum_fcombine(f: torch.Tensor, r: torch.Tensor, table: ChunkTable, dots: torch.Tensor,
                    swap: bool) -> None:
    """Vector-halving Adasum merge on the fp32 running sum ``f`` with the received
    (wire-dtype) copy ``r``: ``dots`` rows are (a.b, |a|^2, |b|^2) with a = the
    lower rank group's vector; ``swap`` means ``f`` holds b.  f <- ca*a + cb*b."""
    _check_table(table, min(f.numel(), r.numel()))
    if _on_gpu(f):
        native().adasum_fcombine(f, r, table.begin, table.len, table.seg, table.seg_c0,
                                 table.seg_nc, dots.reshape(-1).contiguous(), bool(swap))
        return
    d = dots.reshape(-1, 3).tolist()
    for i, (off, n) in enumerate(zip(table.seg_offsets, table.seg_sizes)):
        if n <= 0:
            continue
        dot, na, nb = d[i]
        ca = 1.0 - dot / (2 * na) if na >= 1e-8 else 1.0
        cb = 1.0 - dot / (2 * nb) if nb >= 1e-8 else 1.0
        cf, cr = (cb, ca) if swap else (ca, cb)
        x = f[off:off + n]
        x.copy_(cf * x + cr * r[off:off + n].float())


def tensor_from_ptr(ptr: int, numel: int, dtype: torch.dtype, device) -> torch.Tensor:
    """A 1-D tensor over device memory mivod owns elsewhere (the xGMI mesh's
    IPC staging slot) — no copy; the owner must outlive the view."""
    dev = torch.device(device)
    return native().tensor_from_ptr(int(ptr), int(numel), dtype, dev.index or 0)
