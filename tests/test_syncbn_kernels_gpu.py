"""SyncBatchNorm's kernels (csrc/kernels/mv_syncbn.hip) in one process with emulated ranks:
one batch split into N chunks, each chunk's statistics taken around a DIFFERENT shift, the
records stacked as the allgather would, then merge, apply, backward reduce, the summed
totals, global finalize and dx — against float64 BatchNorm over the concatenated bf16
inputs (dx from float64 autograd; per-rank dgamma / dbeta from the closed form over that
rank's rows with the global x-hat).  Tolerances: those of tests/test_bn_gpu.py; the merge
kernel alone is held to a bound counted from its own roundings (``_merge64``)."""
import pytest
import torch
import torch.nn.functional as F

from mivod.ops import kernels as K

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
U = 2.0 ** -24          # one fp32 rounding, relative
MODES = ["plain", "relu", "add_relu"]


def _chunk(n, c, h, w, dev, gen, mean=30.0):
    """bf16 NHWC, mean ~ 30 and standard deviation ~ 0.5: E[x^2] - E[x]^2 around a far
    shift cancels ~3600-fold, so a careless merge shows.  (Every operand of a rank is made
    by this one sequence of calls, so all have the same strides, 1 x 1 images included.)"""
    x = torch.randn(n, c, h, w, device=dev, generator=gen) * 0.5 + mean
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _rows(t):
    """[n, C, H, W] -> float64 [rows, C] in NHWC row order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double()


def _record(s1, s2, shift, n):
    """A statistics record as record_kernel lays it out: 3 C fp32 words + an int64 count."""
    dev = s1.device
    cnt = torch.tensor([n, 0], dtype=torch.int64).view(torch.int32).to(dev)
    return torch.cat((torch.cat((s1, s2, shift)).float().view(torch.int32), cnt))


def _count_of(rec, c):
    return int(rec[3 * c:].cpu().clone().view(torch.int64)[0])


def _sizes(n):
    """Unequal chunks of 1, 2 and 4 images of 3 x 5 pixels; from two ranks on, the last
    one holds a single row (M2 = 0)."""
    s = [((1, 2, 4)[r % 3], 3, 5) for r in range(n)]
    if n > 1:
        s[-1] = (1, 1, 1)
    return s


def _run(dev, sizes, c, mode, empty_at=None, min_p=1):
    nat = K.native()._syncbn
    gen = torch.Generator(device=dev).manual_seed(11)
    relu, use_res = mode != "plain", mode == "add_relu"
    n = len(sizes)
    xs = [_chunk(b, c, h, w, dev, gen) for b, h, w in sizes]
    ress = [_chunk(b, c, h, w, dev, gen, 0.0) for b, h, w in sizes] if use_res else [None] * n
    gs = [_chunk(b, c, h, w, dev, gen, 0.0) for b, h, w in sizes]
    wt = torch.rand(c, device=dev, generator=gen) + 0.5
    bs = torch.randn(c, device=dev, generator=gen) * 0.1
    rm0 = torch.randn(c, device=dev, generator=gen) * 0.1
    rv0 = torch.rand(c, device=dev, generator=gen) + 0.5

    # ---- forward: local statistics + record per rank, around shift_r = 3 r
    recs, ps = [], []
    for r, x in enumerate(xs):
        rec, p = nat.syncbn_stats(x, torch.full((c,), 3.0 * r, device=dev))
        rec2, _ = nat.syncbn_stats(x, torch.full((c,), 3.0 * r, device=dev))
        assert torch.equal(rec, rec2), "the statistics record is not deterministic"
        assert _count_of(rec, c) == x.numel() // c
        recs.append(rec)
        ps.append(p)
    assert max(ps) >= min_p, ps
    if empty_at is not None:        # a rank without rows: its sums must not be looked at
        one = torch.full((c,), 7.0, device=dev)
        recs.insert(empty_at, _record(one, one, one, 0))
    stack = torch.stack(recs)
    total = sum(x.numel() // c for x in xs)

    ys, keeps, rstats = [], [], []
    vec = count = None
    for r, x in enumerate(xs):
        rm, rv = rm0.clone(), rv0.clone()
        out = nat.syncbn_fwd(x, stack, wt, bs, rm, rv, MOM, EPS, relu, ress[r], use_res)
        if vec is None:
            vec, count = out[1], out[2]
        # every rank merges the same bytes in the same order: the same bits
        assert torch.equal(out[1], vec) and torch.equal(out[2], count)
        ys.append(out[0])
        keeps.append(out[3] if use_res else None)
        rstats.append(torch.cat((rm, rv)))
        assert torch.equal(rstats[r], rstats[0])
    assert int(count) == total

    # ---- float64 reference on the concatenated rows
    xc = torch.cat([_rows(x) for x in xs]).requires_grad_()
    z = F.batch_norm(xc, None, None, wt.double(), bs.double(), True, 0.0, EPS)
    if use_res:
        z = z + torch.cat([_rows(q) for q in ress])
    yk = torch.cat([_rows(y) for y in ys])
    torch.testing.assert_close(yk, (F.relu(z) if relu else z).detach(), rtol=2e-2, atol=2e-2)
    mean = xc.detach().mean(0)
    var = xc.detach().var(0, unbiased=False)
    unb = var * total / max(total - 1, 1)
    torch.testing.assert_close(vec[0].double(), mean, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rstats[0][:c].double(), (1 - MOM) * rm0.double() + MOM * mean,
                               rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rstats[0][c:].double(), (1 - MOM) * rv0.double() + MOM * unb,
                               rtol=1e-4, atol=1e-5)

    # ---- backward: local reduce per rank, the totals summed as the allreduce would
    mode_k = 3 if use_res else (1 if relu else 0)
    loc = [nat.syncbn_bwd_reduce(mode_k, gs[r], xs[r], keeps[r], vec, True) for r in range(n)]
    tot = torch.stack([q[0] for q in loc]).sum(0)
    if use_res:     # mode 2 (mask from the saved bf16 output) sees the same mask as mode 3
        for r in range(n):
            alt = nat.syncbn_bwd_reduce(2, gs[r], xs[r], ys[r], vec, True)
            assert torch.equal(alt[3], loc[r][3])
            for a, b in zip(alt[:3], loc[r][:3]):
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    dxs = [nat.syncbn_bwd_dx(mode_k, loc[r][3] if use_res else gs[r], xs[r], vec, wt, tot, count)
           for r in range(n)]
    # ReLU's derivative through the kernels' own output mask (torch's semantics: an output
    # within rounding of 0 may round either way; the forward check above bounds those)
    gc = torch.cat([_rows(g) for g in gs])
    dz = gc * (yk > 0) if relu else gc
    (z * dz).sum().backward()
    torch.testing.assert_close(torch.cat([_rows(d) for d in dxs]), xc.grad, rtol=3e-2, atol=3e-2)
    xhat = (xc.detach() - mean) * torch.rsqrt(var + EPS)
    o = 0
    for r, x in enumerate(xs):
        k = x.numel() // c
        sl = slice(o, o + k)
        o += k
        torch.testing.assert_close(loc[r][1].double(), (dz[sl] * xhat[sl]).sum(0), rtol=2e-2,
                                   atol=2e-2)
        torch.testing.assert_close(loc[r][2].double(), dz[sl].sum(0), rtol=2e-2, atol=2e-2)
        if use_res:
            torch.testing.assert_close(_rows(loc[r][3]), dz[sl], rtol=2e-2, atol=2e-2)
    return stack, ys, dxs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("c", [8, 24, 264])
def test_syncbn_emulated_ranks(cuda, c, n, mode):
    """C = 8 (the minimum), 24 (a partial finalize group of lanes), 264 (one 256-channel
    slab + an 8-channel one); 3 ranks also carry an empty rank's record in the middle."""
    assert K.available()
    _run(cuda, _sizes(n), c, mode, empty_at=1 if n == 3 else None)


def test_syncbn_many_partials_and_bitwise_repeat(cuda):
    """[8, 64, 56, 56] per rank: the local passes really produce P > 1 partials (asserted),
    and a second run gives the same bits."""
    a = _run(cuda, [(8, 56, 56), (8, 56, 56)], 64, "add_relu", min_p=2)
    b = _run(cuda, [(8, 56, 56), (8, 56, 56)], 64, "add_relu", min_p=2)
    assert torch.equal(a[0], b[0])
    for p, q in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(p, q)


# ---------------------------------------------------------------------------- merge alone
def _merge64(s1, s2, sh, ns):
    """merge_kernel in float64 on exactly the fp32 record values, with a running bound on
    the kernel's error: every fp32 rounding of the kernel adds U * |the value it rounds|,
    and earlier errors are carried by first-order sensitivity (the one squared error, d^2,
    exactly).  Roundings counted from the kernel source —
      per record (4):      (float)n_r, s1 / n_r, shift + ms, fma(-s1, ms, s2)
      per Chan step (11):  (float)n_a, (float)n, n_r / n  [w: 3 with (float)n_r's]
                           d = m_r - mean, d * w, mean + .          [mean: 3]
                           d * d, n_a * w, (d d)(n_a w), m2r + ., m2 + .   [M2: 5]
      finalize (5):        (float)n, M2 / n, + eps, sqrt, 1 / .
    (compiler FMA contraction only removes roundings; '/' and sqrtf are correctly rounded:
    the build passes no fast-math flag).  Returns mean, invstd, their bounds, the count."""
    n = 0
    mean = m2 = e_mean = e_m2 = None
    for r, nr in enumerate(ns):
        if nr <= 0:
            continue
        ms = s1[r] / nr
        e_ms = 2 * U * ms.abs()
        mr = sh[r] + ms
        e_mr = e_ms + U * mr.abs()
        q = s2[r] - s1[r] * ms
        e_m2r = s1[r].abs() * e_ms + U * q.abs()
        m2r = q.clamp(min=0)
        if n == 0:
            n, mean, m2, e_mean, e_m2 = nr, mr, m2r, e_mr, e_m2r
            continue
        fa = n
        n += nr
        w = nr / n
        e_w = 3 * U * w
        d = mr - mean
        e_d = e_mr + e_mean + U * d.abs()
        p = d * w
        e_p = e_d * w + d.abs() * e_w + U * p.abs()
        mean = mean + p
        e_mean = e_mean + e_p + U * mean.abs()
        k = fa * w
        e_k = 5 * U * k
        dd = d * d
        e_dd = 2 * d.abs() * e_d + e_d * e_d + U * dd
        t = dd * k
        e_t = e_dd * k + dd * e_k + U * t
        m2 = m2 + (m2r + t)
        e_m2 = e_m2 + e_m2r + e_t + U * (m2r + t) + U * m2
    var = m2 / n
    e_var = e_m2 / n + 2 * U * var
    v = var + EPS
    e_v = e_var + U * EPS + U * v
    s = v.sqrt()
    e_s = e_v / (2 * s) + U * s
    inv = 1 / s
    e_inv = e_s / (s * s) + U * inv
    return mean, inv, e_mean, e_inv, n


# products of two error terms, dropped above, are below 2^-10 of the first-order bound
SLACK = 1 + 2.0 ** -10


def test_syncbn_merge_alone_against_float64(cuda):
    """The merge kernel on synthetic records (unequal counts, one rank past 2^24 rows, an
    empty rank, a single-row rank, a different shift per rank) against a float64 merge of
    the same fp32 records, within the rounding bound of ``_merge64``; the total count is
    exact."""
    nat = K.native()._syncbn
    c = 264
    ns = [5000, 2 ** 24 + 1, 0, 1, 37, 100352, 7, 640]
    g = torch.Generator().manual_seed(4)
    s1s, s2s, shs, recs = [], [], [], []
    for r, nr in enumerate(ns):
        mu = 30 + torch.randn(c, generator=g, dtype=torch.float64)
        var = 0.25 * (torch.rand(c, generator=g, dtype=torch.float64) + 0.5) * (nr > 1)
        sh = torch.full((c,), 3.0 * r, dtype=torch.float64)
        s1 = (nr * (mu - sh)).float()
        s2 = (nr * (var + (mu - sh) ** 2)).float()
        recs.append(_record(s1.to(cuda), s2.to(cuda), sh.float().to(cuda), nr))
        s1s.append(s1.double())
        s2s.append(s2.double())
        shs.append(sh)
    gamma = (torch.rand(c, generator=g) + 0.5).to(cuda)
    beta = (torch.randn(c, generator=g) * 0.1).to(cuda)
    vec, count = nat.syncbn_merge(torch.stack(recs), gamma, beta, None, None, MOM, EPS)
    mean, inv, e_mean, e_inv, n = _merge64(s1s, s2s, shs, ns)
    assert int(count) == n == sum(ns) and n > 2 ** 24
    got = vec.double().cpu()
    err_mean, err_inv = (got[0] - mean).abs(), (got[1] - inv).abs()
    print("merge: max |mean err| / bound", float((err_mean / e_mean).max()),
          " max |invstd err| / bound", float((err_inv / e_inv).max()))
    assert (err_mean <= SLACK * e_mean).all(), float((err_mean / e_mean).max())
    assert (err_inv <= SLACK * e_inv).all(), float((err_inv / e_inv).max())
    # scale = gamma * invstd (one product), bias = beta - mean * scale (a product and a sum)
    assert torch.equal(vec[2], gamma * vec[1])
    mag = beta.abs().double() + (vec[0].double() * vec[2].double()).abs()
    assert ((vec[3].double() - (beta.double() - vec[0].double() * vec[2].double())).abs()
            <= 2 * U * mag).all()


def test_syncbn_record_count_exact_past_2_24(cuda):
    """2^24 + 1 rows: the record carries the count as an integer (fp32 would say 2^24)."""
    nat = K.native()._syncbn
    m = 2 ** 24 + 1
    x = torch.ones(m, 8, dtype=torch.bfloat16, device=cuda)
    rec, p = nat.syncbn_stats(x, None)
    assert p > 1 and _count_of(rec, 8) == m
    vec, count = nat.syncbn_merge(rec.unsqueeze(0), None, None, None, None, MOM, EPS)
    assert int(count) == m
    torch.testing.assert_close(vec[0], torch.ones(8, device=cuda), rtol=1e-6, atol=0)
