"""float64 references and counted error bounds for the NHWC BatchNorm kernels
(csrc/kernels/mv_bn.hip, csrc/kernels/mv_bn_fin.h).

A helper module, not a test file: tests/test_bn_reference_cpu.py runs an fp32 emulation of
every pass through it and tests/test_bn_kernels_gpu.py the HIP kernels.

The check
---------
Every reference takes exactly the stored inputs (the bf16 activations and the fp32 vectors
cast up exactly) and ``momentum`` / ``eps`` as Python doubles, and computes each output in
float64 together with a per-element magnitude ``mag`` and a rounding count ``c``, as
tests/flat_reference.py does.  An fp32 output passes when, element by element,

    |got - ref| <= c * 2^-24 * mag          (U = 2^-24: one fp32 rounding, relative)

``mag`` is the sum of the absolute values of the terms on the way to the output.  A product
of two computed values carries the product of their magnitudes and the sum of their counts
(+ 1); through 1 / sqrt ``mag`` is carried by first-order sensitivity (without the factor
1/2, so the carried magnitude stays >= the value).  A hyperparameter reaches the kernel
rounded to fp32: one rounding at each use.  FMA contraction only removes roundings.

A bf16 output (y, dz, dx) whose fp32 value before the store is within ``delta`` of the
reference passes when

    |got - ref| <= delta + 2^-8 * (|ref| + delta)

(half an ulp of an 8-significant-bit value near ref); ``delta`` is carried from the
coefficient bounds plus the pass's own roundings.  delta == 0 and ref == 0 demand equality.

The ReLU masks of the backward references are the kernels' own (y_kernel > 0): the forward
check bounds y on both sides of zero, and the mode-3 bitmask must equal y_kernel > 0 bit for
bit, so no element is excluded anywhere.

Launch geometry (make_geo / round_geo / mv_bn_partials, mv_bn.hip:505-574)
---------------------------------------------------------------------------
CB = min(C, 256), TPR = CB / 8 lanes per row, RPI = 256 / TPR rows per iteration, RB = rows
per workgroup (a multiple of RPI), grid (ceil(M / RB), ceil(C / CB)).  A pass asks for
bx = min(resident / gy, ceil(M / 64), cap) row blocks (cap = the partial count for the
reduce passes, unbounded for apply / dx) and RB = roundup(ceil(M / bx), RPI).  ``resident``
(occupancy x CUs) is not known to a test: every bound takes the worst summation depth over
    min(ceil(M/64), cap, CUs / gy)  <=  bx  <=  min(ceil(M/64), cap, 8 CUs / gy)
(one to eight 256-lane workgroups per CU), with CUs from the device properties.

Summation depth of a reduction (n = RB / RPI rows per lane)
----------------------------------------------------------
Stage A, the lane's rows (stats_kernel :127-153, U = 8; bwd_reduce_kernel :369-417, U = 2):
  the unrolled loop adds U rows into a fresh partial sum (U - 1 roundings, 0 + a is exact)
  and that into the lane's sum (1 per iteration), the remainder loop 1 per row:
  n < U: n;  else U - 1 + n // U + n % U.
Stage B, the RPI-term serial LDS column sum (:163-168, :427-432): min(RPI, M), since the
  rows a short input leaves empty add exact zeros.
Stage C, fin_reduce (mv_bn_fin.h:23-58): ceil(P / 128) per accumulator, + 2 to join the
  four accumulators, + 5 xor steps (offsets 2..32), + 4 wave partials.
DEPTH = A + B + C, the worst over the geometries above.  A from-partials entry point has
stage C alone.

Counts (r = rounding of a hyperparameter, * + - / sqrt = one rounding each)
---------------------------------------------------------------------------
stats_kernel (:136-141)
  a = x - shift          1 (relative to |a| itself; 0 without a shift)
  s1 = sum a             1 + DEPTH        against sum |a|
  s2 = sum a*a           a twice 2, * 3, + DEPTH   against sum a^2
finalize_fwd_kernel (:180-195)
  inv_m = 1/(float)M     r, /  -> 2
  ms = s1*inv_m          c_s1 + 2, * -> c_s1 + 3              mag sum|a| / M
  var = s2*inv_m - ms*ms max(c_s2 + 3, 2 c_ms + 1) + 1        mag sum a^2 / M + (sum|a| / M)^2
                         (fmaxf(., 0) moves towards the true value)
  mean = sh + ms         c_ms + 1                             mag |sh| + mag_ms
  invstd = 1/sqrt(var + eps)   (eps r shares) + -> c_var + 1, sqrt, / -> c_var + 3
                         mag (mag_var + eps) / (var + eps)^1.5
  unb = var*(float)M/(float)(M-1)   r, *, r, / -> c_var + 4   (M == 1: var itself)
  1 - momentum           r, - -> 2 against k1 = |momentum| + |1 - momentum|
  rmean = (1-mom)*sh + mom*mean     max(2 + 1, c_mean + r + *) + 1 = c_mean + 3
                         mag k1 |sh| + |mom| mag_mean
  rvar  = (1-mom)*rvar + mom*unb    c_unb + 3                 mag k1 |rvar| + |mom| mag_unb
  scale = gamma*invstd   c_invstd + 1
  bias = beta - mean*scale          c_mean + c_scale + 1, - -> + 2
                         mag |beta| + mag_mean mag_scale
apply_kernel (:238-240), apply_colsum_kernel (:295)
  fma(x, scale, bias) counted as * and + = 2, + residual 3, against |x scale| + |bias| (+ |res|)
  delta_y = U (|x| c_scale mag_scale + c_bias mag_bias + 2 or 3 times the terms' magnitude)
  colsum partial: the stored bf16 values are added exactly as they are, so only the
  summation counts: n + RPI per partial (one serial sum per lane, :296/:307, :319)
bwd_reduce_kernel (:379, :393-394, :414-415)
  d = dy (+ dy2)         0 (1 with a second stream: the fp32 sum of two bf16 values)
  sdz = sum d            c_d + DEPTH          against sum |d|
  sdzx = sum d*(x - mu)  c_d, - 1, * 1 -> c_d + 2 + DEPTH   against sum |d| |x - mu|
  dz = bf16(d)           exact without a second stream, else delta = U |dy + dy2|
finalize_bwd_kernel (:444-453)
  dgamma = sdzx*is       c_sdzx + 1
  dbeta = sdz            c_sdz
  a = gamma*is           1
  b = -a*is*is*sdzx*inv_m      a 1, two * 3, sdzx: c_sdzx + 4, inv_m 2, * -> c_sdzx + 7
  cc = -a*sdz*inv_m - b*mean   max(1 + c_sdz + 1 + 2 + 1, c_b + 1) + 1 = c_b + 2
                         mag |a| mag_sdz / M + mag_b |mean|
bwd_dx_kernel (:485, :499)
  dx = a*e + (b*x + k)   b*x: c_b + 1;  + k: max(c_b + 1, c_cc) + 1 = c_cc + 1;
                         a*e: 2;  + -> c_cc + 2      against |a e| + mag_b |x| + mag_cc

Worst measured err / (U * mag) on an MI355X, as a fraction of c (bf16 outputs: err / bound)
--------------------------------------------------------------------------------------------
(tests/test_bn_kernels_gpu.py, 256 CUs; D = DEPTH of the statistics pass, 14 at M = 1 up to 67
at [524365, 64] and 290 at [3670017, 8]; D2 = DEPTH of the backward reduce; F = fin_depth(P))
  output         c                      read from                      worst / c
  mean           D + 5                  mv_bn.hip:182,184              0.07
  invstd         2 D + 13               :183,185                       0.07
  scale          2 D + 14               :193                           0.07
  bias           3 D + 21               :195                           0.05
  running_mean   D + 8                  :190                           0.10
  running_var    2 D + 17 (M = 1: +13)  :189,191                       0.05
  dgamma         D2 + 3 (+ 1 with dy2)  :394,415,445                   0.15
  dbeta          D2 (+ 1 with dy2)      :393,414,446                   0.08
  ca             1                      :449,451                       0.98
  cb             F + 7                  :450 (bn_bwd_coeffs)           0.19
  cc             F + 9                  :453 (bn_bwd_coeffs)           0.18
  colsum         n + min(RPI, M)        :296,307,319                   0.08
  from partials  the stored sums enter with c = F in place of 1 + D, 3 + D, D2, D2 + 2
  y, dz, dx      bf16 bound             :243,259,390,411,487,501       1.00
  (a tie rounds exactly half an ulp away, so a bf16 output reaches its bound; against the
  kernel's own stored scale / bias, where delta is two or three roundings, y also reaches 1.00)
No kernel missed a bound: no count was raised after the first GPU run and no kernel changed.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

U = 2.0 ** -24
HALF_BF16 = 2.0 ** -8

K_BLOCK, K_VEC, K_CB = 256, 8, 256
MIN_ROWS, P_CAP = 64, 2048
U_STATS, U_APPLY, U_BWD, U_COLSUM = 8, 4, 2, 2
FIN_SUB = 128                    # partial subsets per channel in fin_reduce
ASSUMED_CUS = 256                # the CPU tier's device


class Out(NamedTuple):
    ref: torch.Tensor          # float64
    mag: torch.Tensor          # float64, >= 0
    c: float


def f64(t: torch.Tensor) -> torch.Tensor:
    """float64 on the tensor's own device: the references run where the stored tensors are."""
    return t.detach().double()


def rows(t: torch.Tensor) -> torch.Tensor:
    """float64 [M, C] view of a stored [M, C] or [N, C, H, W] activation."""
    t = f64(t)
    return t if t.dim() != 4 else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _as(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    return rows(got) if got.dim() == 4 else f64(got).reshape(ref.shape)


# worst err / bound seen per output name in this process (printed by the tests)
WORST: dict = {}


def _note(name: str, frac: float) -> None:
    key = name.split(" ")[-1]
    WORST[key] = max(WORST.get(key, 0.0), frac)


def check(name: str, got: torch.Tensor, out: Out) -> float:
    """Assert |got - ref| <= c U mag; returns the worst err / (U mag) (compare with c)."""
    g = _as(got, out.ref)
    assert torch.isfinite(g).all(), f"{name}: non-finite result"
    err = (g - out.ref).abs()
    r = err / (U * out.mag)
    r = torch.where(out.mag > 0, r, torch.where(err == 0, torch.zeros_like(err),
                                                torch.full_like(err, math.inf)))
    if r.numel() == 0:
        return 0.0
    worst = float(r.max())
    bad = r > out.c
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {r.numel()} elements outside the bound, "
                           f"worst err/(U*mag) = {worst:.3g} at {int(r.argmax())}, c = {out.c:g}")
    _note(name, worst / out.c if out.c else 0.0)
    return worst


class Stored(NamedTuple):
    ref: torch.Tensor          # float64, the value before the bf16 store
    delta: torch.Tensor        # float64, bound on the fp32 error before the store


def bf16_bound(s: Stored) -> torch.Tensor:
    return s.delta + HALF_BF16 * (s.ref.abs() + s.delta)


def check_bf16(name: str, got: torch.Tensor, s: Stored) -> float:
    """Assert the bf16-output bound; returns the worst err / bound."""
    g = _as(got, s.ref)
    assert torch.isfinite(g).all(), f"{name}: non-finite result"
    err = (g - s.ref).abs()
    tol = bf16_bound(s)
    if err.numel() == 0:
        return 0.0
    bad = err > tol
    frac = torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err),
                                                       torch.full_like(err, math.inf)))
    worst = float(frac.max())
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {err.numel()} elements outside the bound, "
                           f"worst err/bound = {worst:.3g} at {int(frac.argmax())}")
    _note(name, worst)
    return worst


def outside(changed: torch.Tensor, out: Out) -> float:
    """max |changed - ref| / (c U mag): how far, in bounds, a changed reference lands.  A
    sensitivity guard asserts this > 1."""
    bound = out.c * U * out.mag
    d = (changed - out.ref).abs()
    sel = bound > 0
    return float((d[sel] / bound[sel]).max()) if sel.any() else 0.0


# --------------------------------------------------------------------------- geometry
class Geo(NamedTuple):
    M: int
    C: int
    CB: int
    TPR: int
    RPI: int
    RB: int
    gx: int
    gy: int

    @property
    def n(self) -> int:          # rows per lane of a full block
        return self.RB // self.RPI


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def make_geo(M: int, C: int, rows_per_block: int) -> Geo:
    CB = min(C, K_CB)
    TPR = CB // K_VEC
    RPI = K_BLOCK // TPR
    RB = _cdiv(max(rows_per_block, RPI), RPI) * RPI
    return Geo(M, C, CB, TPR, RPI, RB, _cdiv(M, RB), _cdiv(C, CB))


def partials(M: int, C: int) -> int:
    """mv_bn_partials: the [P][2][C] workspace rows of a reduction pass."""
    gy = _cdiv(C, min(C, K_CB))
    return max(1, min(_cdiv(M, 64), max(P_CAP // gy, 1)))


def round_geo(M: int, C: int, resident: int, cap: int, min_rows: int = MIN_ROWS) -> Geo:
    gy = make_geo(M, C, min_rows).gy
    bx = max(resident // gy, 1)
    bx = min(bx, _cdiv(M, min_rows), cap)
    bx = max(bx, 1)
    return make_geo(M, C, _cdiv(M, bx))


APPLY_CAP = 1 << 30


def geos(M: int, C: int, cus: int, cap: Optional[int] = None) -> list:
    """Every geometry round_geo can choose with one to eight workgroups per CU.
    cap None: a reduce pass (cap = partials); APPLY_CAP: apply / dx."""
    cap = partials(M, C) if cap is None else cap
    lo, hi = round_geo(M, C, cus, cap), round_geo(M, C, 8 * cus, cap)
    seen, out = set(), []
    gy = lo.gy
    bx_lo = max(1, min(max(cus // gy, 1), _cdiv(M, MIN_ROWS), cap))
    bx_hi = max(1, min(max(8 * cus // gy, 1), _cdiv(M, MIN_ROWS), cap))
    for bx in range(bx_lo, bx_hi + 1):
        g = make_geo(M, C, _cdiv(M, bx))
        if g.RB not in seen:
            seen.add(g.RB)
            out.append(g)
    assert lo.RB in seen and hi.RB in seen
    return out


def loops(g: Geo, unroll: int) -> tuple:
    """(the unrolled loop runs in some lane, the remainder loop runs in some lane)."""
    un = rem = False
    for rows in {min(g.RB, g.M - b * g.RB) for b in (0, g.gx - 1)}:
        q, part = divmod(rows, g.RPI)
        counts = {q} | ({q + 1} if part else set())
        un |= any(k >= unroll for k in counts)
        rem |= any(k % unroll for k in counts)
    return un, rem


def lane_depth(n: int, unroll: int) -> int:
    return n if n < unroll else unroll - 1 + n // unroll + n % unroll


def fin_depth(P: int) -> int:
    return _cdiv(P, FIN_SUB) + 2 + 5 + 4


def reduce_depth(M: int, C: int, cus: int, unroll: int) -> int:
    return max(lane_depth(g.n, unroll) + min(g.RPI, M) + fin_depth(g.gx)
               for g in geos(M, C, cus))


def colsum_depth(M: int, C: int, cus: int) -> int:
    return max(g.n + min(g.RPI, M) for g in geos(M, C, cus))


# --------------------------------------------------------------------------- forward
def stats_ref(x: torch.Tensor, shift: Optional[torch.Tensor], depth: int):
    """(S1, S2) of x [M, C] float64 around shift [C] (None: no shift)."""
    a = x if shift is None else x - shift
    c_a = 0 if shift is None else 1
    s2 = (a * a).sum(0)
    return Out(a.sum(0), a.abs().sum(0), c_a + depth), Out(s2, s2.clone(), 2 * c_a + 1 + depth)


def partial_sums(part: torch.Tensor):
    """(S1, S2) of stored fp32 [P, 2, C] partials: fin_reduce's roundings alone."""
    p = f64(part)
    d = fin_depth(p.shape[0])
    return Out(p[:, 0].sum(0), p[:, 0].abs().sum(0), d), Out(p[:, 1].sum(0), p[:, 1].abs().sum(0), d)


def finalize_fwd_ref(S1: Out, S2: Out, M: int, rm, rv, gamma, beta, momentum: float, eps: float,
                     unbiased: bool = True, m_used: Optional[int] = None) -> dict:
    """finalize_fwd_kernel.  ``unbiased=False`` / ``m_used`` build the changed references of
    the sensitivity guards."""
    Mk = M if m_used is None else m_used
    inv_m = 1.0 / Mk
    ms, mag_ms, c_ms = S1.ref * inv_m, S1.mag * inv_m, S1.c + 3
    var = (S2.ref * inv_m - ms * ms).clamp(min=0.0)
    mag_var = S2.mag * inv_m + mag_ms * mag_ms
    c_var = max(S2.c + 3, 2 * c_ms + 1) + 1
    sh = torch.zeros_like(ms) if rm is None else f64(rm)
    mean, mag_mean, c_mean = sh + ms, sh.abs() + mag_ms, c_ms + 1
    ve, mag_ve = var + eps, mag_var + eps
    invstd, mag_inv, c_inv = ve.rsqrt(), mag_ve / ve ** 1.5, c_var + 3
    out = {"var": Out(var, mag_var, c_var), "mean": Out(mean, mag_mean, c_mean),
           "invstd": Out(invstd, mag_inv, c_inv)}
    if rm is not None:
        rvo = f64(rv)
        f = Mk / (Mk - 1.0) if (Mk > 1 and unbiased) else 1.0
        unb, mag_unb, c_unb = var * f, mag_var * f, c_var + (4 if Mk > 1 else 0)
        k1 = abs(momentum) + abs(1.0 - momentum)
        out["running_mean"] = Out((1.0 - momentum) * sh + momentum * mean,
                                  k1 * sh.abs() + abs(momentum) * mag_mean, c_mean + 3)
        out["running_var"] = Out((1.0 - momentum) * rvo + momentum * unb,
                                 k1 * rvo.abs() + abs(momentum) * mag_unb, c_unb + 3)
    g = torch.ones_like(ms) if gamma is None else f64(gamma)
    b = torch.zeros_like(ms) if beta is None else f64(beta)
    sc, mag_sc, c_sc = g * invstd, g.abs() * mag_inv, c_inv + 1
    out["scale"] = Out(sc, mag_sc, c_sc)
    out["bias"] = Out(b - mean * sc, b.abs() + mag_mean * mag_sc, c_mean + c_sc + 2)
    return out


def exact(v: torch.Tensor) -> Out:
    """A stored fp32 vector used as an input: no error."""
    v = f64(v)
    return Out(v, v.abs(), 0)


def apply_ref(x: torch.Tensor, sc: Out, bi: Out, res: Optional[torch.Tensor], relu: bool) -> Stored:
    """apply_kernel on x [M, C] float64 with computed (or ``exact``) scale / bias."""
    pre = x * sc.ref + bi.ref
    terms = (x * sc.ref).abs() + bi.ref.abs()
    n = 2
    if res is not None:
        pre, terms, n = pre + res, terms + res.abs(), 3
    delta = U * (x.abs() * (sc.c * sc.mag) + bi.c * bi.mag + n * terms)
    return Stored(pre.clamp(min=0.0) if relu else pre, delta)


def fwd_ref(x, rm, rv, gamma, beta, momentum, eps, relu, res, cus, S=None, **kw) -> dict:
    """bn_fwd_train / bn_stats on stored tensors (x, res: bf16 [M, C] or channels_last 4-D).
    ``S``: (S1, S2) from stored partials instead of a statistics pass."""
    x2 = rows(x)
    M, C = x2.shape
    if S is None:
        S = stats_ref(x2, None if rm is None else f64(rm), reduce_depth(M, C, cus, U_STATS))
    out = finalize_fwd_ref(S[0], S[1], M, rm, rv, gamma, beta, momentum, eps, **kw)
    out["y"] = apply_ref(x2, out["scale"], out["bias"], None if res is None else rows(res), relu)
    return out


VEC_NAMES = ("mean", "invstd", "scale", "bias")


def check_vec(label: str, vec: torch.Tensor, ref: dict) -> dict:
    return {k: check(f"{label} {k}", vec[i], ref[k]) for i, k in enumerate(VEC_NAMES)}


def check_running(label: str, rm, rv, ref: dict) -> dict:
    return {"running_mean": check(f"{label} running_mean", rm, ref["running_mean"]),
            "running_var": check(f"{label} running_var", rv, ref["running_var"])}


# --------------------------------------------------------------------------- backward
def scatter_dy2(dy2: torch.Tensor, like: torch.Tensor, s: int) -> torch.Tensor:
    """A stride-s second gradient [N, C, ceil(H/s), ceil(W/s)] on the full grid, zero off it."""
    full = torch.zeros(like.shape, dtype=torch.float64, device=like.device)
    full[:, :, ::s, ::s] = f64(dy2)
    return full


def bwd_sums_ref(d: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, c_d: int, depth: int):
    xc = x - mean
    return (Out(d.sum(0), d.abs().sum(0), c_d + depth),
            Out((d * xc).sum(0), (d * xc).abs().sum(0), c_d + 2 + depth))


def finalize_bwd_ref(SDZ: Out, SDZX: Out, M: int, vec: torch.Tensor, gamma, m_used=None) -> dict:
    """finalize_bwd_kernel with the stored [4, C] vec as an exact input."""
    v = f64(vec).reshape(4, -1)
    mean, inv = v[0], v[1]
    g = torch.ones_like(mean) if gamma is None else f64(gamma)
    inv_m = 1.0 / (M if m_used is None else m_used)
    a = g * inv
    b, mag_b, c_b = -a * inv * inv * SDZX.ref * inv_m, a.abs() * inv * inv * SDZX.mag * inv_m, SDZX.c + 7
    cc = -a * SDZ.ref * inv_m - b * mean
    mag_cc = a.abs() * SDZ.mag * inv_m + mag_b * mean.abs()
    return {"dgamma": Out(SDZX.ref * inv, SDZX.mag * inv, SDZX.c + 1), "dbeta": SDZ,
            "ca": Out(a, a.abs(), 1), "cb": Out(b, mag_b, c_b), "cc": Out(cc, mag_cc, c_b + 2)}


WORK_NAMES = ("dgamma", "dbeta", "ca", "cb", "cc")


def dx_ref(d: torch.Tensor, x: torch.Tensor, co: dict, drop_cb: bool = False) -> Stored:
    a, b, k = co["ca"], co["cb"], co["cc"]
    ref = a.ref * d + ((0.0 if drop_cb else b.ref * x) + k.ref)
    delta = U * (k.c + 2) * ((a.ref * d).abs() + b.mag * x.abs() + k.mag)
    return Stored(ref, delta)


def bwd_ref(dy, dy2_full, x, mask, vec, gamma, cus, S=None, **kw) -> dict:
    """bn_bwd on stored tensors.  mask: bool [M, C] (the kernel's own y > 0) or None (mode 0);
    dy2_full: the second gradient on the full grid (float64 rows) or None; ``S``: (SDZ, SDZX)
    from stored partials (then dy is the stored dz)."""
    x2, d = rows(x), rows(dy)
    M, C = x2.shape
    c_d = 0
    if dy2_full is not None:
        d, c_d = d + dy2_full, 1
    if mask is not None:
        d = d * mask
    out = {"dz": Stored(d, U * c_d * d.abs())}
    mean = f64(vec).reshape(4, -1)[0]
    if S is None:
        S = bwd_sums_ref(d, x2, mean, c_d, reduce_depth(M, C, cus, U_BWD))
    out.update(finalize_bwd_ref(S[0], S[1], M, vec, gamma, **kw))
    # the dx pass reads the STORED dz (modes 2, 3); its own rounding is in that bound, so
    # the reference uses the fp64 d and widens delta by |ca| times dz's bound
    out["dx"] = dx_ref(d, x2, out)
    if c_d:
        out["dx"] = Stored(out["dx"].ref, out["dx"].delta + out["ca"].ref.abs() * bf16_bound(out["dz"]))
    return out


# --------------------------------------------------------------------------- partials
def split_points(M: int, P: int, seed: int = 0) -> list:
    """P + 1 non-decreasing row boundaries 0 .. M with repeated points (empty groups)."""
    gen = torch.Generator().manual_seed(seed)
    cut = torch.randint(0, M + 1, (P - 1,), generator=gen).sort().values.tolist() if P > 1 else []
    return [0] + cut + [M]


def make_partials(t1: torch.Tensor, t2: torch.Tensor, P: int, seed: int = 0) -> torch.Tensor:
    """fp32 [P, 2, C]: the float64 [M, C] terms summed over P contiguous row groups (some
    empty -> zero rows), rounded once."""
    M = t1.shape[0]
    pts = torch.tensor(split_points(M, P, seed), device=t1.device)
    zero = torch.zeros(1, t1.shape[1], dtype=torch.float64, device=t1.device)
    cs1, cs2 = torch.cat((zero, t1.cumsum(0))), torch.cat((zero, t2.cumsum(0)))
    p1, p2 = cs1[pts[1:]] - cs1[pts[:-1]], cs2[pts[1:]] - cs2[pts[:-1]]
    empty = (pts[1:] == pts[:-1])
    p1[empty], p2[empty] = 0.0, 0.0
    return torch.stack((p1, p2), 1).float()


# --------------------------------------------------------------------------- fp32 emulation
def _f32(v) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def emu_block_sums(t: torch.Tensor, g: Geo) -> torch.Tensor:
    """fp32 [gx, C] partials of the [M, C] fp32 terms: lane sums, then the RPI column sum."""
    M, C = t.shape
    pad = torch.zeros(g.gx * g.RB - M, C)
    t = torch.cat((t, pad)).view(g.gx, g.n, g.RPI, C)
    return t.sum(1).sum(1)


def emu_fin(p: torch.Tensor) -> torch.Tensor:
    """fin_reduce of fp32 [P, C]: per-subset sums, then across the 128 subsets."""
    P, C = p.shape
    k = _cdiv(P, FIN_SUB)
    p = torch.cat((p, torch.zeros(k * FIN_SUB - P, C))).view(k, FIN_SUB, C)
    return p.sum(0).sum(0)


def emu_finalize_fwd(s1, s2, M, rm, rv, gamma, beta, momentum, eps):
    """finalize_fwd_kernel in fp32 torch; updates rm / rv in place -> vec [4, C]."""
    inv_m = 1.0 / _f32(float(M))
    mom, ep = _f32(momentum), _f32(eps)
    sh = torch.zeros_like(s1) if rm is None else rm.clone()
    ms = s1 * inv_m
    var = (s2 * inv_m - ms * ms).clamp(min=0.0)
    mean = sh + ms
    invstd = 1.0 / torch.sqrt(var + ep)
    if rm is not None:
        unb = var * _f32(float(M)) / _f32(float(M - 1)) if M > 1 else var
        rm.copy_((1.0 - mom) * sh + mom * mean)
        rv.copy_((1.0 - mom) * rv + mom * unb)
    sc = invstd if gamma is None else gamma * invstd
    bi = -(mean * sc) if beta is None else beta - mean * sc
    return torch.stack((mean, invstd, sc, bi))


def emu_stats(x, shift, g: Geo):
    a = x.float() if shift is None else x.float() - shift
    return emu_fin(emu_block_sums(a, g)), emu_fin(emu_block_sums(a * a, g))


def emu_apply(x, sc, bi, res, relu):
    y = x.float() * sc + bi
    if res is not None:
        y = y + res.float()
    if relu:
        y = y.clamp(min=0.0)
    return y.to(torch.bfloat16)


def emu_fwd(x, rm, rv, gamma, beta, momentum, eps, relu, res, g: Geo, use_shift=True):
    """bn_fwd_train in fp32 torch on bf16 [M, C] -> (y bf16, vec); rm / rv updated in place."""
    s1, s2 = emu_stats(x, rm if use_shift else None, g)
    if rm is not None and not use_shift:        # the guard's variant: sums around zero
        vec = emu_finalize_fwd(s1, s2, x.shape[0], None, None, gamma, beta, momentum, eps)
    else:
        vec = emu_finalize_fwd(s1, s2, x.shape[0], rm, rv, gamma, beta, momentum, eps)
    return emu_apply(x, vec[2], vec[3], res, relu), vec


def emu_finalize_bwd(sdz, sdzx, M, vec, gamma):
    mean, inv = vec[0], vec[1]
    gm = torch.ones_like(inv) if gamma is None else gamma
    inv_m = 1.0 / _f32(float(M))
    a = gm * inv
    b = -a * inv * inv * sdzx * inv_m
    return torch.stack((sdzx * inv, sdz, a, b, -a * sdz * inv_m - b * mean))


def emu_bwd(dy, dy2, x, mask, vec, gamma, g: Geo):
    """bn_bwd in fp32 torch -> (dx bf16, work [5, C], dz bf16 or None)."""
    d = dy.float()
    if dy2 is not None:
        d = d + dy2.float()
    if mask is not None:
        d = d * mask
    dz = d.to(torch.bfloat16) if mask is not None else None
    xf = x.float()
    sdz = emu_fin(emu_block_sums(d, g))
    sdzx = emu_fin(emu_block_sums(d * (xf - vec[0]), g))
    work = emu_finalize_bwd(sdz, sdzx, x.shape[0], vec, gamma)
    e = d if dz is None else dz.float()
    dx = (work[2] * e + (work[3] * xf + work[4])).to(torch.bfloat16)
    return dx, work, dz


# --------------------------------------------------------------------------- inputs
CHANNELS = [8, 64, 96, 256, 320, 2048]


def edge_rows(C: int) -> list:
    """M = 1 (the variance guard) and every block-boundary / short-last-block row count."""
    rpi = make_geo(1, C, MIN_ROWS).RPI
    return sorted({1, 2, rpi - 1, rpi + 1, 63, 64, 65, 197, 1568} - {0})


REGIMES = ("near", "far", "far_norun")


def make_case(M: int, C: int, regime: str, seed: int = 0, shape=None) -> dict:
    """Stored inputs of one case, generated on the CPU: x, res, dy, dy2 bf16 [M, C] (or
    channels_last ``shape`` = (N, C, H, W)), gamma, beta, running statistics (None for
    far_norun).  near: x ~ 0.5 + 2 randn, running mean = the batch mean + 0.05 randn;
    far: x ~ 30 + 0.5 randn, running mean 0."""
    gen = torch.Generator().manual_seed(seed * 7919 + M * 31 + C)

    def act(scale=1.0, off=0.0):
        t = (torch.randn(M, C, generator=gen) * scale + off).to(torch.bfloat16)
        if shape is not None:
            n, c, h, w = shape
            t = t.view(n, h, w, c).permute(0, 3, 1, 2)
        return t

    x = act(2.0, 0.5) if regime == "near" else act(0.5, 30.0)
    t = {"x": x, "res": act(), "dy": act(), "dy2": act(),
         "gamma": torch.rand(C, generator=gen) + 0.5, "beta": torch.randn(C, generator=gen) * 0.1,
         "rm": None, "rv": None}
    if regime == "near":
        t["rm"] = (rows(x).mean(0) + 0.05 * torch.randn(C, generator=gen).double()).float()
        t["rv"] = torch.rand(C, generator=gen) + 0.5
    elif regime == "far":
        t["rm"], t["rv"] = torch.zeros(C), torch.rand(C, generator=gen) + 0.5
    return t


def fmt(worst: dict) -> str:
    return ", ".join(f"{k} {v:.2f}" for k, v in worst.items())


# --------------------------------------------------------------------------- the two tiers
def pack_bits(pos: torch.Tensor) -> torch.Tensor:
    """bool [M, C] -> uint8 [M, C / 8], bit j <=> channel 8 k + j (relu_bits, mv_bn.hip:200)."""
    M, C = pos.shape
    w = (1 << torch.arange(8, device=pos.device)).to(torch.int32)
    return (pos.view(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_bits(bits: torch.Tensor) -> torch.Tensor:
    w = (1 << torch.arange(8, device=bits.device)).to(torch.int32)
    return ((bits.to(torch.int32).unsqueeze(-1) & w) != 0).view(bits.shape[0], -1)


def rows_like(t: torch.Tensor) -> torch.Tensor:
    """[M, C] view in the stored dtype."""
    return t if t.dim() != 4 else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class Emu:
    """The fp32 emulation behind the bindings' call shapes (CPU tier): "an honest fp32
    implementation" in the kernels' order of stages, with ``resident`` workgroups."""

    def __init__(self, resident: int):
        self.resident = resident

    def _geo(self, M, C):
        return round_geo(M, C, self.resident, partials(M, C))

    def fwd(self, x, gamma, beta, rm, rv, momentum, eps, relu, res, want_mask):
        x2 = rows_like(x)
        y, vec = emu_fwd(x2, rm, rv, gamma, beta, momentum, eps, relu,
                         None if res is None else rows_like(res), self._geo(*x2.shape))
        return y, vec, (pack_bits(y > 0) if want_mask else None)

    def stats(self, x, gamma, beta, rm, rv, momentum, eps):
        return self.fwd(x, gamma, beta, rm, rv, momentum, eps, False, None, False)[1]

    def bwd(self, mode, dy, x, keep, vec, gamma, affine, dy2, s):
        x2 = rows_like(x)
        mask = None
        if mode == 1:
            mask = (x2.float() * vec[2] + vec[3]) > 0
        elif mode == 2:
            mask = rows_like(keep) > 0
        elif mode == 3:
            mask = unpack_bits(keep)
        if dy2 is not None and s > 1:
            full = torch.zeros(x.shape, dtype=dy2.dtype)
            full[:, :, ::s, ::s] = dy2
            dy2 = full
        dx, work, dz = emu_bwd(rows_like(dy), None if dy2 is None else rows_like(dy2), x2, mask,
                               vec, gamma, self._geo(*x2.shape))
        return dx, (work[0] if affine else None), (work[1] if affine else None), \
            (dz if mode >= 2 else None)

    def apply(self, x, scale, bias, relu, res):
        return emu_apply(rows_like(x), scale, bias, None if res is None else rows_like(res), relu)

    def finalize(self, stats, gamma, beta, rm, rv, momentum, eps, M):
        return emu_finalize_fwd(emu_fin(stats[:, 0]), emu_fin(stats[:, 1]), M, rm, rv, gamma, beta,
                                momentum, eps)

    def bwd_coeffs(self, vec, gamma, part, M):
        return emu_finalize_bwd(emu_fin(part[:, 0]), emu_fin(part[:, 1]), M, vec, gamma)

    def fwd_stats(self, x, stats, gamma, beta, rm, rv, momentum, eps, relu, res, want_mask):
        x2 = rows_like(x)
        vec = self.finalize(stats, gamma, beta, rm, rv, momentum, eps, x2.shape[0])
        y = emu_apply(x2, vec[2], vec[3], None if res is None else rows_like(res), relu)
        return y, vec, (pack_bits(y > 0) if want_mask else None)

    def bwd_from_partials(self, dz, x, vec, gamma, affine, part):
        work = self.bwd_coeffs(vec, gamma, part, rows_like(x).shape[0])
        dx = (work[2] * rows_like(dz).float() + (work[3] * rows_like(x).float() + work[4])).to(
            torch.bfloat16)
        return dx, (work[0] if affine else None), (work[1] if affine else None)

    def apply_colsum(self, x, scale, bias):
        y = emu_apply(x, scale, bias, None, True)
        return y, emu_block_sums(y.float(), self._geo(*x.shape))

    def stats_strided(self, x, s):
        xs = rows_like(x[:, :, ::s, ::s])
        return emu_fwd(xs, None, None, None, None, 0.0, 0.0, False, None, self._geo(*xs.shape))[1]


def _dev(t: dict, dev) -> dict:
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items()}


def _clone(v):
    return None if v is None else v.clone()


def _same(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a, b)


FWD_COMBOS = [(False, False), (True, False), (True, True), (False, True)]   # (relu, residual)
MODE_OF = {(False, False): 0, (False, True): 0, (True, False): 1, (True, True): 2}


def run_forward(impl, t: dict, cus: int, relu: bool, use_res: bool, momentum=0.1, eps=1e-5,
                gamma=True, beta=True, want_mask=False, label="fwd") -> tuple:
    """One training forward against float64, twice (bitwise equal).  Returns (worst ratios,
    the reference, (y, vec, mask bits) of the implementation)."""
    ga, be = (t["gamma"] if gamma else None), (t["beta"] if beta else None)
    res = t["res"] if use_res else None
    ref = fwd_ref(t["x"], t["rm"], t["rv"], ga, be, momentum, eps, relu, res, cus)
    outs = []
    for _ in range(2):
        rm, rv = _clone(t["rm"]), _clone(t["rv"])
        y, vec, bits = impl.fwd(t["x"], ga, be, rm, rv, momentum, eps, relu, res, want_mask)
        outs.append((y, vec, bits, rm, rv))
    for a, b in zip(*outs):
        assert _same(a, b), f"{label}: two calls differ"
    y, vec, bits, rm, rv = outs[0]
    worst = check_vec(label, vec, ref)
    if rm is not None:
        worst.update(check_running(label, rm, rv, ref))
    worst["y"] = check_bf16(f"{label} y", y, ref["y"])
    # the apply pass alone: from the implementation's OWN stored scale / bias (exact inputs)
    # only its two or three roundings remain.  With the coefficient checks above this
    # implies the bound just asserted, and it stays sharp where that one is wide (far shift)
    worst["y_own"] = check_bf16(f"{label} y_own", y, apply_ref(
        rows(t["x"]), exact(vec[2]), exact(vec[3]), None if res is None else rows(res), relu))
    if want_mask:
        assert torch.equal(bits.cpu(), pack_bits(rows_like(y).cpu() > 0)), \
            f"{label}: the bitmask is not y > 0"
    return worst, ref, (y, vec, bits)


def run_backward(impl, t: dict, cus: int, mode: int, fwd_out, gamma=True, affine=True,
                 dy2=None, stride=1, label="bwd") -> tuple:
    """bn_bwd of ``mode`` after the forward that produced ``fwd_out`` = (y, vec, bits),
    against float64 with the mask of the implementation's own output, twice."""
    y, vec, bits = fwd_out
    ga = t["gamma"] if gamma else None
    keep = {0: None, 1: None, 2: y, 3: bits}[mode]
    mask = None if mode == 0 else rows(y) > 0
    full = None
    if dy2 is not None:
        full = rows(dy2) if stride == 1 else rows(scatter_dy2(dy2, t["x"], stride))
    ref = bwd_ref(t["dy"], full, t["x"], mask, vec, ga, cus)
    outs = [impl.bwd(mode, t["dy"], t["x"], keep, vec, ga, affine, dy2, stride) for _ in range(2)]
    for a, b in zip(*outs):
        assert _same(a, b), f"{label}: two calls differ"
    dx, dg, db, dz = outs[0]
    worst = {"dx": check_bf16(f"{label} dx", dx, ref["dx"])}
    if affine:
        worst["dgamma"] = check(f"{label} dgamma", dg, ref["dgamma"])
        worst["dbeta"] = check(f"{label} dbeta", db, ref["dbeta"])
    else:
        assert dg is None and db is None, f"{label}: affine gradients returned"
    if mode >= 2:
        if dy2 is None:      # dz = the masked dy, exactly
            assert torch.equal(rows(dz), ref["dz"].ref), f"{label}: dz is not the masked dy"
        worst["dz"] = check_bf16(f"{label} dz", dz, ref["dz"])
    else:
        assert dz is None
    return worst, ref, outs[0]


def run_geometry_case(impl, M: int, C: int, cus: int, dev, regimes=REGIMES, seed=0,
                      lite=False) -> list:
    """Every forward form and backward mode of one [M, C] case in each data regime; the
    lines "label: output ratio ..." to print.  ``lite`` (the big-row cases): ReLU -> mode 1
    and add+ReLU with the bitmask -> mode 3, which between them run every pass's loops; or a
    list of (residual, mode) pairs."""
    lines = []
    for regime in regimes:
        t = _dev(make_case(M, C, regime, seed), dev)
        tag = f"C={C} M={M} {regime}"
        if lite:
            for use_res, mode in (((False, 1), (True, 3)) if lite is True else lite):
                w, _, out = run_forward(impl, t, cus, True, use_res, want_mask=use_res,
                                        label=f"fwd {tag} res={use_res}")
                lines.append(f"fwd {tag} relu=True res={use_res}: {fmt(w)}")
                wb, _, _ = run_backward(impl, t, cus, mode, out, label=f"bwd{mode} {tag}")
                lines.append(f"bwd{mode} {tag}: {fmt(wb)}")
            continue
        for relu, use_res in FWD_COMBOS:
            w, _, out = run_forward(impl, t, cus, relu, use_res, label=f"fwd {tag} relu={relu} res={use_res}")
            lines.append(f"fwd {tag} relu={relu} res={use_res}: {fmt(w)}")
            mode = MODE_OF[(relu, use_res)]
            if (relu, use_res) == (True, True):
                y_add = out[0]
            if (relu, use_res) == (False, True):
                continue                       # the same backward as (False, False)
            wb, _, _ = run_backward(impl, t, cus, mode, out, label=f"bwd{mode} {tag}")
            lines.append(f"bwd{mode} {tag}: {fmt(wb)}")
        # add+ReLU with the bitmask: the same y, the mask equal to y > 0, backward mode 3
        w, _, out3 = run_forward(impl, t, cus, True, True, want_mask=True, label=f"fwd_mask {tag}")
        assert torch.equal(out3[0], y_add), f"fwd_mask {tag}: y differs from the unmasked forward"
        wb, _, b3 = run_backward(impl, t, cus, 3, out3, label=f"bwd3 {tag}")
        lines.append(f"bwd3 {tag}: {fmt(wb)}")
        # statistics only
        rm, rv = _clone(t["rm"]), _clone(t["rv"])
        vec = impl.stats(t["x"], t["gamma"], t["beta"], rm, rv, 0.1, 1e-5)
        ref = fwd_ref(t["x"], t["rm"], t["rv"], t["gamma"], t["beta"], 0.1, 1e-5, False, None, cus)
        ws = check_vec(f"stats {tag}", vec, ref)
        if rm is not None:
            ws.update(check_running(f"stats {tag}", rm, rv, ref))
        lines.append(f"stats {tag}: {fmt(ws)}")
    return lines


def counts(M: int, C: int, cus: int) -> str:
    """The counts c of one case, to print next to the measured ratios."""
    d8, d2 = reduce_depth(M, C, cus, U_STATS), reduce_depth(M, C, cus, U_BWD)
    c_ms = 1 + d8 + 3
    c_var = max(3 + d8 + 3, 2 * c_ms + 1) + 1
    return (f"c: mean {c_ms + 1} invstd {c_var + 3} scale {c_var + 4} bias {c_ms + c_var + 7} "
            f"running_mean {c_ms + 4} running_var {c_var + 7} dgamma {d2 + 3} dbeta {d2}")


# --------------------------------------------------------------------------- sensitivity guards
def run_guards(impl, cus: int, dev, M: int = 1568, C: int = 64, forward_only=False) -> dict:
    """The implementation passes the case; each changed reference lands outside the bound of
    some output.  Returns {guard: how many bounds outside}."""
    t = _dev(make_case(M, C, "near", 3), dev)
    _, ref, out = run_forward(impl, t, cus, True, False, label="guard fwd")
    x2 = rows(t["x"])
    depth = reduce_depth(M, C, cus, U_STATS)
    rmf, args = f64(t["rm"]), (t["rm"], t["rv"], t["gamma"], t["beta"], 0.1, 1e-5)
    res = {}
    # one dropped row (the last): the mean moves by about |x - mean| / M
    S = stats_ref(x2[:-1], rmf, depth)
    drop = finalize_fwd_ref(S[0], S[1], M, *args)
    res["drop_row"] = max(outside(drop[k].ref, ref[k]) for k in ("mean", "invstd", "running_var"))
    if forward_only:
        return res
    _, bref, _ = run_backward(impl, t, cus, 1, out, label="guard bwd")
    S = stats_ref(x2, rmf, depth)
    res["m_minus_1"] = max(outside(finalize_fwd_ref(S[0], S[1], M, *args, m_used=M - 1)[k].ref, ref[k])
                           for k in ("mean", "invstd"))
    res["biased_running_var"] = outside(
        finalize_fwd_ref(S[0], S[1], M, *args, unbiased=False)["running_var"].ref, ref["running_var"])
    d = rows(t["dy"]) * (rows(out[0]) > 0)
    bad = dx_ref(d, x2, bref, drop_cb=True).ref
    res["drop_cb_x"] = float(((bad - bref["dx"].ref).abs() / bf16_bound(bref["dx"])).max())
    mm = bwd_ref(t["dy"], None, t["x"], rows(out[0]) > 0, out[1], t["gamma"], cus, m_used=M - 1)
    res["bwd_m_minus_1"] = max(outside(mm[k].ref, bref[k]) for k in ("cb", "cc"))
    return res


def run_shift_guard(cus: int, M: int = 1568, C: int = 64) -> float:
    """x ~ 30 + 0.5 randn with the running mean at the batch mean: an fp32 statistics pass
    that ignores the shift (sums around zero) lands outside the variance bound, which is
    taken around the shift.  Returns how many bounds outside."""
    t = make_case(M, C, "far", 5)
    t["rm"] = (rows(t["x"]).mean(0) + 0.05 * torch.randn(C, generator=torch.Generator().manual_seed(9)).double()).float()
    ref = fwd_ref(t["x"], t["rm"], t["rv"], t["gamma"], t["beta"], 0.1, 1e-5, False, None, cus)
    g = round_geo(M, C, 8 * cus, partials(M, C))
    _, good = emu_fwd(t["x"], t["rm"].clone(), t["rv"].clone(), t["gamma"], t["beta"], 0.1, 1e-5,
                      False, None, g)
    check("shift guard invstd", good[1], ref["invstd"])
    _, bad = emu_fwd(t["x"], t["rm"].clone(), t["rv"].clone(), t["gamma"], t["beta"], 0.1, 1e-5,
                     False, None, g, use_shift=False)
    return outside(f64(bad[1]), ref["invstd"])


# --------------------------------------------------------------------------- operand variants
VARIANT_SHAPES = [(197, 64), (1568, 64), (197, 320), (1568, 320)]
MOMENTA = [0.0, 0.1, 1.0]
EPSILONS = [1e-5, 1e-3, 0.5]


def run_variants(impl, M: int, C: int, cus: int, dev) -> list:
    """gamma / beta None, need_affine_grad False, the momentum and eps values."""
    t = _dev(make_case(M, C, "near", 1), dev)
    tag = f"C={C} M={M}"
    lines = []
    for ga, be in ((False, True), (True, False), (False, False)):
        lab = f"{tag} gamma={ga} beta={be}"
        w, _, out = run_forward(impl, t, cus, True, True, gamma=ga, beta=be, label=f"fwd {lab}")
        wb, _, _ = run_backward(impl, t, cus, 2, out, gamma=ga, label=f"bwd2 {lab}")
        lines.append(f"{lab}: {fmt(w)}; {fmt(wb)}")
    for mode, use_res in ((0, False), (1, False), (2, True)):
        _, _, out = run_forward(impl, t, cus, mode > 0, use_res, label=f"fwd {tag}")
        _, _, full = run_backward(impl, t, cus, mode, out, label=f"bwd{mode} {tag}")
        _, _, bare = run_backward(impl, t, cus, mode, out, affine=False,
                                  label=f"bwd{mode} {tag} no affine grad")
        assert torch.equal(bare[0], full[0]) and _same(bare[3], full[3]), \
            f"{tag} mode {mode}: dx / dz change with need_affine_grad"
    for mom in MOMENTA:
        for eps in EPSILONS:
            w, _, _ = run_forward(impl, t, cus, True, False, momentum=mom, eps=eps,
                                  label=f"fwd {tag} momentum={mom} eps={eps}")
            lines.append(f"{tag} momentum={mom} eps={eps}: {fmt(w)}")
    return lines


DY2_SHAPES = [(2, 7, 9), (3, 5, 5), (1, 1, 4), (2, 8, 8)]


def run_dy2(impl, nhw, C: int, stride: int, cus: int, dev) -> list:
    """Modes 2 and 3 with a second gradient stream at ``stride`` against float64 with the
    gradient scattered onto the full grid."""
    n, h, w = nhw
    M = n * h * w
    t = make_case(M, C, "near", 2, shape=(n, C, h, w))
    ho, wo = -(-h // stride), -(-w // stride)
    gen = torch.Generator().manual_seed(M + stride)
    t["dy2"] = torch.randn(n, ho, wo, C, generator=gen).to(torch.bfloat16).permute(0, 3, 1, 2)
    t = _dev(t, dev)
    tag = f"nhw={nhw} C={C} s={stride}"
    _, _, out = run_forward(impl, t, cus, True, True, want_mask=True, label=f"fwd {tag}")
    lines, got = [], {}
    for mode in (2, 3):
        wb, _, got[mode] = run_backward(impl, t, cus, mode, out, dy2=t["dy2"], stride=stride,
                                        label=f"bwd{mode} {tag}")
        lines.append(f"bwd{mode} {tag}: {fmt(wb)}")
    for a, b in zip(got[2], got[3]):
        assert _same(a, b), f"{tag}: mode 2 and mode 3 differ"
    return lines


# --------------------------------------------------------------------------- exact ReLU boundary
def boundary_case(dev) -> dict:
    """[64, 64] inputs of a from-partials forward whose scale is exactly 1 and whose bias is
    beta (statistics: mean 0, var 0.5, eps 0.5, no gamma, no running statistics), so the
    pre-activation x + beta (+ res) is exact: +0, -0, the smallest positive / negative bf16
    normal and exact cancellations at known positions."""
    M, C = 64, 64
    tiny = 2.0 ** -126
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(M, C, generator=gen).to(torch.bfloat16)
    res = (-x.float()).to(torch.bfloat16)             # x + res = +0 exactly
    beta = torch.zeros(C)
    beta[1::2] = -0.0                                 # odd channels: bias -0
    dy = (torch.randn(M, C, generator=gen).abs() + 1.0).to(torch.bfloat16)   # |dy| >= 1
    # rows 0-3: x = +0, -0, +tiny, -tiny with a zero residual of either sign
    for r, v in enumerate((0.0, -0.0, tiny, -tiny)):
        x[r] = v
        res[r, 0::4] = 0.0
        res[r, 1::4] = -0.0
        res[r, 2::4] = -0.0
        res[r, 3::4] = 0.0
    # rows 4-7 keep random x with res = 0: plain signs; the rest cancel to +0
    res[4:8] = 0.0
    part = torch.zeros(1, 2, C)
    part[0, 1] = 0.5 * M
    return _dev({"x": x, "res": res, "beta": beta, "dy": dy, "gamma": None, "part": part,
                 "rm": None, "rv": None, "M": M, "C": C}, dev)


def run_boundary(impl, cus: int, dev) -> None:
    t = boundary_case(dev)
    x, res, beta = rows(t["x"]), rows(t["res"]), f64(t["beta"])
    for use_res in (False, True):
        pre = x + beta + (res if use_res else 0.0)    # exact in float64
        pos = pre > 0
        assert int((pre == 0).sum()) > 100 and int(pos.sum()) > 100
        y, vec, bits = impl.fwd_stats(t["x"], t["part"], None, t["beta"], None, None, 0.1, 0.5,
                                      True, t["res"] if use_res else None, use_res)
        v = f64(vec)
        assert bool((v[2] == 1.0).all()), "scale is not exactly 1"
        assert torch.equal(v[3], beta) and torch.equal(v[0], torch.zeros_like(beta))
        assert torch.equal(rows(y), pre.clamp(min=0.0)), "forward output at the ReLU boundary"
        modes = (2, 3) if use_res else (1,)
        if use_res:
            assert torch.equal(bits.cpu(), pack_bits(pos).cpu()), "mode-3 bit at the ReLU boundary"
        for mode in modes:
            _, _, (dx, dg, db, dz) = run_backward(impl, t, cus, mode, (y, vec, bits), gamma=False,
                                                  label=f"boundary bwd{mode}")
            d = rows(t["dy"]) * pos
            if mode >= 2:
                assert torch.equal(rows(dz), d), f"mode {mode}: masked gradient at the boundary"
            # (mode 1 has no dz: run_backward held dbeta = sum d to its counted bound with the
            # mask y > 0, asserted equal to pre > 0 above; a wrong bit moves it by |dy| >= 1)


# --------------------------------------------------------------------------- other passes
def run_apply(impl, M: int, C: int, dev) -> list:
    """bn_apply: every relu x residual combination with stored scale / bias."""
    t = _dev(make_case(M, C, "near", 4), dev)
    gen = torch.Generator().manual_seed(M + C)
    sc = (torch.randn(C, generator=gen)).to(dev)
    bi = (torch.randn(C, generator=gen)).to(dev)
    lines = []
    for relu, use_res in FWD_COMBOS:
        res = t["res"] if use_res else None
        ys = [impl.apply(t["x"], sc, bi, relu, res) for _ in range(2)]
        assert torch.equal(ys[0], ys[1])
        ref = apply_ref(rows(t["x"]), exact(sc), exact(bi), None if res is None else rows(res), relu)
        lines.append(f"apply C={C} M={M} relu={relu} res={use_res}: y "
                     f"{check_bf16(f'apply C={C} M={M} y_apply', ys[0], ref):.2f}")
    return lines


def run_colsum(impl, M: int, C: int, cus: int, dev) -> str:
    t = _dev(make_case(M, C, "near", 5), dev)
    gen = torch.Generator().manual_seed(M + C + 1)
    sc, bi = torch.randn(C, generator=gen).to(dev), torch.randn(C, generator=gen).to(dev)
    outs = [impl.apply_colsum(t["x"], sc, bi) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    y, part = outs[0]
    wy = check_bf16(f"colsum C={C} M={M} y_colsum", y,
                    apply_ref(rows(t["x"]), exact(sc), exact(bi), None, True))
    assert part.dim() == 2 and part.shape[1] == C and 1 <= part.shape[0] <= partials(M, C)
    yk = rows(y)
    # adding stored bf16 values is the only rounding; the test's own float64 sum over the
    # P partials adds none
    ws = check(f"colsum C={C} M={M} colsum", f64(part).sum(0),
               Out(yk.sum(0), yk.abs().sum(0), colsum_depth(M, C, cus)))
    return f"colsum C={C} M={M}: y {wy:.2f}, sums {ws:.2f} (c = {colsum_depth(M, C, cus)})"


# odd H / W; at least 6 rows on the stride grid, so no channel has zero variance (eps = 0)
STRIDED_SHAPES = [(2, 7, 9), (3, 5, 5), (1, 5, 7), (2, 15, 13)]


def run_stats_strided(impl, nhw, C: int, stride: int, cus: int, dev) -> str:
    """bn_stats_strided on far-shift data (this path has no shift) against float64 over
    x[:, :, ::s, ::s]."""
    n, h, w = nhw
    t = _dev(make_case(n * h * w, C, "far_norun", 6, shape=(n, C, h, w)), dev)
    vecs = [impl.stats_strided(t["x"], stride) for _ in range(2)]
    assert torch.equal(vecs[0], vecs[1])
    xs = rows(f64(t["x"])[:, :, ::stride, ::stride])
    Ms = xs.shape[0]
    S = stats_ref(xs, None, reduce_depth(Ms, C, cus, U_STATS))
    ref = finalize_fwd_ref(S[0], S[1], Ms, None, None, None, None, 0.0, 0.0)
    w_ = check_vec(f"stats_strided nhw={nhw} C={C} s={stride}", vecs[0], ref)
    return f"stats_strided nhw={nhw} C={C} s={stride}: {fmt(w_)}"


# --------------------------------------------------------------------------- from partials
PARTIAL_COUNTS = [1, 2, 127, 128, 129, 384, 385, 512, 513, 1025, 2048]
PARTIAL_CHANNELS = [8, 64, 320]
PARTIAL_ROWS = [100, 3001]         # fewer and more rows than most partial counts


def run_from_partials(impl, P: int, C: int, M: int, cus: int, dev, regime="far") -> list:
    """bn_finalize, bn_fwd_train_stats (with and without the mask), bn_bwd_coeffs and
    bn_bwd_from_partials on [P, 2, C] partials built here: M rows in P contiguous groups
    (some empty), each summed in float64 around the shift and rounded once.  The expected
    result is the float64 finalize OF THOSE fp32 partials."""
    t = _dev(make_case(M, C, regime, 7), dev)
    x2 = rows(t["x"])
    a = x2 - f64(t["rm"])
    part = t["part"] = make_partials(a, a * a, P, seed=P)
    tag = f"P={P} C={C} M={M}"
    args = (t["gamma"], t["beta"], 0.1, 1e-5)
    S = partial_sums(part)
    ref = finalize_fwd_ref(S[0], S[1], M, t["rm"], t["rv"], *args)
    lines = []
    rm, rv = t["rm"].clone(), t["rv"].clone()
    vec = impl.finalize(t["part"], t["gamma"], t["beta"], rm, rv, 0.1, 1e-5, M)
    w = check_vec(f"finalize {tag}", vec, ref)
    w.update(check_running(f"finalize {tag}", rm, rv, ref))
    lines.append(f"finalize {tag}: {fmt(w)} (c_mean = {ref['mean'].c})")
    for want_mask in (False, True):
        rm2, rv2 = t["rm"].clone(), t["rv"].clone()
        y, vec2, bits = impl.fwd_stats(t["x"], t["part"], t["gamma"], t["beta"], rm2, rv2, 0.1,
                                       1e-5, True, t["res"], want_mask)
        assert torch.equal(vec2, vec) and torch.equal(rm2, rm) and torch.equal(rv2, rv), \
            f"fwd_stats {tag}: statistics differ from bn_finalize"
        ref["y"] = apply_ref(x2, ref["scale"], ref["bias"], rows(t["res"]), True)
        check_bf16(f"fwd_stats {tag} y", y, ref["y"])
        check_bf16(f"fwd_stats {tag} y_own", y,
                   apply_ref(x2, exact(vec[2]), exact(vec[3]), rows(t["res"]), True))
        if want_mask:
            assert torch.equal(bits.cpu(), pack_bits(rows_like(y).cpu() > 0))
    # backward: dz = the masked gradient; partials of (dz, dz (x - mean)) around the stored mean
    dz = (rows_like(t["dy"]).float() * (rows_like(y) > 0)).to(torch.bfloat16)
    d = rows(dz)
    mean = f64(vec)[0]
    bpart = make_partials(d, d * (x2 - mean), P, seed=P + 1).to(dev)
    Sb = partial_sums(bpart)
    bref = finalize_bwd_ref(Sb[0], Sb[1], M, vec, t["gamma"])
    work = impl.bwd_coeffs(vec, t["gamma"], bpart, M)
    wb = {k: check(f"bwd_coeffs {tag} {k}", work[i], bref[k]) for i, k in enumerate(WORK_NAMES)}
    lines.append(f"bwd_coeffs {tag}: {fmt(wb)} (c_cb = {bref['cb'].c})")
    dx, dg, db = impl.bwd_from_partials(dz, t["x"], vec, t["gamma"], True, bpart)
    assert torch.equal(dg, work[0]) and torch.equal(db, work[1])
    wd = check_bf16(f"bwd_from_partials {tag} dx", dx, dx_ref(d, x2, bref))
    dx2, dg2, db2 = impl.bwd_from_partials(dz, t["x"], vec, t["gamma"], False, bpart)
    assert torch.equal(dx2, dx) and dg2 is None and db2 is None
    lines.append(f"bwd_from_partials {tag}: dx {wd:.2f}")
    return lines
