"""float64 references and counted error bounds for the fused attention kernels
(csrc/kernels/mv_attn.hip), with an independent port of their dropout hash.

A helper module, not a test file: tests/test_attn_reference_cpu.py runs a torch emulation of
each kernel family's arithmetic (and named mutations of it) through it and
tests/test_attn_kernels_gpu.py the HIP kernels.

The check
---------
The references take exactly what the bindings take: the stored bf16 qkv [b, s, 3, h, 64] cast
up exactly, the fp32 key mask [b, s], the dropout keep mask of the Python port below (never the
kernels' own attn_dropout_mask) and, for the backward, the kernel's STORED out and lse, so that
the forward and the backward are checked independently.  Everything is float64.  The constants
enter as the fp32 values the kernels use (mv_bind_bert.cpp:37, mv_attn.hip:46, :622, :745):
SC = fp32(log2e / 8), LOG2E = fp32(log2e), QS = fp32(SC / LOG2E), and p as fp32.

U = 2^-24 is one fp32 rounding (relative), 2^-8 one bf16 rounding.  An fp32 output passes when
|got - ref| <= bound, a bf16 output whose fp32 value before the store is within ``delta`` of
the reference when

    |got - ref| <= delta + 2^-8 (|ref| + delta).

Nothing is excluded: every element of every output is compared, and a zero bound demands
equality.  First-order analysis: products of two error terms are dropped, except that a bf16
rounding is applied to value + fp32 error.

Scores (log2 domain)
--------------------
S2[q, k] = SC sum_d q_d k_d + mask_k LOG2E.  The error of the computed score is counted
against the two parts of A_k = SC sum_d |q_d k_d| + |mask_k LOG2E|:
  the dot product   64 (two chained 16x16x32 MFMAs, one rounding per accumulated product;
                    the bf16 x bf16 products are exact), * SC 1, + mask term 1  -> C_DOT = 66
                    (fwd_kernel :187,191-192; bwd :566,574; :795,802.  fwd_short_kernel
                    :341,347 adds before the scale, which rides in the exp's fma: 65)
  the mask term     fwd_short_kernel :347: LOG2E / sc 1, * 1, + 1 -> C_MASK = 3 (the others,
                    :192, :528, :747: * 1, + 1 = 2)
  w_k = C_DOT SC sum|q k| + C_MASK |mask LOG2E| + |x_k|, x_k = S2_k - m (forward) or S2_k - lse
  (backward): the last term is the rounding of the subtraction (or of the fma :374) that forms
  the exp's argument.  In fwd_kernel the argument is reached through the running maxima, S2_k -
  m_j and then m_j - m_j+1 ... (:204,210): the maxima only grow, so those roundings sum to at
  most U |x_k| too.  The kernel's own m (and msc = fl(m sc), :365) cancels between the exp
  arguments and lse = m + log2(l), so its value carries no error.
An error eps in the argument is a relative error <= eps of exp2 (ln 2 < 1); exp2f itself
counts 2.  A mask product that overflows fp32 (finfo.min) is -inf, as in the kernels.  A key
with P = 0 exactly (mask -10000: 2^-14427 underflows in float64 too; -inf) adds nothing to any
bound, so the size of its A_k does not matter.

Forward
-------
  l = sum_k e_k     relative error R_l = sum_k p_k w_k + 2 + DL; DL = 34 in fwd_short_kernel
                    (32 in-lane adds :377, two xor steps :379-380) and 20 nblk + 2 in fwd_kernel
                    (per 64-key block 16 adds :212, alpha's exp2f 2, * and + :214; :249-250)
  lse = m + log2(l) (:252, :395)   bound U (sum_k p_k w_k + LOG2E (2 + DL) + 2 |log2 l| + |lse|):
                    a relative error of l is LOG2E times that in log2 units, log2f 2, the add 1.
                    The score errors enter weighted by p_k: d lse / d S2_k = p_k.
  out = Z V, Z = keep P / (1 - p):
    delta = 2^-8 mag + (1 + 2^-8) U (sum_k Z_k |v_kd| (w_k + 2) + mag (R_l + 5 + DO))
            + 2^-126 / (1 - p) sum_k keep_k |v_kd|,          mag = sum_k Z_k |v_kd|
    2^-8: the ONE bf16 rounding of the unnormalised probability that feeds P.V as an MFMA
    operand (pack8 :241, :415); w_k + 2 its fp32 error; 5 = 1 / (1 - p) (-, / : 2), its
    product 1, 1 / l and its product 2 (:160,231,256,261; :398,426,428 the same five in
    another order); DO = s accumulated products (+ nblk rescales :221 in fwd_kernel); the last
    term an exp2f result below the fp32 normal range (l >= 1), over the keys with P > 0.
  A row whose keys are all -inf: out = 0 and lse = -inf exactly (:204,210,256; :372,426).

Backward (bwd_kernel :476-634 with delta_kernel and dq_reduce_kernel; bwd_short_kernel :650-907)
--------------------------------------------------------------------------------------------
  P = exp2(S2 - lse)       relative R_P = w_k + 2 (:574, :802); lse = -inf -> P = 0 (the row
                           is staged as +inf, :549-552, :717-720)
  delta = rowsum(dO out)   C_DELTA = 18 short (:731-734: two adds per j, two xor steps), 11
                           long (:463-467), against sum_d |dO out|
  dP = dO V^T              64 against sum_d |dO v| (:567, :796)
  z = keep P / (1 - p)     fp32 error U z (R_P + 3) (+ 2^-126 keep / (1 - p)), then bf16:
                           E_z = e_z + 2^-8 (z + e_z)  (:578,590; :806,820)
  dS = P (keep dP / (1 - p) - delta)     (:579-581, :807-809)
      e_dS = U (P ((64 + 3) keep |dP|mag / (1 - p) + C_DELTA |delta|mag) + |dS| (2 + R_P))
             (+ 2^-126 |keep dP / (1 - p) - delta|), then bf16 (:584, :814): E_dS as E_z
  dV = Z^T dO              delta = E_z^T |dO| + U s (Z^T |dO|)           (:594, :824)
  dK = QS dS^T Q           delta = QS (E_dS^T |Q| + U (s + 1) |dS|^T |Q|)  (:595,629; :825,899)
  dQ = QS dS K             delta = QS (E_dS |K| + U DQ |dS| |K|), DQ = s + 1 in bwd_short_kernel
                           (:838,844) and 64 + nkb + 1 through the fp32 partials and
                           dq_reduce_kernel's nkb-term sum (:607-615, :916-923)
  each then takes the bf16 output rounding.
  bsum (s <= 128, :846-889): fp32, against the float64 column sums over the tokens of the
  UNROUNDED dQ, dK, dV: bound = sum_tokens delta + C U sum_tokens (|ref| + delta), C = 16 for
  dQ (per 64-query block three adds, * QS, + : 5, :846; two xor steps :873-874; four terms
  :884) and 13 for dK, dV (four xor steps :860-863, * QS :865, eight terms :887).

The dropout port (mv_attn.hip:55-67, mv_common.h mix32, mv_bind_bert.cpp drop_thresh)
-------------------------------------------------------------------------------------
keep[b, h, q, k] = half(mix32(mix32(seed + (b H + h) 0x9E3779B1) ^ (q << 15 | k >> 1)), k & 1)
>= min(65535, floor(p 65536 + 0.5)), the low half for even k; uint32 arithmetic in numpy.

Worst measured err / bound per output
-------------------------------------
(tests/test_attn_kernels_gpu.py on an MI355X, 256 CUs, and the torch emulation on the CPU)
  output   bound                               read from                   MI355X   emulation
  out      bf16, delta above                   :241,261; :415,428          0.77     0.77
  lse      U (sum p w + LOG2E (2 + DL) + ...)  :252; :395                  0.03     0.04
  dq       bf16, QS (E_dS |K| + ...)           :607-615,844,916-927        0.86     0.86
  dk       bf16, QS (E_dS^T |Q| + ...)         :595,629; :825,899          0.84     0.84
  dv       bf16, E_z^T |dO| + ...              :594,630; :824,903          0.86     0.86
  bsum_q   U 16 + sum delta                    :846,873-884                0.33     0.33
  bsum_k   U 13 + sum delta                    :860-865,887                0.37     0.37
  bsum_v   U 13 + sum delta                    :860-866,887                0.39     0.39
  (the bf16 outputs and the column sums are dominated by the bf16 roundings of P and dS,
  which the emulation makes at the same values: hence the equal columns; lse alone is pure fp32)
No kernel missed a bound: no count was raised after the first GPU run.  One kernel change came
out of this suite: the backward kernels gave NaN in every dq, dk, dv element of a batch row
whose keys are all -inf (exp2f(-inf - (-inf))), fixed where lse is staged (:549-552, :717-720).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

U = 2.0 ** -24
HALF_BF16 = 2.0 ** -8
TINY = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)

D, KB, SHORT_MAX = 64, 64, 128
LOG2E32 = np.float32(1.4426950408889634)
SC32 = np.float32(1.4426950408889634 / 8.0)          # the binding's (float)(log2e / 8.0)
QS32 = SC32 / LOG2E32                                  # the kernels' p.scale_log2 / LOG2E
LOG2E, SC, QS = float(LOG2E32), float(SC32), float(QS32)

C_DOT, C_MASK = 66, 3
C_DELTA_SHORT, C_DELTA_LONG = 18, 11
C_BSUM_Q, C_BSUM_KV = 16, 13


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().double()


def nblk(s: int) -> int:
    return -(-s // KB)


def is_short(s: int) -> bool:
    return s <= SHORT_MAX


# --------------------------------------------------------------------------- dropout port
_M32 = np.uint64(0xFFFFFFFF)


def mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def drop_thresh(p: float) -> int:
    assert 0.0 <= p < 1.0
    return int(min(65535.0, math.floor(p * 65536.0 + 0.5)))


def drop_key(seed: int, bh: np.ndarray) -> np.ndarray:
    return mix32((np.uint64(seed & 0xFFFFFFFF) + bh.astype(np.uint64) * np.uint64(0x9E3779B1)) & _M32)


def drop_pair(dkey: np.ndarray, q: np.ndarray, k: np.ndarray) -> np.ndarray:
    ctr = ((q.astype(np.uint64) << np.uint64(15)) & _M32) | (k.astype(np.uint64) >> np.uint64(1))
    return mix32(dkey ^ ctr)


def drop_keep(pair_hash: np.ndarray, k: np.ndarray, thresh: int, swap_halves: bool = False) -> np.ndarray:
    odd = (k.astype(np.uint64) & np.uint64(1)) == np.uint64(1 if not swap_halves else 0)
    u16 = np.where(odd, pair_hash >> np.uint64(16), pair_hash & np.uint64(0xFFFF))
    return u16 >= np.uint64(thresh)


def keep_mask(b: int, h: int, s: int, p: float, seed: int, swap_halves: bool = False) -> torch.Tensor:
    """bool [b, h, s(q), s(k)] on the CPU: True where the probability is kept."""
    bh = np.arange(b * h, dtype=np.uint64).reshape(b * h, 1, 1)
    q = np.arange(s, dtype=np.uint64).reshape(1, s, 1)
    k = np.arange(s, dtype=np.uint64).reshape(1, 1, s)
    hp = drop_pair(drop_key(seed, bh), q, k)
    keep = drop_keep(hp, np.broadcast_to(k, hp.shape), drop_thresh(p), swap_halves)
    return torch.from_numpy(np.ascontiguousarray(keep)).view(b, h, s, s)


def inv_keep(p: float) -> float:
    """1 / (1 - p) with p as the fp32 the binding passes (its two roundings are counted)."""
    return 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0


# --------------------------------------------------------------------------- checks
# worst err / bound seen per output name in this process (printed by the tests)
WORST: dict = {}


def _note(name: str, frac: float) -> None:
    key = name.split(" ")[-1]
    WORST[key] = max(WORST.get(key, 0.0), frac)


def _ratio(err: torch.Tensor, tol: torch.Tensor) -> torch.Tensor:
    return torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err),
                                                       torch.full_like(err, math.inf)))


class Bound(NamedTuple):
    ref: torch.Tensor          # float64
    tol: torch.Tensor          # float64 >= 0: |got - ref| <= tol


class Stored(NamedTuple):
    ref: torch.Tensor          # float64, the value before the bf16 store
    delta: torch.Tensor        # float64, bound on the fp32 error before the store


def bf16_bound(s: Stored) -> torch.Tensor:
    return s.delta + HALF_BF16 * (s.ref.abs() + s.delta)


def ratio(got: torch.Tensor, want) -> torch.Tensor:
    """Element-wise |got - ref| / bound (inf where a zero bound is missed; an infinite
    reference (lse of a fully masked row) demands equality)."""
    ref = want.ref
    tol = bf16_bound(want) if isinstance(want, Stored) else want.tol
    g = f64(got).reshape(ref.shape)
    fin = torch.isfinite(ref)
    err = torch.where(fin, (g - torch.where(fin, ref, torch.zeros_like(ref))).abs(),
                      torch.where(g == ref, torch.zeros_like(ref), torch.full_like(ref, math.inf)))
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    return _ratio(err, torch.where(fin, tol, torch.zeros_like(tol)))


def check(name: str, got: torch.Tensor, want) -> float:
    """Assert the bound on every element; returns the worst err / bound."""
    r = ratio(got, want)
    if r.numel() == 0:
        return 0.0
    worst = float(r.max())
    bad = r > 1.0
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {r.numel()} elements outside the bound, "
                           f"worst err/bound = {worst:.3g} at {int(r.argmax())}")
    _note(name, worst)
    return worst


def fmt(worst: dict) -> str:
    return ", ".join(f"{k} {v:.2f}" for k, v in worst.items())


# --------------------------------------------------------------------------- references
def _split(qkv: torch.Tensor):
    q, k, v = f64(qkv).permute(2, 0, 3, 1, 4).unbind(0)              # [b, h, s, 64]
    return q, k, v


def _heads(t: torch.Tensor) -> torch.Tensor:
    return f64(t).permute(0, 2, 1, 3)                                 # [b, s, h, 64] -> [b, h, s, 64]


def _tokens(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 1, 3)


def mask_log2(mask: Optional[torch.Tensor]):
    """mask LOG2E in float64, -inf where the fp32 product overflows (finfo.min, -inf)."""
    if mask is None:
        return None
    m2 = f64(mask) * LOG2E
    return torch.where(m2 < -FLT_MAX, torch.full_like(m2, -math.inf), m2)


def scores(qkv: torch.Tensor, mask: Optional[torch.Tensor]):
    """(S2, cA) [b, h, s, s]: the log2-domain scores and their counted error magnitude
    C_DOT SC sum|q k| + C_MASK |mask LOG2E| (in units of U; inf for a -inf key)."""
    q, k, _ = _split(qkv)
    S2 = SC * (q @ k.transpose(-1, -2))
    cA = C_DOT * SC * (q.abs() @ k.abs().transpose(-1, -2))
    m2 = mask_log2(mask)
    if m2 is not None:
        S2 = S2 + m2[:, None, None, :]
        cA = cA + C_MASK * m2.abs()[:, None, None, :]
    return S2, cA


class Fwd(NamedTuple):
    out: Stored                # [b, s, h, 64]
    lse: Bound                 # [b, h, s]
    P: torch.Tensor            # [b, h, s, s]
    out64: torch.Tensor        # = out.ref


def fwd_ref(qkv: torch.Tensor, mask: Optional[torch.Tensor], keep: Optional[torch.Tensor],
            p: float) -> Fwd:
    b, s, _, h, _ = qkv.shape
    _, _, v = _split(qkv)
    S2, cA = scores(qkv, mask)
    m = S2.max(-1, keepdim=True).values
    dead = m == -math.inf
    x = torch.where(dead, torch.full_like(S2, -math.inf), S2 - torch.where(dead, torch.zeros_like(m), m))
    e = torch.exp2(x)
    l = e.sum(-1, keepdim=True)
    P = torch.where(dead, torch.zeros_like(e), e / torch.where(dead, torch.ones_like(l), l))
    log2l = torch.where(dead, torch.zeros_like(l), torch.log2(torch.where(dead, torch.ones_like(l), l)))
    lse = torch.where(dead, m, m + log2l)
    zero = torch.zeros_like(P)
    w = torch.where(P > 0, cA + x.abs(), zero)
    pw = (P * w).sum(-1, keepdim=True)
    DL = 34 if is_short(s) else 20 * nblk(s) + 2
    lse_tol = U * (pw + LOG2E * (2 + DL) + 2 * log2l.abs() + torch.where(dead, zero[..., :1], lse.abs()))
    lse_tol = torch.where(dead, zero[..., :1], lse_tol)
    ik = inv_keep(p)
    kz = torch.full_like(P, ik) if keep is None else keep.to(P.device).double() * ik
    Z = kz * P
    va = v.abs()
    mag = Z @ va
    DO = s + (0 if is_short(s) else nblk(s))
    Rl = pw + 2 + DL
    fp32 = (Z * (w + 2)) @ va + mag * (Rl + 5 + DO)
    delta = HALF_BF16 * mag + (1 + HALF_BF16) * U * fp32 + TINY * ((kz * (P > 0)) @ va)
    ref = Z @ v
    return Fwd(Stored(_tokens(ref), _tokens(delta)), Bound(lse.squeeze(-1), lse_tol.squeeze(-1)), P,
               _tokens(ref))


class Bwd(NamedTuple):
    dqkv: Stored               # [b, s, 3, h, 64]
    bsum: Bound                # [b, 3, h, 64]
    P: torch.Tensor


def bwd_ref(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor,
            mask: Optional[torch.Tensor], keep: Optional[torch.Tensor], p: float) -> Bwd:
    """``out`` / ``lse``: the STORED forward results."""
    b, s, _, h, _ = qkv.shape
    q, k, v = _split(qkv)
    o, do = _heads(out), _heads(dout)
    S2, cA = scores(qkv, mask)
    ls = f64(lse).reshape(b, h, s, 1)
    dead = ls == -math.inf
    x = torch.where(dead, torch.full_like(S2, -math.inf), S2 - torch.where(dead, torch.zeros_like(ls), ls))
    P = torch.exp2(x)
    zero = torch.zeros_like(P)
    RP = torch.where(P > 0, cA + x.abs() + 2, zero)
    ik = inv_keep(p)
    kz = torch.full_like(P, ik) if keep is None else keep.to(P.device).double() * ik
    short = is_short(s)
    c_delta = C_DELTA_SHORT if short else C_DELTA_LONG
    delta = (do * o).sum(-1, keepdim=True)
    mag_delta = (do * o).abs().sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    mag_dP = do.abs() @ v.abs().transpose(-1, -2)
    # dV
    Z = kz * P
    e_z = U * Z * (RP + 3) + TINY * kz * (P > 0)
    E_z = e_z + HALF_BF16 * (Z + e_z)
    doa = do.abs()
    dV = Z.transpose(-1, -2) @ do
    d_dV = E_z.transpose(-1, -2) @ doa + U * s * (Z.transpose(-1, -2) @ doa)
    # dS
    t = kz * dP - delta
    dS = P * t
    e_dS = U * (P * ((64 + 3) * kz * mag_dP + c_delta * mag_delta) + dS.abs() * (2 + RP)) + TINY * t.abs() * (P > 0)
    E_dS = e_dS + HALF_BF16 * (dS.abs() + e_dS)
    dSa = dS.abs()
    dQ = QS * (dS @ k)
    DQ = s + 1 if short else 64 + nblk(s) + 1
    d_dQ = QS * (E_dS @ k.abs() + U * DQ * (dSa @ k.abs()))
    dK = QS * (dS.transpose(-1, -2) @ q)
    d_dK = QS * (E_dS.transpose(-1, -2) @ q.abs() + U * (s + 1) * (dSa.transpose(-1, -2) @ q.abs()))
    ref = torch.stack((dQ, dK, dV))                      # [3, b, h, s, 64]
    dl = torch.stack((d_dQ, d_dK, d_dV))
    cs = torch.tensor([C_BSUM_Q, C_BSUM_KV, C_BSUM_KV], dtype=torch.float64,
                      device=ref.device).view(3, 1, 1, 1)
    bs_ref = ref.sum(3).permute(1, 0, 2, 3)              # [b, 3, h, 64]
    bs_tol = (dl.sum(3) + U * cs * (ref.abs() + dl).sum(3)).permute(1, 0, 2, 3)
    return Bwd(Stored(ref.permute(1, 3, 0, 2, 4), dl.permute(1, 3, 0, 2, 4)), Bound(bs_ref, bs_tol), P)


BSUM_NAMES = ("bsum_q", "bsum_k", "bsum_v")
GRAD_NAMES = ("dq", "dk", "dv")


def check_fwd(label: str, out: torch.Tensor, lse: torch.Tensor, ref: Fwd) -> dict:
    return {"out": check(f"{label} out", out, ref.out), "lse": check(f"{label} lse", lse, ref.lse)}


def check_bwd(label: str, dqkv: torch.Tensor, bsum: Optional[torch.Tensor], ref: Bwd) -> dict:
    worst = {}
    for i, nm in enumerate(GRAD_NAMES):
        worst[nm] = check(f"{label} {nm}", dqkv[:, :, i],
                          Stored(ref.dqkv.ref[:, :, i], ref.dqkv.delta[:, :, i]))
    if bsum is not None:
        b, s, _, h, _ = dqkv.shape
        got = bsum.view(b, 3, h, D)
        for i, nm in enumerate(BSUM_NAMES):
            worst[nm] = check(f"{label} {nm}", got[:, i], Bound(ref.bsum.ref[:, i], ref.bsum.tol[:, i]))
    return worst


def worst_ratio(got_fwd, ref: Fwd) -> dict:
    """max err / bound of (out, lse) without asserting: the mutation probes."""
    out, lse = got_fwd
    return {"out": float(ratio(out, ref.out).max()), "lse": float(ratio(lse, ref.lse).max())}


def worst_ratio_bwd(dqkv: torch.Tensor, ref: Bwd) -> dict:
    return {nm: float(ratio(dqkv[:, :, i], Stored(ref.dqkv.ref[:, :, i], ref.dqkv.delta[:, :, i])).max())
            for i, nm in enumerate(GRAD_NAMES)}


# --------------------------------------------------------------------------- inputs
SHORT_S = [1, 15, 16, 17, 63, 64, 65, 127, 128]
LONG_S = [129, 192, 193, 257]
BH = [(3, 2), (2, 3)]
# (b, s, h): every length with both head layouts, and b > h once per kernel family
SHAPES = [(b, s, h) for s in SHORT_S + LONG_S for b, h in BH] + [(5, 65, 1), (5, 193, 1)]
P_DROPS = [0.0, 0.1]
MASK_KINDS = ["none", "pad", "frac"]
SEED = 1234


def make_mask(kind: str, b: int, s: int, gen: torch.Generator) -> Optional[torch.Tensor]:
    """none; pad: -10000 on keys at the front and in the middle (the key s - 1 stays live);
    frac: randn * 2 per key, another row for every batch entry."""
    if kind == "none":
        return None
    if kind == "pad":
        m = torch.zeros(b, s)
        n = s // 8
        m[:, :n] = -10000.0
        m[:, s // 2:s // 2 + n] = -10000.0
        return m
    assert kind == "frac"
    return torch.randn(b, s, generator=gen) * 2.0


def make_case(b: int, s: int, h: int, kind: str, seed: int = 0) -> dict:
    """Stored inputs of one case on the CPU: qkv = randn * 1.5 and dout = randn in bf16, mask."""
    gen = torch.Generator().manual_seed(seed * 7919 + 1000 * b + 10 * s + h)
    qkv = (torch.randn(b, s, 3, h, D, generator=gen) * 1.5).to(torch.bfloat16)
    dout = torch.randn(b, s, h, D, generator=gen).to(torch.bfloat16)
    return {"qkv": qkv, "dout": dout, "mask": make_mask(kind, b, s, gen)}


def to_dev(t: dict, dev) -> dict:
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items()}


# --------------------------------------------------------------------------- fp32 emulation
def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def _decode(bh: int, b: int, h: int, mut) -> tuple:
    return (bh % b, bh // b) if "swap_bh" in mut else (bh // h, bh % h)


def emu_fwd(qkv, mask, keep, p: float, mut=frozenset()):
    """The forward of the family s selects, in fp32 torch on the CPU: fp32 scores and exp2,
    the probabilities rounded to bf16 where pack8 rounds them, fp32 sums.  fwd_short_kernel
    applies 1 / (1 - p) to O with the normalisation, fwd_kernel to the probabilities.
    ``mut``: named mutations (lose_last_key, pad_key, mask_ln, mask_batch0, swap_bh)."""
    b, s, _, h, _ = qkv.shape
    out = torch.zeros(b, s, h, D, dtype=torch.bfloat16)
    lse = torch.zeros(b * h, s)
    sc = torch.tensor(SC32)
    mlog = torch.tensor(np.float32(1.0) if "mask_ln" in mut else LOG2E32)
    ik = torch.tensor(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else torch.tensor(1.0)
    kp_all = None if keep is None else keep.view(b * h, s, s).float()
    ninf = torch.tensor(-math.inf)
    for bh in range(b * h):
        bi, hi = _decode(bh, b, h, mut)
        q, k, v = (qkv[bi, :, j, hi].float() for j in range(3))
        mrow = None if mask is None else mask[0 if "mask_batch0" in mut else bi].float()
        kp = torch.ones(s, s) if kp_all is None else kp_all[bh]
        if "lose_last_key" in mut:
            k, v, kp = k[:-1], v[:-1], kp[:, :-1]
            mrow = None if mrow is None else mrow[:-1]
        if "pad_key" in mut:
            k, v = torch.cat((k, torch.zeros(1, D))), torch.cat((v, torch.zeros(1, D)))
            kp = torch.cat((kp, torch.ones(s, 1)), 1)
            mrow = None if mrow is None else torch.cat((mrow, torch.zeros(1)))
        acc = q @ k.t()
        if is_short(s):
            sv = acc if mrow is None else acc + mrow * (mlog / sc)
            m = sv.max(-1, keepdim=True).values
            msc = m * sc
            e = torch.where(m == ninf, torch.zeros_like(sv), torch.exp2(sv * sc - msc))
            l = e.sum(-1, keepdim=True)
            lse[bh] = (msc + torch.log2(l)).squeeze(-1)
            O = _bf(e * kp) @ v
            inv = torch.where(l > 0, ik / l, torch.zeros_like(l))
            out[bi, :, hi] = (O * inv).to(torch.bfloat16)
        else:
            S = acc * sc
            if mrow is not None:
                S = S + mrow * mlog
            nk = S.shape[1]
            m_run, l_run, O = torch.full((s, 1), -math.inf), torch.zeros(s, 1), torch.zeros(s, D)
            for k0 in range(0, nk, KB):
                blk = S[:, k0:k0 + KB]
                m_new = torch.maximum(m_run, blk.max(-1, keepdim=True).values)
                deadr = m_new == ninf
                alpha = torch.where(deadr, torch.ones_like(m_new), torch.exp2(m_run - m_new))
                e = torch.where(deadr, torch.zeros_like(blk), torch.exp2(blk - m_new))
                l_run = l_run * alpha + e.sum(-1, keepdim=True)
                m_run = m_new
                O = O * alpha + _bf(e * kp[:, k0:k0 + KB] * ik) @ v[k0:k0 + KB]
            lse[bh] = (m_run + torch.log2(l_run)).squeeze(-1)
            inv = torch.where(l_run > 0, 1.0 / l_run, torch.zeros_like(l_run))
            out[bi, :, hi] = (O * inv).to(torch.bfloat16)
    return out, lse.view(b, h, s)


def emu_bwd(qkv, out, lse, dout, mask, keep, p: float, mut=frozenset(), out64=None):
    """The backward of the family s selects in fp32 torch -> (dqkv bf16, bsum fp32
    [b, 3 h 64] of the values before the bf16 store).  ``mut``: no_inv_keep_dp,
    delta_f64_out (delta from ``out64``, the float64 forward, not the stored bf16 out)."""
    b, s, _, h, _ = qkv.shape
    dqkv = torch.zeros(b, s, 3, h, D, dtype=torch.bfloat16)
    bsum = torch.zeros(b, 3, h, D)
    sc, qs = torch.tensor(SC32), torch.tensor(QS32)
    ik = torch.tensor(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else torch.tensor(1.0)
    kp_all = None if keep is None else keep.view(b * h, s, s).float()
    for bh in range(b * h):
        bi, hi = _decode(bh, b, h, mut)
        q, k, v = (qkv[bi, :, j, hi].float() for j in range(3))
        o, do = out[bi, :, hi].float(), dout[bi, :, hi].float()
        kp = torch.ones(s, s) if kp_all is None else kp_all[bh]
        ls = lse.reshape(b * h, s)[bh].reshape(s, 1)
        ls = torch.where(ls == -math.inf, torch.full_like(ls, math.inf), ls)
        S = (q @ k.t()) * sc
        if mask is not None:
            S = S + mask[bi].float() * torch.tensor(LOG2E32)
        pr = torch.exp2(S - ls)
        if "delta_f64_out" in mut:
            delta = (do.double() * out64[bi, :, hi].double()).sum(-1, keepdim=True).float()
        else:
            delta = (do * o).sum(-1, keepdim=True)
        dP = do @ v.t()
        z = kp * pr * ik
        dzd = kp * dP * (torch.tensor(1.0) if "no_inv_keep_dp" in mut else ik)
        ds = _bf(pr * (dzd - delta))
        dV = _bf(z).t() @ do
        dK = (ds.t() @ q) * qs
        if is_short(s):
            dQ = (ds @ k) * qs
        else:
            acc = torch.zeros(s, D)
            for k0 in range(0, s, KB):
                acc = acc + ds[:, k0:k0 + KB] @ k[k0:k0 + KB]
            dQ = acc * qs
        for j, g in enumerate((dQ, dK, dV)):
            dqkv[bi, :, j, hi] = g.to(torch.bfloat16)
            bsum[bi, j, hi] = g.sum(0)
    return dqkv, bsum.view(b, 3 * h * D)
