"""tests/attn_reference.py on the CPU: a torch emulation of each attention kernel family's
arithmetic (fp32 scores, exp2 and sums, bf16 where the kernels round) stays inside every
counted bound at every shape of tests/test_attn_kernels_gpu.py, every named mutation of that
emulation lands at least 4 bounds outside somewhere at the same inputs, and the Python port of
the dropout hash behaves like a fair coin."""
import math

import pytest
import torch

import attn_reference as R

CATCH = 4.0          # a mutation must exceed some bound by this factor


def _keep(b, s, h, p):
    return R.keep_mask(b, h, s, p, R.SEED) if p > 0 else None


_CACHE: dict = {}


def _case(b, s, h, kind, p):
    """One case with its emulated forward / backward and both references, computed once."""
    key = (b, s, h, kind, p)
    if key not in _CACHE:
        t = R.make_case(b, s, h, kind)
        keep = _keep(b, s, h, p)
        fref = R.fwd_ref(t["qkv"], t["mask"], keep, p)
        out, lse = R.emu_fwd(t["qkv"], t["mask"], keep, p)
        bref = R.bwd_ref(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)
        _CACHE[key] = (t, keep, fref, (out, lse), bref)
    return _CACHE[key]


@pytest.mark.parametrize("b,s,h", R.SHAPES)
def test_emulation_inside_every_bound(b, s, h):
    for kind in R.MASK_KINDS:
        for p in R.P_DROPS:
            t, keep, fref, (out, lse), bref = _case(b, s, h, kind, p)
            tag = f"b={b} s={s} h={h} {kind} p={p}"
            w = R.check_fwd(f"emu {tag}", out, lse, fref)
            dqkv, bsum = R.emu_bwd(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)
            w.update(R.check_bwd(f"emu {tag}", dqkv, bsum if R.is_short(s) else None, bref))
            print(f"{tag}: {R.fmt(w)}")


def test_zz_emulation_worst_ratios():
    """Not a check: the emulation's worst err / bound per output over this module's run."""
    print("attention emulation, worst err / bound: " + R.fmt(dict(sorted(R.WORST.items()))))


# --------------------------------------------------------------------------- mutations
def _fwd_mut(b, s, h, kind, p, mut, keep_mut=None):
    t, keep, fref, _, _ = _case(b, s, h, kind, p)
    got = R.emu_fwd(t["qkv"], t["mask"], keep if keep_mut is None else keep_mut, p, frozenset([mut]) if mut else frozenset())
    return R.worst_ratio(got, fref)


@pytest.mark.parametrize("s", [17, 65, 129])
@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("p", R.P_DROPS)
def test_lost_last_key_is_caught(s, kind, p):
    """An off-by-one at the key < s edge: with the front / middle mask layout the key s - 1 is
    live in every mask kind."""
    r = _fwd_mut(3, s, 2, kind, p, "lose_last_key")
    print(f"s={s} {kind} p={p}: {r}")
    assert r["lse"] >= CATCH and r["out"] >= CATCH, r


@pytest.mark.parametrize("s", [1, 17, 63, 65, 127, 129, 193, 257])
@pytest.mark.parametrize("kind", R.MASK_KINDS)
def test_padding_key_is_caught(s, kind):
    """The zero key at index s (score 0, value 0) joins the softmax."""
    r = _fwd_mut(2, s, 3, kind, 0.0, "pad_key")
    print(f"s={s} {kind}: {r}")
    assert r["lse"] >= CATCH, r


@pytest.mark.parametrize("s", [17, 128, 129])
def test_natural_log_mask_is_caught_by_the_fractional_mask(s):
    """mask * 1 where mask * log2(e) is due.  The fractional mask sees it; a mask of 0 /
    -10000 cannot (its dead keys are dead in either unit), which is why the suite has both."""
    r = _fwd_mut(3, s, 2, "frac", 0.0, "mask_ln")
    blind = _fwd_mut(3, s, 2, "pad", 0.0, "mask_ln")
    print(f"s={s}: frac {r}, pad {blind}")
    assert r["lse"] >= CATCH and r["out"] >= CATCH, r
    assert blind["lse"] <= 1.0 and blind["out"] <= 1.0, blind


@pytest.mark.parametrize("s", [17, 129])
def test_mask_row_of_batch_0_is_caught(s):
    r = _fwd_mut(3, s, 2, "frac", 0.0, "mask_batch0")
    print(f"s={s}: {r}")
    assert r["lse"] >= CATCH and r["out"] >= CATCH, r


@pytest.mark.parametrize("b,s,h", [(3, 17, 2), (2, 17, 3), (3, 129, 2), (2, 129, 3)])
def test_swapped_bh_decode_is_caught(b, s, h):
    """bh decoded as (bh % b, bh / b): the lse rows land permuted, and with dropout the
    (b, h) key of the hash belongs to another head's data.  (With h = 1 the two decodings are
    the same function, so the (5, 1) shapes cannot see this one; (3, 2) has b > h too.)"""
    r0 = _fwd_mut(b, s, h, "frac", 0.0, "swap_bh")
    r1 = _fwd_mut(b, s, h, "frac", 0.1, "swap_bh")
    print(f"b={b} s={s} h={h}: p=0 {r0}, p=0.1 {r1}")
    assert r0["lse"] >= CATCH and r1["out"] >= CATCH, (r0, r1)


@pytest.mark.parametrize("s", [16, 129])
def test_swapped_pair_halves_are_caught(s):
    b, h = 3, 2
    swapped = R.keep_mask(b, h, s, 0.1, R.SEED, swap_halves=True)
    r = _fwd_mut(b, s, h, "none", 0.1, None, keep_mut=swapped)
    print(f"s={s}: {r}")
    assert r["out"] >= CATCH, r


@pytest.mark.parametrize("s", [17, 129])
def test_missing_inv_keep_in_dp_is_caught(s):
    t, keep, _, (out, lse), bref = _case(3, s, 2, "frac", 0.1)
    dqkv, _ = R.emu_bwd(t["qkv"], out, lse, t["dout"], t["mask"], keep, 0.1, frozenset(["no_inv_keep_dp"]))
    r = R.worst_ratio_bwd(dqkv, bref)
    print(f"s={s}: {r}")
    assert r["dq"] >= CATCH and r["dk"] >= CATCH, r


@pytest.mark.parametrize("b,s,h", [(3, 1, 2), (2, 1, 3)])
def test_delta_from_the_float64_out_is_caught(b, s, h):
    """delta = rowsum(dO out) must use the STORED bf16 out.  The difference is one bf16
    rounding of out, which dS = P (dP / (1 - p) - delta) shows wherever the two terms nearly
    cancel: at s = 1 with dropout P = 1 and out = bf16(v / (1 - p)), so dS is exactly that
    rounding error against dO and a delta from the unrounded out gives 0 instead.  (At large s
    the bf16 rounding of dS itself hides it: measured below 1 bound at s = 17.)"""
    t, keep, fref, (out, lse), bref = _case(b, s, h, "none", 0.1)
    assert keep.any()
    dqkv, _ = R.emu_bwd(t["qkv"], out, lse, t["dout"], t["mask"], keep, 0.1,
                        frozenset(["delta_f64_out"]), out64=fref.out64)
    r = R.worst_ratio_bwd(dqkv, bref)
    print(f"b={b} h={h}: {r}")
    assert max(r["dq"], r["dk"]) >= CATCH, r


# --------------------------------------------------------------------------- -inf masks
def test_inf_keys_equal_removed_keys():
    """The references with some keys at -inf are the references of the problem without those
    keys: P is exactly 0 there and their dK / dV rows are exactly 0."""
    b, s, h, p = 2, 20, 3, 0.1
    t = R.make_case(b, s, h, "frac")
    dead = torch.tensor([0, 7, 8, 19])
    live = torch.tensor([i for i in range(s) if i not in dead.tolist()])
    t["mask"][:, dead] = -math.inf
    keep = R.keep_mask(b, h, s, p, R.SEED)
    fref = R.fwd_ref(t["qkv"], t["mask"], keep, p)
    assert (fref.P[..., dead] == 0).all() and torch.isfinite(fref.out.delta).all()
    # the same queries over the live keys alone
    q, k, v = R._split(t["qkv"])
    S2 = R.SC * (q @ k[:, :, live].transpose(-1, -2)) + (R.f64(t["mask"])[:, live] * R.LOG2E)[:, None, None, :]
    P = torch.softmax(S2 * math.log(2.0), -1)
    Z = keep[..., live].double() * P * R.inv_keep(p)
    torch.testing.assert_close(fref.out.ref, (Z @ v[:, :, live]).permute(0, 2, 1, 3), rtol=1e-12, atol=1e-13)
    out, lse = R.emu_fwd(t["qkv"], t["mask"], keep, p)
    R.check_fwd("inf keys", out, lse, fref)
    bref = R.bwd_ref(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)
    assert torch.isfinite(bref.dqkv.ref).all() and torch.isfinite(bref.dqkv.delta).all()
    assert (bref.dqkv.ref[:, dead, 1:] == 0).all() and (bref.dqkv.delta[:, dead, 1:] == 0).all()
    dqkv, bsum = R.emu_bwd(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)
    R.check_bwd("inf keys", dqkv, bsum, bref)


@pytest.mark.parametrize("s", [128, 129])
@pytest.mark.parametrize("value", [-math.inf, torch.finfo(torch.float32).min])
def test_fully_masked_batch_row_contract(s, value):
    """out = 0, lse = -inf and zero gradients for the batch row whose keys are all -inf."""
    b, h, p = 3, 2, 0.1
    t = R.make_case(b, s, h, "frac")
    t["mask"][1] = value
    keep = R.keep_mask(b, h, s, p, R.SEED)
    fref = R.fwd_ref(t["qkv"], t["mask"], keep, p)
    assert (fref.out.ref[1] == 0).all() and (fref.out.delta[1] == 0).all()
    assert (fref.lse.ref[1] == -math.inf).all()
    out, lse = R.emu_fwd(t["qkv"], t["mask"], keep, p)
    R.check_fwd("masked row", out, lse, fref)
    bref = R.bwd_ref(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)
    assert torch.isfinite(bref.dqkv.ref).all()
    assert (bref.dqkv.ref[1] == 0).all() and (bref.dqkv.delta[1] == 0).all()
    dqkv, bsum = R.emu_bwd(t["qkv"], out, lse, t["dout"], t["mask"], keep, p)
    R.check_bwd("masked row", dqkv, bsum if R.is_short(s) else None, bref)


# --------------------------------------------------------------------------- dropout port
def test_port_known_values():
    """mix32 by hand: 0 is a fixed point; 1 -> 1 * 0x7feb352d = 0x7feb352d, ^ >> 15 =
    0x7feb352d ^ 0xffd6 = 0x7febcafb, * 0x846ca68b mod 2^32, ^ >> 16."""
    import numpy as np
    assert int(R.mix32(np.array([0], dtype=np.uint64))[0]) == 0
    x = 0x7FEB352D
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(R.mix32(np.array([1], dtype=np.uint64))[0]) == x
    assert R.drop_thresh(0.0) == 0 and R.drop_thresh(0.1) == 6554 and R.drop_thresh(0.9999999) == 65535
    assert R.keep_mask(2, 2, 9, 0.0, 5).all()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_port_keep_fraction_and_pair_independence(p):
    b, h, s = 3, 2, 256
    keep = R.keep_mask(b, h, s, p, R.SEED)
    pk = 1.0 - R.drop_thresh(p) / 65536.0
    n = s * s
    sd = math.sqrt(pk * (1 - pk) / n)
    frac = keep.double().mean((-1, -2))
    assert ((frac - pk).abs() <= 4 * sd).all(), (frac, pk, sd)
    # the two keys of a pair: both kept with probability pk^2
    both = (keep[..., 0::2] & keep[..., 1::2]).double().mean((-1, -2))
    sd2 = math.sqrt(pk * pk * (1 - pk * pk) / (n // 2))
    assert ((both - pk * pk).abs() <= 4 * sd2).all(), (both, pk * pk, sd2)


def test_port_seeds_are_independent():
    b, h, s, p = 3, 2, 256, 0.5
    a, c = R.keep_mask(b, h, s, p, 1), R.keep_mask(b, h, s, p, 2)
    n = b * h * s * s
    eq = float((a == c).double().mean())
    assert abs(eq - 0.5) <= 4 * math.sqrt(0.25 / n), eq
    # and (b, h) entries of one seed from each other
    eq = float((a[0, 0] == a[1, 1]).double().mean())
    assert abs(eq - 0.5) <= 4 * math.sqrt(0.25 / (s * s)), eq
