"""tests/bn_reference.py without a GPU: its float64 references equal double autograd, an
honest fp32 implementation (the emulation, in the kernels' order of stages) stays inside every
counted bound on the GPU tier's case grid with an assumed 256 CUs, the Python launch-geometry
helper matches hand-worked values, and every sensitivity guard fires.  Each test prints its
worst err / (2^-24 mag) next to the counts c (pytest -s shows them)."""
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

CUS = R.ASSUMED_CUS
# one and eight workgroups per CU: the two ends of the geometries the bounds cover
EMUS = {1: R.Emu(CUS), 8: R.Emu(8 * CUS)}


def _close(name, got, want, tol=1e-12, mag=None):
    """1e-12 relative to the result, or to the magnitude ``mag`` of the terms it is the sum
    of (where they cancel, double's own roundings act on the terms)."""
    err = float((got - want).abs().max())
    scale = float((want.abs() if mag is None else mag).max()) or 1.0
    assert err <= tol * scale, f"{name}: {err:.3g} vs magnitude {scale:.3g}"


@pytest.mark.parametrize("M,C", [(2, 8), (33, 64), (197, 96), (65, 320)])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("regime", ["near", "far_norun"])
def test_reference_equals_double_autograd(M, C, mode, regime):
    t = R.make_case(M, C, regime, 0)
    relu, use_res = mode >= 1, mode == 2
    ref = R.fwd_ref(t["x"], t["rm"], t["rv"], t["gamma"], t["beta"], 0.1, 1e-5, relu,
                    t["res"] if use_res else None, CUS)
    x = R.rows(t["x"]).requires_grad_()
    w, b = t["gamma"].double().requires_grad_(), t["beta"].double().requires_grad_()
    res = R.rows(t["res"]).requires_grad_() if use_res else None
    rm = None if t["rm"] is None else t["rm"].double()
    rv = None if t["rv"] is None else t["rv"].double()
    y = F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
    if use_res:
        y = y + res
    if relu:
        y = F.relu(y)
    _close("y", ref["y"].ref, y.detach())
    if rm is not None:
        _close("running_mean", ref["running_mean"].ref, rm)
        _close("running_var", ref["running_var"].ref, rv)
    dy = R.rows(t["dy"])
    y.backward(dy)
    vec = torch.stack([ref[k].ref for k in R.VEC_NAMES])
    bref = R.bwd_ref(t["dy"], None, t["x"], (y.detach() > 0) if relu else None, vec, t["gamma"], CUS)
    _close("dx", bref["dx"].ref, x.grad, mag=bref["dx"].delta / (R.U * (bref["cc"].c + 2)))
    _close("dgamma", bref["dgamma"].ref, w.grad, mag=bref["dgamma"].mag)
    _close("dbeta", bref["dbeta"].ref, b.grad, mag=bref["dbeta"].mag)
    if use_res:
        _close("dz", bref["dz"].ref, res.grad)


def test_reference_single_row_by_hand():
    """M = 1 (torch refuses one value per channel): mean = x, var = 0, invstd = eps^-1/2, the
    running variance decays towards the biased value 0, dx = 0."""
    t = R.make_case(1, 8, "near", 0)
    ref = R.fwd_ref(t["x"], t["rm"], t["rv"], t["gamma"], t["beta"], 0.1, 1e-3, False, None, CUS)
    x = R.rows(t["x"])[0]
    _close("mean", ref["mean"].ref, x)
    assert torch.equal(ref["var"].ref, torch.zeros(8, dtype=torch.float64))
    _close("invstd", ref["invstd"].ref, torch.full((8,), 1e-3 ** -0.5, dtype=torch.float64))
    _close("running_var", ref["running_var"].ref, 0.9 * t["rv"].double())
    _close("running_mean", ref["running_mean"].ref, 0.9 * t["rm"].double() + 0.1 * x)
    _close("y", ref["y"].ref[0], t["beta"].double(), 1e-9)
    vec = torch.stack([ref[k].ref for k in R.VEC_NAMES])
    bref = R.bwd_ref(t["dy"], None, t["x"], None, vec, t["gamma"], CUS)
    assert float(bref["dx"].ref.abs().max()) < 1e-9


@pytest.mark.parametrize("C", R.CHANNELS)
def test_emulation_inside_bounds_on_the_edge_rows(C):
    for M in R.edge_rows(C):
        for occ, emu in EMUS.items():
            lines = R.run_geometry_case(emu, M, C, CUS, "cpu")
        print("\n".join(lines[-3:]))
        print(f"C={C} M={M} " + R.counts(M, C, CUS))


@pytest.mark.parametrize("C,M,occ", [(64, 64 * 8 * CUS + 77, 8), (64, 64 * 8 * CUS + 77, 1),
                                     (2048, 20011, 1)])
def test_emulation_inside_bounds_on_big_rows(C, M, occ):
    """The big-row cases an fp32 CPU pass finishes in seconds: the resident / gy branch and
    gy = 8 with 79 rows per lane.  (The 524k-row and the TPR = 1 cases of the GPU tier take
    the same code with deeper sums; they are left to the GPU.)"""
    lines = R.run_geometry_case(EMUS[occ], M, C, CUS, "cpu", regimes=("far",), lite=[(True, 3)])
    print("\n".join(lines))
    print(f"C={C} M={M} " + R.counts(M, C, CUS))


@pytest.mark.parametrize("M,C", R.VARIANT_SHAPES)
def test_emulation_operand_variants(M, C):
    print("\n".join(R.run_variants(EMUS[8], M, C, CUS, "cpu")))


@pytest.mark.parametrize("nhw", R.DY2_SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_emulation_second_gradient_stream(nhw, stride):
    for C in (64, 320):
        print("\n".join(R.run_dy2(EMUS[8], nhw, C, stride, CUS, "cpu")))


def test_emulation_exact_relu_boundary():
    R.run_boundary(EMUS[8], CUS, "cpu")


@pytest.mark.parametrize("C", R.CHANNELS)
def test_emulation_apply_colsum_strided(C):
    for M in R.edge_rows(C):
        lines = R.run_apply(EMUS[8], M, C, "cpu")
        lines.append(R.run_colsum(EMUS[1], M, C, CUS, "cpu"))
    print("\n".join(lines))
    for nhw in R.STRIDED_SHAPES:
        for s in (2, 3):
            print(R.run_stats_strided(EMUS[8], nhw, C, s, CUS, "cpu"))


@pytest.mark.parametrize("C", R.PARTIAL_CHANNELS)
@pytest.mark.parametrize("P", R.PARTIAL_COUNTS)
def test_emulation_from_partials(P, C):
    for M in R.PARTIAL_ROWS:
        for regime in ("near", "far"):
            lines = R.run_from_partials(EMUS[8], P, C, M, CUS, "cpu", regime)
    print("\n".join(lines))


def test_sensitivity_guards_fire():
    res = R.run_guards(EMUS[8], CUS, "cpu")
    res["ignore_shift"] = R.run_shift_guard(CUS)
    res["drop_row_20011x2048"] = R.run_guards(EMUS[8], CUS, "cpu", 20011, 2048, True)["drop_row"]
    print(R.fmt(res))
    for k, v in res.items():
        assert v > 1.0, f"the bound cannot see {k}: the changed reference is {v:.3g} bounds away"


def test_drop_row_needs_m_times_depth_below_2_24():
    """A dropped row moves a sum by 1 / M of its magnitude and a worst-case bound is
    depth * 2^-24 of it, so no counted bound resolves one row once M * depth > 2^24: the
    guard runs at [20011, 2048] (M * depth ~ 2^20) and not at the 524k-row case."""
    M = 256 * 8 * CUS + 77
    assert M * R.reduce_depth(M, 64, CUS, R.U_STATS) > 2 ** 24
    assert 20011 * R.reduce_depth(20011, 2048, CUS, R.U_STATS) < 2 ** 21


# --------------------------------------------------------------------------- geometry
def _geo(M, C, resident, cap=None):
    return R.round_geo(M, C, resident, R.partials(M, C) if cap is None else cap)


def test_geometry_helper_matches_hand_worked_values():
    full = 8 * CUS                                    # 2048 resident workgroups
    # C = 8: one lane per row, 256 rows per iteration; M < RPI is one short block
    g = _geo(63, 8, full)
    assert (g.TPR, g.RPI, g.RB, g.gx, g.gy) == (1, 256, 256, 1, 1)
    assert R.loops(g, R.U_STATS) == (False, True) and R.loops(g, R.U_BWD) == (False, True)
    # C = 96: 12 lanes per row, 21 rows per iteration (4 idle lanes)
    g = _geo(197, 96, full)
    assert (g.TPR, g.RPI, g.RB, g.gx) == (12, 21, 63, 4)          # ceil(197 / 4) = 50 -> 63
    # C = 320: two slabs (256 + 64 channels), partial cap 2048 / 2
    assert R.partials(10 ** 6, 320) == 1024
    g = _geo(1568, 320, full)
    assert (g.CB, g.RPI, g.RB, g.gx, g.gy) == (256, 8, 64, 25, 2)  # 25 blocks of 64, last 32 rows
    assert R.loops(g, R.U_STATS) == (True, True)     # 8 rows per lane, 4 in the last block
    # a last block shorter than RPI: 65 rows at RPI = 32 -> blocks of 64 and 1
    g = _geo(65, 64, full)
    assert (g.RPI, g.RB, g.gx) == (32, 64, 2)
    # the resident / gy branch: more 64-row blocks than resident workgroups
    M = 64 * 8 * CUS + 77
    g = _geo(M, 64, full, R.APPLY_CAP)
    assert (g.RB, g.gx, g.n) == (96, 1367, 3)        # ceil(131149 / 2048) = 65 -> 96
    assert R.loops(g, R.U_BWD) == (True, True) and R.loops(g, R.U_APPLY) == (False, True)
    # every unrolled loop at RPI = 32
    M = 256 * 8 * CUS + 77
    g = _geo(M, 64, full)
    assert (g.RB, g.gx, g.n) == (288, 1821, 9)       # ceil(524365 / 2048) = 257 -> 288
    assert all(R.loops(g, u)[0] for u in (R.U_STATS, R.U_APPLY, R.U_BWD))
    assert all(R.loops(h, R.U_STATS)[0] for h in R.geos(M, 64, CUS))
    # the same at TPR = 1: the smallest M whose blocks reach 8 * RPI = 2048 rows
    M = 1792 * full + 1
    g = _geo(M, 8, full)
    assert (g.RB, g.gx, g.n) == (2048, 1793, 8) and R.loops(g, R.U_STATS)[0]
    assert not R.loops(_geo(M - 1, 8, full), R.U_STATS)[0]
    # gy = 8: 2048 / 8 partials, a multi-iteration unrolled loop
    g = _geo(20011, 2048, full)
    assert (g.gy, g.RB, g.gx, g.n) == (8, 80, 251, 10) and R.partials(20011, 2048) == 256
    g1 = _geo(20011, 2048, CUS)                      # one workgroup per CU: 32 row blocks
    assert (g1.RB, g1.n) == (632, 79)
    # depths: A + B + C
    assert R.lane_depth(7, 8) == 7 and R.lane_depth(8, 8) == 8 and R.lane_depth(19, 8) == 12
    assert R.fin_depth(1) == 12 and R.fin_depth(128) == 12 and R.fin_depth(129) == 13
    assert R.fin_depth(2048) == 27
    assert R.reduce_depth(20011, 2048, CUS, R.U_STATS) == R.lane_depth(79, 8) + 8 + R.fin_depth(32)
    assert R.reduce_depth(1, 8, CUS, R.U_STATS) == 1 + 1 + R.fin_depth(1)      # M < RPI: stage B = M
