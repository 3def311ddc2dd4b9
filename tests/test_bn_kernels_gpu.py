"""The NHWC BatchNorm kernels (csrc/kernels/mv_bn.hip, mv_bn_fin.h) through their bindings in
mivod._mvk against the float64 references and counted bounds of tests/bn_reference.py: every
forward form and backward mode at every launch geometry and block edge, in the near-shift and
the far-shift data regime, the operand variants, the second gradient stream, the exact ReLU
boundary, bn_apply / bn_apply_colsum / bn_stats_strided, and the from-partials entry points
across fin_reduce's loop boundaries.  Every call is made twice and must repeat bit for bit.
The float64 references run on the GPU (plain torch), so the big-row cases stay quick."""
import pytest
import torch

import bn_reference as R
from mivod.ops.bn import batch_norm_act

mvk = pytest.importorskip("mivod._mvk")

pytestmark = pytest.mark.gpu


class Kernels:
    """The bindings behind the call shapes the runners of bn_reference use."""

    @staticmethod
    def fwd(x, gamma, beta, rm, rv, momentum, eps, relu, res, want_mask):
        if want_mask:
            return tuple(mvk.bn_fwd_train_mask(x, gamma, beta, rm, rv, momentum, eps, res))
        y, vec = mvk.bn_fwd_train(x, gamma, beta, rm, rv, momentum, eps, relu, res)
        return y, vec, None

    @staticmethod
    def fwd_stats(x, stats, gamma, beta, rm, rv, momentum, eps, relu, res, want_mask):
        out = mvk.bn_fwd_train_stats(x, stats, gamma, beta, rm, rv, momentum, eps, relu, res,
                                     want_mask)
        return (out[0], out[1], out[2] if want_mask else None)

    stats = staticmethod(lambda *a: mvk.bn_stats(*a))
    bwd = staticmethod(lambda *a: tuple(mvk.bn_bwd(*a)))
    apply = staticmethod(lambda *a: mvk.bn_apply(*a))
    apply_colsum = staticmethod(lambda *a: tuple(mvk.bn_apply_colsum(*a)))
    stats_strided = staticmethod(lambda *a: mvk.bn_stats_strided(*a))
    finalize = staticmethod(lambda *a: mvk.bn_finalize(*a))
    bwd_coeffs = staticmethod(lambda *a: mvk.bn_bwd_coeffs(*a))
    bwd_from_partials = staticmethod(lambda *a: tuple(mvk.bn_bwd_from_partials(*a)))


K = Kernels()


def _cus(dev) -> int:
    return torch.cuda.get_device_properties(dev).multi_processor_count


EDGES = [(C, M) for C in R.CHANNELS for M in R.edge_rows(C)]


@pytest.mark.parametrize("C,M", EDGES)
def test_edge_rows(cuda, C, M):
    """M = 1 (the variance guard), M < RPI, RPI +- 1, short last blocks, one to many blocks."""
    cus = _cus(cuda)
    print("\n".join(R.run_geometry_case(K, M, C, cus, cuda)))
    print(f"C={C} M={M} " + R.counts(M, C, cus))


@pytest.mark.parametrize("regime", R.REGIMES)
def test_gy8_multi_iteration_unroll(cuda, regime):
    cus, M, C = _cus(cuda), 20011, 2048
    for g in R.geos(M, C, cus):
        assert g.gy == 8 and g.n >= 2 * R.U_APPLY and R.loops(g, R.U_STATS)[0]
    print("\n".join(R.run_geometry_case(K, M, C, cus, cuda, regimes=(regime,))))
    print(f"C={C} M={M} " + R.counts(M, C, cus))


def _big(cuda, M, C, regime, reach):
    cus = _cus(cuda)
    for cap in (None, R.APPLY_CAP):
        for g in R.geos(M, C, cus, cap):
            assert reach(g, cus), f"{g} does not reach what the case names"
    print("\n".join(R.run_geometry_case(K, M, C, cus, cuda, regimes=(regime,), lite=True)))
    print(f"C={C} M={M} " + R.counts(M, C, cus))


@pytest.mark.parametrize("regime", R.REGIMES)
def test_resident_branch(cuda, regime):
    """More 64-row blocks than resident workgroups: bx = resident / gy in round_geo."""
    M = 64 * 8 * _cus(cuda) + 77
    _big(cuda, M, 64, regime, lambda g, cus: R._cdiv(M, 64) > 8 * cus and R.loops(g, R.U_BWD)[0])


@pytest.mark.parametrize("regime", R.REGIMES)
def test_every_unrolled_loop_rpi32(cuda, regime):
    M = 256 * 8 * _cus(cuda) + 77
    _big(cuda, M, 64, regime,
         lambda g, cus: all(R.loops(g, u)[0] for u in (R.U_STATS, R.U_APPLY, R.U_BWD)))


@pytest.mark.parametrize("regime", R.REGIMES)
def test_every_unrolled_loop_tpr1(cuda, regime):
    """C = 8 (one lane per row, RPI = 256): the smallest M whose blocks reach 8 RPI rows with
    as many row blocks as eight workgroups per CU."""
    cus = _cus(cuda)
    M = (8 * 256 - 256) * min(R.P_CAP, 8 * cus) + 1
    _big(cuda, M, 8, regime,
         lambda g, cus: g.TPR == 1 and all(R.loops(g, u)[0] for u in (R.U_STATS, R.U_APPLY, R.U_BWD)))


@pytest.mark.parametrize("M,C", R.VARIANT_SHAPES)
def test_operand_variants(cuda, M, C):
    print("\n".join(R.run_variants(K, M, C, _cus(cuda), cuda)))


@pytest.mark.parametrize("nhw", R.DY2_SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_second_gradient_stream(cuda, nhw, stride):
    for C in (64, 320):
        print("\n".join(R.run_dy2(K, nhw, C, stride, _cus(cuda), cuda)))


def test_exact_relu_boundary(cuda):
    R.run_boundary(K, _cus(cuda), cuda)


@pytest.mark.parametrize("C", R.CHANNELS)
def test_apply_and_colsum(cuda, C):
    cus = _cus(cuda)
    for M in R.edge_rows(C) + [20011]:
        print("\n".join(R.run_apply(K, M, C, cuda)))
        print(R.run_colsum(K, M, C, cus, cuda))


@pytest.mark.parametrize("relu,use_res", R.FWD_COMBOS)
def test_eval_form(cuda, relu, use_res):
    """batch_norm_act(training=False): scale = rsqrt(var + eps) * weight and shift = bias -
    mean * scale are fp32 torch ops in front of bn_apply.  Counts: eps r, +, rsqrt 2 (torch's
    is not correctly rounded), * -> 5 for scale (positive terms: mag = the value); mean *
    scale 6, - -> 7 for shift against |bias| + |mean scale|."""
    n, C, h, w = 3, 96, 5, 7
    t = R._dev(R.make_case(n * h * w, C, "near", 8, shape=(n, C, h, w)), cuda)
    eps = 1e-3
    with torch.no_grad():
        y = batch_norm_act(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], False, 0.1, eps, relu,
                           t["res"] if use_res else None)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    g, b, rm, rv = (R.f64(t[k]) for k in ("gamma", "beta", "rm", "rv"))
    sc = g / (rv + eps).sqrt()
    ref = R.apply_ref(R.rows(t["x"]), R.Out(sc, sc.abs(), 5),
                      R.Out(b - rm * sc, b.abs() + (rm * sc).abs(), 7),
                      R.rows(t["res"]) if use_res else None, relu)
    print(f"eval relu={relu} res={use_res}: y {R.check_bf16('eval y_eval', y, ref):.2f}")


@pytest.mark.parametrize("nhw", R.STRIDED_SHAPES)
@pytest.mark.parametrize("stride", [2, 3])
def test_stats_strided(cuda, nhw, stride):
    for C in (8, 64, 320):
        print(R.run_stats_strided(K, nhw, C, stride, _cus(cuda), cuda))


@pytest.mark.parametrize("C", R.PARTIAL_CHANNELS)
@pytest.mark.parametrize("P", R.PARTIAL_COUNTS)
def test_from_partials(cuda, P, C):
    for M in R.PARTIAL_ROWS:
        for regime in ("near", "far"):
            print("\n".join(R.run_from_partials(K, P, C, M, _cus(cuda), cuda, regime)))


def test_sensitivity_guards_fire(cuda):
    """The kernels pass the case and each changed reference lands outside a bound: one dropped
    row (also at [20011, 2048], the largest case a counted bound can resolve a row in: see
    test_bn_reference_cpu.py::test_drop_row_needs_m_times_depth_below_2_24), M - 1 for M,
    the biased for the unbiased variance, the shift ignored, the cb x term dropped."""
    cus = _cus(cuda)
    res = R.run_guards(K, cus, cuda)
    res["ignore_shift"] = R.run_shift_guard(cus)
    res["drop_row_20011x2048"] = R.run_guards(K, cus, cuda, 20011, 2048, True)["drop_row"]
    print(R.fmt(res))
    for k, v in res.items():
        assert v > 1.0, f"the bound cannot see {k}: the changed reference is {v:.3g} bounds away"


def test_zz_report_worst_ratios(mivod_report):
    """Not a check: the worst err / bound per output over this module's run, for the table in
    bn_reference's docstring."""
    if R.WORST:
        mivod_report("bn kernels, worst err / bound: " + R.fmt(dict(sorted(R.WORST.items()))))
