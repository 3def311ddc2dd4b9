"""The PyTorch fallbacks of the flat-bucket kernels (mivod/ops/kernels.py) against the float64
references and the counted bounds of tests/flat_reference.py, at the sizes and flag sets
tests/test_flat_kernels_gpu.py uses for the HIP kernels.

The fallbacks are plain fp32 PyTorch: that they pass shows that the references and the
counted bounds hold for an honest fp32 implementation, and it is the fallbacks' own test.
Each test prints its worst err / (2^-24 * mag) next to the counted c.
"""
import pytest
import torch

import flat_reference as R
from mivod.ops import kernels as K

CPU = torch.device("cpu")
KINDS = ["sgd", "adam", "adadelta", "lars"]
C_OF = {"sgd": dict(w=R.C_SGD_W, mom=R.C_SGD_MOM),
        "adam": dict(w=R.C_ADAM_W, m=R.C_ADAM_M, v=R.C_ADAM_V),
        "adadelta": dict(w=R.C_ADADELTA_W, sq=R.C_ADADELTA_SQ, acc=R.C_ADADELTA_ACC),
        "lars": dict(w=R.C_LARS_W, mom=R.C_LARS_MOM)}


_lars_args = R.lars_case


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
def test_step_dtype_grid(kind, gdt, mdt):
    n, lars = (R.N_GRID, None) if kind != "lars" else _lars_args()
    worst, _, _ = R.run_step(kind, n, gdt, mdt, CPU, lars=lars)
    print(f"{kind} fallback {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {C_OF[kind]}")


@pytest.mark.parametrize("kind,gdt", [("sgd", torch.float16), ("sgd", torch.bfloat16),
                                      ("lars", torch.float16), ("lars", torch.bfloat16),
                                      ("adam", torch.float16), ("adamw", torch.float16)])
def test_step_sizes(kind, gdt):
    hp, k = None, kind
    if kind == "adam":
        hp = dict(R.HP["adam"], adamw=False)
    elif kind == "adamw":
        k = "adam"
    tot = {}
    for n in R.SIZES:
        nn, lars = (n, None) if k != "lars" else _lars_args(n)
        worst, _, _ = R.run_step(k, nn, gdt, torch.bfloat16, CPU, hp=hp, seed=n, lars=lars)
        tot = {o: max(tot.get(o, 0.0), v) for o, v in worst.items()}
    print(f"{kind} fallback sizes {gdt}/bf16: worst err/(U*mag) {R.fmt(tot)}; c {C_OF[k]}")


@pytest.mark.parametrize("case", sorted(R.SGD_FLAG_CASES))
def test_sgd_flags(case):
    worst, sens = R.run_sgd_flag(case, CPU)
    print(f"sgd fallback {case}: worst {R.fmt(worst)}; the flag moves w by {sens:.3g} bounds")


@pytest.mark.parametrize("adamw", [False, True])
@pytest.mark.parametrize("keras_eps", [False, True])
@pytest.mark.parametrize("step", [1, 7])
def test_adam_flags(adamw, keras_eps, step):
    worst, sens = R.run_adam_flag(adamw, keras_eps, step, CPU)
    print(f"adam fallback adamw={adamw} keras_eps={keras_eps} step={step}: worst {R.fmt(worst)}; "
          f"flags move w by {sens} bounds")


@pytest.mark.parametrize("case", ["first", "flags", "zero_grad", "zero_len", "eps"])
def test_lars_flags(case):
    worst, sens = R.run_lars_flag(case, CPU)
    print(f"lars fallback {case}: worst {R.fmt(worst)}; the flag moves w by {sens} bounds")


@pytest.mark.parametrize("kind", KINDS)
def test_skip_leaves_everything_untouched(kind):
    R.run_skip(kind, CPU)


@pytest.mark.parametrize("kind,gdt", [("sgd", torch.bfloat16), ("adam", torch.float16),
                                      ("lars", torch.float16)])
def test_five_step_trajectory(kind, gdt):
    worst = R.run_trajectory(kind, CPU, gdt, torch.bfloat16)
    print(f"{kind} fallback trajectory: worst err/(step*U*mag) {R.fmt(worst)}; c {C_OF[kind]}")


@pytest.mark.parametrize("wire", R.DTYPES)
@pytest.mark.parametrize("swap", [False, True])
def test_adasum_fcombine(wire, swap):
    worst, f, (f0, r, dots, table) = R.run_fcombine(CPU, wire, swap)
    print(f"adasum_fcombine fallback {wire} swap={swap}: worst err/(U*mag) {worst:.2f}; "
          f"c {R.C_ADASUM}")
    # the same merge through adasum_merge with one Gram row, in place, no emit
    f2 = f0.clone()
    K.adasum_merge(f2, f2, r, table, dots.reshape(-1), 1, swap)
    assert torch.equal(f2, f)


@pytest.mark.parametrize("sd", R.DTYPES)
@pytest.mark.parametrize("dd", R.DTYPES)
@pytest.mark.parametrize("aligned", [False, True])
def test_flat_cast_and_pack_exact(sd, dd, aligned):
    R.run_cast_exact(CPU, sd, dd, aligned)


@pytest.mark.parametrize("dt", R.DTYPES)
def test_nonfinite_detection(dt):
    R.run_nonfinite(CPU, dt)
    R.run_nonfinite(CPU, dt, base_off=1)


@pytest.mark.parametrize("ddt,val", [(torch.float16, 7e4),
                                     (torch.bfloat16, torch.finfo(torch.float32).max)])
def test_cast_overflow_sets_the_flag(ddt, val):
    R.run_cast_overflow(CPU, ddt, val)
