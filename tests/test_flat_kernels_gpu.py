"""The flat-bucket HIP kernels (csrc/kernels/mv_kernels.hip: pack / cast, the non-finite scan,
the fused SGD / Adam / Adadelta / LARS steps, the Adasum merges) against float64, on every
template instantiation and code path: the 3 gradient dtypes x 4 model-copy choices, the
16-byte vector body and the scalar tail, the skip flag, the dyn block, the guarded unaligned
paths.  References, counted bounds (c) and the shared cases are in tests/flat_reference.py;
tests/test_flat_reference_cpu.py runs the PyTorch fallbacks through the same cases.

Each test prints its worst err / (2^-24 * mag) next to the counted c.

Every step kernel guards its vector body: SGD, Adam and Adadelta run on the streaming
skeleton of csrc/kernels/mv_flat_step.h (as does Adagrad, tests/test_adaptive_gpu.py), which
sends every element of an unaligned operand through its one-by-one loads and stores; LARS
guards its own.  The bindings of sgd_step / adam_step / adadelta_step reject an unaligned
operand all the same (tests/test_bindings_validation.py), so the unaligned branch of the
skeleton cannot be reached from Python through these three: the same template code is
exercised unaligned through Adagrad (test_adaptive_gpu.py::test_unaligned), and the guarded
kernels with bodies of their own through test_unaligned_lars and test_unaligned[rmsprop].
"""
import pytest
import torch

import flat_reference as R
from mivod.ops import kernels as K

pytestmark = pytest.mark.gpu

KINDS = ["sgd", "adam", "adadelta", "lars"]
C_OF = {"sgd": dict(w=R.C_SGD_W, mom=R.C_SGD_MOM),
        "adam": dict(w=R.C_ADAM_W, m=R.C_ADAM_M, v=R.C_ADAM_V),
        "adadelta": dict(w=R.C_ADADELTA_W, sq=R.C_ADADELTA_SQ, acc=R.C_ADADELTA_ACC),
        "lars": dict(w=R.C_LARS_W, mom=R.C_LARS_MOM)}
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


# ---- A. fused steps against fp64 ----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
def test_step_dtype_grid(cuda, kind, gdt, mdt):
    """every (TG, TP) instantiation of the four step kernels (model None runs TP = float)"""
    n, lars = (R.N_GRID, None) if kind != "lars" else R.lars_case()
    worst, _, _ = R.run_step(kind, n, gdt, mdt, cuda, lars=lars)
    print(f"{kind} {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {C_OF[kind]}")


@pytest.mark.parametrize("kind,gdt", [("sgd", f16), ("sgd", bf16), ("lars", f16), ("lars", bf16),
                                      ("adam", f16), ("adamw", f16), ("adadelta", f16)])
def test_step_sizes(cuda, kind, gdt):
    """the production pairs at every size around a lane (8), a step (2048) and a chunk (4096)"""
    hp, k = None, kind
    if kind == "adam":
        hp = dict(R.HP["adam"], adamw=False)
    elif kind == "adamw":
        k = "adam"
    tot = {}
    for n in R.SIZES:
        nn, lars = (n, None) if k != "lars" else R.lars_case(n)
        worst, _, _ = R.run_step(k, nn, gdt, bf16, cuda, hp=hp, seed=n, lars=lars)
        tot = {o: max(tot.get(o, 0.0), v) for o, v in worst.items()}
    print(f"{kind} sizes {gdt}/bf16: worst err/(U*mag) {R.fmt(tot)}; c {C_OF[k]}")


@pytest.mark.parametrize("gdt", R.DTYPES)
def test_lars_norms(cuda, gdt):
    """the squared norms seg_partial_kernel -> seg_reduce_kernel leave in the workspace"""
    total, lars = R.lars_case()
    sizes, offs, flags, zero = lars
    t = R.make_inputs("lars", total, gdt, None, cuda, seed=2)
    ref = R.ref_step("lars", t, R.HP["lars"], lars=(sizes, offs, flags))
    ws = {}
    R.call_step("lars", t, R.HP["lars"], workspace=ws, **R.lars_extra(lars, cuda))
    got = ws["norms"][:2 * len(sizes)].view(-1, 2)
    worst = R.check("lars norms", got, ref["norms"])
    print(f"lars norms {gdt}: worst err/(U*mag) {worst:.2f}; c ({R.C_LARS_WN2}, {R.C_LARS_GN2})")


# ---- B. flags -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.SGD_FLAG_CASES))
def test_sgd_flags(cuda, case):
    worst, sens = R.run_sgd_flag(case, cuda)
    print(f"sgd {case}: worst {R.fmt(worst)}; the flag moves w by {sens:.3g} bounds")


@pytest.mark.parametrize("adamw", [False, True])
@pytest.mark.parametrize("keras_eps", [False, True])
@pytest.mark.parametrize("step", [1, 7])
def test_adam_flags(cuda, adamw, keras_eps, step):
    worst, sens = R.run_adam_flag(adamw, keras_eps, step, cuda)
    print(f"adam adamw={adamw} keras_eps={keras_eps} step={step}: worst {R.fmt(worst)}; "
          f"flags move w by {sens} bounds")


@pytest.mark.parametrize("case", ["first", "flags", "zero_grad", "zero_len", "eps"])
def test_lars_flags(cuda, case):
    worst, sens = R.run_lars_flag(case, cuda)
    print(f"lars {case}: worst {R.fmt(worst)}; the flag moves w by {sens} bounds")


# ---- C. skip ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_skip_leaves_everything_untouched(cuda, kind):
    R.run_skip(kind, cuda)


# ---- D. dyn -------------------------------------------------------------------------------
def _dyn_run(kind, cuda, hp, dyn=None):
    n, lars = (4097, None) if kind != "lars" else R.lars_case()
    t = R.make_inputs(kind, n, f16, bf16, cuda, seed=12)
    extra = R.lars_extra(lars, cuda) if lars else {}
    if dyn is not None:
        extra["dyn"] = torch.tensor(dyn, dtype=f32, device=cuda)
    R.call_step(kind, t, hp, **extra)
    return t


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("first", [False, True])
def test_dyn_block_overrides_scalars(cuda, kind, first):
    """dyn = [lr, first, bc1, bc2] wins over bogus scalar lr / first / step, in both
    directions of ``first``, and gives the bits of the scalar call with the same values (a
    size with a tail, a model copy)."""
    hp = dict(R.HP[kind], lr=0.07)
    bogus = dict(hp, lr=99.0)
    dyn = [0.07, float(first), 0.0, 0.0]
    if kind in ("sgd", "lars"):
        hp["first"], bogus["first"] = first, not first
    if kind == "adam":
        step = 1 if first else 5
        hp["step"], bogus["step"] = step, 6 - step
        dyn[2:] = [1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step]
    want = _dyn_run(kind, cuda, hp)
    got = _dyn_run(kind, cuda, bogus, dyn)
    assert _same(got, want), f"{kind}: the dyn block does not reproduce the scalar call"
    assert not _same(_dyn_run(kind, cuda, bogus), want), "the bogus scalars change nothing"


# ---- E. unaligned paths (only kernels that guard their vector body) --------------------------
@pytest.mark.parametrize("sd", R.DTYPES)
@pytest.mark.parametrize("dd", R.DTYPES)
@pytest.mark.parametrize("aligned", [False, True])
def test_pack_unpack_cast_exact(cuda, sd, dd, aligned):
    R.run_cast_exact(cuda, sd, dd, aligned)


@pytest.mark.parametrize("gdt,mdt", [(f16, bf16), (bf16, f32), (f32, None), (f32, f16)])
def test_unaligned_lars(cuda, gdt, mdt):
    lars = (R.UNAL_SIZES, R.UNAL_OFFS, [0, 0, 0, 1], [])
    worst, _, _ = R.run_step("lars", R.UNAL_TOTAL, gdt, mdt, cuda, lars=lars, seed=13)
    print(f"lars unaligned {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {C_OF['lars']}")


@pytest.mark.parametrize("adt,bdt", [(f32, f32), (bf16, bf16), (f16, f16), (f32, bf16), (f32, f16)])
def test_unaligned_seg_dot3(cuda, adt, bdt):
    a, b, _, offs, table = R.ada_inputs(bdt, cuda, R.UNAL_SIZES, R.UNAL_OFFS, fdt=adt)
    got = K.seg_dot3(a, b, table)
    worst = R.check("seg_dot3", got, R.dot3_ref(a, b, R.UNAL_SIZES, offs))
    print(f"seg_dot3 unaligned {adt}x{bdt}: worst err/(U*mag) {worst:.2f}; c {R.C_DOT3}")


@pytest.mark.parametrize("wire", R.DTYPES)
@pytest.mark.parametrize("swap", [False, True])
def test_unaligned_adasum_fcombine(cuda, wire, swap):
    worst, _, _ = R.run_fcombine(cuda, wire, swap, R.UNAL_SIZES, R.UNAL_OFFS)
    print(f"adasum_fcombine unaligned {wire} swap={swap}: worst err/(U*mag) {worst:.2f}; "
          f"c {R.C_ADASUM}")


@pytest.mark.parametrize("dt", R.DTYPES)
def test_unaligned_adasum_combine(cuda, dt):
    a, b, dots, offs, table = R.ada_inputs(dt, cuda, R.UNAL_SIZES, R.UNAL_OFFS, fdt=dt)
    ref = R.adasum_ref(a, b, R.UNAL_SIZES, offs, dots, False)
    K.adasum_combine(a, b, table, dots)
    worst = R.check_stored("adasum_combine", a, ref, dt)
    print(f"adasum_combine unaligned {dt}: worst err/tolerance {worst:.2f}")


# ---- F. non-finite detection ----------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("base_off", [0, 1])
def test_nonfinite_detection(cuda, dt, base_off):
    R.run_nonfinite(cuda, dt, base_off)


@pytest.mark.parametrize("ddt,val", [(f16, 7e4), (bf16, torch.finfo(f32).max)])
@pytest.mark.parametrize("pos", [0, R.N_GRID - 1])
def test_cast_overflow_sets_the_flag(cuda, ddt, val, pos):
    R.run_cast_overflow(cuda, ddt, val, pos)


# ---- G. tensor tables -------------------------------------------------------------------------
def test_pack_130_tensors_two_launches(cuda):
    """130 fp32 tensors -> fp16 (two launches of at most 64 non-empty tensors), zero-element
    tensors between others, a scale, the flag raised by a tensor of the second launch"""
    assert K.native().MAX_TENSORS_PER_LAUNCH == 64
    gen = torch.Generator().manual_seed(14)
    sizes = [int(x) for x in torch.randint(1, 300, (130,), generator=gen)]
    for i, n in {0: 0, 3: 1, 63: 4095, 64: 4096, 65: 4097, 70: 0, 99: 0, 129: 0}.items():
        sizes[i] = n
    ts = [torch.randn(n, generator=gen).to(cuda) for n in sizes]
    offs, total = R.layout(sizes)
    flat = torch.full((total,), 9.0, dtype=f16, device=cuda)
    nf = R.flag_of(cuda)
    K.pack(ts, flat, offs, scale=R.SCALE, nonfinite=nf)
    assert nf.item() == 0
    touched = torch.zeros(total, dtype=torch.bool)
    for t, off in zip(ts, offs):
        assert torch.equal(flat[off:off + t.numel()], R.cast_ref(t, R.SCALE, f16))
        touched[off:off + t.numel()] = True
    assert (flat.cpu()[~touched] == 9.0).all(), "pack wrote outside its slices"
    outs = [torch.empty_like(t) for t in ts]
    K.unpack(outs, flat, offs, scale=2.0)
    for out, off in zip(outs, offs):
        assert torch.equal(out, R.cast_ref(flat[off:off + out.numel()], 2.0, f32))
    assert sizes[100] > 0
    ts[100][sizes[100] - 1] = float("inf")
    K.pack(ts, flat, offs, scale=R.SCALE, nonfinite=nf)
    assert nf.item() == 1, "an inf in tensor 100 (second launch) did not set the flag"


# ---- H. adasum_fcombine against fp64 ------------------------------------------------------------
@pytest.mark.parametrize("wire", R.DTYPES)
@pytest.mark.parametrize("swap", [False, True])
def test_adasum_fcombine_vs_fp64(cuda, wire, swap):
    worst, f, (f0, r, dots, table) = R.run_fcombine(cuda, wire, swap)
    print(f"adasum_fcombine {wire} swap={swap}: worst err/(U*mag) {worst:.2f}; c {R.C_ADASUM}")
    # the same kernel through adasum_merge: one Gram row, fin is f, no emit
    f2 = f0.clone()
    K.adasum_merge(f2, f2, r, table, dots.reshape(-1).contiguous(), 1, swap)
    assert torch.equal(f2, f), "adasum_fcombine differs from adasum_merge(nrows=1)"


# ---- I. five-step trajectories --------------------------------------------------------------------
@pytest.mark.parametrize("kind,gdt", [("sgd", bf16), ("adam", f16), ("lars", f16)])
def test_five_step_trajectory(cuda, kind, gdt):
    worst = R.run_trajectory(kind, cuda, gdt, bf16)
    print(f"{kind} trajectory: worst err/(step*U*mag) {R.fmt(worst)}; c {C_OF[kind]}")
