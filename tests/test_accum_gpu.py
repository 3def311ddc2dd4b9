"""Local gradient accumulation in an fp32 arena on the GPU: accum_kernel's three modes
(csrc/kernels/mv_accum.hip) against float64 and DistributedOptimizer(backward_passes_per_step=k,
accumulation_dtype=torch.float32) on the GPU hook path and on 2 ranks sharing one GPU.  The
references, the counted bounds and the shared cases are in tests/accum_reference.py;
tests/test_accum_cpu.py runs the PyTorch fallbacks through the same cases.

Each test prints its worst err / (2^-24 * mag) next to the counted c, or its worst
err / bound."""
import pytest
import torch

import accum_reference as R
from mivod.ops import kernels as K
from test_accum_cpu import run_accum_ranks
from test_multirank_gpu import _TMO, _one_gpu

pytestmark = pytest.mark.gpu

f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


# ---- A. the three modes -----------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("wdt", R.DTYPES)
def test_accumulate_and_pack_sizes(cuda, gdt, wdt):
    """every size around a lane (8), a step (2048) and a chunk (4096), two tensors per launch
    at 64-element-aligned offsets, from an aligned base (load8 / store8) and from base[1:]
    (one by one): the same bits either way, nothing written outside the segments"""
    wa, ww = R.run_sizes(cuda, gdt, wdt)
    print(f"{gdt} -> {wdt}, k 4: acc worst err/(U*mag) per addition {wa:.2f} (c = j-1 after j "
          f"passes); wire worst err/bound {ww:.2f} (c 5)")


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("scale", R.SCALES)
def test_accumulate_and_pack_passes_and_scales(cuda, k, scale):
    worst = [R.run_window(cuda, [R.N_GRID, R.TAIL], gdt, wdt, k, scale, seed=k)[:2]
             for gdt, wdt in ((bf16, f16), (f16, bf16), (f32, f32))]
    print(f"k {k} scale {scale}: acc worst err/(U*mag) per addition {max(w[0] for w in worst):.2f}"
          f"; wire worst err/bound {max(w[1] for w in worst):.2f} (c {k + 1})")


def test_kernels_give_the_bits_of_the_fallbacks(cuda):
    """the fallbacks do the same fp32 arithmetic in the same order: equal bits, every dtype
    pair, a scale that is no power of two"""
    cpu = torch.device("cpu")
    for gdt in R.DTYPES:
        for wdt in R.DTYPES:
            a = R.run_window(cuda, [R.N_GRID, R.TAIL], gdt, wdt, 4, 0.37, seed=11)
            b = R.run_window(cpu, [R.N_GRID, R.TAIL], gdt, wdt, 4, 0.37, seed=11)
            assert torch.equal(a[2], b[2]), f"{gdt}: accumulator bits differ"
            assert torch.equal(a[3].float(), b[3].float()), f"{gdt}->{wdt}: wire bits differ"


def test_more_tensors_than_one_table(cuda):
    wa, ww = R.run_many(cuda)
    print(f"{len(R.MANY)} tensors: acc {wa:.2f}, wire {ww:.2f}")


@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("wdt", R.DTYPES)
def test_pack_accumulated_flag(cuda, gdt, wdt):
    R.run_flag(cuda, gdt, wdt, 0)
    R.run_flag(cuda, gdt, wdt, 1)


# ---- B. evidence that the feature is what passes -----------------------------------------------------
def test_bf16_accumulation_misses_the_bound_the_arena_meets(cuda):
    """today's arithmetic through the same harness: bf16 ``+=`` of 16 gradients, then K.pack"""
    old, new = R.run_evidence(cuda, 16)
    print(f"k 16: bf16 accumulation + pack {100 * old:.1f} % of the elements outside the bound, "
          f"fp32 arena {100 * new:.1f} %")
    assert old >= 0.5, "the inputs do not tell bf16 accumulation from fp32"
    assert new == 0.0


# ---- C. operand checks --------------------------------------------------------------------------------
def test_accum_bindings_reject_bad_operands(cuda):
    """A bad operand of an otherwise valid GPU call raises before any launch.  Every bad
    operand is a live allocation of its own (too short, of another dtype, or on the host), so
    nothing could be read or written out of bounds even if a check were missing."""
    ac = K.native()._accum
    n = K.CHUNK + 5

    def accumulate(offs=(0,), **bad):
        a = dict(g=torch.ones(n, dtype=bf16, device=cuda), acc=torch.zeros(n, device=cuda))
        a.update(bad)
        ac.accumulate([a["g"]], a["acc"], list(offs), True)

    def last(offs=(0,), **bad):
        a = dict(g=torch.ones(n, dtype=bf16, device=cuda), acc=torch.zeros(n, device=cuda),
                 dst=torch.zeros(n, dtype=f16, device=cuda),
                 flag=torch.zeros(1, dtype=torch.int32, device=cuda))
        a.update(bad)
        ac.pack_accumulated([a["g"]], a["acc"], a["dst"], list(offs), 1.0, a["flag"])

    accumulate()                                                  # the valid calls launch
    last()
    torch.cuda.synchronize()
    cases = [
        (accumulate, "accumulate: acc must be a Float GPU", dict(acc=torch.zeros(n, dtype=bf16, device=cuda))),
        (accumulate, "accumulate: acc must be a Float GPU", dict(acc=torch.zeros(n))),
        (accumulate, "accumulate: acc must be contiguous", dict(acc=torch.zeros(2 * n, device=cuda)[::2])),
        (accumulate, "accumulate: tensor 0 .* exceeds flat buffer", dict(acc=torch.zeros(n - 1, device=cuda))),
        (accumulate, "accumulate: tensor 0 .* exceeds flat buffer", dict(offs=(1,))),
        (accumulate, "accumulate: tensor 0 .* exceeds flat buffer", dict(offs=(-1,))),
        (accumulate, "accumulate: tensors/offsets length mismatch", dict(offs=(0, 64))),
        (accumulate, "accumulate: tensors must be a fp32 / bf16 / fp16 GPU", dict(g=torch.ones(n, dtype=torch.float64, device=cuda))),
        (last, "pack_accumulated: acc must be a Float GPU", dict(acc=torch.zeros(n, dtype=f16, device=cuda))),
        (last, "pack_accumulated: tensor 0 .* exceeds flat buffer", dict(acc=torch.zeros(n - 1, device=cuda))),
        (last, "pack_accumulated: tensor 0 .* exceeds flat buffer", dict(dst=torch.zeros(n - 1, dtype=f16, device=cuda))),
        (last, "pack_accumulated: dst must be a fp32 / bf16 / fp16 GPU", dict(dst=torch.zeros(n, dtype=f16))),
        (last, "pack_accumulated: dst must be contiguous", dict(dst=torch.zeros(2 * n, dtype=f16, device=cuda)[::2])),
        (last, "pack_accumulated: nonfinite must be a Int GPU", dict(flag=torch.zeros(1, dtype=torch.int64, device=cuda))),
        (last, "pack_accumulated: nonfinite must hold at least 1", dict(flag=torch.zeros(0, dtype=torch.int32, device=cuda))),
    ]
    for fn, msg, bad in cases:
        with pytest.raises(RuntimeError, match=msg):
            fn(**bad)


# ---- D. the model level -------------------------------------------------------------------------------
@pytest.fixture
def deterministic():
    """the twin model must reproduce the wrapped model's gradients bit for bit"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_model_plain_sgd_and_release(cuda, deterministic):
    print(f"(a, g) plain SGD, bf16 wire: worst err/bound {R.model_plain_sgd(cuda):.2f}")


@pytest.mark.parametrize("kind", ["fused_sgd", "fused_adam"])
def test_model_fused_fp16_wire_guard(cuda, deterministic, kind):
    print(f"(b) {kind}: worst {R.FR.fmt(R.model_fused(cuda, kind))} (grad: err/bound; the rest "
          f"err/(U*mag), c {R.FR.C_SGD_W if kind == 'fused_sgd' else R.FR.C_ADAM_W})")


def test_model_partial_window(cuda, deterministic):
    print(f"(c) synchronize() after 2 of 4: worst err/bound {R.model_partial(cuda):.2f}")


@pytest.mark.parametrize("kind", ["sgd", "fused_sgd"])
@pytest.mark.parametrize("skip_pass", [1, 3])
@pytest.mark.parametrize("bucket_mb", [1e-5, 64])
def test_model_parameter_unused_in_one_pass(cuda, deterministic, kind, skip_pass, bucket_mb):
    worst, nb = R.model_unused(cuda, kind, skip_pass, bucket_mb)
    assert (nb == 6) == (bucket_mb < 1)
    print(f"(d) {kind}, lin2 unused in pass {skip_pass}, {nb} buckets: worst err/bound {worst:.2f}")


def test_model_gradient_aliasing_its_slot(cuda, deterministic):
    print(f"(e) aliased slots: worst err/bound {R.model_aliased(cuda)}")


def test_model_zero_grad_inside_a_window(cuda, deterministic):
    print(f"(f) zero_grad() after 2 of 4: worst err/bound {R.model_zero_grad(cuda):.2f}")


def test_model_overflow_skips_the_step(cuda, deterministic):
    print(f"(h) window after the skipped one: worst err/bound {R.model_overflow(cuda):.2f}")


# ---- E. ranks -----------------------------------------------------------------------------------------
@pytest.mark.multirank
@pytest.mark.parametrize("scenario", ["dist_average", "dist_adasum"])
def test_distributed_accumulation_ranks_one_gpu(cuda, scenario):
    """2 ranks sharing one GPU over the gloo wire (tests/accum_workers.py), per-rank
    micro-batches: the same bits on both ranks, within the bound of the float64 reference"""
    for o in run_accum_ranks(scenario, "cuda", timeout=_TMO[2], extra_env=_one_gpu(2)):
        print(o[-900:])
