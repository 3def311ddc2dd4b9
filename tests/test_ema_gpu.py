"""The fp32 moving average of the master weights on the GPU: ema_kernel's three modes
(csrc/kernels/mv_ema.hip) against float64 and against the fallbacks' bits, ``ema_decay`` of the
Fused* optimizers alone, on the GPU hook path, on 2 ranks sharing one GPU, and in a captured
HIP graph.  The references, the counted bounds and the shared cases are in
tests/ema_reference.py; tests/test_ema_cpu.py runs the PyTorch fallbacks through the same
cases.

Each test prints its worst err / (2^-24 * mag) next to the counted c, or its worst
err / bound."""
import copy

import pytest
import torch

import ema_reference as R
from mivod.ops import kernels as K
from test_ema_cpu import run_ema_ranks
from test_multirank_gpu import _TMO, _one_gpu

pytestmark = pytest.mark.gpu

f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


# ---- A. the three modes -----------------------------------------------------------------------------
@pytest.mark.parametrize("mdt", R.MODELS)
def test_ema_modes_sizes(cuda, mdt):
    """every size around a lane (8), a step (2048) and a chunk (4096), from an aligned base
    (load8 / store8) and from base[1:] (one by one): the update within the bound and the same
    bits either way, swap and overwrite exact, the guards around every range untouched"""
    print(f"model {mdt}: update worst err/(U*mag) {R.run_sizes(cuda, mdt):.2f} (c {R.C_EMA})")


@pytest.mark.parametrize("mdt", R.MODELS)
def test_ema_exact_paths_and_skip(cuda, mdt):
    for off in (0, 1):
        R.run_exact(cuda, mdt, base_off=off)
        R.run_skip(cuda, mdt, base_off=off)


def test_kernels_give_the_bits_of_the_fallbacks(cuda):
    """the fallbacks do the same fp32 operations in the same order: equal bits in every mode,
    with a decay that is no power of two"""
    cpu = torch.device("cpu")
    for mdt in R.MODELS:
        for n in (9, R.N_GRID):
            for off in (0, 1):
                a = R.run_modes(cuda, n, mdt, off, decay=R.DECAY, seed=11)
                b = R.run_modes(cpu, n, mdt, off, decay=R.DECAY, seed=11)
                assert torch.equal(a[1], b[1]), f"n={n} off={off}: update bits differ"
                assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
                if mdt is not None:
                    assert torch.equal(a[4], b[4]), f"{mdt}: model bits differ"


def test_ema_bindings_reject_bad_operands(cuda):
    """A bad operand of an otherwise valid GPU call raises before any launch.  Every bad
    operand is a live allocation of its own (too short, of another dtype, or on the host), so
    nothing could be read or written out of bounds even if a check were missing."""
    em = K.native()._ema
    n = K.CHUNK + 5

    def good():
        return dict(w=torch.ones(n, device=cuda), e=torch.zeros(n, device=cuda),
                    model=torch.zeros(n, dtype=bf16, device=cuda),
                    skip=torch.zeros(1, dtype=torch.int32, device=cuda), decay=0.9)

    def update(**bad):
        a = good()
        a.update(bad)
        em.ema_update(a["w"], a["e"], a["decay"], a["skip"])

    def swap(**bad):
        a = good()
        a.update(bad)
        em.ema_swap(a["w"], a["e"], a["model"], a["skip"])

    def overwrite(**bad):
        a = good()
        a.update(bad)
        em.ema_overwrite(a["w"], a["e"], a["model"], a["skip"])

    update()                                                      # the valid calls launch
    swap()
    overwrite()
    torch.cuda.synchronize()
    cases = [
        (update, "ema_update: master must be a Float GPU", dict(w=torch.ones(n, dtype=bf16, device=cuda))),
        (update, "ema_update: master must be a Float GPU", dict(w=torch.ones(n))),
        (update, "ema_update: master must be contiguous", dict(w=torch.ones(2 * n, device=cuda)[::2])),
        (update, "ema_update: ema must be a Float GPU", dict(e=torch.zeros(n, dtype=f16, device=cuda))),
        (update, "ema_update: ema must be a Float GPU", dict(e=torch.zeros(n))),
        (update, "ema_update: ema must be contiguous", dict(e=torch.zeros(2 * n, device=cuda)[::2])),
        (update, "ema_update: ema must hold exactly", dict(e=torch.zeros(n - 1, device=cuda))),
        (update, "ema_update: ema must hold exactly", dict(e=torch.zeros(n + 1, device=cuda))),
        (update, "ema_update: skip must be a Int GPU", dict(skip=torch.zeros(1, dtype=torch.int64, device=cuda))),
        (update, "ema_update: skip must be a Int GPU", dict(skip=torch.zeros(1, dtype=torch.int32))),
        (update, "ema_update: skip must hold at least 1", dict(skip=torch.zeros(0, dtype=torch.int32, device=cuda))),
        (update, "ema_update: decay must be in", dict(decay=1.0)),
        (update, "ema_update: decay must be in", dict(decay=-0.01)),
        (update, "ema_update: decay must be in", dict(decay=float("nan"))),
        (swap, "ema_swap: ema must hold exactly", dict(e=torch.zeros(n - 1, device=cuda))),
        (swap, "ema_swap: model must hold exactly", dict(model=torch.zeros(n - 1, dtype=bf16, device=cuda))),
        (swap, "ema_swap: model must be a fp32 / bf16 / fp16 GPU", dict(model=torch.zeros(n, dtype=torch.float64, device=cuda))),
        (swap, "ema_swap: model must be a fp32 / bf16 / fp16 GPU", dict(model=torch.zeros(n, dtype=bf16))),
        (swap, "ema_swap: model must be contiguous", dict(model=torch.zeros(2 * n, dtype=bf16, device=cuda)[::2])),
        (swap, "ema_swap: skip must be a Int GPU", dict(skip=torch.zeros(1, device=cuda))),
        (overwrite, "ema_overwrite: master must hold|ema_overwrite: ema must hold exactly", dict(w=torch.ones(n - 1, device=cuda))),
        (overwrite, "ema_overwrite: model must hold exactly", dict(model=torch.zeros(n + 3, dtype=f16, device=cuda))),
        (overwrite, "ema_overwrite: ema must be a Float GPU", dict(e=torch.zeros(n, dtype=bf16, device=cuda))),
    ]
    for fn, msg, bad in cases:
        with pytest.raises((RuntimeError, ValueError), match=msg):
            fn(**bad)


# ---- B. evidence that the feature is what passes -----------------------------------------------------
def test_bf16_average_misses_the_bound_the_arena_meets(cuda):
    """today's arithmetic through the same harness: a bf16 ``lerp_`` average of the bf16 model
    copy (AveragedModel / ModelEma on this code base) against the fp32 arena average"""
    old, new, worst = R.run_evidence(cuda)
    print(f"decay {R.EVIDENCE_DECAY}, {R.EVIDENCE_STEPS} steps: bf16 lerp_ {100 * old:.1f} % of "
          f"the elements outside the bound, fp32 arena {100 * new:.1f} % (worst err/bound "
          f"{worst:.3f})")
    assert old >= 0.9, "the inputs do not tell a bf16 average from the fp32 arena average"
    assert new == 0.0


# ---- C. the optimizers -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.OPTIMIZERS)
@pytest.mark.parametrize("dtype", [bf16, f32])
def test_optimizer_average_follows_the_masters(cuda, kind, dtype):
    worst, _, _ = R.model_optimizer(cuda, kind, dtype)
    print(f"{kind} {dtype}, 4 steps: worst err/bound {worst:.3f} (c {R.C_EMA} per update)")


@pytest.mark.parametrize("dtype", [bf16, f32])
def test_ema_parameters_swaps_and_restores(cuda, dtype):
    R.model_swap(cuda, dtype)


@pytest.mark.parametrize("dtype", [bf16, f32])
def test_state_dict_roundtrip(cuda, dtype):
    R.model_state_dict(cuda, dtype)


def test_checkpoint_roundtrip(cuda, tmp_path):
    R.model_state_dict(cuda, bf16, tmp_path)


def test_state_dict_keys_without_ema_are_unchanged(cuda):
    assert R.state_keys(cuda, "sgd", bf16) == ["master_param", "momentum_buffer", "step"]
    assert R.state_keys(cuda, "adam", f32) == ["exp_avg", "exp_avg_sq", "step"]


# ---- D. the hook path ----------------------------------------------------------------------------------
@pytest.fixture
def hvd_torch():
    import mivod.torch as hvd
    hvd.init()
    yield hvd
    hvd.shutdown()


@pytest.mark.parametrize("mode", R.HOOK_MODES)
def test_hook_path_one_rank(cuda, hvd_torch, monkeypatch, mode):
    if mode == "guard_bucket":
        monkeypatch.setenv("MIVOD_GUARD_MODE", "bucket")
    else:
        monkeypatch.delenv("MIVOD_GUARD_MODE", raising=False)
    print(f"{mode}: worst err/bound {R.hook_path(cuda, mode):.3f} (c {R.C_EMA} per update)")


@pytest.mark.parametrize("bad_step", [2, 1])
def test_hook_path_overflow_skips_step_and_average(cuda, hvd_torch, monkeypatch, bad_step):
    """one inf gradient element (a value on the fp16 wire, not a fault): the guard's flag skips
    the step's updates and the average's alike"""
    monkeypatch.delenv("MIVOD_GUARD_MODE", raising=False)
    worst = R.hook_overflow(cuda, bad_step=bad_step)
    print(f"inf at step {bad_step}: worst err/bound {worst:.3f}")


@pytest.mark.multirank
@pytest.mark.parametrize("mode", ["overlapped", "guard_step"])
def test_hook_path_ranks_one_gpu(cuda, mode):
    """2 ranks sharing one GPU over the gloo wire (tests/ema_workers.py), per-rank batches:
    the same average bits on both ranks, within the bound of the float64 reference"""
    for o in run_ema_ranks("dist_ema", "cuda", mode, timeout=_TMO[2], extra_env=_one_gpu(2)):
        print(o[-600:])


# ---- E. graph --------------------------------------------------------------------------------------------
def test_graphed_step_with_ema_matches_eager(cuda, hvd_torch):
    """make_graphed_step with FusedSGD(ema_decay): the warmup takes the copying update, the
    captured update launches carry the decay; 3 replays give the bits of 3 eager steps"""
    hvd = hvd_torch
    base = R.make_mlp(cuda, bf16)
    models = [copy.deepcopy(base), copy.deepcopy(base)]
    opts = [hvd.DistributedOptimizer(R.make_opt("sgd", m.parameters(), 0.9),
                                     named_parameters=m.named_parameters()) for m in models]
    batches = R.make_batches(cuda, bf16, 5, seed=4)
    x = batches[0][0].clone()
    y = batches[0][1].clone()

    def stepper(m, o):
        def step():
            loss = R.loss_of(m, (x, y))
            loss.backward()
            o.step()
            o.zero_grad(set_to_none=True)
            return loss.detach()
        return step

    eager = stepper(models[0], opts[0])
    for _ in range(2):           # the graphed side runs 2 eager warmup steps on the same batch
        eager()
    graphed = hvd.make_graphed_step(stepper(models[1], opts[1]), opts[1], model=models[1],
                                    warmup=2)
    assert all(a.ema_updates == 2 for a in opts[1]._mv_arenas), "the capture was counted"
    for bx, by in batches[2:]:
        x.copy_(bx)
        y.copy_(by)
        eager()
        graphed()
        torch.cuda.synchronize()
    assert graphed.replays == 3
    for a, b in zip(opts[0]._mv_arenas, opts[1]._mv_arenas):
        assert a.ema_updates == b.ema_updates == 5 and a.step == b.step == 5
        assert torch.equal(a.master, b.master), "graph replays and eager steps differ"
        assert torch.equal(a.ema, b.ema), "the graphed average differs from the eager one"
        assert not torch.equal(b.ema, b.master)
