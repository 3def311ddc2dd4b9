"""Global gradient-norm clipping on the GPU: grad_sumsq_kernel and clip_finalize_kernel
(csrc/kernels/mv_clip.hip) and the gclip operand of every K6 step kernel against float64 and
against their own unclipped launches, max_grad_norm of mivod.optim.Fused* standalone, under a
captured HIP graph and under DistributedOptimizer.  The references, the counted bounds (c) and
the shared cases are in tests/clip_reference.py; tests/test_clip_cpu.py runs the PyTorch
fallbacks through the same cases.

Each test prints its worst err / (2^-24 * mag) next to the counted c."""
import copy

import pytest
import torch
import torch.nn.functional as F

import clip_reference as R
from mivod.ops import kernels as K
from test_clip_cpu import run_clip_ranks
from test_multirank_gpu import _TMO, _one_gpu

pytestmark = pytest.mark.gpu

f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


# ---- A. grad_sumsq ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES)
def test_grad_sumsq_sizes(cuda, dt):
    """every size around a lane (8), a step (2048) and a chunk (4096), from an aligned base
    (load8) and from base[1:] (one by one): the same bits either way"""
    worst = 0.0
    for n in R.SIZES:
        wa, pa = R.run_sumsq(cuda, n, dt, 0, seed=n)
        wb, pb = R.run_sumsq(cuda, n, dt, 1, seed=n)
        assert torch.equal(pa, pb), f"n={n}: an offset view changes the bits"
        worst = max(worst, wa, wb)
    print(f"grad_sumsq {dt}: worst err/(U*mag) {worst:.2f}; c {R.C_PARTIAL}")


@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("base_off", [0, 1])
def test_grad_sumsq_flag(cuda, dt, base_off):
    R.run_sumsq_flag(cuda, dt, base_off)


# ---- B. clip_finalize ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FINALIZE_CASES)
def test_clip_finalize(cuda, case):
    worst = [R.run_finalize(cuda, count, case) for count in R.FINALIZE_COUNTS]
    if worst[0] is not None:
        print(f"clip_finalize {case}: worst err/(U*mag) coef {max(w[0] for w in worst):.2f}, "
              f"norm {max(w[1] for w in worst):.2f}; c {R.C_CLIP}")


# ---- C. every step kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.STEP_KINDS)
@pytest.mark.parametrize("n", R.STEP_SIZES)
def test_step_with_gclip_is_the_step_of_the_scaled_gscale(cuda, kind, n):
    """a kernel that forgot the multiplier, applied it twice or applied it after the
    weight-decay term cannot give the bits of the unclipped launch with gscale * c"""
    R.run_step_clip(kind, n, cuda)


# ---- D. the model level -------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.OPTIMIZERS)
@pytest.mark.parametrize("mdt", [f32, bf16])
def test_fused_optimizer_with_max_grad_norm(cuda, name, mdt):
    worst, coefs = R.run_model(cuda, mdt, name)
    print(f"{name} {mdt}: coefficients {[round(c, 4) for c in coefs]}; worst err/(U*mag) "
          f"{R.FR.fmt(worst)}; c = the step's + {R.C_GCLIP}, norm {R.C_NORM}")


# ---- F. DistributedOptimizer ----------------------------------------------------------------------
@pytest.mark.multirank
@pytest.mark.parametrize("wire", ["fp16", "none"])
def test_distributed_clip_ranks_one_gpu(cuda, wire):
    """2 ranks sharing one GPU over the gloo wire (tests/clip_workers.dist_clip): fp16 wire
    with the guard on (the norm and the scan are one launch) and no compression with the guard
    off (the separate norm pass)."""
    for o in run_clip_ranks("dist_clip", "cuda", wire, timeout=_TMO[2], extra_env=_one_gpu(2)):
        print(o[-900:])


# ---- G. HIP graph -----------------------------------------------------------------------------------
# The 8 images are memorised within a few steps: measured on an MI355X, the gradient norm at the
# three compared steps is 0.033, 0.0017 and 0.0007.  1e-3 lies inside that range, so replays
# run on both sides of the threshold; the test asserts only that at least one clips.  Adam's
# update barely depends on the gradient's scale, so the eager / graph comparison keeps the
# tolerances of the unclipped test.
GRAPH_MAX_NORM = 1e-3


def test_graphed_clipped_adamw_step_matches_eager(cuda):
    """make_graphed_step with FusedAdamW(max_grad_norm) on the small model of
    tests/test_graphs_gpu.py: the norm pass, the finalize and the clipped updates are captured
    like the other kernels; replays equal eager steps over 3 steps with an LR change between
    them, and the steps do clip."""
    import mivod.torch as hvd
    from mivod.optim import FusedAdamW
    from test_graphs_gpu import _small_resnet

    hvd.init()
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    base = _small_resnet().to(cuda)
    models = [copy.deepcopy(base), copy.deepcopy(base)]
    opts = [hvd.DistributedOptimizer(FusedAdamW(m.parameters(), lr=2e-3, weight_decay=0.01,
                                                max_grad_norm=GRAPH_MAX_NORM),
                                     named_parameters=m.named_parameters()) for m in models]
    g = torch.Generator(device=cuda).manual_seed(7)
    x = torch.rand(8, 3, 64, 64, device=cuda, generator=g).to(bf16).contiguous(
        memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), device=cuda, generator=g)

    def stepper(m, o):
        def step():
            loss = F.cross_entropy(m(x).float(), y)
            loss.backward()
            o.step()
            o.zero_grad(set_to_none=True)
            return loss.detach()
        return step

    eager = stepper(models[0], opts[0])
    for _ in range(2):           # the graphed side runs 2 eager warmup steps
        eager()
    graphed = hvd.make_graphed_step(stepper(models[1], opts[1]), opts[1], model=models[1],
                                    warmup=2)
    lrs = [None, 0.5, 0.25]
    clipped = 0
    for lr in lrs:
        if lr is not None:
            for o in opts:
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * lr
        le = eager()
        lg = graphed()
        torch.cuda.synchronize()
        torch.testing.assert_close(lg, le, rtol=1e-2, atol=1e-2)
        ne, ng = float(opts[0].grad_norm()), float(opts[1].grad_norm())
        assert ne > 0 and abs(ng - ne) <= 2e-2 * ne, (ne, ng)
        clipped += float(opts[1]._mv_clip_block[0]) < 1.0
        print(f"graphed AdamW: grad norm eager {ne:.5g} graph {ng:.5g}, coefficient "
              f"{float(opts[1]._mv_clip_block[0]):.5g}")
    assert clipped, "no replay clipped: max_grad_norm is above every norm of this model"
    assert graphed.replays == len(lrs)
    for (n, p), q in zip(models[0].named_parameters(), models[1].parameters()):
        torch.testing.assert_close(q.float(), p.float(), rtol=2e-2, atol=2e-2, msg=n)
    torch.backends.cudnn.deterministic = False
    assert opts[1]._mvd_steps == opts[0]._mvd_steps
    hvd.shutdown()


# ---- H. operand checks ----------------------------------------------------------------------------
def test_clip_bindings_reject_bad_operands(cuda):
    """A bad operand of an otherwise valid GPU call raises before any launch.  Every bad
    operand is a live allocation of its own (too short, of another dtype, or on the host), so
    nothing could be read or written out of bounds even if a check were missing."""
    cl = K.native()._clip
    n = 2 * K.CHUNK + 5

    def sumsq(**bad):
        a = dict(x=torch.ones(n, dtype=f16, device=cuda), partial=torch.zeros(3, device=cuda),
                 flag=torch.zeros(1, dtype=torch.int32, device=cuda))
        a.update(bad)
        cl.grad_sumsq(a["x"], a["partial"], a["flag"])

    def finalize(total=3, **bad):
        a = dict(partial=torch.ones(3, device=cuda), clip=torch.zeros(2, device=cuda))
        a.update(bad)
        cl.clip_finalize(a["partial"], total, 0.5, 1.0, a["clip"])

    def sgd(**bad):
        a = dict(gclip=torch.ones(1, device=cuda))
        a.update(bad)
        cl.sgd_step(torch.zeros(64, device=cuda), torch.zeros(64, device=cuda), None, None, 0.1,
                    0.0, 0.0, 0.0, 1.0, False, False, None, None, a["gclip"])

    sumsq()                                                       # the valid calls launch
    cl.grad_sumsq(torch.ones(n, dtype=f16, device=cuda), torch.zeros(3, device=cuda), None)
    finalize()
    sgd()
    torch.cuda.synchronize()
    cases = [
        (sumsq, "grad_sumsq: partial must hold at least 3", dict(partial=torch.zeros(2, device=cuda))),
        (sumsq, "grad_sumsq: partial must be a Float GPU", dict(partial=torch.zeros(3, dtype=bf16, device=cuda))),
        (sumsq, "grad_sumsq: partial must be a Float GPU", dict(partial=torch.zeros(3))),
        (sumsq, "grad_sumsq: partial must be contiguous", dict(partial=torch.zeros(6, device=cuda)[::2])),
        (sumsq, "grad_sumsq: flag must be a Int GPU", dict(flag=torch.zeros(1, dtype=torch.int64, device=cuda))),
        (sumsq, "grad_sumsq: x must be a fp32 / bf16 / fp16 GPU", dict(x=torch.ones(n, dtype=torch.float64, device=cuda))),
        (finalize, "clip_finalize: clip must hold at least 2", dict(clip=torch.zeros(1, device=cuda))),
        (finalize, "clip_finalize: clip must be a Float GPU", dict(clip=torch.zeros(2, dtype=f16, device=cuda))),
        (finalize, "clip_finalize: partial must hold at least 4", dict(total=4)),
        (finalize, "clip_finalize: total must be >= 0", dict(total=-1)),
        (sgd, "sgd_step: gclip must be a Float GPU", dict(gclip=torch.ones(1, dtype=bf16, device=cuda))),
        (sgd, "sgd_step: gclip must be a Float GPU", dict(gclip=torch.ones(1))),
        (sgd, "sgd_step: gclip must hold at least 1", dict(gclip=torch.ones(0, device=cuda))),
    ]
    for fn, msg, bad in cases:
        with pytest.raises(RuntimeError, match=msg):
            fn(**bad)
    # the same check guards every clipped step: one call each with a gclip of the wrong dtype
    bad = torch.ones(1, dtype=bf16, device=cuda)
    for kind in R.STEP_KINDS:
        t, run = R.build_step(kind, 4097, cuda)
        with pytest.raises(RuntimeError, match="_step: gclip must be a Float GPU"):
            run(t, gclip=bad)
