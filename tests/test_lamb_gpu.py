"""The LAMB HIP kernels (csrc/kernels/mv_kernels.hip: lamb_moments_kernel -> seg_reduce_kernel<2>
-> lamb_apply_kernel) against float64 on every template instantiation and code path, and
FusedLAMB under a captured HIP graph and under DistributedOptimizer.  The reference, the
counted bounds (c) and the shared cases are in tests/lamb_reference.py; tests/test_lamb_cpu.py
runs the PyTorch fallback through the same cases.

Each test prints its worst err / (2^-24 * mag) next to the counted c."""
import copy

import pytest
import torch
import torch.nn.functional as F

import lamb_reference as R
from mivod.ops import kernels as K
from test_lamb_cpu import run_lamb_ranks
from test_multirank_gpu import _TMO, _one_gpu

pytestmark = pytest.mark.gpu

f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


# ---- A. the step against fp64 ----------------------------------------------------------------
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
@pytest.mark.parametrize("step", [1, 7])
def test_lamb_dtype_grid(cuda, gdt, mdt, step):
    """every TG of stage 1 and TP of stage 2 (model None runs TP = float), and the norms the
    segment reduce leaves in the workspace"""
    total, layout = R.grid_layout()
    ws = {}
    worst, ref, _ = R.run_lamb(total, gdt, mdt, cuda, layout, hp=dict(R.HP_LAMB, step=step),
                               zero_grad=R.LAMB_ZERO_GRAD, workspace=ws)
    got = ws["norms"][:2 * len(layout[0])].view(-1, 2)
    worst["norms"] = R.check("lamb norms", got, ref["norms"])
    print(f"lamb {gdt}/{mdt} step {step}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF}")


@pytest.mark.parametrize("gdt", [f16, bf16])
@pytest.mark.parametrize("step", [1, 7])
def test_lamb_sizes(cuda, gdt, step):
    """every size around a lane (8), a step (2048) and a chunk (4096)"""
    tot = {}
    for n in R.SIZES:
        total, layout = R.pair_layout(n)
        ws = {}
        worst, ref, _ = R.run_lamb(total, gdt, bf16, cuda, layout,
                                   hp=dict(R.HP_LAMB, step=step), seed=n, workspace=ws)
        worst["norms"] = R.check(f"lamb norms n={n}", ws["norms"][:4].view(-1, 2), ref["norms"])
        tot = {o: max(tot.get(o, 0.0), x) for o, x in worst.items()}
    print(f"lamb sizes {gdt}/bf16 step {step}: worst err/(U*mag) {R.fmt(tot)}; c {R.C_OF}")


@pytest.mark.parametrize("case", sorted(R.LAMB_FLAG_CASES))
def test_lamb_flags(cuda, case):
    worst, sens = R.run_lamb_flag(case, cuda)
    print(f"lamb {case}: worst {R.fmt(worst)}; the variant moves w by {sens} bounds")


@pytest.mark.parametrize("gdt,mdt", [(f16, bf16), (bf16, f32), (f32, None), (f32, f16)])
def test_lamb_unaligned(cuda, gdt, mdt):
    """segments at offsets no vector access may use: the scalar path of both stages"""
    ws = {}
    worst, ref, _ = R.run_lamb(R.UNAL_TOTAL, gdt, mdt, cuda, R.UNAL_LAYOUT, seed=13, workspace=ws)
    worst["norms"] = R.check("lamb norms", ws["norms"][:8].view(-1, 2), ref["norms"])
    print(f"lamb unaligned {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF}")


def test_lamb_two_launches_are_bitwise_equal(cuda):
    total, layout = R.grid_layout()
    t0 = R.lamb_inputs(total, f16, bf16, cuda, layout, seed=11)
    a, b = R.clone_inputs(t0), R.clone_inputs(t0)
    wa, wb = {}, {}
    R.call_lamb(a, R.HP_LAMB, layout, cuda, workspace=wa)
    R.call_lamb(b, R.HP_LAMB, layout, cuda, workspace=wb)
    for k in ("w", "m", "v", "model"):
        assert torch.equal(a[k], b[k]), k
    ns = 2 * len(layout[0])
    assert torch.equal(wa["norms"][:ns], wb["norms"][:ns])
    assert not torch.equal(a["w"], t0["w"])


# ---- B. skip and dyn ---------------------------------------------------------------------------
def test_lamb_skip_leaves_everything_untouched(cuda):
    R.run_lamb_skip(cuda)


def _dyn_run(cuda, hp, dyn=None):
    total, layout = R.grid_layout()
    t = R.lamb_inputs(total, f16, bf16, cuda, layout, seed=12)
    extra = {} if dyn is None else dict(dyn=torch.tensor(dyn, dtype=f32, device=cuda))
    R.call_lamb(t, hp, layout, cuda, **extra)
    return t


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))


@pytest.mark.parametrize("step", [1, 5])
def test_lamb_dyn_block_overrides_scalars(cuda, step):
    """dyn = [lr, -, bc1, bc2] wins over a bogus scalar lr and step and gives the bits of
    the scalar call with the same values; the bogus scalars alone do change the result."""
    hp = dict(R.HP_LAMB, lr=0.07, step=step)
    bogus = dict(hp, lr=99.0, step=6 - step)
    dyn = [0.07, 123.0, 1 - hp["beta1"] ** step, 1 - hp["beta2"] ** step]
    want = _dyn_run(cuda, hp)
    got = _dyn_run(cuda, bogus, dyn)
    assert _same(got, want), "the dyn block does not reproduce the scalar call"
    assert not _same(_dyn_run(cuda, bogus), want), "the bogus scalars change nothing"


# ---- C. operand checks ---------------------------------------------------------------------------
def test_lamb_binding_rejects_bad_secondary_operands(cuda):
    """A bad secondary operand of an otherwise valid GPU call raises before any launch.
    Non-contiguous operands are base[::2] views, so every pointer stays inside a live
    allocation; the short norms buffer is refused by its size and never dereferenced."""
    lb = K.native()._lamb
    n = 128
    tb = K.make_chunk_table([64, 64], cuda)

    def call(**bad):
        a = dict(g=torch.zeros(n, device=cuda), w=torch.zeros(n, device=cuda),
                 m=torch.zeros(n, device=cuda), v=torch.zeros(n, device=cuda),
                 sflag=torch.zeros(2, dtype=torch.int32, device=cuda),
                 partial=torch.zeros(4, device=cuda), norms=torch.zeros(4, device=cuda))
        a.update(bad)
        lb.lamb_step(a["g"], a["w"], a["m"], a["v"], None, tb.begin, tb.len, tb.seg, tb.seg_c0,
                     tb.seg_nc, a["sflag"], a["partial"], a["norms"], 1e-3, 0.9, 0.999, 1e-6,
                     0.01, 1.0, 1, None, None)

    call()                                                        # the valid call launches
    torch.cuda.synchronize()
    cases = {
        "exp_avg must": dict(m=torch.zeros(n, dtype=bf16, device=cuda)),
        "norms must hold at least 4": dict(norms=torch.zeros(3, device=cuda)),
        "exp_avg_sq must be contiguous": dict(v=torch.zeros(2 * n, device=cuda)[::2]),
        "exp_avg_sq must hold exactly": dict(v=torch.zeros(2 * n, device=cuda)),
        "sflag must": dict(sflag=torch.zeros(2, dtype=torch.int64, device=cuda)),
        "partial must hold at least 4": dict(partial=torch.zeros(3, device=cuda)),
    }
    for msg, bad in cases.items():
        with pytest.raises(RuntimeError, match=f"lamb_step: {msg}"):
            call(**bad)


# ---- D. HIP graph ----------------------------------------------------------------------------------
def test_graphed_lamb_step_matches_eager(cuda):
    """make_graphed_step with FusedLAMB on the small model of tests/test_graphs_gpu.py:
    replays equal eager steps over 3 steps with an LR change between them (lr, bc1 and bc2
    reach both LAMB kernels through the dyn block)."""
    import mivod.torch as hvd
    from mivod.optim import FusedLAMB
    from test_graphs_gpu import _small_resnet

    hvd.init()
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    base = _small_resnet().to(cuda)
    models = [copy.deepcopy(base), copy.deepcopy(base)]
    opts = [hvd.DistributedOptimizer(FusedLAMB(m.parameters(), lr=2e-3, weight_decay=0.01),
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
    for lr in lrs:
        if lr is not None:
            for o in opts:
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * lr
        le = eager()
        lg = graphed()
        torch.cuda.synchronize()
        torch.testing.assert_close(lg, le, rtol=1e-2, atol=1e-2)
    assert graphed.replays == len(lrs)
    for (n, p), q in zip(models[0].named_parameters(), models[1].parameters()):
        torch.testing.assert_close(q.float(), p.float(), rtol=2e-2, atol=2e-2, msg=n)
    torch.backends.cudnn.deterministic = False
    assert opts[1]._mvd_steps == opts[0]._mvd_steps
    hvd.shutdown()


# ---- E. DistributedOptimizer ------------------------------------------------------------------------
@pytest.mark.multirank
def test_distributed_fused_lamb_ranks_one_gpu(cuda):
    """2 ranks sharing one GPU over the gloo wire, fp16 compression, overflow guard on
    (tests/lamb_workers.dist_lamb): after 2 steps each rank's parameters equal a
    single-process FusedLAMB fed the averaged gradients within the wire's rounding; a step
    with an injected non-finite gradient is skipped on both ranks (w, m and v bitwise
    unchanged); parameters and moments are bitwise equal across ranks at the end."""
    for o in run_lamb_ranks("cuda", timeout=_TMO[2], extra_env=_one_gpu(2)):
        print(o[-600:])
