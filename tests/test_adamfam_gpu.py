"""The Adam-family HIP kernels of csrc/kernels/mv_adamfam.hip (Adam / AdamW with amsgrad, Adamax,
NAdam) against float64 on every template instantiation and code path, the Fused* classes under
a captured HIP graph and under DistributedOptimizer, and the Keras classes on a GPU.  The
references, the counted bounds (c) and the shared cases are in tests/adamfam_reference.py;
tests/test_adamfam_cpu.py runs the PyTorch fallbacks through the same cases.

All three kernels run on the streaming skeleton of csrc/kernels/mv_flat_step.h and their
bindings take any offset, so test_unaligned runs the skeleton's scalar path with two and with
three state streams.  Bad operands are refused by the bindings' host-side checks before any
launch.

Each test prints its worst err / (2^-24 * mag) next to the counted c."""
import copy

import pytest
import torch

import adamfam_reference as R
from test_adamfam_cpu import keras_step, run_adamfam_ranks

pytestmark = pytest.mark.gpu

f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


# ---- A. the steps against fp64 -----------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
def test_dtype_grid(cuda, kind, gdt, mdt):
    """every TG x TP instantiation (model None runs TP = float) at 3 chunks + 5 elements"""
    worst, _, _ = R.run_step(kind, R.N_GRID, gdt, mdt, cuda)
    print(f"{kind} {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("gdt", [f16, bf16])
def test_sizes(cuda, kind, gdt):
    """every size around a lane (8), a step (2048) and a chunk (4096)"""
    tot = {}
    for n in R.SIZES:
        worst, _, _ = R.run_step(kind, n, gdt, bf16, cuda, seed=n)
        tot = {o: max(tot.get(o, 0.0), x) for o, x in worst.items()}
    print(f"{kind} sizes {gdt}/bf16: worst err/(U*mag) {R.fmt(tot)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("gdt,mdt", [(f16, bf16), (bf16, f32), (f32, None), (f32, f16)])
def test_unaligned(cuda, kind, gdt, mdt):
    """views at offsets no vector access may use: the scalar path of every element"""
    worst = R.run_unaligned(kind, gdt, mdt, cuda)
    print(f"{kind} unaligned {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("adamw,keras_eps,step", [(False, False, 1), (True, False, 7),
                                                  (False, True, 7), (True, True, 1)])
def test_amsgrad_flags_and_sensitivity(cuda, adamw, keras_eps, step):
    worst, sens = R.run_amsgrad_flags(adamw, keras_eps, step, cuda)
    print(f"amsgrad adamw={adamw} keras_eps={keras_eps} step={step}: worst {R.fmt(worst)}; "
          f"moved by {R.fmt(sens)} bounds")


@pytest.mark.parametrize("keras_eps", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adamax_flags_and_sensitivity(cuda, keras_eps, weight_decay):
    worst, sens = R.run_adamax_flags(keras_eps, weight_decay, cuda)
    print(f"adamax keras_eps={keras_eps} wd={weight_decay}: worst {R.fmt(worst)}; moved by "
          f"{R.fmt(sens)} bounds")


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("momentum_decay", [0.0, 0.5])
def test_nadam_flags_and_sensitivity(cuda, decoupled, momentum_decay):
    worst, sens = R.run_nadam_flags(decoupled, momentum_decay, cuda)
    print(f"nadam decoupled={decoupled} momentum_decay={momentum_decay}: worst {R.fmt(worst)}; "
          f"moved by {R.fmt(sens)} bounds")


def test_adamax_zero_divisor_takes_no_update(cuda):
    worst = R.run_adamax_zero_divisor(cuda)
    print(f"adamax zero divisor: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF['adamax']}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_two_launches_are_bitwise_equal(cuda, kind):
    t0 = R.adamfam_inputs(kind, R.N_GRID, f16, bf16, cuda, seed=11)
    a, b = R.clone_inputs(t0), R.clone_inputs(t0)
    R.call_step(kind, a, R.HP[kind])
    R.call_step(kind, b, R.HP[kind])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["w"], t0["w"])


# ---- B. skip, dyn and gclip ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_skip_leaves_everything_untouched(cuda, kind):
    R.run_skip(kind, cuda)


@pytest.mark.parametrize("kind", R.KINDS)
def test_dyn_block_overrides_the_scalar_arguments(cuda, kind):
    """the dyn block wins over bogus scalars (lr, and the step that feeds bc1, bc2 and NAdam's
    cg, cm): the result matches the reference for the block's values, [lr, -, bc1, bc2] for
    amsgrad and Adamax and [lr, cg, cm, bc2] for NAdam; the bogus scalars alone do change the
    result."""
    hp, bogus, block, extra = R.dyn_case(kind)
    t0 = R.adamfam_inputs(kind, R.N_GRID, f16, bf16, cuda, seed=12)
    ref = R.ref_step(kind, t0, hp, **extra)
    got, plain = R.clone_inputs(t0), R.clone_inputs(t0)
    R.call_step(kind, got, bogus, dyn=torch.tensor(block, device=cuda))
    worst = R.check_outputs(f"{kind} dyn", kind, got, ref)
    R.call_step(kind, plain, bogus)
    assert not torch.equal(plain["w"], got["w"]), "the bogus scalars change nothing"
    print(f"{kind} dyn: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_clipped_launch_is_the_launch_of_the_product(cuda, kind):
    R.run_clip(kind, cuda)


def _bad_operands(dev):
    """(binding, the valid call's arguments, the index and name of every secondary operand)"""
    from mivod import _mvk
    n = 64

    def z(dtype=f32, k=n):
        return torch.zeros(k, dtype=dtype, device=dev)

    tail = (None, None, None)
    return [
        ("adam_amsgrad_step", _mvk._adamfam.adam_amsgrad_step,
         [z(bf16), z(), z(), z(), z(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, False, False,
          *tail], {1: "master", 2: "exp_avg", 3: "exp_avg_sq", 4: "max_exp_avg_sq"}, (15, 16, 17)),
        ("adamax_step", _mvk._adamfam.adamax_step,
         [z(bf16), z(), z(), z(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, False, *tail],
         {1: "master", 2: "exp_avg", 3: "exp_inf"}, (13, 14, 15)),
        ("nadam_step", _mvk._adamfam.nadam_step,
         [z(bf16), z(), z(), z(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.5, 0.5, 0.5, False,
          *tail], {1: "master", 2: "exp_avg", 3: "exp_avg_sq"}, (15, 16, 17)),
    ]


def test_a_bad_secondary_operand_raises_by_name(cuda):
    """wrong dtype, wrong size (too large), non-contiguous (a base[::2] view) and CPU tensors
    in every secondary operand, a short dyn / a float skip / an empty gclip: refused by the
    host-side checks before any launch, with the binding and the operand named.  The valid
    call with an offset view of every operand runs (these steps take any offset)."""
    for name, fn, args, secondary, (i_dyn, i_skip, i_clip) in _bad_operands(cuda):
        fn(*args)                                            # the valid call
        n = args[0].numel()
        for i, what in secondary.items():
            for bad in (torch.zeros(n, dtype=bf16, device=cuda),
                        torch.zeros(2 * n, dtype=f32, device=cuda),
                        torch.zeros(2 * n, dtype=f32, device=cuda)[::2],
                        torch.zeros(n, dtype=f32)):
                a = list(args)
                a[i] = bad
                with pytest.raises(RuntimeError, match=f"{name}: {what} must"):
                    fn(*a)
        a = list(args)
        a[4 if name != "adam_amsgrad_step" else 5] = torch.zeros(n + 8, dtype=bf16, device=cuda)
        with pytest.raises(RuntimeError, match=f"{name}: model numel mismatch"):
            fn(*a)
        for i, what, bad in ((i_dyn, "dyn", torch.zeros(3, device=cuda)),
                             (i_skip, "skip", torch.zeros(1, device=cuda)),
                             (i_clip, "gclip", torch.zeros(0, device=cuda))):
            a = list(args)
            a[i] = bad
            with pytest.raises(RuntimeError, match=f"{name}: {what} must"):
                fn(*a)
        a = list(args)
        a[{"adam_amsgrad_step": 12, "adamax_step": 11}.get(name, 13)] = 0
        with pytest.raises(RuntimeError, match=f"{name}: "):
            fn(*a)                                           # step 0 / bc2 0
        off = [torch.zeros(n + 1, dtype=y.dtype, device=cuda)[1:] if torch.is_tensor(y) else y
               for y in args]
        assert all(x.data_ptr() % 16 for x in off if torch.is_tensor(x))
        fn(*off)
    torch.cuda.synchronize()


# ---- C. HIP graph --------------------------------------------------------------------------------
class _Elementwise(torch.nn.Module):
    """parameters whose gradients come from elementwise kernels only, so that an eager step
    and a replayed one compute the same bits"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.a = torch.nn.Parameter(torch.randn(4097, generator=g))
        self.b = torch.nn.Parameter(torch.randn(33, 20, generator=g))
        self.c = torch.nn.Parameter(torch.randn(7, generator=g))

    def forward(self, x):
        return ((self.a.float() * x[:4097]).tanh().sum()
                + (self.b.float().reshape(-1) * x[:660]).sin().sum()
                + (self.c.float() * x[:7]).pow(2).sum())


def _graph_pair(cuda, make):
    """two copies of the model, each under DistributedOptimizer (world size 1) as in
    tests/test_graphs_gpu.py, and the step function of one of them"""
    import mivod.torch as hvd
    base = _Elementwise().to(cuda).to(bf16)
    models = [copy.deepcopy(base), copy.deepcopy(base)]
    opts = [hvd.DistributedOptimizer(make(m.parameters()), named_parameters=m.named_parameters())
            for m in models]
    x = torch.randn(4097, device=cuda, generator=torch.Generator(device=cuda).manual_seed(7))

    def stepper(m, o):
        def step():
            loss = m(x)
            loss.backward()
            o.step()
            o.zero_grad(set_to_none=True)
            return loss.detach()
        return step

    return models, opts, stepper


@pytest.mark.parametrize("kind", ["amsgrad", "adamw_amsgrad", "adamax", "nadam"])
def test_graphed_step_equals_eager_bitwise(cuda, kind):
    """make_graphed_step with each new optimizer: four replays with the lr changed between them
    (it, the bias corrections and NAdam's two weights reach the kernel through the dyn block
    the optimizer supplies) equal four eager steps bit for bit, in the master weights, the
    state and the model."""
    import mivod.torch as hvd
    from mivod.optim import FusedAdam, FusedAdamax, FusedAdamW, FusedNAdam

    def make(params):
        if kind == "amsgrad":
            return FusedAdam(params, lr=1e-2, weight_decay=1e-3, amsgrad=True)
        if kind == "adamw_amsgrad":
            return FusedAdamW(params, lr=1e-2, weight_decay=1e-2, amsgrad=True)
        if kind == "adamax":
            return FusedAdamax(params, lr=1e-2, weight_decay=1e-3)
        return FusedNAdam(params, lr=1e-2, weight_decay=1e-3, momentum_decay=0.05)

    hvd.init()
    models, opts, stepper = _graph_pair(cuda, make)
    eager = stepper(models[0], opts[0])
    for _ in range(2):           # the graphed side runs 2 eager warmup steps
        eager()
    graphed = hvd.make_graphed_step(stepper(models[1], opts[1]), opts[1], model=models[1],
                                    warmup=2)
    (a,), (b,) = opts[0]._mv_arenas, opts[1]._mv_arenas
    for lr in (None, 0.5, 0.25, 2.0):
        if lr is not None:
            for o in opts:
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * lr
        w0 = a.master.clone()
        le, lg = eager(), graphed()
        torch.cuda.synchronize()
        assert torch.equal(le, lg)
        assert torch.equal(a.master, b.master) and torch.equal(a.model, b.model)
        for n in a.state:
            assert torch.equal(a.state[n], b.state[n]), n
        assert not torch.equal(a.master, w0)
    assert graphed.replays == 4 and a.step == b.step == 6
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p, q)
    hvd.shutdown()


# ---- D. DistributedOptimizer ---------------------------------------------------------------------
@pytest.mark.multirank
def test_distributed_fused_amsgrad_guard_world1(cuda):
    """World size 1 on mivod's RCCL communicator with every collective forced, fp16 wire,
    overflow guard on (tests/adamfam_workers.guard_world1): a clean step matches fp64 within
    the bound; a step with an injected inf leaves master, state and model copy bitwise
    unchanged and is counted."""
    for o in run_adamfam_ranks("guard_world1", 1, "cuda", timeout=160,
                               extra_env={"MIVOD_TRANSPORT": "rccl",
                                          "MIVOD_FORCE_COLLECTIVES": "1"}):
        print(o[-800:])


# ---- E. Keras ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_keras_step_on_a_gpu_matches_the_cpu_fallback(cuda, kind):
    """one apply_gradients of Keras Adam(amsgrad=True) / Adamax / Nadam on GPU parameters and on
    CPU copies: both within the counted bound of the fp64 step from the zero state, so within
    two bounds of each other"""
    gpu, refs, w0 = keras_step(kind, cuda)
    cpu, _, _ = keras_step(kind, torch.device("cpu"))
    worst = 0.0
    for pg, pc, ref, w in zip(gpu, cpu, refs, w0):
        worst = max(worst, R.check(f"keras {kind} gpu", pg, ref),
                    R.check(f"keras {kind} cpu", pc, ref))
        assert not torch.equal(pg, w.reshape(-1))
    print(f"keras {kind}: worst err/(U*mag) {worst:.2f}; c {R.C_OF[kind]['w']}")
