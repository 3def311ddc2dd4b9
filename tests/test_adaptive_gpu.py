"""The RMSprop and Adagrad HIP kernels (csrc/kernels/mv_adaptive.hip) against float64 on every
template instantiation and code path, FusedRMSprop / FusedAdagrad under a captured HIP graph
and under DistributedOptimizer, and the Keras classes on a GPU.  The references, the counted
bounds (c) and the shared cases are in tests/adaptive_reference.py; tests/test_adaptive_cpu.py
runs the PyTorch fallbacks through the same cases.

Both kernels guard their vector body: RMSprop in a loop of its own, Adagrad through the
streaming skeleton of csrc/kernels/mv_flat_step.h that the SGD, Adam and Adadelta kernels also
run on.  test_unaligned[adagrad-*] is the one place that skeleton runs on unaligned operands
(the bindings of sgd_step / adam_step / adadelta_step refuse them,
tests/test_bindings_validation.py).

Each test prints its worst err / (2^-24 * mag) next to the counted c."""
import copy

import pytest
import torch

import adaptive_reference as R
from test_adaptive_cpu import run_adaptive_ranks

pytestmark = pytest.mark.gpu

f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
KINDS = ["rmsprop", "adagrad"]


# ---- A. the steps against fp64 -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
def test_dtype_grid(cuda, kind, gdt, mdt):
    """every TG x TP instantiation (model None runs TP = float) at 3 chunks + 5 elements"""
    worst, _, _ = R.run_step(kind, R.N_GRID, gdt, mdt, cuda)
    print(f"{kind} {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gdt", [f16, bf16])
def test_sizes(cuda, kind, gdt):
    """every size around a lane (8), a step (2048) and a chunk (4096)"""
    tot = {}
    for n in R.SIZES:
        worst, _, _ = R.run_step(kind, n, gdt, bf16, cuda, seed=n)
        tot = {o: max(tot.get(o, 0.0), x) for o, x in worst.items()}
    print(f"{kind} sizes {gdt}/bf16: worst err/(U*mag) {R.fmt(tot)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gdt,mdt", [(f16, bf16), (bf16, f32), (f32, None), (f32, f16)])
def test_unaligned(cuda, kind, gdt, mdt):
    """views at offsets no vector access may use: the scalar path of every element"""
    worst = R.run_unaligned(kind, gdt, mdt, cuda)
    print(f"{kind} unaligned {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("centered,momentum", R.RMSPROP_FLAGS)
def test_rmsprop_flags_and_sensitivity(cuda, centered, momentum):
    worst, sens = R.run_rmsprop_flags(centered, momentum, cuda)
    print(f"rmsprop centered={centered} momentum={momentum}: worst {R.fmt(worst)}; moved by "
          f"{R.fmt(sens)} bounds")


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adagrad_flags_and_sensitivity(cuda, weight_decay):
    worst, sens = R.run_adagrad_flags(weight_decay, cuda)
    print(f"adagrad wd={weight_decay}: worst {R.fmt(worst)}; moved by {R.fmt(sens)} bounds")


def test_rmsprop_clamps_a_negative_variance(cuda):
    worst = R.run_clamp(cuda)
    print(f"rmsprop clamp: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF['rmsprop']}")


@pytest.mark.parametrize("kind", KINDS)
def test_two_launches_are_bitwise_equal(cuda, kind):
    t0 = R.adaptive_inputs(kind, R.N_GRID, f16, bf16, cuda, seed=11)
    a, b = R.clone_inputs(t0), R.clone_inputs(t0)
    R.call_step(kind, a, R.HP[kind])
    R.call_step(kind, b, R.HP[kind])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["w"], t0["w"])


# ---- B. skip and dyn -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_skip_leaves_everything_untouched(cuda, kind):
    R.run_skip(kind, cuda)


@pytest.mark.parametrize("kind", KINDS)
def test_dyn_block_overrides_the_scalar_lr(cuda, kind):
    """dyn = [lr, -, -, -] wins over a bogus scalar lr: the result matches the reference for
    dyn[0]; the bogus scalar alone does change the result."""
    hp = dict(R.HP[kind], lr=0.07)
    bogus = dict(hp, lr=99.0)
    t0 = R.adaptive_inputs(kind, R.N_GRID, f16, bf16, cuda, seed=12)
    ref = R.ref_step(kind, t0, hp)
    got, plain = R.clone_inputs(t0), R.clone_inputs(t0)
    R.call_step(kind, got, bogus, dyn=torch.tensor([0.07, 123.0, 0.5, 0.5], device=cuda))
    worst = R.check_outputs(f"{kind} dyn", kind, got, ref)
    R.call_step(kind, plain, bogus)
    assert not torch.equal(plain["w"], got["w"]), "the bogus scalar changes nothing"
    print(f"{kind} dyn: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


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


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_step_equals_eager_bitwise(cuda, kind):
    """make_graphed_step with FusedRMSprop (momentum and centered) / FusedAdagrad: three
    replays with the lr changed between them (it reaches the kernel through the dyn block)
    equal three eager steps bit for bit, in the master weights, the state and the model."""
    import mivod.torch as hvd
    from mivod.optim import FusedAdagrad, FusedRMSprop

    def make(params):
        if kind == "rmsprop":
            return FusedRMSprop(params, lr=1e-2, momentum=0.9, centered=True, weight_decay=1e-3)
        return FusedAdagrad(params, lr=1e-2, weight_decay=1e-3, initial_accumulator_value=0.1)

    hvd.init()
    models, opts, stepper = _graph_pair(cuda, make)
    eager = stepper(models[0], opts[0])
    for _ in range(2):           # the graphed side runs 2 eager warmup steps
        eager()
    graphed = hvd.make_graphed_step(stepper(models[1], opts[1]), opts[1], model=models[1],
                                    warmup=2)
    (a,), (b,) = opts[0]._mv_arenas, opts[1]._mv_arenas
    for lr in (None, 0.5, 0.25):
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
    assert graphed.replays == 3 and a.step == b.step == 5
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p, q)
    hvd.shutdown()


def test_graphed_adagrad_refuses_lr_decay(cuda):
    """the dyn block carries the rate but no step count: lr_decay != 0 raises at capture"""
    import mivod.torch as hvd
    from mivod.optim import FusedAdagrad
    hvd.init()
    models, opts, stepper = _graph_pair(cuda, lambda p: FusedAdagrad(p, lr=1e-2, lr_decay=0.1))
    with pytest.raises(NotImplementedError, match="lr_decay"):
        hvd.make_graphed_step(stepper(models[1], opts[1]), opts[1], model=models[1], warmup=1)
    torch.cuda.synchronize()
    assert not opts[1]._mv_graph
    hvd.shutdown()


# ---- D. DistributedOptimizer ---------------------------------------------------------------------
@pytest.mark.multirank
def test_distributed_fused_rmsprop_guard_world1(cuda):
    """World size 1 on mivod's RCCL communicator with every collective forced, fp16 wire,
    overflow guard on (tests/adaptive_workers.guard_world1): a clean step matches fp64 within
    the bound; a step with an injected inf leaves master, state and model copy bitwise
    unchanged and is counted."""
    for o in run_adaptive_ranks("guard_world1", 1, "cuda", timeout=160,
                                extra_env={"MIVOD_TRANSPORT": "rccl",
                                           "MIVOD_FORCE_COLLECTIVES": "1"}):
        print(o[-800:])


# ---- E. Keras ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_keras_step_on_a_gpu_matches_the_cpu_fallback(cuda, kind):
    """one apply_gradients of Keras RMSprop / Adagrad on GPU parameters and on CPU copies:
    both within the counted bound of the fp64 step from the (zero / initial) state, so within
    two bounds of each other"""
    from mivod.kerasfw import optimizers as O
    gen = torch.Generator().manual_seed(5)
    shapes = [(4097,), (33, 20), (7,)]
    w0 = [torch.randn(s, generator=gen) for s in shapes]
    gs = [torch.randn(s, generator=gen) for s in shapes]
    res = {}
    for dev in (cuda, torch.device("cpu")):
        opt = (O.RMSprop(lr=0.01, rho=0.9, momentum=0.5, centered=True) if kind == "rmsprop"
               else O.Adagrad(lr=0.01, initial_accumulator_value=0.1))
        ps = [torch.nn.Parameter(w.clone().to(dev)) for w in w0]
        opt.apply_gradients(zip([g.to(dev) for g in gs], ps))
        res[dev.type] = [p.detach().cpu() for p in ps]
        assert type(opt._impl).__name__ == ("FusedRMSprop" if kind == "rmsprop" else "FusedAdagrad")
    worst = 0.0
    for w, g, pg, pc in zip(w0, gs, res["cuda"], res["cpu"]):
        w, g = w.reshape(-1), g.reshape(-1)
        z = torch.zeros_like(w)
        if kind == "rmsprop":
            ref = R.rmsprop_ref(g, w, z, z, z, lr=0.01, alpha=0.9, eps=1e-7, momentum=0.5,
                                centered=True)["w"]
        else:
            ref = R.adagrad_ref(g, w, z + 0.1, lr=0.01, eps=1e-7)["w"]
        worst = max(worst, R.check(f"keras {kind} gpu", pg.reshape(-1), ref),
                    R.check(f"keras {kind} cpu", pc.reshape(-1), ref))
        assert not torch.equal(pg.reshape(-1), w)
    print(f"keras {kind}: worst err/(U*mag) {worst:.2f}; c {R.C_OF[kind]['w']}")
