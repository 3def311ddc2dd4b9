"""RMSprop and Adagrad without a GPU: the PyTorch fallbacks of mivod.ops.kernels.rmsprop_step /
adagrad_step, mivod.optim.FusedRMSprop / FusedAdagrad, the Keras front end and a 2-rank gloo
DistributedOptimizer, against the float64 references and the counted bounds of
tests/adaptive_reference.py (tests/test_adaptive_gpu.py runs the HIP kernels through the same
cases).  Each test prints its worst err / (2^-24 * mag) next to the counted c."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

import adaptive_reference as R
from mivod.ops import kernels as K
from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)

sys.path.insert(0, os.path.join(ROOT, "examples"))

CPU = torch.device("cpu")
f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64


def run_adaptive_ranks(scenario, n, device_type, timeout=120, extra_env=None):
    """``n`` ranks of ``adaptive_workers.<scenario>``, in the shape of
    tests/test_lamb_cpu.run_lamb_ranks: one process per rank writing to its own temporary file,
    one deadline for all.  At the first non-zero exit or at the deadline every rank still
    running dumps its stacks and is stopped; nothing is retried."""
    port = free_port()
    procs, files = [], []
    _release_parent_gpu_cache()
    for r in range(n):
        env = dict(os.environ)
        env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(r),
                    "WORLD_SIZE": str(n), "LOCAL_RANK": str(r), "LOCAL_WORLD_SIZE": str(n),
                    "MIVOD_TRANSPORT": "gloo", "OMP_NUM_THREADS": "1", "PYTHONUNBUFFERED": "1",
                    "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", "")})
        env.pop("HOROVOD_RANK", None)
        env.setdefault("MIVOD_TEST_DUMP_AFTER", str(max(timeout - 15, 5)))
        if extra_env:
            env.update(extra_env)
        f = tempfile.TemporaryFile(mode="w+")
        files.append(f)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "adaptive_workers.py"),
                                       scenario, device_type], env=env, stdout=f,
                                      stderr=subprocess.STDOUT, text=True))
    t0 = time.monotonic()
    first_fail, timed_out = None, False
    while any(p.poll() is None for p in procs):
        now = time.monotonic()
        bad = [(r, p.returncode, now - t0) for r, p in enumerate(procs)
               if p.returncode not in (None, 0)]
        if bad:
            first_fail = bad[0]
            break
        if now - t0 >= timeout:
            timed_out = True
            break
        time.sleep(0.1)
    stopped = [r for r, p in enumerate(procs) if p.poll() is None]
    for r in stopped:
        try:
            procs[r].send_signal(signal.SIGUSR1)      # faulthandler: dump every thread
        except ProcessLookupError:
            pass
    if stopped:
        time.sleep(2.0)
    for r in stopped:
        if procs[r].poll() is None:
            procs[r].kill()
        procs[r].wait()
    outs = []
    for f in files:
        f.seek(0)
        outs.append(f.read())
        f.close()
    if first_fail is None:
        first_fail = next(((r, p.returncode, 0.0) for r, p in enumerate(procs)
                           if p.returncode != 0 and r not in stopped), None)
    if timed_out or first_fail or any(f"OK {r}" not in o for r, o in enumerate(outs)):
        head = (f"{scenario} x{n}: ranks still running after {timeout} s" if timed_out else
                f"{scenario} x{n}: failed")
        raise AssertionError(describe_ranks(head, procs, outs, stopped, first_fail))
    return outs


# ---- the references against torch.optim, both in float64 ---------------------------------------
def _close(name, got, want, mag):
    err = (got - want).abs()
    assert (err <= 1e-12 * mag).all(), f"{name}: |ref - torch| up to {float(err.max()):.3g}"


@pytest.mark.parametrize("hp", [
    dict(), dict(momentum=0.9), dict(centered=True), dict(centered=True, momentum=0.9),
    dict(centered=True, momentum=0.9, weight_decay=0.1), dict(alpha=0.9, eps=1e-3)],
    ids=["plain", "momentum", "centered", "centered_momentum", "weight_decay", "alpha_eps"])
def test_rmsprop_ref_is_torch_rmsprop_in_float64(hp):
    """three steps from a zero state: w and every state buffer to 1e-12 * mag"""
    hp = dict(dict(lr=0.01, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False),
              **hp)
    gen = torch.Generator().manual_seed(0)
    n = 257
    p = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=f64))
    opt = torch.optim.RMSprop([p], foreach=False, **hp)
    w = p.detach().clone()
    sq, ga, buf = torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64)
    for step in range(3):
        g = torch.randn(n, generator=gen, dtype=f64)
        p.grad = g.clone()
        opt.step()
        ref = R.rmsprop_ref(g, w, sq, ga, buf if hp["momentum"] else None, **hp)
        st = opt.state[p]
        _close(f"step {step} w", ref["w"].ref, p.detach(), ref["w"].mag)
        _close(f"step {step} sq", ref["sq"].ref, st["square_avg"], ref["sq"].mag)
        w, sq = ref["w"].ref, ref["sq"].ref
        if hp["centered"]:
            _close(f"step {step} ga", ref["ga"].ref, st["grad_avg"], ref["ga"].mag)
            ga = ref["ga"].ref
        if hp["momentum"]:
            _close(f"step {step} buf", ref["buf"].ref, st["momentum_buffer"], ref["buf"].mag)
            buf = ref["buf"].ref


@pytest.mark.parametrize("hp", [
    dict(), dict(weight_decay=0.1), dict(lr_decay=0.5), dict(initial_accumulator_value=0.3),
    dict(lr_decay=0.1, initial_accumulator_value=0.1, weight_decay=0.05, eps=1e-3)],
    ids=["plain", "weight_decay", "lr_decay", "initial_accumulator", "all"])
def test_adagrad_ref_is_torch_adagrad_in_float64(hp):
    hp = dict(dict(lr=0.05, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0,
                   eps=1e-10), **hp)
    gen = torch.Generator().manual_seed(1)
    n = 257
    p = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=f64))
    opt = torch.optim.Adagrad([p], foreach=False, **hp)
    w = p.detach().clone()
    acc = torch.full((n,), hp["initial_accumulator_value"], dtype=f64)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen, dtype=f64)
        p.grad = g.clone()
        opt.step()
        clr = hp["lr"] / (1 + (step - 1) * hp["lr_decay"])
        ref = R.adagrad_ref(g, w, acc, lr=clr, eps=hp["eps"], weight_decay=hp["weight_decay"])
        _close(f"step {step} w", ref["w"].ref, p.detach(), ref["w"].mag)
        _close(f"step {step} sum", ref["sum"].ref, opt.state[p]["sum"], ref["sum"].mag)
        w, acc = ref["w"].ref, ref["sum"].ref


# ---- the fallbacks against the references --------------------------------------------------------
@pytest.mark.parametrize("kind", ["rmsprop", "adagrad"])
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
def test_dtype_grid(kind, gdt, mdt):
    worst, _, _ = R.run_step(kind, R.N_GRID, gdt, mdt, CPU)
    print(f"{kind} {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", ["rmsprop", "adagrad"])
@pytest.mark.parametrize("gdt", [f16, bf16])
def test_sizes(kind, gdt):
    """every size around a lane (8), a step (2048) and a chunk (4096)"""
    tot = {}
    for n in R.SIZES:
        worst, _, _ = R.run_step(kind, n, gdt, bf16, CPU, seed=n)
        tot = {o: max(tot.get(o, 0.0), x) for o, x in worst.items()}
    print(f"{kind} sizes {gdt}/bf16: worst err/(U*mag) {R.fmt(tot)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("centered,momentum", R.RMSPROP_FLAGS)
def test_rmsprop_flags_and_sensitivity(centered, momentum):
    worst, sens = R.run_rmsprop_flags(centered, momentum, CPU)
    print(f"rmsprop centered={centered} momentum={momentum}: worst {R.fmt(worst)}; moved by "
          f"{R.fmt(sens)} bounds")


@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adagrad_flags_and_sensitivity(weight_decay):
    worst, sens = R.run_adagrad_flags(weight_decay, CPU)
    print(f"adagrad wd={weight_decay}: worst {R.fmt(worst)}; moved by {R.fmt(sens)} bounds")


def test_rmsprop_clamps_a_negative_variance():
    worst = R.run_clamp(CPU)
    print(f"rmsprop clamp: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF['rmsprop']}")


@pytest.mark.parametrize("kind", ["rmsprop", "adagrad"])
def test_skip_leaves_everything_untouched(kind):
    R.run_skip(kind, CPU)


def test_rmsprop_step_needs_the_buffers_its_flags_use():
    t = R.adaptive_inputs("rmsprop", 64, f32, None, CPU, centered=False, momentum=False)
    with pytest.raises(ValueError, match="grad_avg"):
        R.call_step("rmsprop", t, dict(R.HP["rmsprop"], momentum=0.0))
    with pytest.raises(ValueError, match="momentum buffer"):
        R.call_step("rmsprop", t, dict(R.HP["rmsprop"], centered=False))


# ---- the optimizers ------------------------------------------------------------------------------
def _module(dtype, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(20, 33), torch.nn.LayerNorm(33),
                            torch.nn.Linear(33, 5))
    return m.to(dtype)


def _set_grads(model, gen):
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)


RMS_KW = dict(lr=0.02, alpha=0.9, eps=1e-6, weight_decay=0.05, momentum=0.8, centered=True)
ADA_KW = dict(lr=0.02, lr_decay=0.1, weight_decay=0.05, initial_accumulator_value=0.1, eps=1e-6)
RMS_NAMES = {"square_avg": "sq", "grad_avg": "ga", "momentum_buffer": "buf"}


def _make(kind, params, **over):
    from mivod.optim import FusedAdagrad, FusedRMSprop
    if kind == "rmsprop":
        return FusedRMSprop(params, **dict(RMS_KW, **over))
    return FusedAdagrad(params, **dict(ADA_KW, **over))


def _snapshot(a):
    return dict({"w": a.master.clone()}, **{n: t.clone() for n, t in a.state.items()})


def _check_fused_step(kind, opt, a, before, label):
    """the arena after a step against the fp64 reference on the state stored before it"""
    grp = opt.param_groups[0]
    if kind == "rmsprop":
        ref = R.rmsprop_ref(a.grad, before["w"], before["square_avg"], before.get("grad_avg"),
                            before.get("momentum_buffer"), lr=grp["lr"], alpha=grp["alpha"],
                            eps=grp["eps"], weight_decay=grp["weight_decay"],
                            momentum=grp["momentum"], centered=grp["centered"])
        names = {n: RMS_NAMES[n] for n in a.state}
    else:
        clr = grp["lr"] / (1 + (a.step - 1) * grp["lr_decay"])
        ref = R.adagrad_ref(a.grad, before["w"], before["sum"], lr=clr, eps=grp["eps"],
                            weight_decay=grp["weight_decay"])
        names = {"sum": "sum"}
    worst = {"w": R.check(f"{label} w", a.master, ref["w"])}
    for n, short in names.items():
        worst[short] = R.check(f"{label} {n}", a.state[n], ref[short])
    for i, p in enumerate(a.params):
        assert torch.equal(p.detach(), a.slot(a.master, i).to(p.dtype)), "model copy"
    print(f"{label}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", ["rmsprop", "adagrad"])
@pytest.mark.parametrize("dtype", [bf16, f32])
def test_fused_three_steps_against_fp64(kind, dtype):
    """Standalone step(): every step's master weights and state against the reference on the
    state stored before that step; the parameters are the RNE rounding of the master."""
    model = _module(dtype)
    opt = _make(kind, model.parameters())
    (a,) = opt._mv_build()
    if kind == "adagrad":
        assert (a.state["sum"] == ADA_KW["initial_accumulator_value"]).all()
    gen = torch.Generator().manual_seed(1)
    for step in (1, 2, 3):
        _set_grads(model, gen)
        before = _snapshot(a)
        opt.step()
        assert a.step == step
        _check_fused_step(kind, opt, a, before, f"Fused {kind} {dtype} step {step}")
    want = {"rmsprop": {"square_avg", "grad_avg", "momentum_buffer", "step"},
            "adagrad": {"sum", "step"}}[kind]
    assert set(opt.state[a.params[0]]) >= want


def test_fused_rmsprop_allocates_only_the_state_it_uses():
    from mivod.optim import FusedRMSprop
    for kw, want in ((dict(), {"square_avg"}),
                     (dict(momentum=0.5), {"square_avg", "momentum_buffer"}),
                     (dict(centered=True), {"square_avg", "grad_avg"}),
                     (dict(momentum=0.5, centered=True),
                      {"square_avg", "momentum_buffer", "grad_avg"})):
        model = _module(f32)
        opt = FusedRMSprop(model.parameters(), **kw)
        (a,) = opt._mv_build()
        assert set(a.state) == want, kw
        _set_grads(model, torch.Generator().manual_seed(3))
        before = _snapshot(a)
        opt.step()
        _check_fused_step("rmsprop", opt, a, before, f"FusedRMSprop {kw}")
        assert set(opt.state[a.params[0]]) - {"step"} == want
    # the class attribute stays empty: the state names are per instance
    assert FusedRMSprop._state_names == []


@pytest.mark.parametrize("kind", ["rmsprop", "adagrad"])
@pytest.mark.parametrize("dtype", [bf16, f32])
def test_fused_state_dict_round_trip_continues_bitwise(kind, dtype):
    model = _module(dtype)
    opt = _make(kind, model.parameters())
    gen = torch.Generator().manual_seed(2)
    for _ in range(2):
        _set_grads(model, gen)
        opt.step()
    sd = opt.state_dict()
    model2 = _module(dtype, seed=9)
    model2.load_state_dict(model.state_dict())
    opt2 = _make(kind, model2.parameters())
    opt2.load_state_dict(sd)
    for _ in range(2):
        _set_grads(model, gen)
        for p, q in zip(model.parameters(), model2.parameters()):
            q.grad = p.grad.clone()
        opt.step()
        opt2.step()
    (a,), (b,) = opt._mv_arenas, opt2._mv_arenas
    assert a.step == b.step == 4
    assert torch.equal(a.master, b.master) and torch.equal(a.model, b.model)
    for n in a.state:
        assert torch.equal(a.state[n], b.state[n]), n
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("kind", ["rmsprop", "adagrad"])
def test_torch_optim_state_dict_loads_and_the_next_step_matches(kind):
    """two steps of torch.optim.RMSprop / Adagrad on an fp32 model, its state dict loaded into
    the fused class on a copy of the model: the arena holds torch's state bit for bit, and the
    third step matches the fp64 reference on it (and so torch's own third step)."""
    model = _module(f32)
    tkw = dict(RMS_KW if kind == "rmsprop" else ADA_KW)
    topt = (torch.optim.RMSprop if kind == "rmsprop" else torch.optim.Adagrad)(
        model.parameters(), foreach=False, **tkw)
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        _set_grads(model, gen)
        topt.step()
    model2 = _module(f32, seed=9)
    model2.load_state_dict(model.state_dict())
    opt = _make(kind, model2.parameters())
    opt.load_state_dict(topt.state_dict())
    (a,) = opt._mv_arenas
    assert a.step == 2
    index = {id(q): i for i, q in enumerate(a.params)}
    for p, q in zip(model.parameters(), model2.parameters()):
        for n in a.state:
            assert torch.equal(a.slot(a.state[n], index[id(q)]), topt.state[p][n]), n
    _set_grads(model, gen)
    for p, q in zip(model.parameters(), model2.parameters()):
        q.grad = p.grad.clone()
    before = _snapshot(a)
    opt.step()
    topt.step()
    _check_fused_step(kind, opt, a, before, f"Fused {kind} after torch's state")
    for p, q in zip(model.parameters(), model2.parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-6)


def test_exports_and_defaults():
    import mivod.optim
    from mivod.optim import FusedAdagrad, FusedOptimizer, FusedRMSprop
    assert {"FusedRMSprop", "FusedAdagrad"} <= set(mivod.optim.__all__)
    assert issubclass(FusedRMSprop, FusedOptimizer) and issubclass(FusedAdagrad, FusedOptimizer)
    d = FusedRMSprop([torch.nn.Parameter(torch.zeros(3))]).defaults
    assert (d["lr"], d["alpha"], d["eps"], d["weight_decay"], d["momentum"], d["centered"]) == \
        (1e-2, 0.99, 1e-8, 0, 0, False)
    d = FusedAdagrad([torch.nn.Parameter(torch.zeros(3))]).defaults
    assert (d["lr"], d["lr_decay"], d["weight_decay"], d["initial_accumulator_value"],
            d["eps"]) == (1e-2, 0, 0, 0, 1e-10)


# ---- Keras ---------------------------------------------------------------------------------------
def test_keras_rmsprop_and_adagrad_build_fused_optimizers():
    import mivod.kerasfw as keras
    from mivod.kerasfw import optimizers as O
    from mivod.optim import FusedAdagrad, FusedRMSprop
    p = [torch.nn.Parameter(torch.zeros(5))]
    rms = O.get("rmsprop")
    impl = rms._make_impl(p)
    assert isinstance(impl, FusedRMSprop)
    d = impl.defaults
    assert (d["lr"], d["alpha"], d["eps"], d["momentum"], d["centered"]) == \
        (0.001, 0.9, 1e-7, 0.0, False)
    impl = O.RMSprop(momentum=0.5, centered=True)._make_impl(p)
    assert (impl.defaults["momentum"], impl.defaults["centered"]) == (0.5, True)
    ada = O.get("adagrad")
    impl = ada._make_impl(p)
    assert isinstance(impl, FusedAdagrad)
    d = impl.defaults
    assert (d["lr"], d["initial_accumulator_value"], d["eps"], d["lr_decay"]) == \
        (0.001, 0.1, 1e-7, 0)
    m = keras.Sequential([keras.layers.Dense(2, input_shape=(3,))])
    m.compile(optimizer="adagrad", loss="mse")
    assert isinstance(m.optimizer, O.Adagrad)


def test_keras_serialize_round_trips_the_new_hyperparameters():
    from mivod.kerasfw import optimizers as O
    a = O.RMSprop(lr=0.01, rho=0.8, epsilon=1e-5, decay=0.1, momentum=0.7, centered=True)
    cfg = O.serialize(a)
    assert cfg["class_name"] == "RMSprop"
    assert (cfg["config"]["momentum"], cfg["config"]["centered"]) == (0.7, True)
    b = O.deserialize(cfg)
    assert type(b) is O.RMSprop and O.serialize(b) == cfg
    assert (float(b.lr), b.rho, b.epsilon, b.decay, float(b.momentum), b.centered) == \
        (0.01, 0.8, 1e-5, 0.1, 0.7, True)
    a = O.Adagrad(lr=0.02, initial_accumulator_value=0.3, epsilon=1e-5, decay=0.2)
    cfg = O.serialize(a)
    assert cfg["class_name"] == "Adagrad"
    b = O.deserialize(cfg)
    assert type(b) is O.Adagrad and O.serialize(b) == cfg
    assert (float(b.lr), b.initial_accumulator_value, b.epsilon, b.decay) == (0.02, 0.3, 1e-5, 0.2)


def test_keras_default_compile_trains_the_mnist_convnet_on_the_fused_path():
    """compile() without an optimizer is RMSprop: three batches lower the loss, through
    FusedRMSprop, and the optimizer's variables are its square_avg slots."""
    import mivod.keras as hvd
    import mivod.kerasfw as keras
    from keras_mnist_convnet import build_convnet
    from mivod.optim import FusedRMSprop
    hvd.init()
    np.random.seed(0)
    torch.manual_seed(0)
    (x, y), _ = keras.datasets.mnist.load_data()
    x = x[:384].reshape(-1, 28, 28, 1).astype("float32") / 255
    y = keras.utils.to_categorical(y[:384], 10)
    m = build_convnet((28, 28, 1), 10)
    m.compile(loss="categorical_crossentropy")
    assert type(m.optimizer).__name__ == "RMSprop"
    loss0 = float(np.atleast_1d(m.evaluate(x, y, batch_size=128, verbose=0))[0])
    m.fit(x, y, batch_size=128, epochs=1, verbose=0)
    loss1 = float(np.atleast_1d(m.evaluate(x, y, batch_size=128, verbose=0))[0])
    assert m.optimizer.iterations == 3
    assert isinstance(m.optimizer._impl, FusedRMSprop)
    assert loss1 < loss0, (loss0, loss1)
    var = m.optimizer.variables()
    assert len(var) == len(m.trainable_weights) and all(bool((v >= 0).all()) for v in var)
    assert any(bool((v > 0).any()) for v in var)


# ---- the bindings --------------------------------------------------------------------------------
def test_adaptive_bindings_reject_cpu_operands_by_name():
    """mivod._mvk._adaptive runs mv_checks.h's operand checks before any launch: a CPU tensor
    is refused as "<step>: <first operand> must ..."."""
    if not K.available():
        pytest.skip("mivod._mvk is not built")
    ad = K.native()._adaptive
    assert {n for n in dir(ad) if not n.startswith("_")} == {"rmsprop_step", "adagrad_step"}
    x = torch.zeros(64)
    with pytest.raises(RuntimeError, match="rmsprop_step: grad must"):
        ad.rmsprop_step(x, x.clone(), x.clone(), None, None, None, 1e-2, 0.99, 1e-8, 0.0, 0.0, 1.0,
                        None, None)
    with pytest.raises(RuntimeError, match="adagrad_step: grad must"):
        ad.adagrad_step(x, x.clone(), x.clone(), None, 1e-2, 1e-10, 0.0, 1.0, None, None)


# ---- DistributedOptimizer ------------------------------------------------------------------------
@pytest.mark.multirank
def test_distributed_fused_rmsprop_gloo_ranks():
    """DistributedOptimizer(FusedRMSprop) on 2 gloo CPU ranks (the fallback step): the scenario
    of tests/adaptive_workers.dist_rmsprop."""
    for o in run_adaptive_ranks("dist_rmsprop", 2, "cpu"):
        print(o)
