"""Adam with amsgrad, Adamax and NAdam without a GPU: the PyTorch fallbacks of
mivod.ops.kernels.adam_amsgrad_step / adamax_step / nadam_step, mivod.optim.FusedAdam(amsgrad=) /
FusedAdamax / FusedNAdam, the Keras front end and a 2-rank gloo DistributedOptimizer, against the
float64 references and the counted bounds of tests/adamfam_reference.py (tests/test_adamfam_gpu.py
runs the HIP kernels through the same cases).  Each test prints its worst err / (2^-24 * mag)
next to the counted c."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import adamfam_reference as R
from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)

CPU = torch.device("cpu")
f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64


def run_adamfam_ranks(scenario, n, device_type, timeout=120, extra_env=None):
    """``n`` ranks of ``adamfam_workers.<scenario>``, in the shape of
    tests/test_adaptive_cpu.run_adaptive_ranks: one process per rank writing to its own
    temporary file, one deadline for all.  At the first non-zero exit or at the deadline every
    rank still running dumps its stacks and is stopped; nothing is retried."""
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "adamfam_workers.py"),
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
    assert (err <= 1e-10 * mag).all(), f"{name}: |ref - torch| up to {float(err.max()):.3g}"


TORCH_CASES = {
    "adam_amsgrad": (torch.optim.Adam, dict(lr=0.01, betas=(0.9, 0.99), eps=1e-6,
                                            weight_decay=0.1, amsgrad=True)),
    "adamw_amsgrad": (torch.optim.AdamW, dict(lr=0.01, betas=(0.9, 0.99), eps=1e-6,
                                              weight_decay=0.1, amsgrad=True)),
    "adamax": (torch.optim.Adamax, dict(lr=0.01, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1)),
    "nadam": (torch.optim.NAdam, dict(lr=0.01, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1,
                                      momentum_decay=4e-3)),
    "nadam_decoupled": (torch.optim.NAdam, dict(lr=0.01, betas=(0.9, 0.99), eps=1e-6,
                                                weight_decay=0.1, momentum_decay=0.02,
                                                decoupled_weight_decay=True)),
}


@pytest.mark.parametrize("case", list(TORCH_CASES))
def test_reference_is_torch_optim_in_float64(case):
    """five steps from a zero state: w, every state buffer and NAdam's mu_product to 1e-10
    relative (the two differ only in the order of operations in double).  torch keeps its
    scalar state (mu_product) in the default dtype, so that is float64 here too."""
    default = torch.get_default_dtype()
    torch.set_default_dtype(f64)
    try:
        _reference_against_torch(case)
    finally:
        torch.set_default_dtype(default)


def _reference_against_torch(case):
    cls, kw = TORCH_CASES[case]
    gen = torch.Generator().manual_seed(0)
    n = 257
    p = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=f64))
    opt = cls([p], foreach=False, **kw)
    w = p.detach().clone()
    z = torch.zeros(n, dtype=f64)
    st = {"m": z, "v": z, "vmax": z, "u": z}
    hp = dict(lr=kw["lr"], beta1=kw["betas"][0], beta2=kw["betas"][1], eps=kw["eps"],
              weight_decay=kw["weight_decay"])
    for step in range(1, 6):
        g = torch.randn(n, generator=gen, dtype=f64)
        p.grad = g.clone()
        opt.step()
        ts = opt.state[p]
        if case.endswith("amsgrad"):
            ref = R.adam_amsgrad_ref(g, w, st["m"], st["v"], st["vmax"], step=step,
                                     adamw=cls is torch.optim.AdamW, design=False, **hp)
            names = {"m": "exp_avg", "v": "exp_avg_sq", "vmax": "max_exp_avg_sq"}
        elif case == "adamax":
            ref = R.adamax_ref(g, w, st["m"], st["u"], step=step, design=False, **hp)
            names = {"m": "exp_avg", "u": "exp_inf"}
        else:
            ref = R.nadam_ref(g, w, st["m"], st["v"], step=step,
                              momentum_decay=kw["momentum_decay"],
                              decoupled=kw.get("decoupled_weight_decay", False), design=False,
                              **hp)
            names = {"m": "exp_avg", "v": "exp_avg_sq"}
            assert abs(ref["mu_product"] - float(ts["mu_product"])) <= 1e-10 * ref["mu_product"]
        _close(f"{case} step {step} w", ref["w"].ref, p.detach(), ref["w"].mag)
        for short, name in names.items():
            _close(f"{case} step {step} {name}", ref[short].ref, ts[name], ref[short].mag)
            st[short] = ref[short].ref
        w = ref["w"].ref
        assert float(ts["step"]) == step


# ---- the fallbacks against the references --------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
def test_dtype_grid(kind, gdt, mdt):
    worst, _, _ = R.run_step(kind, R.N_GRID, gdt, mdt, CPU)
    print(f"{kind} {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("gdt", [f16, bf16])
def test_sizes(kind, gdt):
    """every size around a lane (8), a step (2048) and a chunk (4096)"""
    tot = {}
    for n in R.SIZES:
        worst, _, _ = R.run_step(kind, n, gdt, bf16, CPU, seed=n)
        tot = {o: max(tot.get(o, 0.0), x) for o, x in worst.items()}
    print(f"{kind} sizes {gdt}/bf16: worst err/(U*mag) {R.fmt(tot)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("gdt,mdt", [(f16, bf16), (bf16, f32), (f32, None), (f32, f16)])
def test_unaligned(kind, gdt, mdt):
    worst = R.run_unaligned(kind, gdt, mdt, CPU)
    print(f"{kind} unaligned {gdt}/{mdt}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")


@pytest.mark.parametrize("adamw,keras_eps,step", [(False, False, 1), (True, False, 7),
                                                  (False, True, 7), (True, True, 1)])
def test_amsgrad_flags_and_sensitivity(adamw, keras_eps, step):
    worst, sens = R.run_amsgrad_flags(adamw, keras_eps, step, CPU)
    print(f"amsgrad adamw={adamw} keras_eps={keras_eps} step={step}: worst {R.fmt(worst)}; "
          f"moved by {R.fmt(sens)} bounds")


@pytest.mark.parametrize("keras_eps", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
def test_adamax_flags_and_sensitivity(keras_eps, weight_decay):
    worst, sens = R.run_adamax_flags(keras_eps, weight_decay, CPU)
    print(f"adamax keras_eps={keras_eps} wd={weight_decay}: worst {R.fmt(worst)}; moved by "
          f"{R.fmt(sens)} bounds")


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("momentum_decay", [0.0, 0.5])
def test_nadam_flags_and_sensitivity(decoupled, momentum_decay):
    worst, sens = R.run_nadam_flags(decoupled, momentum_decay, CPU)
    print(f"nadam decoupled={decoupled} momentum_decay={momentum_decay}: worst {R.fmt(worst)}; "
          f"moved by {R.fmt(sens)} bounds")


def test_adamax_zero_divisor_takes_no_update():
    worst = R.run_adamax_zero_divisor(CPU)
    print(f"adamax zero divisor: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF['adamax']}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_skip_leaves_everything_untouched(kind):
    R.run_skip(kind, CPU)


@pytest.mark.parametrize("kind", R.KINDS)
def test_clipped_step_is_the_step_of_the_product(kind):
    R.run_clip(kind, CPU)


def test_bindings_live_in_a_submodule_and_check_their_first_operand():
    """mivod._mvk._adamfam holds the three bindings (the top-level surface is a snapshot and does
    not change); on CPU tensors each raises "<binding>: grad must ..." before anything else"""
    mvk = pytest.importorskip("mivod._mvk")
    assert {"adam_amsgrad_step", "adamax_step", "nadam_step"} <= set(dir(mvk._adamfam))
    assert not {"adam_amsgrad_step", "adamax_step", "nadam_step", "adamfam"} & set(dir(mvk))
    g, w = torch.zeros(64, dtype=bf16), torch.zeros(64)
    calls = {
        "adam_amsgrad_step": lambda: mvk._adamfam.adam_amsgrad_step(
            g, w, w.clone(), w.clone(), w.clone(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1,
            False, False, None, None, None),
        "adamax_step": lambda: mvk._adamfam.adamax_step(
            g, w, w.clone(), w.clone(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, False, None,
            None, None),
        "nadam_step": lambda: mvk._adamfam.nadam_step(
            g, w, w.clone(), w.clone(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.5, 0.5, 0.5,
            False, None, None, None)}
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=f"{name}: grad must"):
            call()


# ---- the optimizers ------------------------------------------------------------------------------
def _module(dtype, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(20, 33), torch.nn.LayerNorm(33),
                            torch.nn.Linear(33, 5))
    return m.to(dtype)


def _set_grads(model, gen):
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)


CLASSES = ["adam_amsgrad", "adamw_amsgrad", "adamax", "adamax_keras", "nadam", "nadam_decoupled"]
NAMES = {"exp_avg": "m", "exp_avg_sq": "v", "max_exp_avg_sq": "vmax", "exp_inf": "u"}
BETAS = (0.9, 0.99)


def _make(cls, params, **over):
    from mivod.optim import FusedAdam, FusedAdamax, FusedAdamW, FusedNAdam
    kw = dict(lr=0.02, betas=BETAS, eps=1e-6, weight_decay=0.05)
    if cls == "adam_amsgrad":
        return FusedAdam(params, amsgrad=True, **dict(kw, **over))
    if cls == "adamw_amsgrad":
        return FusedAdamW(params, amsgrad=True, **dict(kw, **over))
    if cls.startswith("adamax"):
        return FusedAdamax(params, keras_eps=cls == "adamax_keras", **dict(kw, **over))
    return FusedNAdam(params, momentum_decay=0.01, decoupled_weight_decay=cls == "nadam_decoupled",
                      **dict(kw, **over))


def _torch_twin(cls, params):
    kw = dict(lr=0.02, betas=BETAS, eps=1e-6, weight_decay=0.05, foreach=False)
    if cls == "adam_amsgrad":
        return torch.optim.Adam(params, amsgrad=True, **kw)
    if cls == "adamw_amsgrad":
        return torch.optim.AdamW(params, amsgrad=True, **kw)
    if cls == "adamax":
        return torch.optim.Adamax(params, **kw)
    return torch.optim.NAdam(params, momentum_decay=0.01,
                             decoupled_weight_decay=cls == "nadam_decoupled", **kw)


def _snapshot(a):
    return dict({"w": a.master.clone()}, **{n: t.clone() for n, t in a.state.items()})


def fused_ref(opt, a, before, gscale=1.0, grad=None):
    """the fp64 reference of the step ``a.step`` of a Fused* optimizer on the state stored
    before it"""
    grp = a.group
    grad = a.grad if grad is None else grad
    hp = dict(lr=grp["lr"], beta1=grp["betas"][0], beta2=grp["betas"][1], eps=grp["eps"],
              weight_decay=grp["weight_decay"], gscale=gscale, step=a.step)
    kind = type(opt).__name__
    if kind in ("FusedAdam", "FusedAdamW"):
        return "amsgrad", R.adam_amsgrad_ref(
            grad, before["w"], before["exp_avg"], before["exp_avg_sq"], before["max_exp_avg_sq"],
            adamw=grp["adamw"], keras_eps=grp["keras_eps"], design=False, **hp)
    if kind == "FusedAdamax":
        return "adamax", R.adamax_ref(grad, before["w"], before["exp_avg"], before["exp_inf"],
                                      keras_eps=grp["keras_eps"], design=False, **hp)
    return "nadam", R.nadam_ref(grad, before["w"], before["exp_avg"], before["exp_avg_sq"],
                                momentum_decay=grp["momentum_decay"],
                                decoupled=grp["decoupled_weight_decay"], design=False, **hp)


def check_fused_step(opt, a, before, label, gscale=1.0, grad=None):
    kind, ref = fused_ref(opt, a, before, gscale, grad)
    worst = {"w": R.check(f"{label} w", a.master, ref["w"])}
    for n in a.state:
        worst[NAMES[n]] = R.check(f"{label} {n}", a.state[n], ref[NAMES[n]])
    print(f"{label}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF[kind]}")
    return ref


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("dtype", [bf16, f32])
def test_fused_five_steps_against_fp64(cls, dtype):
    """Standalone step(): every step's master weights and state against the reference on the
    state stored before that step; the parameters are the RNE rounding of the master; NAdam's
    mu_product in the state dict is the reference's."""
    model = _module(dtype)
    opt = _make(cls, model.parameters())
    (a,) = opt._mv_build()
    gen = torch.Generator().manual_seed(1)
    for step in range(1, 6):
        _set_grads(model, gen)
        before = _snapshot(a)
        opt.step()
        assert a.step == step
        ref = check_fused_step(opt, a, before, f"{cls} {dtype} step {step}")
        for i, p in enumerate(a.params):
            assert torch.equal(p.detach(), a.slot(a.master, i).to(p.dtype)), "model copy"
        if cls.startswith("nadam"):
            got = float(opt.state_dict()["state"][0]["mu_product"])      # fp32, as torch's
            assert abs(got - ref["mu_product"]) <= 2.0 ** -24 * ref["mu_product"]
    want = {"adam": {"exp_avg", "exp_avg_sq", "max_exp_avg_sq"}, "adamax": {"exp_avg", "exp_inf"},
            "nadam": {"exp_avg", "exp_avg_sq"}}[cls.split("_")[0].replace("adamw", "adam")]
    assert set(a.state) == want and set(opt.state[a.params[0]]) >= want | {"step"}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("dtype", [bf16, f32])
def test_fused_state_dict_round_trip_continues_bitwise(cls, dtype):
    model = _module(dtype)
    opt = _make(cls, model.parameters())
    gen = torch.Generator().manual_seed(2)
    for _ in range(2):
        _set_grads(model, gen)
        opt.step()
    sd = opt.state_dict()
    model2 = _module(dtype, seed=9)
    model2.load_state_dict(model.state_dict())
    opt2 = _make(cls, model2.parameters())
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


@pytest.mark.parametrize("cls", ["adam_amsgrad", "adamw_amsgrad", "adamax", "nadam",
                                 "nadam_decoupled"])
def test_torch_optim_state_dict_loads_and_the_next_step_matches(cls):
    """two steps of the torch.optim class on an fp32 model, its state dict loaded into the fused
    class on a copy of the model: the arena holds torch's state bit for bit (max_exp_avg_sq,
    exp_inf by torch's names), the derived mu_product is torch's, and the third step matches
    the fp64 reference on it (and so torch's own third step)."""
    model = _module(f32)
    topt = _torch_twin(cls, model.parameters())
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        _set_grads(model, gen)
        topt.step()
    model2 = _module(f32, seed=9)
    model2.load_state_dict(model.state_dict())
    opt = _make(cls, model2.parameters())
    opt.load_state_dict(topt.state_dict())
    (a,) = opt._mv_arenas
    assert a.step == 2
    index = {id(q): i for i, q in enumerate(a.params)}
    for p, q in zip(model.parameters(), model2.parameters()):
        for n in a.state:
            assert torch.equal(a.slot(a.state[n], index[id(q)]), topt.state[p][n]), n
    if cls.startswith("nadam"):
        p0 = next(iter(model.parameters()))
        assert abs(float(opt.state_dict()["state"][0]["mu_product"])
                   - float(topt.state[p0]["mu_product"])) <= 1e-7       # torch keeps it in fp32
    _set_grads(model, gen)
    for p, q in zip(model.parameters(), model2.parameters()):
        q.grad = p.grad.clone()
    before = _snapshot(a)
    opt.step()
    topt.step()
    check_fused_step(opt, a, before, f"{cls} after torch's state")
    for p, q in zip(model.parameters(), model2.parameters()):
        torch.testing.assert_close(q, p, rtol=1e-5, atol=1e-6)


def test_exports_defaults_and_state_names():
    import mivod.optim
    from mivod.optim import FusedAdam, FusedAdamax, FusedAdamW, FusedNAdam, FusedOptimizer
    assert {"FusedAdamax", "FusedNAdam"} <= set(mivod.optim.__all__)
    assert issubclass(FusedAdamax, FusedOptimizer) and issubclass(FusedNAdam, FusedOptimizer)
    p = [torch.nn.Parameter(torch.zeros(3))]
    d = FusedAdamax(p).defaults
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"], d["keras_eps"]) == \
        (2e-3, (0.9, 0.999), 1e-8, 0.0, False)
    d = FusedNAdam(p).defaults
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"], d["momentum_decay"],
            d["decoupled_weight_decay"]) == (2e-3, (0.9, 0.999), 1e-8, 0.0, 4e-3, False)
    # amsgrad is per instance; the class attribute stays
    assert FusedAdam(p, amsgrad=True)._state_names == ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"]
    assert FusedAdamW(p, amsgrad=True)._state_names[-1] == "max_exp_avg_sq"
    assert FusedAdam(p)._state_names == ["exp_avg", "exp_avg_sq"]
    assert FusedAdam._state_names == ["exp_avg", "exp_avg_sq"]
    assert FusedAdam(p).defaults["amsgrad"] is False and FusedAdam(p, amsgrad=1).defaults["amsgrad"]
    assert set(FusedAdam(p)._mv_build()[0].state) == {"exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("bad", [dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)),
                                 dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1)])
def test_invalid_hyperparameters_raise(bad):
    from mivod.optim import FusedAdam, FusedAdamax, FusedAdamW, FusedNAdam
    p = [torch.nn.Parameter(torch.zeros(3))]
    for make in (lambda **kw: FusedAdam(p, amsgrad=True, **kw),
                 lambda **kw: FusedAdamW(p, amsgrad=True, **kw),
                 lambda **kw: FusedAdamax(p, **kw), lambda **kw: FusedNAdam(p, **kw)):
        with pytest.raises(ValueError):
            make(**bad)
    with pytest.raises(ValueError, match="momentum_decay"):
        FusedNAdam(p, momentum_decay=-1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamax(p, max_grad_norm=0.0)


def test_nadam_mu_product_follows_the_step_count_and_the_current_beta1():
    """the product is derived from the step and the group's current values: a rollback of the
    step count (a graph capture's) or a changed beta1 re-derives it"""
    from mivod.optim import FusedNAdam
    opt = FusedNAdam([torch.nn.Parameter(torch.zeros(3))], momentum_decay=0.01)
    for step in (5, 2, 9, 0):
        assert abs(opt.mu_product(step, 0.9, 0.01) - R.nadam_schedule(step, 0.9, 0.01)[2]) <= 1e-15
    assert abs(opt.mu_product(4, 0.8, 0.01) - R.nadam_schedule(4, 0.8, 0.01)[2]) <= 1e-15
    model = _module(f32)
    opt = FusedNAdam(model.parameters(), momentum_decay=0.01)
    (a,) = opt._mv_build()
    a.step = 3
    assert opt._mv_dyn_values(a)[1:3] == list(opt._mv_coefficients(a)[:2])
    mu, mu_next, prod = R.nadam_schedule(3, 0.9, 0.01)
    want = [2e-3, (1 - mu) / (1 - prod), mu_next / (1 - prod * mu_next), 1 - 0.999 ** 3]
    assert all(abs(x - y) <= 1e-15 for x, y in zip(opt._mv_dyn_values(a), want))


def test_dyn_values_keeps_its_results_for_the_existing_optimizers():
    from mivod.optim import FusedAdam, FusedSGD
    from mivod.torch.graphs import dyn_values
    for opt in (FusedAdam(_module(f32).parameters(), lr=0.3, betas=(0.8, 0.95)),
                FusedSGD(_module(f32).parameters(), lr=0.3, momentum=0.9)):
        (a,) = opt._mv_build()
        for step in (1, 4):
            a.step = step
            betas = a.group.get("betas")
            want = [0.3, 1.0 if step == 1 else 0.0,
                    1 - betas[0] ** step if betas else 1.0, 1 - betas[1] ** step if betas else 1.0]
            assert dyn_values(a) == want == opt._mv_dyn_values(a)


@pytest.mark.parametrize("cls", ["adam_amsgrad", "adamax", "nadam"])
def test_max_grad_norm_clips_the_step(cls):
    """max_grad_norm reaches the new steps: the step equals, within the bound, the reference
    with gscale = the coefficient the optimizer measured"""
    model = _module(f32)
    opt = _make(cls, model.parameters(), weight_decay=0.0)
    opt.max_grad_norm = 0.5
    (a,) = opt._mv_build()
    _set_grads(model, torch.Generator().manual_seed(6))
    before = _snapshot(a)
    opt.step()
    norm = float(opt.grad_norm())
    assert norm > 5.0
    coef = float(opt._mv_clip_block[0])
    assert abs(coef - 0.5 / (norm + 1e-6)) <= 1e-6 * coef
    check_fused_step(opt, a, before, f"{cls} clipped", gscale=coef)


# ---- Keras ---------------------------------------------------------------------------------------
def test_keras_adam_amsgrad_trains_a_step_and_serialises():
    import mivod.kerasfw as keras
    from mivod.kerasfw import optimizers as O
    from mivod.optim import FusedAdam
    opt = O.Adam(lr=0.01, amsgrad=True)
    cfg = O.serialize(opt)
    assert cfg["config"]["amsgrad"] is True
    twin = O.deserialize(cfg)
    assert type(twin) is O.Adam and twin.amsgrad is True and O.serialize(twin) == cfg
    assert O.Adam().amsgrad is False and O.serialize(O.Adam())["config"]["amsgrad"] is False
    gen = torch.Generator().manual_seed(5)
    w0, g = torch.randn(300, generator=gen), torch.randn(300, generator=gen)
    p = torch.nn.Parameter(w0.clone())
    opt.apply_gradients([(g, p)])
    assert isinstance(opt._impl, FusedAdam) and opt._impl._mv_amsgrad
    assert opt._impl.param_groups[0]["keras_eps"] is True
    z = torch.zeros(300)
    ref = R.adam_amsgrad_ref(g, w0, z, z, z, lr=0.01, eps=1e-7, keras_eps=True, design=False)
    worst = R.check("keras adam amsgrad", p.detach(), ref["w"])
    assert torch.equal(opt._impl.state[p]["max_exp_avg_sq"], opt._impl.state[p]["exp_avg_sq"])
    print(f"keras Adam(amsgrad): worst err/(U*mag) {worst:.2f}; c {R.C_AMS_W}")
    m = keras.Sequential([keras.layers.Dense(2, input_shape=(3,))])
    m.compile(optimizer=O.Adam(amsgrad=True), loss="mse")
    assert m.optimizer.amsgrad is True


def test_keras_adamax_and_nadam_build_fused_optimizers():
    import mivod.kerasfw as keras
    from mivod.kerasfw import optimizers as O
    from mivod.optim import FusedAdamax, FusedNAdam
    p = [torch.nn.Parameter(torch.zeros(5))]
    impl = O.get("adamax")._make_impl(p)
    assert isinstance(impl, FusedAdamax)
    d = impl.defaults
    assert (d["lr"], d["betas"], d["eps"], d["keras_eps"]) == (0.002, (0.9, 0.999), 1e-7, True)
    impl = O.get("nadam")._make_impl(p)
    assert isinstance(impl, FusedNAdam)
    d = impl.defaults
    assert (d["lr"], d["betas"], d["eps"], d["momentum_decay"]) == \
        (0.002, (0.9, 0.999), 1e-7, 0.004)
    assert O.Nadam(schedule_decay=0.1)._make_impl(p).defaults["momentum_decay"] == 0.1
    for name, cls in (("adamax", O.Adamax), ("nadam", O.Nadam)):
        m = keras.Sequential([keras.layers.Dense(2, input_shape=(3,))])
        m.compile(optimizer=name, loss="mse")
        assert isinstance(m.optimizer, cls)
    a = O.Nadam(lr=0.01, beta_1=0.8, beta_2=0.95, epsilon=1e-5, schedule_decay=0.1, decay=0.2)
    cfg = O.serialize(a)
    b = O.deserialize(cfg)
    assert cfg["class_name"] == "Nadam" and type(b) is O.Nadam and O.serialize(b) == cfg
    assert (float(b.lr), b.beta_1, b.beta_2, b.epsilon, b.schedule_decay, b.decay) == \
        (0.01, 0.8, 0.95, 1e-5, 0.1, 0.2)
    a = O.Adamax(lr=0.01, beta_1=0.8, beta_2=0.95, epsilon=1e-5)
    cfg = O.serialize(a)
    b = O.deserialize(cfg)
    assert cfg["class_name"] == "Adamax" and type(b) is O.Adamax and O.serialize(b) == cfg


def keras_step(kind, dev):
    """one apply_gradients of the Keras class on parameters on ``dev``: (results on the CPU,
    the fp64 references with Keras' epsilon placement)"""
    from mivod.kerasfw import optimizers as O
    gen = torch.Generator().manual_seed(5)
    shapes = [(4097,), (33, 20), (7,)]
    w0 = [torch.randn(s, generator=gen) for s in shapes]
    gs = [torch.randn(s, generator=gen) for s in shapes]
    opt = {"amsgrad": lambda: O.Adam(lr=0.01, amsgrad=True), "adamax": lambda: O.Adamax(lr=0.01),
           "nadam": lambda: O.Nadam(lr=0.01)}[kind]()
    ps = [torch.nn.Parameter(w.clone().to(dev)) for w in w0]
    opt.apply_gradients(zip([g.to(dev) for g in gs], ps))
    assert type(opt._impl).__name__ == {"amsgrad": "FusedAdam", "adamax": "FusedAdamax",
                                        "nadam": "FusedNAdam"}[kind]
    refs = []
    for w, g in zip(w0, gs):
        w, g = w.reshape(-1), g.reshape(-1)
        z = torch.zeros_like(w)
        if kind == "amsgrad":
            ref = R.adam_amsgrad_ref(g, w, z, z, z, lr=0.01, eps=1e-7, keras_eps=True,
                                     design=False)
        elif kind == "adamax":
            ref = R.adamax_ref(g, w, z, z, lr=0.01, eps=1e-7, keras_eps=True, design=False)
        else:
            ref = R.nadam_ref(g, w, z, z, lr=0.01, eps=1e-7, momentum_decay=0.004, design=False)
        refs.append(ref["w"])
    return [p.detach().cpu().reshape(-1) for p in ps], refs, w0


@pytest.mark.parametrize("kind", R.KINDS)
def test_keras_step_matches_the_reference_with_keras_epsilon(kind):
    got, refs, w0 = keras_step(kind, CPU)
    worst = max(R.check(f"keras {kind}", p, ref) for p, ref in zip(got, refs))
    assert all(not torch.equal(p, w.reshape(-1)) for p, w in zip(got, w0))
    print(f"keras {kind}: worst err/(U*mag) {worst:.2f}; c {R.C_OF[kind]['w']}")


# ---- DistributedOptimizer ------------------------------------------------------------------------
def test_distributed_adamax_and_amsgrad_two_gloo_ranks():
    """DistributedOptimizer(FusedAdamax) and DistributedOptimizer(FusedAdam(amsgrad=True,
    max_grad_norm=...)) on 2 gloo CPU ranks (tests/adamfam_workers.dist_pair): within the bound
    of the reference on the averaged gradient, parameters and state bitwise equal on both
    ranks; with backward_passes_per_step, accumulation_dtype, gradient_predivide_factor and
    the fp16 wire's guard and grad_scale in the second scenario."""
    for scenario in ("dist_pair", "dist_options"):
        for o in run_adamfam_ranks(scenario, 2, "cpu"):
            print(o[-1500:])
