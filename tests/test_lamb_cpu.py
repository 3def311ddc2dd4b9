"""LAMB without a GPU: the PyTorch fallback of mivod.ops.kernels.lamb_step and
mivod.optim.FusedLAMB against the float64 reference and the counted bounds of
tests/lamb_reference.py (tests/test_lamb_gpu.py runs the HIP kernels through the same cases).
Each test prints its worst err / (2^-24 * mag) next to the counted c."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import lamb_reference as R
from mivod.ops import kernels as K
from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)

CPU = torch.device("cpu")
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


def run_lamb_ranks(device_type, timeout=120, extra_env=None):
    """2 ranks of ``lamb_workers.dist_lamb``, in the shape of
    tests/test_syncbn_cpu.run_syncbn_ranks: one process per rank writing to its own temporary
    file, one deadline for both.  At the first non-zero exit or at the deadline every rank
    still running dumps its stacks and is stopped; nothing is retried."""
    n, port = 2, free_port()
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "lamb_workers.py"),
                                       "dist_lamb", device_type], env=env, stdout=f,
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
        head = (f"dist_lamb x{n}: ranks still running after {timeout} s" if timed_out else
                f"dist_lamb x{n}: failed")
        raise AssertionError(describe_ranks(head, procs, outs, stopped, first_fail))
    return outs


@pytest.mark.multirank
def test_distributed_fused_lamb_gloo_ranks():
    """DistributedOptimizer(FusedLAMB) on 2 gloo CPU ranks with the fp16 wire (the fallback
    step): the scenario of tests/lamb_workers.dist_lamb."""
    for o in run_lamb_ranks("cpu"):
        print(o)


@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("mdt", R.MODELS)
@pytest.mark.parametrize("step", [1, 7])
def test_lamb_dtype_grid(gdt, mdt, step):
    total, layout = R.grid_layout()
    worst, ref, _ = R.run_lamb(total, gdt, mdt, CPU, layout, hp=dict(R.HP_LAMB, step=step),
                               zero_grad=R.LAMB_ZERO_GRAD)
    assert [t == 1.0 for t in ref["trust"]] == [True, False, False, False, True, True, False]
    print(f"lamb {gdt}/{mdt} step {step}: worst err/(U*mag) {R.fmt(worst)}; c {R.C_OF}")


@pytest.mark.parametrize("gdt", [f16, bf16])
@pytest.mark.parametrize("step", [1, 7])
def test_lamb_sizes(gdt, step):
    """every size around a lane (8), a step (2048) and a chunk (4096)"""
    tot = {}
    for n in R.SIZES:
        total, layout = R.pair_layout(n)
        worst, _, _ = R.run_lamb(total, gdt, bf16, CPU, layout, hp=dict(R.HP_LAMB, step=step),
                                 seed=n)
        tot = {o: max(tot.get(o, 0.0), x) for o, x in worst.items()}
    print(f"lamb sizes {gdt}/bf16 step {step}: worst err/(U*mag) {R.fmt(tot)}; c {R.C_OF}")


@pytest.mark.parametrize("case", sorted(R.LAMB_FLAG_CASES))
def test_lamb_flags(case):
    worst, sens = R.run_lamb_flag(case, CPU)
    print(f"lamb {case}: worst {R.fmt(worst)}; the variant moves w by {sens} bounds")


def test_lamb_skip_leaves_everything_untouched():
    R.run_lamb_skip(CPU)


def test_lamb_table_must_fit_the_buffers():
    total, layout = R.grid_layout()
    t = R.lamb_inputs(total, f32, None, CPU, layout)
    short = {k: (x[:total - 200] if torch.is_tensor(x) else x) for k, x in t.items()}
    with pytest.raises(ValueError, match="chunk table covers"):
        R.call_lamb(short, R.HP_LAMB, layout, CPU)


# ---- the optimizer ------------------------------------------------------------------------
def _module(dtype, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(20, 33), torch.nn.LayerNorm(33),
                            torch.nn.Linear(33, 5))
    return m.to(dtype)


def _set_grads(model, gen):
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)


@pytest.mark.parametrize("dtype", [bf16, f32])
@pytest.mark.parametrize("exclude_1d", [True, False])
def test_fused_lamb_three_steps_against_fp64(dtype, exclude_1d):
    """Standalone step(): every step's master weights and moments against lamb_ref on the
    state stored before that step; the parameters are the RNE rounding of the master."""
    from mivod.optim import FusedLAMB
    model = _module(dtype)
    opt = FusedLAMB(model.parameters(), lr=0.02, weight_decay=0.05, exclude_1d=exclude_1d)
    (a,) = opt._mv_build()
    sizes = [p.numel() for p in a.params]
    flags = [1 if (exclude_1d and p.dim() <= 1) else 0 for p in a.params]
    assert {p.dim() for p in a.params} == {1, 2} and (sum(flags) == 4) == exclude_1d
    layout = (sizes, a.offsets, flags)
    gen = torch.Generator().manual_seed(1)
    for step in (1, 2, 3):
        _set_grads(model, gen)
        before = {"w": a.master.clone(), "m": a.state["exp_avg"].clone(),
                  "v": a.state["exp_avg_sq"].clone()}
        opt.step()
        assert a.step == step
        grp = opt.param_groups[0]
        ref = R.lamb_ref(a.grad, before["w"], before["m"], before["v"], *layout, lr=grp["lr"],
                         beta1=grp["betas"][0], beta2=grp["betas"][1], eps=grp["eps"],
                         weight_decay=grp["weight_decay"], step=step)
        assert any(t != 1.0 for t in ref["trust"])
        worst = {"w": R.check(f"step {step} w", a.master, ref["w"]),
                 "m": R.check(f"step {step} m", a.state["exp_avg"], ref["m"]),
                 "v": R.check(f"step {step} v", a.state["exp_avg_sq"], ref["v"])}
        for i, p in enumerate(a.params):
            assert torch.equal(p.detach(), a.slot(a.master, i).to(dtype)), "model copy"
        print(f"FusedLAMB {dtype} exclude_1d={exclude_1d} step {step}: worst err/(U*mag) "
              f"{R.fmt(worst)}; c {R.C_OF}")
    assert set(opt.state[a.params[0]]) >= {"exp_avg", "exp_avg_sq", "step"}


@pytest.mark.parametrize("dtype", [bf16, f32])
def test_fused_lamb_state_dict_round_trip_continues_bitwise(dtype):
    from mivod.optim import FusedLAMB
    kw = dict(lr=0.02, weight_decay=0.05)
    model = _module(dtype)
    opt = FusedLAMB(model.parameters(), **kw)
    gen = torch.Generator().manual_seed(2)
    for _ in range(2):
        _set_grads(model, gen)
        opt.step()
    sd = opt.state_dict()
    model2 = _module(dtype, seed=9)
    model2.load_state_dict(model.state_dict())
    opt2 = FusedLAMB(model2.parameters(), **kw)
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
    for n in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(a.state[n], b.state[n]), n
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)


def test_fused_lamb_is_exported_and_keeps_betas():
    import mivod.optim
    from mivod.optim import FusedLAMB, FusedOptimizer
    assert "FusedLAMB" in mivod.optim.__all__ and issubclass(FusedLAMB, FusedOptimizer)
    opt = FusedLAMB([torch.nn.Parameter(torch.zeros(3))])
    d = opt.defaults
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"], d["exclude_1d"]) == \
        (1e-3, (0.9, 0.999), 1e-6, 0.01, True)
    assert FusedLAMB._state_names == ["exp_avg", "exp_avg_sq"]


def test_lamb_binding_rejects_cpu_operands_by_name():
    """mivod._mvk._lamb runs mv_checks.h's operand checks before any launch: a CPU tensor is
    refused as "lamb_step: <first operand> must ..."."""
    if not K.available():
        pytest.skip("mivod._mvk is not built")
    lb = K.native()._lamb
    assert {n for n in dir(lb) if not n.startswith("_")} == {"lamb_step"}
    x = torch.zeros(64)
    tb = K.make_chunk_table([64], CPU)
    with pytest.raises(RuntimeError, match="lamb_step: grad must"):
        lb.lamb_step(x, x.clone(), x.clone(), x.clone(), None, tb.begin, tb.len, tb.seg,
                     tb.seg_c0, tb.seg_nc, torch.zeros(1, dtype=torch.int32), torch.zeros(2),
                     torch.zeros(2), 1e-3, 0.9, 0.999, 1e-6, 0.01, 1.0, 1, None, None)
