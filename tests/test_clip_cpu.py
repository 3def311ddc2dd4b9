"""Global gradient-norm clipping without a GPU: the PyTorch fallbacks of grad_sumsq,
clip_finalize and the gclip operand of every fused step (mivod/ops/kernels.py), max_grad_norm of
mivod.optim.Fused* and of DistributedOptimizer on gloo CPU ranks, against the float64
references and the counted bounds of tests/clip_reference.py (tests/test_clip_gpu.py runs the
HIP kernels through the same cases).  Each test prints its worst err / (2^-24 * mag) next to
the counted c."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import clip_reference as R
from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)

CPU = torch.device("cpu")
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


def run_clip_ranks(scenario, device_type, *args, timeout=120, extra_env=None):
    """2 ranks of ``clip_workers.<scenario>``, in the shape of
    tests/test_lamb_cpu.run_lamb_ranks: one process per rank writing to its own temporary
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
        env.pop("MIVOD_GUARD_MODE", None)
        env.setdefault("MIVOD_TEST_DUMP_AFTER", str(max(timeout - 15, 5)))
        if extra_env:
            env.update(extra_env)
        f = tempfile.TemporaryFile(mode="w+")
        files.append(f)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "clip_workers.py"),
                                       scenario, device_type, *args], env=env, stdout=f,
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


# ---- A. grad_sumsq ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES)
def test_grad_sumsq_sizes(dt):
    worst = 0.0
    for n in R.SIZES:
        wa, pa = R.run_sumsq(CPU, n, dt, 0, seed=n)
        wb, pb = R.run_sumsq(CPU, n, dt, 1, seed=n)
        assert torch.equal(pa, pb), f"n={n}: an offset view changes the bits"
        worst = max(worst, wa, wb)
    print(f"grad_sumsq {dt}: worst err/(U*mag) {worst:.2f}; c {R.C_PARTIAL}")


@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("base_off", [0, 1])
def test_grad_sumsq_flag(dt, base_off):
    R.run_sumsq_flag(CPU, dt, base_off)


def test_grad_sumsq_refuses_a_short_partial():
    with pytest.raises(ValueError, match="partial must hold at least 2"):
        R.K.grad_sumsq(torch.zeros(4097), torch.zeros(1))


# ---- B. clip_finalize ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FINALIZE_CASES)
def test_clip_finalize(case):
    worst = [R.run_finalize(CPU, count, case) for count in R.FINALIZE_COUNTS]
    if worst[0] is not None:
        print(f"clip_finalize {case}: worst err/(U*mag) coef {max(w[0] for w in worst):.2f}, "
              f"norm {max(w[1] for w in worst):.2f}; c {R.C_CLIP}")


# ---- C. every step ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.STEP_KINDS)
@pytest.mark.parametrize("n", R.STEP_SIZES)
def test_step_with_gclip_is_the_step_of_the_scaled_gscale(kind, n):
    R.run_step_clip(kind, n, CPU)


# ---- D. the model level -------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.OPTIMIZERS)
@pytest.mark.parametrize("mdt", [f32, bf16])
def test_fused_optimizer_with_max_grad_norm(name, mdt):
    worst, coefs = R.run_model(CPU, mdt, name)
    print(f"{name} {mdt}: coefficients {[round(c, 4) for c in coefs]}; worst err/(U*mag) "
          f"{R.FR.fmt(worst)}; c = the step's + {R.C_GCLIP}, norm {R.C_NORM}")


# ---- E. arguments -------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan")])
def test_max_grad_norm_must_be_positive_and_finite(bad):
    from mivod.optim import (FusedAdadelta, FusedAdagrad, FusedAdam, FusedAdamW, FusedLAMB,
                             FusedLARS, FusedRMSprop, FusedSGD)
    for cls in (FusedSGD, FusedAdam, FusedAdamW, FusedAdadelta, FusedLARS, FusedLAMB,
                FusedRMSprop, FusedAdagrad):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)
    opt = FusedSGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, max_grad_norm=1.0)
    opt.param_groups[0]["params"][0].grad = torch.ones(3)
    opt.max_grad_norm = bad                      # a plain attribute: checked when it is used
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step()


def test_max_grad_norm_is_no_group_option_and_not_saved():
    from mivod.optim import FusedAdamW
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=2.0)
    assert opt.max_grad_norm == 2.0
    assert "max_grad_norm" not in opt.param_groups[0] and "max_grad_norm" not in opt.defaults
    assert "max_grad_norm" not in str(opt.state_dict())
    with pytest.raises(RuntimeError, match="grad_norm"):
        opt.grad_norm()


@pytest.mark.multirank
def test_bucket_guard_mode_and_disagreeing_ranks_raise():
    """MIVOD_GUARD_MODE=bucket with max_grad_norm raises at wrap time; ranks that disagree on
    max_grad_norm raise through the plan hash (tests/clip_workers.clip_args)."""
    for o in run_clip_ranks("clip_args", "cpu", extra_env={"MIVOD_GUARD_MODE": "bucket"}):
        print(o)


# ---- F. DistributedOptimizer ----------------------------------------------------------------------
@pytest.mark.multirank
@pytest.mark.parametrize("wire", ["fp16", "none"])
def test_distributed_clip_gloo_ranks(wire):
    """DistributedOptimizer(FusedSGD(max_grad_norm)) on 2 gloo CPU ranks (the fallbacks): the
    scenario of tests/clip_workers.dist_clip."""
    for o in run_clip_ranks("dist_clip", "cpu", wire):
        print(o)
