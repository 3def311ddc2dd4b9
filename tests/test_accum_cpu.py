"""Local gradient accumulation in an fp32 arena without a GPU: the PyTorch fallbacks of
accumulate and pack_accumulated (mivod/ops/kernels.py) and DistributedOptimizer(
backward_passes_per_step=k, accumulation_dtype=torch.float32) on the CPU and on gloo CPU ranks,
against the float64 references and the counted bounds of tests/accum_reference.py
(tests/test_accum_gpu.py runs the HIP kernels through the same cases).  Each test prints its
worst err / (2^-24 * mag) next to the counted c, or its worst err / bound."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import accum_reference as R
from mivod.ops import kernels as K
from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)

CPU = torch.device("cpu")
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


def run_accum_ranks(scenario, device_type, *args, timeout=120, extra_env=None):
    """2 ranks of ``accum_workers.<scenario>``, in the shape of
    tests/test_clip_cpu.run_clip_ranks (test_multiprocess.run_ranks starts mp_workers.py
    only): one process per rank writing to its own temporary file, one deadline for both.  At
    the first non-zero exit or at the deadline every rank still running dumps its stacks and
    is stopped; nothing is retried."""
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "accum_workers.py"),
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


# ---- A. the three modes -----------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("wdt", R.DTYPES)
def test_accumulate_and_pack_sizes(gdt, wdt):
    wa, ww = R.run_sizes(CPU, gdt, wdt)
    print(f"{gdt} -> {wdt}, k 4: acc worst err/(U*mag) per addition {wa:.2f} (c = j-1 after j "
          f"passes); wire worst err/bound {ww:.2f} (c 5)")


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("scale", R.SCALES)
def test_accumulate_and_pack_passes_and_scales(k, scale):
    worst = [R.run_window(CPU, [R.N_GRID, R.TAIL], gdt, wdt, k, scale, seed=k)[:2]
             for gdt, wdt in ((bf16, f16), (f16, bf16), (f32, f32))]
    print(f"k {k} scale {scale}: acc worst err/(U*mag) per addition {max(w[0] for w in worst):.2f}"
          f"; wire worst err/bound {max(w[1] for w in worst):.2f} (c {k + 1})")


def test_more_tensors_than_one_table():
    wa, ww = R.run_many(CPU)
    print(f"{len(R.MANY)} tensors: acc {wa:.2f}, wire {ww:.2f}")


@pytest.mark.parametrize("gdt", R.DTYPES)
@pytest.mark.parametrize("wdt", R.DTYPES)
def test_pack_accumulated_flag(gdt, wdt):
    R.run_flag(CPU, gdt, wdt, 0)
    R.run_flag(CPU, gdt, wdt, 1)


# ---- B. evidence that the feature is what passes -----------------------------------------------------
def test_bf16_accumulation_misses_the_bound_the_arena_meets():
    """today's arithmetic through the same harness: bf16 ``+=`` of 16 gradients, then K.pack"""
    old, new = R.run_evidence(CPU, 16)
    print(f"k 16: bf16 accumulation + pack {100 * old:.1f} % of the elements outside the bound, "
          f"fp32 arena {100 * new:.1f} %")
    assert old >= 0.5, "the inputs do not tell bf16 accumulation from fp32"
    assert new == 0.0


# ---- C. arguments -------------------------------------------------------------------------------------
def test_accumulation_dtype_argument():
    import mivod.torch as hvd
    hvd.init()
    for bad in (bf16, f16, torch.float64, "float32"):
        with pytest.raises(ValueError, match="accumulation_dtype"):
            net = R.make_net(CPU)
            hvd.DistributedOptimizer(torch.optim.SGD(net.parameters(), lr=0.1),
                                     backward_passes_per_step=2, accumulation_dtype=bad)
    # one pass per step: accepted, no effect (no accumulator, the plain pack)
    net = R.make_net(CPU)
    opt = hvd.DistributedOptimizer(torch.optim.SGD(net.parameters(), lr=0.1),
                                   accumulation_dtype=f32)
    R.loss_of(net, R.make_batches(CPU, 1)[0]).backward()
    opt.step()
    assert not opt._mvd_accum and not opt._mvd_acc


def test_fallbacks_refuse_a_wrong_accumulator():
    with pytest.raises(ValueError, match="acc must be a contiguous fp32"):
        K.accumulate([torch.zeros(4)], torch.zeros(8, dtype=bf16), [0], True)
    with pytest.raises(ValueError, match="length mismatch"):
        K.pack_accumulated([torch.zeros(4)], torch.zeros(8), torch.zeros(8), [0, 4])


def test_accum_bindings_reject_cpu_operands_by_name():
    if not K.available():
        pytest.skip("mivod._mvk is not built")
    ac = K.native()._accum
    assert {n for n in dir(ac) if not n.startswith("_")} == {"accumulate", "pack_accumulated"}
    x = torch.zeros(64)
    with pytest.raises(RuntimeError, match="accumulate: tensors must"):
        ac.accumulate([x], x.clone(), [0], True)
    with pytest.raises(RuntimeError, match="pack_accumulated: tensors must"):
        ac.pack_accumulated([x], x.clone(), x.clone(), [0], 1.0, None)


# ---- D. the model level -------------------------------------------------------------------------------
def test_model_plain_sgd_and_release():
    print(f"(a, g) plain SGD, bf16 wire: worst err/bound {R.model_plain_sgd(CPU):.2f}")


@pytest.mark.parametrize("kind", ["fused_sgd", "fused_adam"])
def test_model_fused_fp16_wire_guard(kind):
    print(f"(b) {kind}: worst {R.FR.fmt(R.model_fused(CPU, kind))} (grad: err/bound; the rest "
          f"err/(U*mag), c {R.FR.C_SGD_W if kind == 'fused_sgd' else R.FR.C_ADAM_W})")


def test_model_partial_window():
    print(f"(c) synchronize() after 2 of 4: worst err/bound {R.model_partial(CPU):.2f}")


@pytest.mark.parametrize("kind", ["sgd", "fused_sgd"])
@pytest.mark.parametrize("skip_pass", [1, 3])
@pytest.mark.parametrize("bucket_mb", [1e-5, 64])
def test_model_parameter_unused_in_one_pass(kind, skip_pass, bucket_mb):
    worst, nb = R.model_unused(CPU, kind, skip_pass, bucket_mb)
    assert (nb == 6) == (bucket_mb < 1)
    print(f"(d) {kind}, lin2 unused in pass {skip_pass}, {nb} buckets: worst err/bound {worst:.2f}")


def test_model_gradient_aliasing_its_slot():
    print(f"(e) aliased slots: worst err/bound {R.model_aliased(CPU)}")


def test_model_zero_grad_inside_a_window():
    print(f"(f) zero_grad() after 2 of 4: worst err/bound {R.model_zero_grad(CPU):.2f}")


def test_model_overflow_skips_the_step():
    print(f"(h) window after the skipped one: worst err/bound {R.model_overflow(CPU):.2f}")


# ---- E. ranks -----------------------------------------------------------------------------------------
@pytest.mark.multirank
@pytest.mark.parametrize("scenario", ["dist_average", "dist_adasum"])
def test_distributed_accumulation_gloo_ranks(scenario):
    """2 gloo CPU ranks with per-rank micro-batches (tests/accum_workers.py): the reduced
    gradient has the same bits on both and lies within the bound of the float64 reference."""
    for o in run_accum_ranks(scenario, "cpu"):
        print(o)


@pytest.mark.multirank
def test_ranks_that_disagree_on_accumulation_dtype_raise():
    for o in run_accum_ranks("accum_args", "cpu"):
        print(o)
