"""hvd.SyncBatchNorm without a GPU: the plain-torch path over gloo CPU ranks against a
float64 reference, the size-1 module against torch.nn.BatchNorm2d, and the exported names.
Also home of ``run_syncbn_ranks``, the runner of tests/syncbn_workers.py scenarios
(tests/test_syncbn_gpu.py imports it)."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import pytest
import torch

from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)


def run_syncbn_ranks(scenario, n=2, timeout=120, extra_env=None):
    """``n`` ranks of ``syncbn_workers.<scenario>``, in the shape of
    tests/test_multiprocess.run_ranks: one process per rank writing to its own temporary
    file, the same environment, one deadline for the whole world.  At the first non-zero
    exit or at the deadline every rank still running dumps its stacks and is stopped;
    nothing is retried."""
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "syncbn_workers.py"),
                                       scenario], env=env, stdout=f, stderr=subprocess.STDOUT,
                                      text=True))
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


@pytest.mark.multirank
@pytest.mark.parametrize("n", [2, 3])
def test_syncbn_fallback_gloo_ranks(n):
    """fp32 on gloo CPU ranks with unequal batches, 2-D and 4-D input, plain / ReLU /
    add+ReLU: outputs, dx, local dgamma / dbeta and running statistics against float64 on
    the concatenated batch; running statistics bitwise equal across ranks."""
    run_syncbn_ranks("cpu_fallback", n, timeout=120)


@pytest.fixture
def hvd1():
    import mivod.torch as hvd
    was = hvd.is_initialized()
    if not was:
        hvd.init()
    yield hvd
    if not was:
        hvd.shutdown()


def test_syncbn_needs_init(monkeypatch):
    import mivod.torch as hvd
    from mivod.common import basics
    monkeypatch.setattr(basics.state(), "initialized", False)
    m = hvd.SyncBatchNorm(4)
    with pytest.raises(ValueError, match="has not been initialized"):
        m(torch.randn(2, 4, 3, 3))
    m.eval()                                   # inference needs no world
    assert m(torch.randn(2, 4, 3, 3)).shape == (2, 4, 3, 3)


def test_syncbn_size1_equals_batchnorm2d(hvd1):
    """One rank: training and evaluation equal torch.nn.BatchNorm2d — outputs, gradients,
    running statistics, num_batches_tracked (momentum None: the cumulative average)."""
    assert hvd1.size() == 1
    for momentum in (0.1, None):
        torch.manual_seed(0)
        m = hvd1.SyncBatchNorm(6, momentum=momentum)
        ref = torch.nn.BatchNorm2d(6, momentum=momentum)
        with torch.no_grad():
            m.weight.copy_(torch.rand(6) + 0.5)
            m.bias.copy_(torch.randn(6) * 0.1)
        ref.load_state_dict(m.state_dict())
        for step in range(3):
            x = torch.randn(4, 6, 5, 3) * 2 + 1
            g = torch.randn(4, 6, 5, 3)
            x1, x2 = x.clone().requires_grad_(), x.clone().requires_grad_()
            y, yr = m(x1), ref(x2)
            y.backward(g)
            yr.backward(g)
            torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(m.weight.grad, ref.weight.grad, rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(m.bias.grad, ref.bias.grad, rtol=1e-4, atol=1e-5)
            m.zero_grad()
            ref.zero_grad()
        sd, sdr = m.state_dict(), ref.state_dict()
        assert int(sd["num_batches_tracked"]) == int(sdr["num_batches_tracked"]) == 3
        torch.testing.assert_close(sd["running_mean"], sdr["running_mean"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(sd["running_var"], sdr["running_var"], rtol=1e-5, atol=1e-6)
        m.eval()
        ref.eval()
        x = torch.randn(2, 6, 4, 4)
        torch.testing.assert_close(m(x), ref(x), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(m(x, x, True), torch.relu(ref(x) + x), rtol=1e-5, atol=1e-6)


def test_syncbn_bindings_reject_cpu_operands_by_name():
    """mivod._mvk._syncbn runs mv_checks.h's operand checks before any launch: a CPU tensor
    is refused as "<binding>: <first operand> must ..." (the contract
    tests/test_bindings_validation.py holds mivod._mvk's own bindings to)."""
    from mivod.ops import kernels as K
    sb = K.native()._syncbn
    x = torch.zeros(1, 64, 8, 8, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    recs = torch.zeros(1, 3 * 64 + 4, dtype=torch.int32)
    vec, tot = torch.zeros(4, 64), torch.zeros(2, 64)
    count = torch.zeros(1, dtype=torch.int64)
    calls = {
        "syncbn_stats": ("x", lambda: sb.syncbn_stats(x, None)),
        "syncbn_merge": ("records", lambda: sb.syncbn_merge(recs, None, None, None, None, 0.1,
                                                            1e-5)),
        "syncbn_fwd": ("x", lambda: sb.syncbn_fwd(x, recs, None, None, None, None, 0.1, 1e-5,
                                                  True, None, False)),
        "syncbn_bwd_reduce": ("dy", lambda: sb.syncbn_bwd_reduce(1, x, x.clone(), None, vec, True)),
        "syncbn_bwd_dx": ("d", lambda: sb.syncbn_bwd_dx(0, x, x.clone(), vec, None, tot, count)),
    }
    assert set(calls) == {n for n in dir(sb) if not n.startswith("_")}
    for name, (operand, call) in calls.items():
        with pytest.raises(RuntimeError, match=f"{name}: {operand} must"):
            call()


def test_syncbn_exported_and_not_a_fused_batchnorm2d():
    import horovod.torch as hvd
    import mivod.torch as mvt
    from mivod.ops.bn import BatchNorm2d
    assert hvd.SyncBatchNorm is mvt.SyncBatchNorm
    assert issubclass(hvd.SyncBatchNorm, torch.nn.modules.batchnorm._BatchNorm)
    # the ResNet fast paths select on ops.bn.BatchNorm2d and would use local statistics
    assert not issubclass(hvd.SyncBatchNorm, BatchNorm2d)
    assert not issubclass(hvd.SyncBatchNorm, torch.nn.BatchNorm2d)
