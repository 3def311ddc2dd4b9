"""Driver-visible runs of the benchmark entry points that `bench.py` does not cover
(VERDICT r4 "driver-visible evidence for config 5"): BERT-Large pre-training with fp16 wire
compression + Adasum + FusedAdamW at BASELINE.json config 5's shape (benchmarks/bench_bert.py
default: bs 512 x seq 128 per GPU, bf16), and the named GPU collective latency through mivod's
RCCL communicator at world 1 with both executors.  Each asserts the run is sane (one JSON line,
finite loss, result checked) and reports its number in the pytest terminal summary.
`bench.py` itself is run once at a tiny shape for its `--full` / `--dump-outputs` options.
"""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(args, timeout, env=None):
    import torch
    torch.cuda.empty_cache()              # the child gets the card's memory
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable] + args, cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout[-3000:]
    return json.loads(lines[-1])


def test_bench_bert_config5(cuda, mivod_report):
    r = _run(["benchmarks/bench_bert.py", "--steps", "6", "--warmup", "3"], timeout=400)
    assert r["n_gpus"] == 1 and r["steps"] == 6 and r["value"] > 0
    assert math.isfinite(r["loss"])
    cfg = r["config"]
    assert cfg["model"] == "BERT-large" and cfg["global_batch"] == 512 and cfg["seq_len"] == 128
    mivod_report(f"BERT-Large bf16 pre-training, {cfg['global_batch']} x {cfg['seq_len']} per GPU, fp16 wire + Adasum, FusedAdamW "
                 f"(benchmarks/bench_bert.py, 6 steps): {r['value']:.1f} {r['unit']}, "
                 f"{r['ms_per_step']:.2f} ms/step, loss {r['loss']}")


def test_bench_full_and_dump_outputs_small(cuda, tmp_path):
    """bench.py at a tiny shape: --steps sets the timed steps, --full adds the comm record,
    --dump-outputs writes the last step's loss / logits / parameter sample as float32."""
    import numpy as np
    d = tmp_path / "dump"
    r = _run(["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
              "--image", "64", "--full", "--dump-outputs", str(d)], timeout=200)
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
    assert abs(r["value"] - 8 / (r["ms_per_step"] * 1e-3)) <= 0.01 * r["value"]
    assert r["comm"]["buckets"] >= 1 and r["comm"]["grad_bytes_per_step"] > 0
    got = {f: np.load(d / f) for f in os.listdir(d)}
    assert sorted(got) == ["logits.npy", "loss.npy", "params_sample.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["logits.npy"].shape == (8, 1000) and got["loss.npy"].shape == (1,)
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
    # the dumped loss is the cross entropy of the dumped logits, up to the labels: bounded by
    # the log-sum-exp spread of the rows
    lg = got["logits.npy"].astype(np.float64)
    lse = np.log(np.exp(lg - lg.max(1, keepdims=True)).sum(1)) + lg.max(1)
    assert (lse - lg.max(1)).mean() - 1e-3 <= got["loss.npy"][0] <= (lse - lg.min(1)).mean() + 1e-3


@pytest.mark.parametrize("mode", ["native", "python"])
def test_named_gpu_allreduce_latency(cuda, mivod_report, mode):
    r = _run(["benchmarks/bench_named_ops.py", "--device", "gpu", "--mode", mode, "--iters", "500"],
             timeout=200, env={"MIVOD_TRANSPORT": "rccl", "MIVOD_FORCE_COLLECTIVES": "1"})
    assert r["correct"]
    if mode == "native":
        # every response run by the C++ engine loop through csrc/comm/gexec.hip
        assert r["gpu_loop_executed"] >= 500 and r["gpu_native_responses"] >= 500
    else:
        assert r["gpu_native_responses"] == 0 and r["gpu_loop_executed"] == 0
    mivod_report(f"named GPU allreduce_async + synchronize, world 1 forced RCCL, {mode} executor: "
                 f"{r['us_per_op']:.1f} us/op")


@pytest.mark.parametrize("mode", ["native", "python"])
def test_named_gpu_allgather_latency(cuda, mivod_report, mode):
    """Named GPU allgather: the native executor sizes the output from the coordinator's
    response (no size exchange, no host sync on the comm stream) — round 6."""
    r = _run(["benchmarks/bench_named_ops.py", "--device", "gpu", "--mode", mode, "--iters", "500",
              "--op", "allgather"],
             timeout=200, env={"MIVOD_TRANSPORT": "rccl", "MIVOD_FORCE_COLLECTIVES": "1"})
    assert r["correct"]
    if mode == "native":
        assert r["gpu_native_gathers"] >= 500 and r["gpu_loop_executed"] >= 500
    else:
        assert r["gpu_native_gathers"] == 0 and r["gpu_loop_executed"] == 0
    mivod_report(f"named GPU allgather_async + synchronize, world 1 forced RCCL, {mode} executor: "
                 f"{r['us_per_op']:.1f} us/op")
