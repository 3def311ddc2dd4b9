"""CPU tier: bench.py's JSON contract and its multi-rank self-diagnosis
(VERDICT r2 "Next round" item 1): timeout defaults for multi-rank runs, the
measured per-bucket allreduce record, and what RCCL reports about itself."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mivod.utils import benchutil as BU  # noqa: E402


def test_multi_rank_timeout_defaults():
    env = {"WORLD_SIZE": "8"}
    applied = BU.multi_rank_defaults(env)
    assert env["MIVOD_RCCL_TIMEOUT_S"] == "300"
    assert env["HOROVOD_STALL_SHUTDOWN_TIME_SECONDS"] == "300"
    assert set(applied) == {"MIVOD_RCCL_TIMEOUT_S", "HOROVOD_STALL_SHUTDOWN_TIME_SECONDS"}
    # user settings win; a single rank keeps horovod's library default (no timeout)
    env = {"HOROVOD_SIZE": "2", "MIVOD_RCCL_TIMEOUT_S": "42"}
    BU.multi_rank_defaults(env)
    assert env["MIVOD_RCCL_TIMEOUT_S"] == "42"
    env = {"WORLD_SIZE": "1"}
    assert BU.multi_rank_defaults(env) == {} and "MIVOD_RCCL_TIMEOUT_S" not in env


def test_watchdog_timeout_resolution(monkeypatch):
    from mivod.common import basics
    from mivod.common.config import Config
    monkeypatch.delenv("MIVOD_RCCL_TIMEOUT_S", raising=False)
    monkeypatch.setenv("HOROVOD_STALL_SHUTDOWN_TIME_SECONDS", "300")
    assert basics.rccl_timeout_s(Config.from_env()) == 300.0
    monkeypatch.setenv("MIVOD_RCCL_TIMEOUT_S", "12")
    assert basics.rccl_timeout_s(Config.from_env()) == 12.0
    monkeypatch.delenv("MIVOD_RCCL_TIMEOUT_S")
    monkeypatch.delenv("HOROVOD_STALL_SHUTDOWN_TIME_SECONDS")
    assert basics.rccl_timeout_s(Config.from_env()) == 0.0


def test_comm_timing_record_busbw():
    # 2 steps x 2 buckets on 8 ranks: 100 MB in 1 ms -> algbw 100 GB/s, busbw x 2*7/8
    t = [("bucket.0", 10 ** 8, 1.0), ("bucket.1", 10 ** 6, 0.5),
         ("bucket.0", 10 ** 8, 1.0), ("bucket.1", 10 ** 6, 0.5)]
    r = BU.comm_timing_record(t, steps=2, size=8)
    assert r["allreduce_ms"] == 1.5
    b0 = r["per_bucket"][0]
    assert b0["bucket"] == "bucket.0" and b0["ms"] == 1.0
    assert abs(b0["busbw_GBps"] - 100.0 * 1.75) < 1e-6
    assert r["busbw_GBps"] > 0 and r["algbw_GBps"] > 0
    empty = BU.comm_timing_record([], steps=2, size=1)
    assert empty["allreduce_ms"] is None and empty["per_bucket"] == []


def test_bench_record_schema():
    bench = importlib.import_module("bench")
    args = argparse.Namespace(steps=20, warmup=5, batch=2048, image=224, optimizer="sgd",
                              compression="none", graph=False)
    comm = {"buckets": 5, **BU.comm_timing_record([("bucket.0", 4 * 2 ** 20, 0.2)], 1, 2),
            "rccl": {"version": 22606, "header_version": 22707, "nranks": 2, "ctas": [0, 0]}}
    rec = bench.make_record(args, 2, 31000.0, 132.0, "rccl", comm)
    line = json.loads(json.dumps(rec))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in line, k
    assert line["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 4096
    assert line["config"]["parallelism"] == "dp2" and line["dtype"] == "bf16"
    c = line["comm"]
    assert c["rccl"]["nranks"] == 2 and c["allreduce_ms"] == 0.2
    assert c["per_bucket"][0]["busbw_GBps"] > 0


def test_bench_plain_record_and_options(monkeypatch):
    """A plain run's line keeps the headline keys and has no comm record; the comm
    record is behind --full, the outputs behind --dump-outputs DIR."""
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    rec = json.loads(json.dumps(bench.make_record(args, 1, 19000.0, 107.8, "local", None)))
    assert "comm" not in rec
    assert rec["metric"] == bench.BASELINE_METRIC and rec["value"] == 19000.0
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True
    assert rec["dtype"] == "bf16" and rec["ms_per_step"] == 107.8 and rec["steps"] == 7
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "some/dir"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "some/dir"


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs: float32 .npy files; a parameter above the sample size is cut to
    the same seeded sample on every call, a smaller one is kept whole."""
    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    n = bench.DUMP_PARAM_SAMPLE
    big = torch.arange(3 * n + 5, dtype=torch.float32).reshape(-1, 1)
    small = torch.tensor([1.5, -2.0, 0.25], dtype=torch.bfloat16)
    loss = torch.tensor(6.9077)
    logits = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    got = []
    for sub in ("a", "b"):
        d = tmp_path / sub
        bench.dump_outputs(str(d), loss, logits, [big, small])
        assert sorted(os.listdir(d)) == ["logits.npy", "loss.npy", "params_sample.npy"]
        got.append({f: np.load(d / f) for f in os.listdir(d)})
        assert all(a.dtype == np.float32 for a in got[-1].values())
    a, b = got
    assert a["loss.npy"].shape == (1,) and abs(float(a["loss.npy"][0]) - 6.9077) < 1e-6
    assert np.array_equal(a["logits.npy"], np.arange(12, dtype=np.float32).reshape(3, 4))
    ps = a["params_sample.npy"]
    assert ps.shape == (n + 3,) and np.array_equal(ps, b["params_sample.npy"])
    # the sample holds distinct elements of the big parameter, in index order
    assert np.all(np.diff(ps[:n]) > 0) and ps[n - 1] <= 3 * n + 4
    assert np.array_equal(ps[n:], np.array([1.5, -2.0, 0.25], dtype=np.float32))


def test_rccl_info_reports_versions():
    """The comm module reports the run-time RCCL version (ncclGetVersion) next to
    the header it was compiled against, and flags a major.minor skew."""
    try:
        from mivod import _mvcomm
    except ImportError:
        import pytest
        pytest.skip("mivod._mvcomm not built")
    rt, hdr = _mvcomm.rccl_version(), _mvcomm.header_version()
    assert rt > 20000 and hdr > 20000
    note = _mvcomm.version_note()
    assert (note == "") == (rt // 100 == hdr // 100)
    info = BU.rccl_info()
    assert info["version"] == rt and info["header_version"] == hdr


class _FakeTr:
    def __init__(self, name, size):
        self.name, self.size = name, size

    def count(self):
        return self.size

    ctas = (0, 0)


def _fake_state(monkeypatch, backend, tr, size, mesh=None):
    from mivod.common import basics
    st = basics.state()
    monkeypatch.setattr(st, "backend", backend, raising=False)
    monkeypatch.setattr(st, "gpu", tr, raising=False)
    monkeypatch.setattr(st, "size", size, raising=False)
    monkeypatch.setattr(st, "mesh", mesh, raising=False)


def test_rccl_info_is_unambiguous_per_transport(monkeypatch):
    """nranks is ncclCommCount for mivod's RCCL communicator ONLY; a gloo / torch
    group reports its size under its own key, and the local (size-1) path has
    no GPU group at all.  check_rccl_world refuses an RCCL world of the wrong size."""
    import pytest
    # rccl: nranks from the communicator
    _fake_state(monkeypatch, "rccl", _FakeTr("rccl", 8), 8)
    info = BU.rccl_info()
    assert info["transport"] == "rccl" and info["nranks"] == 8 and "gloo-gpu" not in info
    BU.check_rccl_world(info, 8)
    with pytest.raises(SystemExit):
        BU.check_rccl_world(info, 4)
    # gloo-gpu (shared-GPU rehearsal): no RCCL communicator exists
    _fake_state(monkeypatch, "gloo-gpu", _FakeTr("gloo-gpu", 8), 8)
    info = BU.rccl_info()
    assert info["nranks"] is None and info["gloo-gpu"] == {"group_size": 8}
    BU.check_rccl_world(info, 8)          # not RCCL: nothing to check
    # torch ProcessGroupNCCL A/B transport: also not mivod's communicator
    _fake_state(monkeypatch, "torch-nccl", _FakeTr("torch-nccl", 2), 2)
    info = BU.rccl_info()
    assert info["nranks"] is None and info["torch-nccl"] == {"group_size": 2}
    # local (world 1): no GPU group
    _fake_state(monkeypatch, "local", None, 1)
    info = BU.rccl_info()
    assert info["transport"] == "local" and info["nranks"] is None
    BU.check_rccl_world(info, 1)
