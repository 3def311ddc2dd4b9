"""The fp32 moving average of the master weights without a GPU: the PyTorch fallbacks of
ema_update / ema_swap / ema_overwrite (mivod/ops/kernels.py), ``ema_decay`` of the Fused*
optimizers alone, under DistributedOptimizer on the CPU and on gloo CPU ranks, and the Keras
front end's ``use_ema``, against the float64 references and the counted bounds of
tests/ema_reference.py (tests/test_ema_gpu.py runs the HIP kernels through the same cases).
Each test prints its worst err / (2^-24 * mag) next to the counted c, or its worst
err / bound."""
import os
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import torch

import ema_reference as R
from mivod.ops import kernels as K
from test_multiprocess import (HERE, ROOT, _release_parent_gpu_cache, describe_ranks,
                               free_port)

sys.path.insert(0, os.path.join(ROOT, "examples"))

CPU = torch.device("cpu")
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32


def run_ema_ranks(scenario, device_type, *args, timeout=120, extra_env=None):
    """2 ranks of ``ema_workers.<scenario>``, in the shape of
    tests/test_accum_cpu.run_accum_ranks: one process per rank writing to its own temporary
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "ema_workers.py"),
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
@pytest.mark.parametrize("mdt", R.MODELS)
def test_ema_modes_sizes(mdt):
    print(f"model {mdt}: update worst err/(U*mag) {R.run_sizes(CPU, mdt):.2f} (c {R.C_EMA})")


@pytest.mark.parametrize("mdt", R.MODELS)
def test_ema_exact_paths_and_skip(mdt):
    for off in (0, 1):
        R.run_exact(CPU, mdt, base_off=off)
        R.run_skip(CPU, mdt, base_off=off)


def test_ema_fallbacks_reject_bad_operands():
    n = 100
    w, e = torch.zeros(n), torch.zeros(n)
    for decay in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay must be in"):
            K.ema_update(w, e, decay=decay)
    with pytest.raises(ValueError, match="ema must be a contiguous fp32"):
        K.ema_update(w, torch.zeros(n, dtype=bf16), decay=0.9)
    with pytest.raises(ValueError, match="exactly 100 elements"):
        K.ema_update(w, torch.zeros(n - 1), decay=0.9)
    with pytest.raises(ValueError, match="exactly 100 elements"):
        K.ema_swap(w, e, torch.zeros(n + 1, dtype=bf16))
    with pytest.raises(ValueError, match="master must be a contiguous fp32"):
        K.ema_overwrite(torch.zeros(2 * n)[::2], e, None)


# ---- B. evidence that the feature is what passes -----------------------------------------------------
def test_bf16_average_misses_the_bound_the_arena_meets():
    """today's arithmetic through the same harness: a bf16 ``lerp_`` average of the bf16 model
    copy (AveragedModel / ModelEma on this code base) against the fp32 arena average"""
    old, new, worst = R.run_evidence(CPU)
    print(f"decay {R.EVIDENCE_DECAY}, {R.EVIDENCE_STEPS} steps: bf16 lerp_ {100 * old:.1f} % of "
          f"the elements outside the bound, fp32 arena {100 * new:.1f} % (worst err/bound "
          f"{worst:.3f})")
    assert old >= 0.9, "the inputs do not tell a bf16 average from the fp32 arena average"
    assert new == 0.0


# ---- C. the optimizers -------------------------------------------------------------------------------
def test_ema_decay_is_validated_like_max_grad_norm():
    from mivod.optim import FusedSGD
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (-0.5, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="ema_decay must be in"):
            FusedSGD(p, ema_decay=bad)
    opt = FusedSGD(p, ema_decay=0.5)
    opt.ema_decay = 1.5
    p[0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="ema_decay must be in"):
        opt.step()
    with pytest.raises(RuntimeError, match="no step has run with ema_decay"):
        with FusedSGD([torch.nn.Parameter(torch.zeros(3))]).ema_parameters():
            pass


@pytest.mark.parametrize("kind", R.OPTIMIZERS)
@pytest.mark.parametrize("dtype", [bf16, f32])
def test_optimizer_average_follows_the_masters(kind, dtype):
    worst, _, _ = R.model_optimizer(CPU, kind, dtype)
    print(f"{kind} {dtype}, 4 steps: worst err/bound {worst:.3f} (c {R.C_EMA} per update)")


def test_every_fused_optimizer_takes_ema_decay():
    import mivod.optim as O
    names = [n for n in dir(O) if n.startswith("Fused") and n != "FusedOptimizer"]
    assert len(names) >= 10, names
    for n in names:
        lin = torch.nn.Linear(5, 3)
        opt = getattr(O, n)(lin.parameters(), ema_decay=0.5)
        for _ in range(2):
            lin(torch.ones(2, 5)).sum().backward()
            opt.step()
            opt.zero_grad()
        a = opt._mv_arenas[0]
        assert a.ema_updates == 2 and a.ema is not None and not torch.equal(a.ema, a.master), n


def test_ema_decay_toggles_between_steps():
    net = R.make_mlp(CPU, bf16)
    opt = R.make_opt("sgd", net.parameters(), None)
    b = R.make_batches(CPU, bf16, 3)
    R.train(opt, net, b[:1], CPU, record=False)
    assert opt._mv_arenas[0].ema is None
    opt.ema_decay = 0.5
    R.train(opt, net, b[1:2], CPU, record=False)
    a = opt._mv_arenas[0]
    assert a.ema_updates == 1 and torch.equal(a.ema, a.master)
    opt.ema_decay = None
    held = a.ema.clone()
    R.train(opt, net, b[2:], CPU, record=False)
    assert a.ema_updates == 1 and torch.equal(a.ema, held) and a.step == 3


@pytest.mark.parametrize("dtype", [bf16, f32])
def test_ema_parameters_swaps_and_restores(dtype):
    R.model_swap(CPU, dtype)


@pytest.mark.parametrize("dtype", [bf16, f32])
def test_state_dict_roundtrip(dtype):
    R.model_state_dict(CPU, dtype)


def test_checkpoint_roundtrip(tmp_path):
    R.model_state_dict(CPU, bf16, tmp_path)


def test_state_dict_keys_without_ema_are_unchanged():
    assert R.state_keys(CPU, "sgd", bf16) == ["master_param", "momentum_buffer", "step"]
    assert R.state_keys(CPU, "adam", f32) == ["exp_avg", "exp_avg_sq", "step"]
    assert R.state_keys(CPU, "lamb", bf16) == ["exp_avg", "exp_avg_sq", "master_param", "step"]


# ---- D. the hook path ----------------------------------------------------------------------------------
@pytest.fixture
def hvd_torch():
    import mivod.torch as hvd
    hvd.init()
    yield hvd
    hvd.shutdown()


@pytest.mark.parametrize("mode", R.HOOK_MODES)
def test_hook_path_one_rank(hvd_torch, monkeypatch, mode):
    if mode == "guard_bucket":
        monkeypatch.setenv("MIVOD_GUARD_MODE", "bucket")
    else:
        monkeypatch.delenv("MIVOD_GUARD_MODE", raising=False)
    print(f"{mode}: worst err/bound {R.hook_path(CPU, mode):.3f} (c {R.C_EMA} per update)")


@pytest.mark.parametrize("bad_step", [2, 1])
def test_hook_path_overflow_skips_step_and_average(hvd_torch, monkeypatch, bad_step):
    monkeypatch.delenv("MIVOD_GUARD_MODE", raising=False)
    worst = R.hook_overflow(CPU, bad_step=bad_step)
    print(f"inf at step {bad_step}: worst err/bound {worst:.3f}")


def test_ema_parameters_refused_inside_a_step(hvd_torch):
    net = R.make_mlp(CPU, bf16)
    opt = R.wrap(net, "overlapped", 0.9)
    b = R.make_batches(CPU, bf16, 2)
    R.train(opt, net, b[:1], CPU, record=False)
    R.loss_of(net, b[1]).backward()
    with pytest.raises(AssertionError, match="cannot be exchanged"):
        with opt.ema_parameters():
            pass
    opt.step()
    opt.zero_grad()
    with opt.ema_parameters():
        pass


@pytest.mark.multirank
@pytest.mark.parametrize("mode", ["overlapped", "guard_step"])
def test_hook_path_two_gloo_ranks(mode):
    for o in run_ema_ranks("dist_ema", "cpu", mode):
        print(o[-600:])


# ---- F. Keras ----------------------------------------------------------------------------------------------
def _keras_data(batches=4, n=8):
    rng = np.random.RandomState(0)
    x = rng.rand(batches * n, 28, 28, 1).astype("float32")
    y = np.eye(10, dtype="float32")[rng.randint(0, 10, batches * n)]
    return x, y, n


def _keras_model(opt):
    import mivod.kerasfw as keras  # noqa: F401
    from keras_mnist_convnet import build_convnet
    torch.manual_seed(0)
    m = build_convnet((28, 28, 1), 10)
    m.compile(loss="categorical_crossentropy", optimizer=opt)
    return m


def _keras_check(m, seq, decay):
    worst = 0.0
    for i, got in enumerate(m.get_weights()):
        ref, bound = R.sequence_ref([torch.from_numpy(s[i].copy()) for s in seq], decay)
        worst = max(worst, R.check(f"variable {i}", torch.from_numpy(got.copy()), ref, bound))
    return worst


def test_keras_use_ema_finalize_and_config():
    import mivod.keras as hvd
    import mivod.kerasfw as keras
    hvd.init()
    opt = keras.optimizers.SGD(0.05, use_ema=True, ema_momentum=0.9)
    m = _keras_model(opt)
    x, y, n = _keras_data()
    seq = []
    for b in range(4):
        m.train_on_batch(x[b * n:(b + 1) * n], y[b * n:(b + 1) * n])
        seq.append(m.get_weights())
    assert opt._impl.ema_decay == 0.9
    opt.finalize_variable_values(m.trainable_weights)
    worst = _keras_check(m, seq, 0.9)
    assert any(not np.array_equal(a, b) for a, b in zip(m.get_weights(), seq[-1]))
    print(f"keras SGD use_ema, 4 batches: worst err/bound {worst:.3f}")
    cfg = opt.get_config()
    assert cfg["use_ema"] is True and cfg["ema_momentum"] == 0.9 and \
        cfg["ema_overwrite_frequency"] is None
    wrapped = hvd.DistributedOptimizer(opt)
    assert wrapped.use_ema and wrapped.ema_momentum == 0.9
    plain = keras.optimizers.SGD(0.05)
    assert sorted(plain.get_config()) == ["decay", "learning_rate", "momentum", "name", "nesterov"]
    assert not hvd.DistributedOptimizer(plain).use_ema
    plain.finalize_variable_values()              # without use_ema: nothing to do
    for cls in keras.optimizers.OPTIMIZERS.values():
        assert cls(use_ema=True, ema_momentum=0.5).get_config()["ema_momentum"] == 0.5
        assert "use_ema" not in cls().get_config()


def test_keras_ema_overwrite_frequency():
    import mivod.kerasfw as keras
    opt = keras.optimizers.SGD(0.05, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=2)
    m = _keras_model(opt)
    x, y, n = _keras_data()
    for it in range(1, 5):
        m.train_on_batch(x[(it - 1) * n:it * n], y[(it - 1) * n:it * n])
        assert opt.iterations == it
        same = all(torch.equal(a.master, a.ema) for a in opt._impl._mv_arenas)
        # iteration 1: the copying first update, equal without an overwrite; 2 and 4 overwrite;
        # 3 does not, so there the weights have left the average
        assert same == (it != 3), f"iteration {it}: weights equal the average: {same}"
    with pytest.raises(ValueError, match="ema_overwrite_frequency"):
        keras.optimizers.SGD(use_ema=True, ema_overwrite_frequency=0)


def test_keras_fit_finalizes_at_the_end():
    import mivod.kerasfw as keras
    x, y, n = _keras_data()
    seqs = {}

    class Record(keras.callbacks.Callback):
        def on_train_batch_end(self, batch, logs=None):
            seqs.setdefault("w", []).append(self.model.get_weights())

    opt = keras.optimizers.SGD(0.05, use_ema=True, ema_momentum=0.9)
    m = _keras_model(opt)
    m.fit(x, y, batch_size=n, epochs=1, verbose=0, shuffle=False, callbacks=[Record()])
    assert len(seqs["w"]) == 4
    worst = _keras_check(m, seqs["w"], 0.9)
    print(f"fit, 4 batches: the weights are the average, worst err/bound {worst:.3f}")
    # with an overwrite frequency fit does not finalize
    opt = keras.optimizers.SGD(0.05, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3)
    m = _keras_model(opt)
    m.fit(x, y, batch_size=n, epochs=1, verbose=0, shuffle=False)
    assert not all(torch.equal(a.master, a.ema) for a in opt._impl._mv_arenas)


def test_keras_save_and_load_model_keep_the_average(tmp_path):
    import mivod.kerasfw as keras
    opt = keras.optimizers.SGD(0.05, use_ema=True, ema_momentum=0.9)
    m = _keras_model(opt)
    x, y, n = _keras_data()
    for b in range(3):
        m.train_on_batch(x[b * n:(b + 1) * n], y[b * n:(b + 1) * n])
    path = str(tmp_path / "m.h5")
    m.save(path)
    m2 = keras.load_model(path)
    o2 = m2.optimizer
    assert o2.use_ema and o2.ema_momentum == 0.9 and o2.iterations == 3
    for a, b in zip(opt._impl._mv_arenas, o2._impl._mv_arenas):
        assert b.ema_updates == 3 and torch.equal(a.ema.cpu(), b.ema.cpu())
    # one more batch on the loaded model: a decayed update of the restored average, not a copy
    # (its own weights are the reference: two models' convolutions need not agree in bits)
    held = [b.ema.clone().cpu() for b in o2._impl._mv_arenas]
    m2.train_on_batch(x[3 * n:], y[3 * n:])
    for b, e0 in zip(o2._impl._mv_arenas, held):
        assert b.ema_updates == 4
        ref, bound = R.update_ref(b.master.cpu(), e0, 0.9)
        R.check("the update after load_model", b.ema.cpu(), ref, bound)
        assert not torch.equal(b.ema, b.master)
