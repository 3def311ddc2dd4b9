"""ema_decay under mivod.torch.DistributedOptimizer, multi-rank scenarios, run as
`python tests/ema_workers.py <scenario> <device type> [...]` in 2 processes by
tests/test_ema_cpu.py (gloo CPU ranks, the fallbacks) and tests/test_ema_gpu.py (ranks sharing
one GPU over the gloo wire, the HIP kernels).  Every rank records its own master sequence,
computes the float64 reference itself, asserts, and prints "OK <rank>"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ema_reference as R  # noqa: E402
import mivod.torch as hvd  # noqa: E402

STEPS = 4
DECAY = 0.9


def _same_all(rows, what=""):
    odd = [q for q in range(1, rows.shape[0]) if not torch.equal(rows[0], rows[q])]
    assert not odd, f"{what}: ranks {odd} differ from rank 0"


def dist_ema(device_type, mode="overlapped"):
    """Per-rank batches, the same initial model: no collective is added, every rank holds the
    same master bits and therefore the same average bits, each within the accumulated bound
    of the float64 average of its recorded masters."""
    hvd.init()
    dev = hvd.device()
    assert dev.type == device_type, (dev, device_type)
    assert hvd.size() == 2
    net = R.make_mlp(dev, R.bf16)
    opt = R.wrap(net, mode, DECAY)
    batches = R.make_batches(dev, R.bf16, STEPS, seed=100 + hvd.rank())
    seq = R.train(opt, net, batches, dev)
    worst = R.check_arenas(f"2 ranks, {mode}", opt, seq, DECAY)
    print(f"2 ranks, {mode}: worst err/bound {worst:.3f} (c {R.C_EMA})", flush=True)
    flat = torch.cat([a.ema.reshape(-1) for a in opt._mv_arenas]
                     + [a.master.reshape(-1) for a in opt._mv_arenas])
    assert torch.isfinite(flat).all()
    _same_all(hvd.allgather(flat.unsqueeze(0)), "average and master weights")
    assert all(a.ema_updates == STEPS for a in opt._mv_arenas)
    # broadcast_optimizer_state carries the average and its count like the master
    if hvd.rank() == 1:
        for a in opt._mv_arenas:
            a.ema.zero_()
            a.ema_updates = 0
    hvd.broadcast_optimizer_state(opt, root_rank=0)
    R._sync(dev)
    flat2 = torch.cat([a.ema.reshape(-1) for a in opt._mv_arenas])
    assert torch.equal(flat2, flat[:flat2.numel()]), "the broadcast did not restore the average"
    assert all(a.ema_updates == STEPS for a in opt._mv_arenas)
    r = hvd.rank()
    hvd.shutdown()
    print("OK", r)


if __name__ == "__main__":
    # a hung rank prints every thread's stack and exits before the runner's limit
    import faulthandler
    import signal
    _dump = float(os.environ.get("MIVOD_TEST_DUMP_AFTER", "0"))
    if _dump > 0:
        faulthandler.dump_traceback_later(_dump, exit=True)
    faulthandler.register(signal.SIGUSR1, all_threads=True)
    globals()[sys.argv[1]](*sys.argv[2:])
