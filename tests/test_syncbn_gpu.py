"""hvd.SyncBatchNorm's fused path with real ranks: 2 and 4 processes sharing ONE MI355X over
the gloo wire (MIVOD_TRANSPORT=gloo-gpu), and one rank on mivod's RCCL communicator with
every collective forced, so RCCL's allgather and allreduce carry the records.  The scenario
(tests/syncbn_workers.gpu_model): conv -> SyncBatchNorm(relu) -> conv ->
SyncBatchNorm(residual, relu) with 2 + rank images per rank, two DistributedOptimizer steps."""
import pytest

from test_multirank_gpu import _TMO, _one_gpu
from test_syncbn_cpu import run_syncbn_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.multirank]


@pytest.mark.parametrize("n", [2, 4])
def test_syncbn_model_ranks_one_gpu(cuda, n):
    """First step: outputs and dx equal the single-process reference on the concatenated
    batch; after two steps parameters and running statistics are bitwise equal on all ranks."""
    run_syncbn_ranks("gpu_model", n, timeout=_TMO[n], extra_env=_one_gpu(n))


def test_syncbn_model_rccl_world1(cuda):
    """World size 1 with MIVOD_FORCE_COLLECTIVES=1: the record allgather and the totals'
    allreduce really run on RCCL (the worker checks the communicator's call count)."""
    run_syncbn_ranks("gpu_model", 1, timeout=160,
                     extra_env={"MIVOD_TRANSPORT": "rccl", "MIVOD_FORCE_COLLECTIVES": "1"})
