"""``hvd.SyncBatchNorm``: batch normalization whose batch statistics cover every rank.

Parity: horovod's ``horovod/torch/sync_batch_norm.py`` (added after the 0.18.1 survey,
SURVEY.md): mean and variance over the global batch, ranks may hold different batch sizes,
weight and bias gradients stay local sums (``DistributedOptimizer`` averages them).

MI355X design: channels_last bf16 activations keep the fused BN passes of
``csrc/kernels/mv_bn.hip``; the cross-rank part is four small kernels
(``csrc/kernels/mv_syncbn.hip``) around ONE collective per direction — an allgather of a
fixed-size record per rank (sums around the rank's own shift, exact row count) merged in
rank order so every rank gets the same bits, and a sum of the [2, C] gradient totals.  Both
are direct collectives in the issue order shared with the gradient buckets
(``mivod.parallel.order``).  Other inputs (CPU, fp32, NCHW, 2-D / 3-D / 5-D) take the same
mathematics in plain torch over ``mivod.parallel.collectives``.

Not a subclass of ``mivod.ops.bn.BatchNorm2d``: the ResNet fast paths select on that type
and would normalize with local statistics.  ``forward(x, residual=None, relu=False)`` has
that class's shape, so those paths can learn about it later.
"""
from __future__ import annotations

import torch
from torch.nn.modules.batchnorm import _BatchNorm

from ..common import basics
from ..ops.bn import sync_batch_norm_act


class SyncBatchNorm(_BatchNorm):
    """Drop-in for ``torch.nn.BatchNorm{1,2,3}d`` (same parameters, buffers, state_dict)
    with ``forward(x, residual=None, relu=False)`` = ``act(bn(x) + residual)``."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._mv_steps = 0   # host-side num_batches_tracked (no GPU add per call)

    def _check_input_dim(self, x):
        if x.dim() < 2:
            raise ValueError(f"expected at least 2D input (got {x.dim()}D input)")

    def _train_momentum(self) -> float:
        """Momentum of this training forward (counts the step, as forward does)."""
        momentum = 0.0 if self.momentum is None else self.momentum
        if self.training and self.track_running_stats:
            self._mv_steps += 1
            if self.momentum is None:
                momentum = 1.0 / float(self._mv_steps + int(self.num_batches_tracked.item()))
        return momentum

    def forward(self, x, residual=None, relu=False):
        self._check_input_dim(x)
        bn_training = self.training or (self.running_mean is None and self.running_var is None)
        if bn_training:
            basics.size()            # ValueError before hvd.init(), as every collective op
        momentum = self._train_momentum()
        rm = self.running_mean if (not self.training or self.track_running_stats) else None
        rv = self.running_var if (not self.training or self.track_running_stats) else None
        return sync_batch_norm_act(x, self.weight, self.bias, rm, rv, bn_training, momentum,
                                   self.eps, relu, residual)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        if self._mv_steps and self.num_batches_tracked is not None:
            with torch.no_grad():
                self.num_batches_tracked.add_(self._mv_steps)
            self._mv_steps = 0
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, *args, **kwargs):
        self._mv_steps = 0
        super()._load_from_state_dict(*args, **kwargs)
