"""Fused flat-arena optimizers (hand-written gfx950 kernels on GPU)."""
from .fused import (Arena, FusedAdadelta, FusedAdagrad, FusedAdam, FusedAdamax, FusedAdamW,
                    FusedLAMB, FusedLARS, FusedNAdam, FusedOptimizer, FusedRMSprop, FusedSGD)

__all__ = ["Arena", "FusedOptimizer", "FusedSGD", "FusedAdam", "FusedAdamW", "FusedAdadelta",
           "FusedLARS", "FusedLAMB", "FusedRMSprop", "FusedAdagrad", "FusedAdamax", "FusedNAdam"]
