"""Fused flat-arena optimizers (hand-written gfx950 kernels on GPU)."""
from .fused import (Arena, FusedAdadelta, FusedAdam, FusedAdamW, FusedLAMB, FusedLARS,
                    FusedOptimizer, FusedSGD)

__all__ = ["Arena", "FusedOptimizer", "FusedSGD", "FusedAdam", "FusedAdamW", "FusedAdadelta",
           "FusedLARS", "FusedLAMB"]
