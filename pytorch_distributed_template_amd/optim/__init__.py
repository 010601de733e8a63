"""Optimizers. ``optimizer.type`` in config resolves here first, then in torch.optim."""
from .fused import FusedSGD, FusedAdam, FusedAdamW, FusedLARS, FusedLAMB  # noqa: F401
from .ema import ModelEMA  # noqa: F401
from .lr_scheduler import WarmupCosineLR  # noqa: F401
