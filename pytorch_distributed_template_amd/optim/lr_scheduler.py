"""LR schedulers the recipes need beyond ``torch.optim.lr_scheduler`` (``lr_scheduler.type`` in a
config resolves here first, then there)."""
from __future__ import annotations

import math

from torch.optim.lr_scheduler import LRScheduler


class WarmupCosineLR(LRScheduler):
    """A linear warm-up followed by half a cosine, in closed form of the step count ``s``
    (``last_epoch``: the number of ``step()`` calls; with ``trainer.lr_step: "iteration"`` that
    is the number of optimizer steps)::

        s <  warmup_steps:  f(s) = a + (1 - a) s / warmup_steps             a = warmup_start_factor
        s >= warmup_steps:  f(s) = m + (1 - m) (1 + cos(pi q)) / 2          m = min_lr_ratio
                            q = min(1, (s - warmup_steps) / max(1, total_steps - warmup_steps))
        lr(s) = base_lr f(s)

    so the ramp reaches ``base_lr`` at ``s = warmup_steps`` and the cosine ``m base_lr`` at
    ``s = total_steps``, where it stays. A plain ``LRScheduler`` subclass: ``state_dict()`` is the
    base class's."""

    def __init__(self, optimizer, warmup_steps, total_steps, warmup_start_factor=0.0, min_lr_ratio=0.0,
                 last_epoch=-1):
        if warmup_steps < 0 or total_steps < warmup_steps:
            raise ValueError(f"WarmupCosineLR: need 0 <= warmup_steps <= total_steps, got {warmup_steps}, "
                             f"{total_steps}")
        self.warmup_steps = int(warmup_steps)
        self.total_steps = int(total_steps)
        self.warmup_start_factor = float(warmup_start_factor)
        self.min_lr_ratio = float(min_lr_ratio)
        super().__init__(optimizer, last_epoch)

    def factor(self, s):
        if s < self.warmup_steps:
            a = self.warmup_start_factor
            return a + (1.0 - a) * s / self.warmup_steps
        q = min(1.0, (s - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps))
        m = self.min_lr_ratio
        return m + (1.0 - m) * 0.5 * (1.0 + math.cos(math.pi * q))

    def get_lr(self):
        f = self.factor(self.last_epoch)
        return [base * f for base in self.base_lrs]
