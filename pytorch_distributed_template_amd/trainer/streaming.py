"""Streaming validation (``trainer.eval_mode: "stream"``): the loss sum and the top-k correct
counts of a validation pass are added up on the device, batch by batch, and cross the ranks in one
small all-reduce at the end of the pass. No logits are kept, nothing is gathered, and the host
does not wait for a batch.

The per-batch work is one ``ops.fused.eval_stats_update`` (``csrc/eval_stats.hip`` on the native
path). What can be streamed is what has a row-wise form: the losses of ``models.loss.EVAL_FORMS``
and the metrics of ``models.metric.COUNT_FORMS``.
"""
from __future__ import annotations

import torch

from ..models import loss as module_loss
from ..models.loss import EVAL_FORMS
from ..models.metric import COUNT_FORMS
from ..ops import fused
from ..utils import dist as pdist

EVAL_MODES = ("gather", "stream")


def eval_mode(config):
    """``trainer.eval_mode`` of a config: ``"gather"`` (the default: logits of the whole set to rank
    0, scored there) or ``"stream"``; anything else is an error."""
    mode = config["trainer"].get("eval_mode", "gather")
    if mode not in EVAL_MODES:
        raise ValueError(f'trainer.eval_mode must be "gather" or "stream", got {mode!r}')
    return mode


class StreamingEval:
    """Accumulates one validation pass. Built from the criterion and the metric functions of the
    registries; raises ``ValueError`` naming the loss or metric that has no streamed form."""

    def __init__(self, criterion, metric_ftns, device):
        # The streamed form is looked up by the registry function's name, and the smoothing is the
        # table's: ``runtime.build_criterion_metrics`` hands out the registry functions themselves,
        # so a config can only produce their defaults. A callable bound to other arguments (a
        # ``functools.partial``, a lambda) has no registry name, and a wrapper that borrows one is
        # not the registry's function: both are refused below rather than scored at a smoothing
        # they do not use.
        loss_name = getattr(criterion, "__name__", repr(criterion))
        if loss_name not in EVAL_FORMS or getattr(module_loss, loss_name, None) is not criterion:
            raise ValueError(f'trainer.eval_mode "stream": the loss {loss_name!r} has no row-wise form '
                             f"(streamable: {sorted(EVAL_FORMS)})")
        self.kind, self.eps = EVAL_FORMS[loss_name]
        self.names = [getattr(m, "__name__", repr(m)) for m in metric_ftns]
        for name in self.names:
            if name not in COUNT_FORMS:
                raise ValueError(f'trainer.eval_mode "stream": the metric {name!r} has no count form '
                                 f"(streamable: {sorted(COUNT_FORMS)})")
        self.ks = tuple(sorted({COUNT_FORMS[n] for n in self.names}))
        if len(self.ks) > fused.EVAL_MAX_K:
            raise ValueError(f'trainer.eval_mode "stream": {len(self.ks)} distinct k (at most {fused.EVAL_MAX_K})')
        self.device = device
        self.reset()

    def reset(self):
        self.loss_sum, self.counts = fused.eval_stats_new(self.ks, self.device)

    def update(self, output, target):
        """Add one batch (no host sync)."""
        if not torch.is_tensor(target):
            raise ValueError("streaming validation scores hard labels: got a mixed batch's "
                             f"{type(target).__name__} (validation loaders must not mix)")
        fused.eval_stats_update(output, target, self.loss_sum, self.counts, self.ks, kind=self.kind, eps=self.eps)

    def result(self, prefix=""):
        """``{prefix + "loss": loss sum / rows, prefix + <metric>: correct at its k / rows}`` over
        every rank's batches (the same dict on every rank): one all-reduce of a float64 vector --
        the loss sum and the counts, which are exact below 2^53 -- and the pass's only host read.
        Raises ``ValueError`` if any target was out of range."""
        stats = torch.cat([self.loss_sum, self.counts.to(torch.float64)])
        if pdist.get_world_size() > 1:
            torch.distributed.all_reduce(stats)
        stats = stats.tolist()
        loss_sum, rows, bad = stats[0], int(stats[1]), int(stats[2])
        if bad:
            raise ValueError(f"validation: {bad} of {rows} target(s) out of range [0, num_classes)")
        correct = dict(zip(self.ks, stats[3:]))
        out = {prefix + "loss": loss_sum / max(rows, 1)}
        for name in self.names:
            out[prefix + name] = int(correct[COUNT_FORMS[name]]) / max(rows, 1)
        return out
