"""softmax cross-entropy, the streaming evaluation statistics, and the NLL loss with its lazy target check"""
from __future__ import annotations

import ctypes
import os

import torch

from .lib import _chk, _load, _p, _s, c_int, fallback
from .tuning import _capturing


class _XEnt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, eps):
        lib = _load()
        logits = logits.contiguous()
        B, V = logits.shape
        is_bf16 = logits.dtype == torch.bfloat16
        if not is_bf16 and logits.dtype != torch.float32:
            logits = logits.float()
        target = target.to(torch.long).contiguous()
        assert target.numel() == B
        lse = torch.empty(B, dtype=torch.float32, device=logits.device)
        rows = torch.empty(B, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        _chk(lib.pdt_xent_fwd(_p(logits), int(is_bf16), _p(target), _p(lse), _p(rows), _p(loss), B, V, float(eps),
                              _s()), "xent_fwd")
        ctx.save_for_backward(logits, target, lse)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target, lse = ctx.saved_tensors
        B, V = logits.shape
        g = g.float().reshape(1).contiguous()
        dl = torch.empty((B, V), dtype=torch.bfloat16, device=logits.device)
        _chk(_load().pdt_xent_bwd(_p(logits), int(logits.dtype == torch.bfloat16), _p(target), _p(lse), _p(g),
                                  _p(dl), B, V, float(ctx.eps), _s()), "xent_bwd")
        return dl, None, None


class _XEntPair(torch.autograd.Function):
    """Cross-entropy against paired targets (``pdt_xent_pair_fwd`` / ``_bwd``): row ``b`` is
    ``lam[b]`` of class ``ta[b]`` and ``1 - lam[b]`` of class ``tb[b]``."""

    @staticmethod
    def forward(ctx, logits, ta, tb, lam, eps):
        lib = _load()
        logits = logits.contiguous()
        B, V = logits.shape
        is_bf16 = logits.dtype == torch.bfloat16
        if not is_bf16 and logits.dtype != torch.float32:
            logits = logits.float()
        ta, tb = ta.to(torch.long).contiguous(), tb.to(torch.long).contiguous()
        lam = lam.to(torch.float32).contiguous()
        assert ta.numel() == B and tb.numel() == B and lam.numel() == B
        assert ta.device == logits.device and tb.device == logits.device and lam.device == logits.device
        lse = torch.empty(B, dtype=torch.float32, device=logits.device)
        rows = torch.empty(B, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        _chk(lib.pdt_xent_pair_fwd(_p(logits), int(is_bf16), _p(ta), _p(tb), _p(lam), _p(lse), _p(rows), _p(loss), B,
                                   V, float(eps), _s()), "xent_pair_fwd")
        ctx.save_for_backward(logits, ta, tb, lam, lse)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, ta, tb, lam, lse = ctx.saved_tensors
        B, V = logits.shape
        g = g.float().reshape(1).contiguous()
        dl = torch.empty((B, V), dtype=torch.bfloat16, device=logits.device)
        _chk(_load().pdt_xent_pair_bwd(_p(logits), int(logits.dtype == torch.bfloat16), _p(ta), _p(tb), _p(lam),
                                       _p(lse), _p(g), _p(dl), B, V, float(ctx.eps), _s()), "xent_pair_bwd")
        return dl, None, None, None, None


def softmax_cross_entropy_pair(logits, label_a, label_b, lam, label_smoothing=0.0):
    """Mean cross-entropy of [B, V] ``logits`` against ``lam * onehot(label_a) + (1 - lam) *
    onehot(label_b)`` (label-smoothed), without building that matrix."""
    assert logits.dim() == 2
    return _XEntPair.apply(logits, label_a, label_b, lam, float(label_smoothing))


def softmax_cross_entropy(logits, target, label_smoothing=0.0):
    if logits.dim() != 2:
        fallback("softmax_cross_entropy", f"logits of shape {tuple(logits.shape)} (kernel: [B, V])")
        return torch.nn.functional.cross_entropy(logits.float(), target, label_smoothing=label_smoothing)
    return _XEnt.apply(logits, target, float(label_smoothing))


EVAL_KINDS = {"ce": 0, "nll": 1}  # pdt_eval_stats' loss kinds
_EVAL_KS = {}  # (k, ...) -> the host int array the entry point reads (kept alive: built once per tuple)


def eval_stats(logits, target, ks, loss_sum, counts, kind="ce", eps=0.0, loss_rows=None, rank=None):
    """``pdt_eval_stats``: score the rows of ``logits`` [B, V] (bf16 or fp32, last dimension dense,
    any row stride) against ``target`` [B] and ADD the batch into ``loss_sum`` (float64 [1]) and
    ``counts`` (int64 [2 + len(ks)]: rows, out-of-range targets, rows with rank < k for each k).
    Two launches, no host sync. Returns the per-row ``(loss_rows fp32 [B], rank int32 [B])`` (given,
    or allocated here)."""
    if logits.dim() != 2:
        raise ValueError(f"eval_stats: logits of shape {tuple(logits.shape)} (kernel: [B, V])")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        logits = logits.float()
    B, V = logits.shape
    if V > 1 and logits.stride(1) != 1:
        logits = logits.contiguous()
    ld = logits.stride(0) if B > 1 else V
    if ld < V:  # (an expanded or overlapping view)
        logits, ld = logits.contiguous(), V
    dev = logits.device
    target = target.to(torch.long).contiguous()
    ks = tuple(int(k) for k in ks)
    if target.numel() != B or target.device != dev:
        raise ValueError(f"eval_stats: target {tuple(target.shape)} on {target.device} for logits "
                         f"{tuple(logits.shape)} on {dev}")
    if loss_sum.dtype != torch.float64 or loss_sum.numel() != 1 or counts.dtype != torch.int64 \
            or counts.numel() != 2 + len(ks) or not counts.is_contiguous() or loss_sum.device != dev \
            or counts.device != dev:
        raise ValueError("eval_stats: loss_sum must be float64 [1] and counts contiguous int64 [2 + len(ks)] on "
                         "the logits' device")
    if loss_rows is None:
        loss_rows = torch.empty(B, dtype=torch.float32, device=dev)
    if rank is None:
        rank = torch.empty(B, dtype=torch.int32, device=dev)
    assert loss_rows.dtype == torch.float32 and rank.dtype == torch.int32
    assert loss_rows.numel() == B and rank.numel() == B and loss_rows.is_contiguous() and rank.is_contiguous()
    host_ks = _EVAL_KS.get(ks)
    if host_ks is None:
        host_ks = _EVAL_KS[ks] = (c_int * max(len(ks), 1))(*ks)
    _chk(_load().pdt_eval_stats(_p(logits), int(logits.dtype == torch.bfloat16), ld, _p(target), EVAL_KINDS[kind],
                                float(eps), ctypes.addressof(host_ks), len(ks), _p(loss_rows), _p(rank),
                                _p(loss_sum), _p(counts), B, V, _s()), "eval_stats")
    return loss_rows, rank


class _TargetCheck:
    """Lazy device-side check of NLL targets: each forward's count of out-of-range
    targets is copied (non-blocking) to pinned host memory; the NEXT call reads it once
    its event has completed and raises -- no host sync inside the step. The loss of
    the offending batch itself is already NaN (csrc/lenet.hip nll_fwd_kernel).
    ``PDT_CHECK_TARGETS=sync`` checks every call synchronously instead."""

    def __init__(self):
        self.pending = []  # (event, pinned host tensor)

    def record(self, bad: torch.Tensor):
        if _capturing():  # inside a HIP-graph capture: no host copies / events (the NaN loss remains)
            return
        if os.environ.get("PDT_CHECK_TARGETS", "lazy") == "sync":
            n = float(bad.item())
            if n:
                raise ValueError(f"nll_loss: {int(n)} target(s) out of range [0, num_classes)")
            return
        host = torch.empty(1, dtype=torch.float32, pin_memory=True)
        host.copy_(bad.reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, host))

    MAX_PENDING = 64  # beyond this the oldest check is waited for (never dropped)

    def poll(self, block=False):
        """Raise if any finished check saw an out-of-range target. ``block``: wait for every
        pending check (end of an epoch / run: the last batches' checks are read too). Every
        check is kept until it has been read; when more than MAX_PENDING are queued the
        oldest is waited for instead of dropped."""
        if _capturing():
            return
        keep = []
        for i, (ev, host) in enumerate(self.pending):
            if not (block or len(self.pending) - i > self.MAX_PENDING) and not ev.query():
                keep.append((ev, host))
                continue
            ev.synchronize()
            if float(host[0]):
                self.pending = []
                raise ValueError(f"nll_loss: {int(host[0])} target(s) out of range [0, num_classes) "
                                 "in an earlier batch (its loss was NaN)")
        self.pending = keep


def check_targets_pending():
    """Read every outstanding NLL target check (blocking); raises on an out-of-range target.
    The Trainer calls it at the end of each epoch."""
    _TARGETS.poll(block=True)


_TARGETS = _TargetCheck()


class _NLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target, ignore_index):
        _TARGETS.poll()
        logp = logp.float().contiguous()
        target = target.to(torch.long).contiguous()
        B, C = logp.shape
        assert target.numel() == B
        out = torch.empty(3, dtype=torch.float32, device=logp.device)  # loss, count, #out-of-range targets
        _chk(_load().pdt_nll_fwd(_p(logp), _p(target), B, C, int(ignore_index), _p(out[0]), _p(out[1]),
                                 _p(out[2]), _s()), "nll_fwd")
        _TARGETS.record(out[2])
        ctx.save_for_backward(target, out)
        ctx.meta = (B, C, int(ignore_index))
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        target, out = ctx.saved_tensors
        B, C, ignore = ctx.meta
        d = torch.empty((B, C), dtype=torch.float32, device=target.device)
        _chk(_load().pdt_nll_bwd(_p(target), _p(g.float().reshape(1).contiguous()), _p(out[1]), B, C, ignore, _p(d),
                                 _s()), "nll_bwd")
        return d, None, None


def nll_loss(logp, target, ignore_index=-100):
    return _NLL.apply(logp, target, ignore_index)
