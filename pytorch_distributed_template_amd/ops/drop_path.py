"""Stochastic depth (drop-path): the per-sample branch scales, in torch.

The draw is defined in ``csrc/drop_path.hip`` (the kernel ``pdt_drop_path_scales`` launches); this
module mirrors it bit for bit, so the torch / CPU path and the native path see the same masks for
the same ``(seed, step)``. All in uint32 (carried in int64 here), ``hash32`` being the mixer of
``csrc/misc.hip`` and ``data/synthetic.py``::

    k0 = hash32(seed ^ step * 0x9E3779B9)
    k1 = hash32(k0 ^ j * 0x85EBCA6B)            branch j: 2i attention, 2i + 1 MLP of block i
    h  = hash32(k1 ^ sample * 0xC2B2AE35)       sample: the GLOBAL index rank * B + b
    u  = (h >> 8) / 2^24                        exact in fp32, in [0, 1)

Sample ``b`` keeps branch ``j`` iff ``u >= p[j]`` (fp32), and its scale is then ``1 / (1 - p[j])``
(formed on the host, rounded to fp32), else 0. A draw depends on the sample's global index alone,
so it does not change with the number of ranks, and ranks draw different masks.
"""
from __future__ import annotations

import torch

_M32 = 0xFFFFFFFF


def _hash32(x: torch.Tensor) -> torch.Tensor:
    """``hash32`` of the kernels on int64 tensors holding uint32 values (wrapping products)."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def drop_path_rates(rate: float, depth: int) -> list:
    """Block ``i``'s drop probability ``rate * i / (depth - 1)`` (timm's linear rule; a model of
    one block gets 0)."""
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop_path_rate must be in [0, 1), got {rate}")
    return [float(rate) * i / (depth - 1) if depth > 1 else 0.0 for i in range(depth)]


def branch_constants(rates) -> tuple:
    """``(p, inv_keep)`` as fp32 tensors of ``2 * len(rates)`` entries: each block's rate for its
    attention and its MLP branch, and ``1 / (1 - p)`` -- what the kernel and the mirror compare
    with and scale by."""
    p = torch.tensor([r for r in rates for _ in range(2)], dtype=torch.float64)
    return p.to(torch.float32), (1.0 / (1.0 - p)).to(torch.float32)


def drop_path_hash(seed: int, step: int, n_branches: int, samples: torch.Tensor) -> torch.Tensor:
    """``h`` above for every (branch, sample): int64 ``[n_branches, len(samples)]`` holding uint32
    values; ``samples``: int64 global sample indices."""
    k0 = _hash32(torch.tensor(((int(seed) & _M32) ^ ((int(step) & _M32) * 0x9E3779B9 & _M32)), dtype=torch.int64))
    j = torch.arange(n_branches, dtype=torch.int64)
    k1 = _hash32(k0 ^ (j * 0x85EBCA6B & _M32))
    s = (samples.to(torch.int64).cpu() & _M32) * 0xC2B2AE35 & _M32
    return _hash32(k1[:, None] ^ s[None, :])


def drop_path_table(seed: int, step: int, p: torch.Tensor, inv_keep: torch.Tensor, batch: int, rank: int = 0,
                    device=None) -> torch.Tensor:
    """The scale table ``[len(p), batch]`` (fp32) of ``(seed, step)`` for the ranks' samples
    ``rank * batch + [0, batch)``: 0 where the branch is dropped, ``inv_keep[j]`` where kept."""
    p = p.detach().to("cpu", torch.float32)
    inv_keep = inv_keep.detach().to("cpu", torch.float32)
    samples = int(rank) * int(batch) + torch.arange(int(batch), dtype=torch.int64)
    h = drop_path_hash(seed, step, p.numel(), samples)
    u = (h >> 8).to(torch.float32) * (1.0 / 16777216.0)
    table = torch.where(u >= p[:, None], inv_keep[:, None].expand_as(u), torch.zeros((), dtype=torch.float32))
    return table.to(device) if device is not None else table


def scaled_add(y: torch.Tensor, r: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``r + scale[b] * y`` with sample ``b`` the leading dimension, in fp32 at least, rounded to
    ``y``'s dtype; a dropped sample (scale 0) takes ``r`` itself, whatever ``y`` holds there."""
    ct = torch.promote_types(y.dtype, torch.float32)
    s = scale.to(ct).reshape(-1, *([1] * (y.dim() - 1)))
    out = torch.where(s != 0, r.to(ct) + s * y.to(ct), r.to(ct))
    return out.to(y.dtype)
