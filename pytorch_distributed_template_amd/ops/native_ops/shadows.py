"""bf16 weight shadows (cast once per parameter version)"""
from __future__ import annotations

import weakref

import torch

from .lib import _chk, _cl, _load, _p, _s

_SHADOWS: dict = {}


def _same_tensor(ent_ref, w) -> bool:
    # id() and data_ptr() are both recycled after a tensor dies (a new Parameter of
    # the same size can get both): the cache entry must point at THIS object
    return ent_ref is not None and ent_ref() is w


def register_shadow(param: torch.Tensor, shadow: torch.Tensor):
    """Optimizers that write a bf16 copy while stepping register it here."""
    _SHADOWS[id(param)] = (shadow, param._version, param.data_ptr(), weakref.ref(param))


def bf16_weight(w: torch.Tensor, pad_cin_to: int | None = None) -> torch.Tensor:
    """bf16 copy of an fp32 weight in [Cout][..][Cin] (channels_last) storage."""
    if w.dtype == torch.bfloat16 and pad_cin_to is None:
        return _cl(w)
    key = (id(w), pad_cin_to)
    ent = _SHADOWS.get(key if pad_cin_to else id(w))
    if ent is not None and ent[1] == w._version and ent[2] == w.data_ptr() and _same_tensor(ent[3], w):
        return ent[0]
    src = _cl(w.detach())
    if pad_cin_to is not None and src.shape[1] != pad_cin_to:
        src = torch.nn.functional.pad(src, (0, 0, 0, 0, 0, pad_cin_to - src.shape[1]))
        src = _cl(src)
    out = torch.empty_like(src, dtype=torch.bfloat16, memory_format=torch.channels_last) if src.dim() == 4 \
        else torch.empty_like(src, dtype=torch.bfloat16)
    if src.dtype == torch.float32:
        _chk(_load().pdt_cast_f32_bf16(_p(src), _p(out), src.numel(), _s()), "cast")
    else:
        out.copy_(src)
    _SHADOWS[key if pad_cin_to else id(w)] = (out, w._version, w.data_ptr(), _weak(w))
    return out


def _weak(t):
    try:
        return weakref.ref(t)
    except TypeError:
        return None


_WT: dict = {}


def bf16_weight_t(w: torch.Tensor) -> torch.Tensor:
    """bf16 W^T [K][Nout] of an fp32 [Nout][K] weight, cached per parameter version."""
    ent = _WT.get(id(w))
    if ent is not None and ent[0] == w._version and ent[1] == w.data_ptr() and _same_tensor(ent[3], w):
        return ent[2]
    Nout, K = w.shape
    wt = torch.empty((K, Nout), dtype=torch.bfloat16, device=w.device)
    _chk(_load().pdt_transpose_cast(_p(w.detach().float().contiguous()), _p(wt), Nout, K, _s()), "transpose")
    _WT[id(w)] = (w._version, w.data_ptr(), wt, _weak(w))
    return wt
