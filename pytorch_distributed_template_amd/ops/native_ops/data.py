"""raw kernel wrappers: synthetic images and the packed-image augmentation"""
from __future__ import annotations

import ctypes

import torch

from .lib import _chk, _load, _p, _s, c_float


def fill_uniform_(t: torch.Tensor, seed: int):
    assert t.dtype == torch.bfloat16 and t.numel() % 8 == 0
    _chk(_load().pdt_fill_uniform_bf16(_p(t), t.numel(), seed & 0xFFFFFFFF, _s()), "fill")
    return t


def synthetic_images_at(buf, idx, C, seed, labels, num_classes):
    """Samples ``idx`` (int64 [B], device) of the index-addressable synthetic dataset into
    ``buf`` (bf16 [B, H, W, Cp], channels >= C zeroed) and ``labels`` (int64 [B])."""
    B, H, W, Cp = buf.shape
    assert buf.dtype == torch.bfloat16 and buf.is_contiguous() and Cp % 4 == 0 and C <= Cp
    assert idx.dtype == torch.int64 and idx.numel() == B and idx.device == buf.device
    assert labels.dtype == torch.int64 and labels.numel() == B and labels.device == buf.device
    _chk(_load().pdt_synth_images_bf16(_p(buf), _p(idx), B, H * W, C, Cp, seed & 0xFFFFFFFF, _p(labels),
                                       int(num_classes), _s()), "synth_images")


_ERASE_MODES = {"const": 0, "pixel": 1}


def _is(t, dtype, shape, src):
    return t is not None and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() \
        and t.device == src.device


def _crop_resize_norm(src, idx, box, mixed, erased, mode, out, mean, std):
    """The checks and the call behind the three functions below: ``mixed`` None or ``(pidx, pbox,
    rect, w_own)``, ``erased`` None or ``(erect, ekey)`` with its ``mode``."""
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()
    assert out.dtype == torch.bfloat16 and out.dim() == 4 and out.is_contiguous() and out.device == src.device
    B, S, S2, Cp = out.shape
    assert S == S2 and Cp % 4 == 0 and B > 0
    assert _is(box, torch.int32, (B, 5), src)
    assert _is(idx, torch.int64, (B,), src) if idx is not None else src.shape[0] >= B
    pidx = pbox = rect = w_own = None
    if mixed is not None:
        pidx, pbox, rect, w_own = mixed
        assert _is(pidx, torch.int64, (B,), src) and _is(pbox, torch.int32, (B, 5), src)
        assert _is(rect, torch.int32, (B, 4), src) and _is(w_own, torch.float32, (B,), src)
    if erased is not None:
        erect, ekey = erased
        assert erect.dim() == 3 and 1 <= erect.shape[1] <= 8 and _is(erect, torch.int32, (B, erect.shape[1], 4), src)
        assert _is(ekey, torch.int32, (B,), src)
        assert mode in _ERASE_MODES, mode
    assert len(mean) == 3 and len(std) == 3 and all(float(s) > 0 for s in std)
    m = (c_float * 3)(*[float(v) for v in mean])
    inv = (c_float * 3)(*[1.0 / float(v) for v in std])
    n, Hs, Ws, _ = src.shape
    head = (_p(src), Hs, Ws, _p(idx), _p(box))
    tail = (_p(out), B, S, Cp, ctypes.addressof(m), ctypes.addressof(inv), _s())
    if erased is not None:
        _chk(_load().pdt_crop_resize_norm_erase_u8_bf16(*head, _p(pidx), _p(pbox), _p(rect), _p(w_own), _p(erect),
                                                        int(erect.shape[1]), _p(ekey), _ERASE_MODES[mode], *tail),
             "crop_resize_norm_erase")
    elif mixed is not None:
        _chk(_load().pdt_crop_resize_norm_mix_u8_bf16(*head, _p(pidx), _p(pbox), _p(rect), _p(w_own), *tail),
             "crop_resize_norm_mix")
    else:
        _chk(_load().pdt_crop_resize_norm_u8_bf16(*head, *tail), "crop_resize_norm")


def crop_resize_normalize(src, idx, box, out, mean, std):
    """The packed-image input pipeline in one launch (``csrc/image_aug.hip``): output ``b`` is the
    crop ``box[b] = (y0, x0, h, w, flip)`` of stored image ``idx[b]`` (``idx`` None: image ``b``),
    resized bilinearly (``align_corners=False``, no antialias) to ``S x S``, flipped horizontally
    when ``flip``, and normalized ``(v / 255 - mean[c]) / std[c]``.

    ``src`` uint8 [n, Hs, Ws, 3]; ``idx`` int64 [B] or None; ``box`` int32 [B, 5]; ``out`` bf16
    [B, S, S, Cp] (channel 3 is written as 0); all on one device. ``mean`` / ``std``: 3 floats.
    The kernel trusts the boxes and indices: validate them on the host (``data/packed.py``)."""
    _crop_resize_norm(src, idx, box, None, None, None, out, mean, std)


def crop_resize_normalize_mix(src, idx, box, pidx, pbox, rect, w_own, out, mean, std):
    """:func:`crop_resize_normalize` with Mixup / CutMix in the same launch: output ``b`` is mixed
    with its partner's augmented view -- the crop ``pbox[b]`` (the partner's own box and flip) of
    stored image ``pidx[b]``. Inside the rectangle ``rect[b] = (y0, x0, y1, x1)`` (half-open,
    output coordinates; empty when ``y0 == y1`` or ``x0 == x1``) a pixel is the partner's; outside
    it is the own one when ``w_own[b] == 1``, else ``w_own * own + (1 - w_own) * partner``, formed
    in fp32 before the normalization and the one rounding to bf16.

    ``pidx`` int64 [B]; ``pbox`` int32 [B, 5]; ``rect`` int32 [B, 4] inside ``[0, S]^2``; ``w_own``
    float32 [B] in [0, 1]; the rest as in :func:`crop_resize_normalize`. The kernel trusts them
    all: validate on the host (``data/packed.py``: ``validate_boxes``, ``validate_mix``)."""
    _crop_resize_norm(src, idx, box, (pidx, pbox, rect, w_own), None, None, out, mean, std)


def crop_resize_normalize_erase(src, idx, box, mixed, erect, ekey, mode, out, mean, std):
    """:func:`crop_resize_normalize` (``mixed`` None) or :func:`crop_resize_normalize_mix`
    (``mixed = (pidx, pbox, rect, w_own)``) with Random Erasing in the same launch: a pixel of output
    ``b`` inside any of its rectangles ``erect[b, r] = (y0, x0, y1, x1)`` (half-open, output
    coordinates; empty when ``y0 == y1`` or ``x0 == x1``) loads nothing and is +0 (``mode``
    ``"const"``) or an N(0, 1) draw per channel (``"pixel"``: a counter-based hash of ``ekey[b]``,
    the pixel and the channel, Box-Muller, rounded once to bf16 -- the formula in
    ``csrc/image_aug.hip``). Every other pixel, and the pad channel, are the bits the call without
    erasing writes.

    ``erect`` int32 [B, R, 4] inside ``[0, S]^2``, R in 1..8; ``ekey`` int32 [B] holding the uint32
    keys' bits; the rest as in the two functions above. The kernel trusts them all: validate on the
    host (``data/packed.py``: ``validate_erase``)."""
    _crop_resize_norm(src, idx, box, mixed, (erect, ekey), mode, out, mean, std)


def synthetic_images(shape, dtype, device, seed=0, channels_last=True):
    n, c, h, w = shape
    if channels_last:
        x = torch.empty(shape, dtype=torch.bfloat16, device=device, memory_format=torch.channels_last)
    else:
        x = torch.empty(shape, dtype=torch.bfloat16, device=device)
    fill_uniform_(x, seed)
    return x if dtype == torch.bfloat16 else x.to(dtype)
