"""Real images from a *packed image set*, augmented on the device.

A packed image set is a directory of three files (``scripts/pack_images.py`` builds one per
split from a class-per-folder image tree; decoding happens once, offline):

* ``images.npy`` -- uint8 ``[N, Hs, Ws, 3]``, C order, RGB, one stored size per set
  (e.g. 256 x 256); opened with ``np.load(..., mmap_mode="r")``.
* ``labels.npy`` -- int64 ``[N]``.
* ``meta.json`` -- ``num_classes``, optional ``classes`` (names), optional ``mean`` / ``std``.

:class:`PackedImageLoader` (``train_loader.type``) is sharded like
:class:`~.synthetic.SyntheticImageNetLoader` (``DistributedSampler`` in training,
``set_epoch`` reshuffles; the unpadded :class:`~.samplers.EvalShardSampler` in evaluation)
and MI355X-first like it: the host moves indices, crop boxes and at most raw uint8 pixels,
and one HIP launch (``csrc/image_aug.hip``) turns the batch's stored images into the
random-resized-cropped (training) or center-cropped (evaluation), flipped, normalized bf16
batch in the zero-padded 4-channel NHWC storage the space-to-depth stem reads in place
(``pdt_nhwc_pad``). Three modes:

* **resident** -- ``images.npy`` is uploaded to HBM once as uint8; a batch is one small H2D
  copy (indices, labels, boxes) and one launch that gathers by index.
* **staged** -- one background thread runs up to ``prefetch`` batches ahead: it gathers the
  batch's images from the memmap (sorted indices) into a ring of pinned buffers and copies
  them to a device staging ring on a side stream; the consumer makes its stream wait on the
  copy's event (no host sync) and launches the same kernel.
* **torch** -- CPU device, no native library, or a non-bf16 dtype: the same math in torch
  (per-sample crop + ``F.interpolate`` in fp32).

The augmentation parameters are counter-based: a sample's crop box and flip are a pure
function of ``(seed, epoch, global sample index)`` -- independent of world size, batch size
and the sample's position in the batch.

**Mixup / CutMix** (``mixup_alpha``, ``cutmix_alpha``, ``mix_prob``, ``mix_switch_prob``,
``mix_mode``; off by default, training only) follow timm's ``Mixup``: the batch is paired with
its reverse (``partner[b] = B-1-b``), and the partner's *augmented view* (its own crop box and
flip) is pasted into a rectangle (CutMix) or blended in with weight ``1 - w_own`` (Mixup). The
blend happens inside the same launch, on the fp32 0..255 values before normalization and the
single bf16 rounding: there is no second batch buffer and no extra pass. The loader then yields
``(images, MixedTarget(label_a, label_b, lam))`` -- two labels and one weight per row, what the
paired-target cross-entropy (``csrc/xent.hip``) consumes; a dense soft-target matrix is never
built. Unlike the crop boxes, the mix depends on batch composition: the pairing does by
construction, and the draws (:func:`mix_params`) are keyed by ``(seed, epoch, first global
sample index of the batch)`` -- reproducible and independent of which thread computes them, but
not of batch size or world size. Nobody has trained a model to convergence with this recipe
here; what is tested is that the mixed batch and the loss are the ones the parameters describe.

**Random Erasing** (``re_prob``, ``re_mode``, ``re_count``, ``re_area``, ``re_aspect``; off by
default, training only) follows timm's ``RandomErasing``: with probability ``re_prob`` a sample
gets ``re_count`` rectangles (:func:`random_erasing_rects`), and every output element inside one
is replaced -- by an independent N(0, 1) draw in normalized space (``"pixel"``) or by +0
(``"const"``). It comes last, after Mixup / CutMix, and leaves the target alone. It is a decision
at the kernel's final store in the same launch (the ERASE instantiations of
``csrc/image_aug.hip``): an erased pixel loads no taps, and there is no pass over the batch
afterwards. Like the crop boxes, rectangles and fill are counter-based -- a pure function of
``(seed, epoch, global sample index)`` and, for the fill, ``(oy, ox, channel)``, from a hash
stream salted apart from the crop-box draws -- so they do not depend on batch size, world size,
position in the batch or loader mode, and switching erasing on changes no crop box, flip or mix
parameter. With ``re_prob = 0`` the loader runs the uploads and entry points it runs without the
arguments. Untrained here, like the rest of the recipe. Two helpers beside the functions the
loader calls: :func:`u32_bits` (the int32 bit pattern of uint32 values carried in int64, as the
kernel reads the keys) and :func:`erase_noise` (the kernel's draws in float64, which
:func:`erase_images_torch` rounds to fp32).
"""
from __future__ import annotations

import json
import math
import queue
import threading
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DistributedSampler

from ..utils import dist as pdist
from .samplers import EvalShardSampler
from .synthetic import _DTYPES, _M32, _default_device, _hash32

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_PACKER_HINT = "build a packed image set with scripts/pack_images.py"


class PackedImageSet:
    """An opened packed image set: ``images`` (uint8 memmap [N, Hs, Ws, 3]), ``labels``
    (int64 ndarray [N]), ``num_classes``, ``classes`` (names or None), ``mean`` / ``std``
    (3-tuples or None), ``meta`` (the raw ``meta.json``)."""

    def __init__(self, images, labels, meta):
        self.images = images
        self.labels = labels
        self.meta = meta
        self.num_classes = int(meta["num_classes"])
        self.classes = meta.get("classes")
        self.mean = tuple(float(v) for v in meta["mean"]) if meta.get("mean") is not None else None
        self.std = tuple(float(v) for v in meta["std"]) if meta.get("std") is not None else None

    def __len__(self):
        return int(self.images.shape[0])

    def __getitem__(self, i):
        return torch.from_numpy(np.array(self.images[int(i)])), int(self.labels[int(i)])

    @property
    def stored_size(self):
        return int(self.images.shape[1]), int(self.images.shape[2])


def open_packed(data_dir) -> PackedImageSet:
    """Open and validate the packed image set in ``data_dir``."""
    d = Path(data_dir)
    if not d.is_dir():
        raise FileNotFoundError(f"packed image set not found: {d} is not a directory -- {_PACKER_HINT}")
    for name in ("images.npy", "labels.npy", "meta.json"):
        if not (d / name).is_file():
            raise FileNotFoundError(f"packed image set {d} has no {name} -- {_PACKER_HINT}")
    images = np.load(d / "images.npy", mmap_mode="r")
    labels = np.load(d / "labels.npy")
    meta = json.loads((d / "meta.json").read_text())
    if images.dtype != np.uint8:
        raise ValueError(f"{d}/images.npy: dtype must be uint8, got {images.dtype}")
    if images.ndim != 4:
        raise ValueError(f"{d}/images.npy: shape must be [N, H, W, 3], got rank {images.ndim}")
    if images.shape[3] != 3:
        raise ValueError(f"{d}/images.npy: images must have 3 channels (RGB), got {images.shape[3]}")
    if not images.flags["C_CONTIGUOUS"] or images.shape[0] == 0:
        raise ValueError(f"{d}/images.npy: must be a non-empty C-order array")
    if labels.dtype != np.int64 or labels.ndim != 1:
        raise ValueError(f"{d}/labels.npy: must be int64 [N], got {labels.dtype} rank {labels.ndim}")
    if labels.shape[0] != images.shape[0]:
        raise ValueError(f"{d}: {images.shape[0]} images but {labels.shape[0]} labels")
    if not isinstance(meta, dict) or "num_classes" not in meta:
        raise ValueError(f"{d}/meta.json: must be an object with num_classes")
    nc = int(meta["num_classes"])
    if labels.min() < 0 or labels.max() >= nc:
        raise ValueError(f"{d}/labels.npy: labels must lie in [0, num_classes={nc})")
    for key in ("mean", "std"):
        if meta.get(key) is not None and len(meta[key]) != 3:
            raise ValueError(f"{d}/meta.json: {key} must have 3 entries")
    return PackedImageSet(images, labels, meta)


# ----------------------------------------------------------------------------- boxes
_TRIES = 10
_DRAWS = 4 * _TRIES + 1  # (area, ratio, y, x) per try, then the flip


def _sample_state(indices, epoch, seed) -> torch.Tensor:
    """uint32 (in int64) [B]: the crop-box stream's state of each sample, a hash of (seed, epoch, i)."""
    idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
    s = _hash32(((idx & _M32) * 0x9E3779B9 & _M32) ^ (int(seed) & _M32))
    return _hash32(s ^ ((int(epoch) & _M32) * 0x85EBCA6B & _M32) ^ ((idx >> 32) & _M32))


def _draws(state, j) -> torch.Tensor:
    """float64 [B, len(j)] in [0, 1): draws ``j`` (int64, from 1) of the streams with ``state`` [B]."""
    h = _hash32(((j * 0xC2B2AE35) & _M32)[None, :] ^ state[:, None])
    return (h >> 8).to(torch.float64) / 16777216.0


def _uniforms(indices, epoch, seed) -> torch.Tensor:
    """float64 [B, _DRAWS] in [0, 1): draw j of sample i is a hash of (seed, epoch, i, j)."""
    return _draws(_sample_state(indices, epoch, seed), torch.arange(1, _DRAWS + 1, dtype=torch.int64))


def random_resized_crop_boxes(indices, epoch, seed, Hs, Ws, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                              hflip=0.5) -> torch.Tensor:
    """int32 [B, 5] = (y0, x0, h, w, flip) for global sample ``indices``: torchvision's
    RandomResizedCrop on an ``Hs x Ws`` image -- up to 10 tries of area = Hs Ws U(scale), a
    log-uniform aspect ratio, ``w = round(sqrt(area r))``, ``h = round(sqrt(area / r))``,
    accepted when the box fits, then a uniform offset; otherwise the center crop clipped to
    the ratio bounds -- plus a horizontal flip with probability ``hflip``. Each row is a pure
    function of ``(seed, epoch, index)``."""
    Hs, Ws = int(Hs), int(Ws)
    u = _uniforms(indices, epoch, seed)
    B = u.shape[0]
    t = u[:, :4 * _TRIES].reshape(B, _TRIES, 4)
    area = Hs * Ws * (scale[0] + t[..., 0] * (scale[1] - scale[0]))
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    ar = torch.exp(lr0 + t[..., 1] * (lr1 - lr0))
    w = torch.round(torch.sqrt(area * ar)).to(torch.int64)
    h = torch.round(torch.sqrt(area / ar)).to(torch.int64)
    ok = (w > 0) & (w <= Ws) & (h > 0) & (h <= Hs)
    first = torch.argmax(ok.to(torch.int64), dim=1)  # first accepted try (0 when none is)
    rows = torch.arange(B)
    w, h = w[rows, first], h[rows, first]
    y0 = torch.floor(t[rows, first, 2] * (Hs - h + 1).clamp(min=1)).to(torch.int64)
    x0 = torch.floor(t[rows, first, 3] * (Ws - w + 1).clamp(min=1)).to(torch.int64)
    # fallback: the center crop with the aspect ratio clipped to the bounds
    in_ratio = Ws / Hs
    if in_ratio < ratio[0]:
        fw, fh = Ws, int(round(Ws / ratio[0]))
    elif in_ratio > ratio[1]:
        fh, fw = Hs, int(round(Hs * ratio[1]))
    else:
        fw, fh = Ws, Hs
    fw, fh = min(max(fw, 1), Ws), min(max(fh, 1), Hs)
    none = ~ok.any(dim=1)
    h = torch.where(none, torch.full_like(h, fh), h)
    w = torch.where(none, torch.full_like(w, fw), w)
    y0 = torch.where(none, torch.full_like(y0, (Hs - fh) // 2), y0)
    x0 = torch.where(none, torch.full_like(x0, (Ws - fw) // 2), x0)
    flip = (u[:, -1] < float(hflip)).to(torch.int64)
    return torch.stack([y0, x0, h, w, flip], dim=1).to(torch.int32)


def center_crop_boxes(B, Hs, Ws, crop_fraction=0.875) -> torch.Tensor:
    """int32 [B, 5]: the centered ``round(Hs f) x round(Ws f)`` box, no flip (evaluation). A
    256 store with ``f = 0.875`` gives the 224 x 224 box at (16, 16): at image size 224 the
    resize is the identity."""
    h = min(max(int(round(Hs * crop_fraction)), 1), int(Hs))
    w = min(max(int(round(Ws * crop_fraction)), 1), int(Ws))
    row = torch.tensor([(Hs - h) // 2, (Ws - w) // 2, h, w, 0], dtype=torch.int32)
    return row.repeat(int(B), 1)


def validate_boxes(box, Hs, Ws):
    """Raise unless every box lies inside the ``Hs x Ws`` image with ``h, w >= 1`` (the
    kernel trusts its boxes)."""
    b = box.to(torch.int64)
    y0, x0, h, w = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    bad = (y0 < 0) | (x0 < 0) | (h < 1) | (w < 1) | (y0 + h > Hs) | (x0 + w > Ws)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"crop box {box[i].tolist()} of batch entry {i} is outside the {Hs}x{Ws} image")


def validate_indices(indices, n):
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise IndexError(f"sample index out of range for a packed image set of {n} images: "
                         f"[{int(idx.min())}, {int(idx.max())}]")
    return idx


# ----------------------------------------------------------------------------- mixing
class MixedTarget(NamedTuple):
    """The target of a mixed batch: row ``b`` is ``lam[b]`` of class ``label_a[b]`` and
    ``1 - lam[b]`` of class ``label_b[b]``. ``label_a`` / ``label_b`` int64 [B], ``lam`` float32
    [B], on the loader's device. ``fused.softmax_cross_entropy`` takes it in place of labels."""
    label_a: torch.Tensor
    label_b: torch.Tensor
    lam: torch.Tensor


_MIX_MODES = ("batch", "elem")
_M64 = (1 << 64) - 1


def check_mix_args(mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, mix_mode):
    """Raise ValueError on a negative alpha, a probability outside [0, 1] or an unknown mode."""
    for name, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
        if not (float(v) >= 0.0) or math.isinf(float(v)):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    for name, v in (("mix_prob", mix_prob), ("mix_switch_prob", mix_switch_prob)):
        if not (0.0 <= float(v) <= 1.0):
            raise ValueError(f"{name} must lie in [0, 1], got {v!r}")
    if mix_mode not in _MIX_MODES:
        raise ValueError(f"mix_mode must be one of {_MIX_MODES}, got {mix_mode!r}")


def mix_params(indices, epoch, seed, S, mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, mix_switch_prob=0.5,
               mix_mode="batch"):
    """Mixup / CutMix parameters of the batch of global sample ``indices`` at output size ``S``
    (timm's ``Mixup``), as host tensors ``(partner, w_own, rect, lam)``:

    * ``partner`` int64 [B] = ``B-1-b``: the batch is paired with its reverse (the middle element
      of an odd batch, and a batch of 1, pair with themselves);
    * ``w_own`` float32 [B]: the weight of the sample's own pixels outside the rectangle;
    * ``rect`` int32 [B, 4] = ``(y0, x0, y1, x1)``, half-open, output coordinates: the partner's
      pixels are pasted there (empty when ``y0 == y1`` or ``x0 == x1``);
    * ``lam`` float32 [B]: the own label's share in the loss.

    With probability ``mix_prob`` a draw mixes (otherwise ``lam = w_own = 1``, empty rectangle);
    the method is CutMix with probability ``mix_switch_prob`` when both alphas are positive, else
    whichever alpha is positive; ``lam0 ~ Beta(alpha, alpha)``. Mixup: ``w_own = lam = lam0``.
    CutMix: a ``int(S sqrt(1 - lam0))``-sided square around a uniform centre, clipped to the
    image, ``w_own = 1`` and ``lam = 1 - clipped area / S^2``. ``"batch"`` draws once and
    broadcasts, ``"elem"`` draws per sample.

    A pure function of its arguments: one Philox stream keyed by ``(seed, epoch, indices[0])``,
    drawn vectorised in a fixed order."""
    check_mix_args(mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, mix_mode)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    B, S = int(idx.size), int(S)
    if B == 0 or S <= 0:
        raise ValueError("mix_params needs a non-empty batch and S >= 1")
    ma, ca = float(mixup_alpha), float(cutmix_alpha)
    key = [int(seed) & _M64, ((int(epoch) & _M32) << 32) | (int(idx[0]) & _M32)]
    rng = np.random.Generator(np.random.Philox(key=key))
    n = 1 if mix_mode == "batch" else B
    u_mix, u_switch = rng.random(n), rng.random(n)
    lam_mixup = rng.beta(ma, ma, n) if ma > 0 else np.ones(n)
    lam_cut = rng.beta(ca, ca, n) if ca > 0 else np.ones(n)
    cy, cx = rng.integers(0, S, n), rng.integers(0, S, n)

    mixes = (u_mix < float(mix_prob)) & ((ma > 0) | (ca > 0))
    cut = (u_switch < float(mix_switch_prob)) if (ma > 0 and ca > 0) else np.full(n, ca > 0)
    cut = cut & mixes
    mixup = mixes & ~cut
    side = (S * np.sqrt(1.0 - lam_cut)).astype(np.int64)  # ch = cw = int(S r)
    half = side // 2
    y0, y1 = np.clip(cy - half, 0, S), np.clip(cy + half, 0, S)
    x0, x1 = np.clip(cx - half, 0, S), np.clip(cx + half, 0, S)
    rect = np.where(cut[:, None], np.stack([y0, x0, y1, x1], axis=1), 0).astype(np.int32)
    area = (rect[:, 2] - rect[:, 0]).astype(np.int64) * (rect[:, 3] - rect[:, 1])
    lam = np.where(cut, 1.0 - area / float(S * S), np.where(mixup, lam_mixup, 1.0)).astype(np.float32)
    w_own = np.where(mixup, lam_mixup, 1.0).astype(np.float32)
    if n != B:
        rect, lam, w_own = np.repeat(rect, B, axis=0), np.repeat(lam, B), np.repeat(w_own, B)
    partner = np.arange(B - 1, -1, -1, dtype=np.int64)
    return (torch.from_numpy(partner), torch.from_numpy(np.ascontiguousarray(w_own)),
            torch.from_numpy(np.ascontiguousarray(rect)), torch.from_numpy(np.ascontiguousarray(lam)))


def validate_mix(partner, w_own, rect, lam, S):
    """Raise unless every rectangle lies inside ``[0, S]^2`` with ``y0 <= y1`` and ``x0 <= x1``,
    ``0 <= w_own <= 1``, ``0 <= lam <= 1`` and every partner lies in ``[0, B)`` (the kernel
    trusts what it is given)."""
    B = int(partner.shape[0])
    if tuple(rect.shape) != (B, 4) or tuple(w_own.shape) != (B,) or tuple(lam.shape) != (B,):
        raise ValueError(f"mix parameters of a batch of {B}: shapes {tuple(w_own.shape)}, {tuple(rect.shape)}, "
                         f"{tuple(lam.shape)}")
    r = rect.to(torch.int64)
    bad = (r[:, 0] < 0) | (r[:, 1] < 0) | (r[:, 2] > S) | (r[:, 3] > S) | (r[:, 0] > r[:, 2]) | (r[:, 1] > r[:, 3])
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"cut rectangle {rect[i].tolist()} of batch entry {i} is outside the {S}x{S} output")
    for name, v in (("w_own", w_own), ("lam", lam)):
        bad = ~((v >= 0) & (v <= 1))  # NaN is bad too
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            raise ValueError(f"{name} = {float(v[i])} of batch entry {i} is outside [0, 1]")
    bad = (partner < 0) | (partner >= B)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"partner {int(partner[i])} of batch entry {i} is outside the batch of {B}")


def mix_images_torch(x, partner, w_own, rect):
    """The mix in torch on normalized fp32 views ``x`` [B, 3, S, S]: Mixup's blend
    ``w x + (1 - w) x[partner]`` outside the rectangle, the partner's pixels inside it."""
    B, _, S, _ = x.shape
    xp = x[partner]
    w = w_own.to(torch.float32).view(B, 1, 1, 1)
    out = torch.where(w == 1, x, w * x + (1 - w) * xp)
    yy = torch.arange(S).view(1, S, 1)
    xx = torch.arange(S).view(1, 1, S)
    r = rect.to(torch.int64)
    inside = ((yy >= r[:, 0].view(B, 1, 1)) & (yy < r[:, 2].view(B, 1, 1))
              & (xx >= r[:, 1].view(B, 1, 1)) & (xx < r[:, 3].view(B, 1, 1)))
    return torch.where(inside[:, None], xp, out)


# ----------------------------------------------------------------------------- erasing
_ERASE_MODES = ("pixel", "const")
_ERASE_SALT = 0x45524153  # "ERAS": the erase stream of a sample is keyed apart from its crop-box stream
_RE_AREA = (0.02, 1 / 3)
_RE_ASPECT = (0.3, 1 / 0.3)


def check_erase_args(re_prob, re_mode, re_count, re_area, re_aspect):
    """Raise ValueError on a probability outside [0, 1], an unknown mode, ``re_count`` outside 1..8,
    a non-positive or reversed area or aspect range, or an area maximum above 1."""
    if not (0.0 <= float(re_prob) <= 1.0):
        raise ValueError(f"re_prob must lie in [0, 1], got {re_prob!r}")
    if re_mode not in _ERASE_MODES:
        raise ValueError(f"re_mode must be one of {_ERASE_MODES}, got {re_mode!r}")
    if isinstance(re_count, bool) or not isinstance(re_count, (int, np.integer)) or not (1 <= int(re_count) <= 8):
        raise ValueError(f"re_count must be an integer in 1..8, got {re_count!r}")
    for name, v in (("re_area", re_area), ("re_aspect", re_aspect)):
        if len(v) != 2 or not (0.0 < float(v[0]) <= float(v[1])) or math.isinf(float(v[1])):
            raise ValueError(f"{name} must be a (min, max) pair with 0 < min <= max, got {v!r}")
    if float(re_area[1]) > 1.0:
        raise ValueError(f"re_area's maximum must be at most 1 (a fraction of the output), got {re_area!r}")


def _erase_state(indices, epoch, seed) -> torch.Tensor:
    """uint32 (in int64) [B]: the erase stream's state of each sample -- the crop-box stream's
    state (:func:`_sample_state`), hashed once more with a salt."""
    return _hash32(_sample_state(indices, epoch, seed) ^ _ERASE_SALT)


def erase_keys(indices, epoch, seed) -> torch.Tensor:
    """The noise key of each global sample in ``indices``: uint32 values in int64 [B] (draw 0 of
    the sample's erase stream; the rectangles use draws 1...). A pure function of ``(seed, epoch,
    index)``."""
    return _hash32(_erase_state(indices, epoch, seed))


def random_erasing_rects(indices, epoch, seed, S, re_prob=0.25, re_count=1, re_area=_RE_AREA,
                         re_aspect=_RE_ASPECT) -> torch.Tensor:
    """int32 [B, re_count, 4] = (y0, x0, y1, x1), half-open, in the ``S x S`` output: timm's
    ``RandomErasing`` boxes of global sample ``indices``. With probability ``1 - re_prob`` a sample
    has no rectangle; otherwise each of its ``re_count`` rectangles makes up to 10 tries of area =
    ``S S U(re_area) / re_count`` and a log-uniform aspect ``r``, ``h = round(sqrt(area r))``,
    ``w = round(sqrt(area / r))``, accepted when ``h < S`` and ``w < S``, then a uniform corner such
    that it lies inside the output. A rectangle with no accepted try (or of no pixel) is all zeros.
    Each row is a pure function of ``(seed, epoch, index)``: draw ``j`` of the sample's erase stream
    is ``hash32(j * 0xC2B2AE35 ^ state)``, ``j = 1`` the decision, then (area, aspect, y, x) per try."""
    check_erase_args(re_prob, "pixel", re_count, re_area, re_aspect)
    S, R = int(S), int(re_count)
    if S <= 0:
        raise ValueError("random_erasing_rects needs S >= 1")
    s = _erase_state(indices, epoch, seed)
    B = s.shape[0]
    u = _draws(s, torch.arange(1, 2 + 4 * _TRIES * R, dtype=torch.int64))
    erased = u[:, 0] < float(re_prob)
    t = u[:, 1:].reshape(B, R, _TRIES, 4)
    area = S * S * (float(re_area[0]) + t[..., 0] * (float(re_area[1]) - float(re_area[0]))) / R
    lr0, lr1 = math.log(float(re_aspect[0])), math.log(float(re_aspect[1]))
    ar = torch.exp(lr0 + t[..., 1] * (lr1 - lr0))
    h = torch.round(torch.sqrt(area * ar)).to(torch.int64)
    w = torch.round(torch.sqrt(area / ar)).to(torch.int64)
    ok = (h < S) & (w < S)
    first = torch.argmax(ok.to(torch.int64), dim=2, keepdim=True)  # first accepted try (0 when none is)
    h, w = torch.gather(h, 2, first)[..., 0], torch.gather(w, 2, first)[..., 0]
    y0 = torch.floor(torch.gather(t[..., 2], 2, first)[..., 0] * (S - h + 1)).to(torch.int64)
    x0 = torch.floor(torch.gather(t[..., 3], 2, first)[..., 0] * (S - w + 1)).to(torch.int64)
    keep = erased[:, None] & ok.any(dim=2) & (h > 0) & (w > 0)
    rect = torch.stack([y0, x0, y0 + h, x0 + w], dim=2)
    return torch.where(keep[..., None], rect, torch.zeros_like(rect)).to(torch.int32)


def validate_erase(rects, S):
    """Raise unless ``rects`` is int32 [B, R, 4] with R in 1..8 and every rectangle lies inside
    ``[0, S]^2`` with ``y0 <= y1`` and ``x0 <= x1`` (the kernel trusts what it is given)."""
    if rects.dim() != 3 or rects.shape[2] != 4 or not (1 <= rects.shape[1] <= 8):
        raise ValueError(f"erase rectangles must be [B, 1..8, 4], got {tuple(rects.shape)}")
    r = rects.to(torch.int64)
    bad = ((r[..., 0] < 0) | (r[..., 1] < 0) | (r[..., 2] > S) | (r[..., 3] > S) | (r[..., 0] > r[..., 2])
           | (r[..., 1] > r[..., 3]))
    if bool(bad.any()):
        i, k = (int(v) for v in torch.nonzero(bad)[0])
        raise ValueError(f"erase rectangle {rects[i, k].tolist()} ({k}) of batch entry {i} is outside the "
                         f"{S}x{S} output")


def u32_bits(keys) -> torch.Tensor:
    """int32 tensor with the bits of uint32 values carried in int64 (what the kernel reads)."""
    k = torch.as_tensor(keys, dtype=torch.int64)
    return torch.where(k >= 1 << 31, k - (1 << 32), k).to(torch.int32)


def erase_noise(keys, pos, S):
    """float64 N(0, 1) draws of the kernel's noise (``csrc/image_aug.hip``) at ``pos`` = int64
    [n, 3] rows ``(b, oy, ox)``: [n, 3], one column per channel. ``keys``: uint32 in int64 [B]."""
    kq = _hash32(keys.to(torch.int64)[pos[:, 0]] ^ (((pos[:, 1] * S + pos[:, 2]) & _M32) * 0x9E3779B9 & _M32))
    c = torch.arange(3, dtype=torch.int64)
    h1 = _hash32(kq[:, None] ^ ((2 * c + 1) * 0x85EBCA6B & _M32)[None, :])
    h2 = _hash32(kq[:, None] ^ ((2 * c + 2) * 0x85EBCA6B & _M32)[None, :])
    u1 = ((h1 >> 8) + 1).to(torch.float64) / 16777216.0
    t = (h2 >> 8).to(torch.float64) / 8388608.0
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(math.pi * t)


def erase_images_torch(x, rects, keys, mode):
    """The erase in torch on normalized fp32 views ``x`` [B, 3, S, S]: every element inside any of
    the sample's rectangles becomes +0 (``"const"``) or the kernel's N(0, 1) draw for ``(keys[b],
    oy, ox, channel)`` (``"pixel"``), formed in float64 and rounded to fp32."""
    if mode not in _ERASE_MODES:
        raise ValueError(f"re_mode must be one of {_ERASE_MODES}, got {mode!r}")
    B, _, S, _ = x.shape
    r = rects.to(torch.int64).view(B, -1, 1, 1, 4)
    yy = torch.arange(S).view(1, 1, S, 1)
    xx = torch.arange(S).view(1, 1, 1, S)
    inside = ((yy >= r[..., 0]) & (yy < r[..., 2]) & (xx >= r[..., 1]) & (xx < r[..., 3])).any(dim=1)  # [B, S, S]
    out = x.clone()
    if mode == "const":
        return out.masked_fill_(inside[:, None], 0.0)
    pos = torch.nonzero(inside)
    out.permute(0, 2, 3, 1)[inside] = erase_noise(keys, pos, S).to(x.dtype)
    return out


def crop_resize_normalize_torch(images, box, S, mean, std, dtype=torch.float32):
    """The kernel's math in torch: ``images`` uint8 [B, Hs, Ws, 3] -> [B, 3, S, S] ``dtype``
    (computed in fp32): per-sample crop, bilinear ``F.interpolate`` (``align_corners=False``, no
    antialias), horizontal flip, ``(v / 255 - mean) / std``."""
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    out = []
    for img, (y0, x0, h, w, flip) in zip(images, box.tolist()):
        crop = img[y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].to(torch.float32)
        r = F.interpolate(crop, size=(S, S), mode="bilinear", align_corners=False, antialias=False)
        if flip:
            r = r.flip(3)
        out.append((r / 255.0 - m) / s)
    return torch.cat(out).to(dtype)


# ----------------------------------------------------------------------------- parameter block
def _param_layout(B, mixing, R):
    """The pinned parameter block of a batch of ``B`` in int32 words: field name -> (word offset,
    word count, dtype, shape). The samples' gather indices, labels and boxes; with ``mixing`` their
    partners' (``pidx`` / ``plabels`` / ``pbox``), the cut rectangles, ``w_own`` and ``lam``; with
    ``R`` > 0 erase rectangles per sample, those and one key per sample behind everything else. The
    int64 vectors come first, so they are 8-byte aligned for any ``B``."""
    fields = [("kidx", torch.int64, (B,)), ("labels", torch.int64, (B,))]
    if mixing:
        fields += [("pidx", torch.int64, (B,)), ("plabels", torch.int64, (B,))]
    fields.append(("box", torch.int32, (B, 5)))
    if mixing:
        fields += [("pbox", torch.int32, (B, 5)), ("rect", torch.int32, (B, 4)), ("w_own", torch.float32, (B,)),
                   ("lam", torch.float32, (B,))]
    if R:
        fields += [("erect", torch.int32, (B, R, 4)), ("ekey", torch.int32, (B,))]
    layout, off = {}, 0
    for name, dtype, shape in fields:
        words = math.prod(shape) * (2 if dtype == torch.int64 else 1)
        layout[name] = (off, words, dtype, shape)
        off += words
    return layout


def _block_views(buf, layout):
    """The fields of ``layout`` as views into the int32 block ``buf``."""
    return {name: buf[off:off + n].view(dtype).view(shape) for name, (off, n, dtype, shape) in layout.items()}


# ----------------------------------------------------------------------------- loader
class PackedImageLoader:
    """Config-facing loader over a packed image set (see the module docstring).

    Yields ``(images [B, 3, S, S], labels int64 [B])`` on ``device`` -- with Mixup / CutMix
    switched on (``mixup_alpha`` / ``cutmix_alpha`` > 0 and ``training``), ``(images,
    MixedTarget)``. Random Erasing (``re_prob`` > 0 and ``training``) changes pixels only, never
    the target. On the native path
    (CUDA device, kernel library present, bf16, ``channels_last``) ``images`` is a view into
    bf16 ``[B, S, S, 4]`` tagged ``pdt_nhwc_pad = 4``; otherwise the torch path returns
    ``dtype`` (``channels_last`` strides when asked).

    ``mean`` / ``std``: the arguments, else ``meta.json``'s, else the ImageNet constants.
    ``resident``: True, False or ``"auto"`` (resident when ``images.npy`` is at most
    ``resident_limit_gb``). ``num_workers`` is accepted and ignored: there are no worker
    processes."""

    def __init__(self, data_dir, batch_size, training=True, image_size=224, shuffle=True, seed=0,
                 scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), hflip=0.5, crop_fraction=0.875, mean=None, std=None,
                 resident="auto", resident_limit_gb=16, prefetch=2, dtype=None, channels_last=True, device=None,
                 num_workers=0, mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, mix_switch_prob=0.5,
                 mix_mode="batch", re_prob=0.0, re_mode="pixel", re_count=1, re_area=_RE_AREA, re_aspect=_RE_ASPECT):
        check_mix_args(mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, mix_mode)
        check_erase_args(re_prob, re_mode, re_count, re_area, re_aspect)
        self.dataset = open_packed(data_dir)
        ds = self.dataset
        self.batch_size = int(batch_size)
        self.training = bool(training)
        self.image_size = int(image_size)
        self.seed = int(seed)
        self.scale, self.ratio, self.hflip = tuple(scale), tuple(ratio), float(hflip)
        self.crop_fraction = float(crop_fraction)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.mix_switch_prob, self.mix_mode = float(mix_prob), float(mix_switch_prob), mix_mode
        # samples are mixed in training only, and only when a method is switched on
        self.mixing = bool(training) and (self.mixup_alpha > 0 or self.cutmix_alpha > 0)
        self.re_prob, self.re_mode, self.re_count = float(re_prob), re_mode, int(re_count)
        self.re_area, self.re_aspect = tuple(float(v) for v in re_area), tuple(float(v) for v in re_aspect)
        # samples are erased in training only
        self.erasing = bool(training) and self.re_prob > 0
        self.mean = tuple(mean) if mean is not None else (ds.mean or IMAGENET_MEAN)
        self.std = tuple(std) if std is not None else (ds.std or IMAGENET_STD)
        assert len(self.mean) == 3 and len(self.std) == 3 and all(s > 0 for s in self.std)
        self.device = torch.device(device) if device is not None else _default_device()
        if dtype is None:
            dtype = "bfloat16" if self.device.type == "cuda" else "float32"
        self.dtype = _DTYPES[dtype] if isinstance(dtype, str) else dtype
        self.channels_last = bool(channels_last)
        self.prefetch = max(1, int(prefetch))
        self.epoch = 0

        rank, world = pdist.get_rank(), pdist.get_world_size()
        if self.training:
            self.sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle, seed=self.seed)
        else:
            self.sampler = EvalShardSampler(ds, rank=rank, world_size=world)
        self.n_samples = len(self.sampler)

        if resident not in (True, False, "auto"):
            raise ValueError(f"resident must be true, false or 'auto', got {resident!r}")
        self.native = self._native()
        if not self.native:
            self.mode = "torch"
        elif resident is True or (resident == "auto" and ds.images.nbytes <= float(resident_limit_gb) * 2 ** 30):
            self.mode = "resident"
        else:
            self.mode = "staged"
        self._src = None        # resident: the whole set on the device
        self._ring = None       # staged: [(pinned, device)] slots
        self._side = None
        self._copied = None
        self._stage_thread = None  # staged: the pass under way (the ring serves one at a time)

    # ------------------------------------------------------------------ surface
    def _native(self) -> bool:
        if self.device.type != "cuda" or self.dtype != torch.bfloat16 or not self.channels_last:
            return False
        from ..ops import native_ops
        return native_ops.available()

    def __len__(self):
        return math.ceil(self.n_samples / self.batch_size)

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)
        self.sampler.set_epoch(self.epoch)

    def _index_batches(self):
        idx = list(self.sampler)
        return [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]

    def boxes(self, indices, epoch=None) -> torch.Tensor:
        """The validated crop boxes (int32 [B, 5], host) of global sample ``indices`` in ``epoch``
        (default: the current one)."""
        Hs, Ws = self.dataset.stored_size
        if self.training:
            box = random_resized_crop_boxes(indices, self.epoch if epoch is None else epoch, self.seed, Hs, Ws,
                                            self.scale, self.ratio, self.hflip)
        else:
            box = center_crop_boxes(len(indices), Hs, Ws, self.crop_fraction)
        validate_boxes(box, Hs, Ws)
        return box

    def mix(self, indices, epoch=None):
        """The validated mix parameters ``(partner, w_own, rect, lam)`` (host) of the batch of
        global sample ``indices`` in ``epoch`` (default: the current one); None when the loader
        does not mix."""
        if not self.mixing:
            return None
        m = mix_params(indices, self.epoch if epoch is None else epoch, self.seed, self.image_size,
                       self.mixup_alpha, self.cutmix_alpha, self.mix_prob, self.mix_switch_prob, self.mix_mode)
        validate_mix(*m, self.image_size)
        return m

    def erase(self, indices, epoch=None):
        """The validated Random Erasing parameters ``(rects, keys)`` (host: int32 [B, re_count, 4],
        uint32 in int64 [B]) of global sample ``indices`` in ``epoch`` (default: the current one);
        None when the loader does not erase."""
        if not self.erasing:
            return None
        epoch = self.epoch if epoch is None else epoch
        rects = random_erasing_rects(indices, epoch, self.seed, self.image_size, self.re_prob, self.re_count,
                                     self.re_area, self.re_aspect)
        validate_erase(rects, self.image_size)
        return rects, erase_keys(indices, epoch, self.seed)

    def __iter__(self):
        if self.mode == "torch":
            return self._iter_torch()
        if self.mode == "resident":
            return self._iter_resident()
        return self._iter_staged()

    # ------------------------------------------------------------------ torch path
    def _iter_torch(self):
        ds = self.dataset
        fmt = torch.channels_last if self.channels_last else torch.contiguous_format
        epoch = self.epoch  # one pass, one epoch's boxes, whatever set_epoch does meanwhile
        for indices in self._index_batches():
            idx = validate_indices(indices, len(ds))
            box = self.boxes(indices, epoch)
            order = np.argsort(idx, kind="stable")
            imgs = np.empty((len(idx),) + ds.images.shape[1:], dtype=np.uint8)
            imgs[order] = ds.images[idx[order]]
            mix = self.mix(indices, epoch)
            erase = self.erase(indices, epoch)
            y = torch.from_numpy(ds.labels[idx])
            if mix is None and erase is None:
                x = crop_resize_normalize_torch(torch.from_numpy(imgs), box, self.image_size, self.mean, self.std,
                                                self.dtype)
                yield x.contiguous(memory_format=fmt).to(self.device), y.to(self.device)
                continue
            x = crop_resize_normalize_torch(torch.from_numpy(imgs), box, self.image_size, self.mean, self.std)
            target = y.to(self.device)
            if mix is not None:
                partner, w_own, rect, lam = mix
                x = mix_images_torch(x, partner, w_own, rect)  # blend and paste in fp32
                target = MixedTarget(target, y[partner].to(self.device), lam.to(self.device))
            if erase is not None:
                x = erase_images_torch(x, *erase, self.re_mode)  # last, as timm: the target does not change
            yield x.to(self.dtype).contiguous(memory_format=fmt).to(self.device), target

    # ------------------------------------------------------------------ native paths
    def _upload(self, kidx, labels, box, mix, erase):
        """One small H2D copy of one pinned buffer (:func:`_param_layout`): the kernel gather indices,
        labels and boxes; of a mixed batch also those of the partners (``kidx[partner]``: in staged
        mode the partner is read from the same staging slot), the rectangles, ``w_own`` and ``lam``;
        with ``erase`` its rectangles and keys. Returns the target (the labels or a MixedTarget) and
        the device views ``(kidx, box, mixed or None, erased or None)``, ``mixed = (pidx, pbox, rect,
        w_own)`` and ``erased = (erect, ekey)``."""
        kidx = torch.from_numpy(np.ascontiguousarray(kidx, dtype=np.int64))
        labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64))
        vals = {"kidx": kidx, "labels": labels, "box": box}
        if mix is not None:
            partner, w_own, rect, lam = mix
            vals.update(pidx=kidx[partner], plabels=labels[partner], pbox=box[partner], rect=rect, w_own=w_own, lam=lam)
        if erase is not None:
            vals.update(erect=erase[0], ekey=u32_bits(erase[1]))
        layout = _param_layout(len(kidx), mix is not None, 0 if erase is None else erase[0].shape[1])
        host = torch.empty(sum(n for _, n, _, _ in layout.values()), dtype=torch.int32, pin_memory=True)
        for name, view in _block_views(host, layout).items():
            view.copy_(vals[name])
        d = _block_views(host.to(self.device, non_blocking=True), layout)
        target = d["labels"] if mix is None else MixedTarget(d["labels"], d["plabels"], d["lam"])
        mixed = None if mix is None else (d["pidx"], d["pbox"], d["rect"], d["w_own"])
        return target, (d["kidx"], d["box"], mixed, None if erase is None else (d["erect"], d["ekey"]))

    def _batch(self, src, kidx, labels, box, mix, erase=None):
        """Upload one batch's parameters and launch: ``(images, labels or MixedTarget)``."""
        target, args = self._upload(kidx, labels, box, mix, erase)
        return self._launch(src, *args), target

    def _launch(self, src, kidx, box, mixed=None, erased=None):
        from ..ops.native_ops.data import _crop_resize_norm
        B, S = box.shape[0], self.image_size
        buf = torch.empty((B, S, S, 4), dtype=torch.bfloat16, device=self.device)
        _crop_resize_norm(src, kidx, box, mixed, erased, self.re_mode, buf, self.mean, self.std)
        x = buf[..., :3].permute(0, 3, 1, 2)
        x.pdt_nhwc_pad = 4
        return x

    def _resident_src(self):
        if self._src is None:
            im = self.dataset.images
            src = torch.empty(im.shape, dtype=torch.uint8, device=self.device)
            step = max(1, (256 << 20) // max(1, im[0].nbytes))  # 256-MB pieces: host memory stays flat
            for i in range(0, im.shape[0], step):
                src[i:i + step].copy_(torch.from_numpy(np.array(im[i:i + step])))
            self._src = src
        return self._src

    def _iter_resident(self):
        ds = self.dataset
        src = self._resident_src()
        epoch = self.epoch
        for indices in self._index_batches():
            idx = validate_indices(indices, len(ds))
            yield self._batch(src, idx, ds.labels[idx], self.boxes(indices, epoch), self.mix(indices, epoch),
                              self.erase(indices, epoch))

    def _staging_ring(self):
        if self._ring is None:
            shape = (self.batch_size,) + tuple(self.dataset.images.shape[1:])
            self._ring = [(torch.empty(shape, dtype=torch.uint8, pin_memory=True),
                           torch.empty(shape, dtype=torch.uint8, device=self.device))
                          for _ in range(self.prefetch + 1)]
            self._side = torch.cuda.Stream(device=self.device)
            # each slot's last H2D copy, kept across passes: the next pass must not gather into a
            # pinned slot whose copy from the previous pass is still queued (inf_loop starts the
            # next pass at once, and the device runs steps behind the host)
            self._copied = [None] * len(self._ring)
        return self._ring

    def _iter_staged(self):
        ds = self.dataset
        if self._stage_thread is not None and self._stage_thread.is_alive():
            raise RuntimeError("PackedImageLoader (staged): a pass is still under way -- its staging ring "
                               "serves one pass at a time; finish or drop that iterator first")
        ring = self._staging_ring()
        side = self._side
        batches = self._index_batches()
        epoch = self.epoch  # the producer runs ahead: set_epoch must not change a pass under way
        nslots = len(ring)
        ready = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        released = [threading.Event() for _ in range(nslots)]  # the consumer launched on this slot
        release_ev = [None] * nslots                           # ... and this event follows its kernel
        copied = self._copied                                   # the slot's last H2D copy (any pass)
        # the device staging buffers may still be read by kernels of the previous pass
        side.wait_stream(torch.cuda.current_stream(self.device))

        def put(item):
            while not stop.is_set():
                try:
                    ready.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def produce():
            try:
                torch.cuda.set_device(self.device)
                for n, indices in enumerate(batches):
                    slot = n % nslots
                    pinned, staged = ring[slot]
                    if n >= nslots:
                        while not released[slot].wait(0.05):
                            if stop.is_set():
                                return
                        released[slot].clear()
                        side.wait_event(release_ev[slot])  # the device slot's last reader
                    if copied[slot] is not None:
                        # the pinned slot's last copy, of this pass or the one before: a host wait
                        # in this thread only
                        copied[slot].synchronize()
                    idx = validate_indices(indices, len(ds))
                    box = self.boxes(indices, epoch)
                    mix = self.mix(indices, epoch)
                    erase = self.erase(indices, epoch)
                    order = np.argsort(idx, kind="stable")
                    B = len(idx)
                    np.take(ds.images, idx[order], axis=0, out=pinned[:B].numpy())
                    kidx = np.empty(B, dtype=np.int64)
                    kidx[order] = np.arange(B, dtype=np.int64)  # output b reads staged image kidx[b]
                    with torch.cuda.stream(side):
                        staged[:B].copy_(pinned[:B], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    copied[slot] = ev
                    if not put(("batch", slot, B, kidx, ds.labels[idx], box, mix, erase, ev)):
                        return
                put(("end",))
            except BaseException as e:  # re-raised in the consumer
                put(("error", e))

        thread = threading.Thread(target=produce, name="PackedImageLoader-stage", daemon=True)
        thread.start()
        self._stage_thread = thread
        try:
            while True:
                item = ready.get()
                if item[0] == "end":
                    break
                if item[0] == "error":
                    raise item[1]
                _, slot, B, kidx, labels, box, mix, erase, ev = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                x, y = self._batch(ring[slot][1], kidx, labels, box, mix, erase)
                rel = torch.cuda.Event()
                rel.record(cur)
                release_ev[slot] = rel
                released[slot].set()
                yield x, y
        finally:
            stop.set()
            thread.join(timeout=10)
            torch.cuda.current_stream(self.device).wait_stream(side)
