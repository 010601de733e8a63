"""Shared float64 reference and fixtures for the packed-image tests.

reference(): crop -> F.interpolate(bilinear, align_corners=False, no antialias) in float64 ->
horizontal flip -> (v / 255 - mean) / std. Nothing here touches the code under test.
"""
import json

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def reference(images, idx, box, S, mean=MEAN, std=STD):
    """float64 [B, 3, S, S]. images: uint8 [N, Hs, Ws, 3] (tensor or ndarray); idx: the source
    image of each output (None: output b reads image b); box: rows (y0, x0, h, w, flip)."""
    images = torch.as_tensor(np.asarray(images))
    box = [tuple(int(v) for v in r) for r in (box.tolist() if hasattr(box, "tolist") else box)]
    idx = list(range(len(box))) if idx is None else [int(i) for i in idx]
    m = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    out = []
    for i, (y0, x0, h, w, flip) in zip(idx, box):
        crop = images[i, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].to(torch.float64)
        r = F.interpolate(crop, size=(S, S), mode="bilinear", align_corners=False, antialias=False)
        if flip:
            r = torch.flip(r, dims=(3,))
        out.append((r / 255.0 - m) / s)
    return torch.cat(out)


def assert_pixels_close(out, ref, what=""):
    """|out - ref| <= 2^-7 |ref| + 1e-5: bf16 output against the float64 reference (one bf16
    ulp is at most 2^-7 relative: half for round-to-nearest, half for a tie flipped by fp32
    evaluation order; 1e-5 covers fp32 cancellation where v/255 ~ mean)."""
    out, ref = out.to(torch.float64).cpu(), ref.to(torch.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = (out - ref).abs()
    bound = ref.abs() * 2.0 ** -7 + 1e-5
    worst = float((err / bound).max())
    print(f"{what}: max |out-ref| = {float(err.max()):.3e}, max err/bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: err/bound = {worst:.3f}"


def make_set(path, n, Hs, Ws, num_classes=5, seed=0, meta_extra=None):
    """Write a seeded random packed image set into ``path``; returns (images, labels)."""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(n, Hs, Ws, 3), dtype=np.uint8)
    labels = rng.integers(0, num_classes, size=n, dtype=np.int64)
    path.mkdir(parents=True, exist_ok=True)
    np.save(path / "images.npy", images)
    np.save(path / "labels.npy", labels)
    meta = {"num_classes": num_classes}
    meta.update(meta_extra or {})
    (path / "meta.json").write_text(json.dumps(meta))
    return images, labels
