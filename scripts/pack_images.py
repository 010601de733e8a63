#!/usr/bin/env python
"""Build a packed image set (data/packed.py) from a class-per-folder image tree.

    python scripts/pack_images.py ~/imagenet data/imagenet_packed --split train
    python scripts/pack_images.py ~/imagenet data/imagenet_packed --split val

Layout: ``--split NAME`` reads ``SRC/NAME/<class>/<image>`` and writes the set into
``DST/NAME/`` (so a dataset is ``DST/train`` + ``DST/val``, the ``data_dir`` of the train and
the evaluation loaders); without ``--split`` it reads ``SRC/<class>/<image>`` and writes
``DST/``. Classes are the sorted folder names. Every image is decoded once (PIL), converted
to RGB, resized so its short side is ``--size`` (default 256, bilinear) and center-cropped to
``size x size``. ``images.npy`` is written through ``np.lib.format.open_memmap``: memory
stays flat however large the set is.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".gif", ".webp", ".ppm", ".tif", ".tiff")


def list_images(src: Path):
    classes = sorted(p.name for p in src.iterdir() if p.is_dir())
    if not classes:
        raise SystemExit(f"{src}: no class folders")
    items = []
    for label, name in enumerate(classes):
        for p in sorted((src / name).rglob("*")):
            if p.is_file() and p.suffix.lower() in EXTENSIONS:
                items.append((p, label))
    if not items:
        raise SystemExit(f"{src}: no images under its class folders")
    return classes, items


def load_square(path: Path, size: int) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        w, h = im.size
        if w <= h:
            nw, nh = size, max(size, int(round(h * size / w)))
        else:
            nw, nh = max(size, int(round(w * size / h))), size
        im = im.resize((nw, nh), Image.BILINEAR)
        left, top = (nw - size) // 2, (nh - size) // 2
        im = im.crop((left, top, left + size, top + size))
        return np.asarray(im, dtype=np.uint8)


def pack(src, dst, size=256, split=None, mean=None, std=None, quiet=False):
    src, dst = Path(src), Path(dst)
    if split:
        src, dst = src / split, dst / split
    if not src.is_dir():
        raise SystemExit(f"{src} is not a directory")
    classes, items = list_images(src)
    dst.mkdir(parents=True, exist_ok=True)
    images = np.lib.format.open_memmap(dst / "images.npy", mode="w+", dtype=np.uint8,
                                       shape=(len(items), size, size, 3))
    labels = np.empty(len(items), dtype=np.int64)
    for i, (path, label) in enumerate(items):
        images[i] = load_square(path, size)
        labels[i] = label
        if not quiet and (i + 1) % 10000 == 0:
            print(f"{i + 1}/{len(items)}", file=sys.stderr)
    images.flush()
    del images
    np.save(dst / "labels.npy", labels)
    meta = {"num_classes": len(classes), "classes": classes, "size": size}
    if mean is not None:
        meta["mean"] = list(mean)
    if std is not None:
        meta["std"] = list(std)
    (dst / "meta.json").write_text(json.dumps(meta, indent=1))
    if not quiet:
        print(f"packed {len(items)} images of {len(classes)} classes at {size}x{size} into {dst}")
    return dst


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", help="image tree: SRC[/SPLIT]/<class>/<image>")
    ap.add_argument("dst", help="output directory: the set is written into DST[/SPLIT]")
    ap.add_argument("--split", default=None, help="train | val | any subfolder name")
    ap.add_argument("--size", type=int, default=256, help="stored size (short side resized to it, center crop)")
    ap.add_argument("--mean", type=float, nargs=3, default=None, help="normalization mean recorded in meta.json")
    ap.add_argument("--std", type=float, nargs=3, default=None, help="normalization std recorded in meta.json")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)
    pack(a.src, a.dst, a.size, a.split, a.mean, a.std, a.quiet)


if __name__ == "__main__":
    main()
