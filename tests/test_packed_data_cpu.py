"""Packed image sets on the host (data/packed.py): the on-disk format and its validator, the
counter-based crop boxes, the loader's torch path against the float64 reference
(tests/packed_ref.py), sharding, the packer script and the config surface."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as R  # noqa: E402

from pytorch_distributed_template_amd import data as module_data  # noqa: E402
from pytorch_distributed_template_amd.data import (PackedImageLoader, center_crop_boxes, open_packed,  # noqa: E402
                                                   random_resized_crop_boxes)

ROOT = Path(__file__).resolve().parents[1]
HS, WS = 40, 56


# ----------------------------------------------------------------------------- format
def test_open_packed_round_trip(tmp_path):
    images, labels = R.make_set(tmp_path / "s", 7, HS, WS, num_classes=3, seed=1,
                                meta_extra={"classes": ["a", "b", "c"], "mean": [0.5, 0.5, 0.5],
                                            "std": [0.25, 0.25, 0.25]})
    s = open_packed(tmp_path / "s")
    assert len(s) == 7 and s.stored_size == (HS, WS) and s.num_classes == 3 and s.classes == ["a", "b", "c"]
    assert s.images.dtype == np.uint8 and isinstance(s.images, np.memmap)
    assert np.array_equal(s.images, images) and np.array_equal(s.labels, labels)
    assert s.mean == (0.5, 0.5, 0.5) and s.std == (0.25, 0.25, 0.25)


def test_open_packed_rejects_malformed(tmp_path):
    d = tmp_path / "s"
    R.make_set(d, 4, 8, 8)
    (d / "labels.npy").unlink()
    with pytest.raises(FileNotFoundError, match="labels.npy"):
        open_packed(d)
    R.make_set(d, 4, 8, 8)
    np.save(d / "images.npy", np.zeros((4, 8, 8, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="uint8"):
        open_packed(d)
    np.save(d / "images.npy", np.zeros((4, 8, 8, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="3 channels"):
        open_packed(d)
    np.save(d / "images.npy", np.zeros((4, 8, 24), dtype=np.uint8))
    with pytest.raises(ValueError, match="rank"):
        open_packed(d)
    np.save(d / "images.npy", np.zeros((5, 8, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="5 images but 4 labels"):
        open_packed(d)
    with pytest.raises(FileNotFoundError, match="pack_images.py"):
        open_packed(tmp_path / "nowhere")


# ----------------------------------------------------------------------------- boxes
def test_random_resized_crop_boxes_properties():
    n = 4096
    idx = torch.arange(n)
    box = random_resized_crop_boxes(idx, epoch=3, seed=7, Hs=HS, Ws=WS)
    assert box.dtype == torch.int32 and tuple(box.shape) == (n, 5)
    y0, x0, h, w, flip = (box[:, i].long() for i in range(5))
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= HS).all() and (x0 + w <= WS).all()
    assert torch.equal(box, random_resized_crop_boxes(idx, epoch=3, seed=7, Hs=HS, Ws=WS))
    # a sample's box does not depend on the batch it comes in or its position there
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    pbox = random_resized_crop_boxes(perm, epoch=3, seed=7, Hs=HS, Ws=WS)
    assert torch.equal(pbox, box[perm])
    for i in (0, 17, n - 1):
        alone = random_resized_crop_boxes([i], epoch=3, seed=7, Hs=HS, Ws=WS)
        first = random_resized_crop_boxes([i, 5, 9], epoch=3, seed=7, Hs=HS, Ws=WS)
        last = random_resized_crop_boxes([1000, 2, i], epoch=3, seed=7, Hs=HS, Ws=WS)
        assert torch.equal(alone[0], box[i]) and torch.equal(first[0], box[i]) and torch.equal(last[2], box[i])
    assert not torch.equal(box, random_resized_crop_boxes(idx, epoch=4, seed=7, Hs=HS, Ws=WS))
    assert not torch.equal(box, random_resized_crop_boxes(idx, epoch=3, seed=8, Hs=HS, Ws=WS))
    share = float(flip.float().mean())
    assert 0.45 <= share <= 0.55, share
    # the areas follow the scale range, the ratios the ratio range (rounding aside)
    assert float((h * w).float().mean()) / (HS * WS) > 0.3 and len(torch.unique(box[:, :4], dim=0)) > n // 2


def test_random_resized_crop_full_frame_and_fallback():
    box = random_resized_crop_boxes(torch.arange(64), 0, 0, 48, 48, scale=(1, 1), ratio=(1, 1), hflip=0.0)
    assert (box == torch.tensor([0, 0, 48, 48, 0], dtype=torch.int32)).all()
    # no try can fit (area of the whole frame at an aspect ratio the frame does not have):
    # the center crop clipped to the ratio bounds
    box = random_resized_crop_boxes(torch.arange(8), 0, 0, 40, 80, scale=(1, 1), ratio=(1, 1), hflip=0.0)
    assert (box == torch.tensor([0, 20, 40, 40, 0], dtype=torch.int32)).all()


def test_center_crop_boxes():
    box = center_crop_boxes(3, 256, 256, 0.875)
    assert box.dtype == torch.int32 and box.tolist() == [[16, 16, 224, 224, 0]] * 3
    assert center_crop_boxes(1, HS, WS, 1.0).tolist() == [[0, 0, HS, WS, 0]]


# ----------------------------------------------------------------------------- loader (CPU)
def test_loader_cpu_eval_matches_reference(tmp_path):
    images, labels = R.make_set(tmp_path / "s", 10, HS, WS, seed=2)
    dl = PackedImageLoader(tmp_path / "s", batch_size=4, training=False, image_size=32, device="cpu")
    assert dl.mode == "torch" and len(dl) == 3 and dl.n_samples == 10 and len(dl.dataset) == 10
    batches = list(dl)
    assert [x.shape for x, _ in batches] == [(4, 3, 32, 32), (4, 3, 32, 32), (2, 3, 32, 32)]
    x = torch.cat([x for x, _ in batches])
    y = torch.cat([y for _, y in batches])
    assert x.dtype == torch.float32 and y.dtype == torch.int64
    assert batches[0][0].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, torch.from_numpy(labels))
    ref = R.reference(images, None, center_crop_boxes(10, HS, WS, 0.875), 32)
    err = float((x.double() - ref).abs().max())
    print(f"fp32 torch path vs float64 reference: max abs err {err:.3e}")
    assert err <= 1e-5


def test_loader_cpu_training_is_counter_based(tmp_path):
    images, labels = R.make_set(tmp_path / "s", 10, HS, WS, seed=3)
    a = PackedImageLoader(tmp_path / "s", batch_size=4, image_size=32, seed=5, device="cpu")
    b = PackedImageLoader(tmp_path / "s", batch_size=4, image_size=32, seed=5, device="cpu")
    ba, bb = list(a), list(b)
    assert len(ba) == 3 and all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(ba, bb))
    order0 = list(a.sampler)
    box0 = a.boxes(list(range(10)))
    # the batch is the reference of (that order, those boxes)
    ref = R.reference(images, order0[:4], a.boxes(order0[:4]), 32)
    assert float((ba[0][0].double() - ref).abs().max()) <= 1e-5
    assert torch.equal(ba[0][1], torch.from_numpy(labels[order0[:4]]))
    a.set_epoch(1)
    assert list(a.sampler) != order0 and sorted(a.sampler) == sorted(order0)
    assert not torch.equal(a.boxes(list(range(10))), box0)
    assert not torch.equal(next(iter(a))[0], ba[0][0])


def test_set_epoch_does_not_change_a_pass_under_way(tmp_path):
    """Trainer calls set_epoch while an endless pass (inf_loop) may still be running: the pass
    keeps the order and the boxes of the epoch it started in."""
    R.make_set(tmp_path / "s", 10, HS, WS, seed=6)
    a = PackedImageLoader(tmp_path / "s", batch_size=4, image_size=16, seed=5, device="cpu")
    whole = list(a)
    it = iter(a)
    first = next(it)
    a.set_epoch(1)
    rest = list(it)
    assert torch.equal(first[0], whole[0][0])
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(rest, whole[1:]))
    assert not torch.equal(next(iter(a))[0], whole[0][0])  # the next pass is epoch 1's


def test_loader_eval_shards_are_disjoint_and_cover(tmp_path, monkeypatch):
    from pytorch_distributed_template_amd.utils import dist as pdist
    _, labels = R.make_set(tmp_path / "s", 11, 8, 8, seed=4)
    seen, train_seen = [], []
    for rank in (0, 1):
        monkeypatch.setattr(pdist, "get_rank", lambda r=rank: r)
        monkeypatch.setattr(pdist, "get_world_size", lambda: 2)
        ev = PackedImageLoader(tmp_path / "s", batch_size=4, training=False, image_size=8, device="cpu")
        seen.append(list(ev.sampler))
        assert ev.n_samples == len(seen[-1])
        assert torch.equal(torch.cat([y for _, y in ev]), torch.from_numpy(labels[seen[-1]]))
        tr = PackedImageLoader(tmp_path / "s", batch_size=4, image_size=8, device="cpu")
        train_seen.append(list(tr.sampler))
    assert not set(seen[0]) & set(seen[1]) and sorted(seen[0] + seen[1]) == list(range(11))
    # training: padded to equal steps per rank, every sample seen
    assert len(train_seen[0]) == len(train_seen[1]) == 6 and set(train_seen[0] + train_seen[1]) == set(range(11))


def test_loader_rejects_bad_index_and_box(tmp_path):
    from pytorch_distributed_template_amd.data.packed import validate_boxes, validate_indices
    with pytest.raises(IndexError):
        validate_indices([0, 10], 10)
    validate_boxes(torch.tensor([[0, 0, 8, 8, 0]], dtype=torch.int32), 8, 8)
    for bad in ([-1, 0, 4, 4, 0], [0, 0, 0, 4, 0], [5, 0, 4, 4, 0], [0, 5, 4, 4, 1]):
        with pytest.raises(ValueError):
            validate_boxes(torch.tensor([bad], dtype=torch.int32), 8, 8)


# ----------------------------------------------------------------------------- packer
def test_pack_images_script(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import importlib.util
    spec = importlib.util.spec_from_file_location("pack_images", ROOT / "scripts" / "pack_images.py")
    pack_images = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pack_images)
    rng = np.random.default_rng(0)
    sizes = {"cat": [(40, 60), (64, 33), (50, 50)], "ant": [(33, 90), (128, 40), (36, 36)]}
    for name, shapes in sizes.items():
        (tmp_path / "tree" / "train" / name).mkdir(parents=True)
        for i, (h, w) in enumerate(shapes):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(
                tmp_path / "tree" / "train" / name / f"{i}.png")
    pack_images.main([str(tmp_path / "tree"), str(tmp_path / "out"), "--split", "train", "--size", "32", "--quiet"])
    s = open_packed(tmp_path / "out" / "train")
    assert len(s) == 6 and s.stored_size == (32, 32) and s.num_classes == 2 and s.classes == ["ant", "cat"]
    assert s.labels.tolist() == [0, 0, 0, 1, 1, 1]
    # the square 36x36 source keeps its content (a plain resize): not blank, not constant
    assert s.images[2].std() > 10


def test_package_does_not_import_pil():
    import subprocess
    code = "import sys; import pytorch_distributed_template_amd.data; assert 'PIL' not in sys.modules"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ----------------------------------------------------------------------------- config
def _cfg(tmp_path, data_dir):
    return {
        "name": "P",
        "arch": {"type": "ResNet50", "args": {}},
        "train_loader": {"type": "PackedImageLoader",
                         "args": {"data_dir": str(data_dir), "batch_size": 4, "image_size": 16, "device": "cpu",
                                  "num_workers": 4}},
        "optimizer": {"type": "SGD", "args": {"lr": 0.1}},
        "loss": "label_smoothing_cross_entropy",
        "metrics": ["accuracy"],
        "trainer": {"epochs": 1, "save_dir": str(tmp_path / "ck"), "save_period": 1, "verbosity": 2,
                    "monitor": "off", "tensorboard": False},
    }


def test_config_builds_packed_loader(tmp_path):
    from pytorch_distributed_template_amd.config import ConfigParser
    R.make_set(tmp_path / "s", 6, 20, 20)
    cfg = ConfigParser(_cfg(tmp_path, tmp_path / "s"), run_id="P1")
    dl = cfg.init_obj("train_loader", module_data)
    assert isinstance(dl, PackedImageLoader) and dl.batch_size == 4 and dl.training
    x, y = next(iter(dl))
    assert x.shape == (4, 3, 16, 16) and y.shape == (4,)
    cfg = ConfigParser(_cfg(tmp_path, tmp_path / "missing"), run_id="P2")
    with pytest.raises(FileNotFoundError, match=r"scripts/pack_images\.py"):
        cfg.init_obj("train_loader", module_data)


def test_shipped_packed_config(tmp_path):
    cfg = json.loads((ROOT / "config" / "resnet50_bf16_packed.json").read_text())
    base = json.loads((ROOT / "config" / "resnet50_bf16.json").read_text())
    assert cfg["loss"] == "label_smoothing_cross_entropy"
    for k, split, training in (("train_loader", "train", True), ("valid_loader", "val", False),
                               ("test_loader", "val", False)):
        assert cfg[k]["type"] == "PackedImageLoader"
        assert cfg[k]["args"]["data_dir"] == f"data/imagenet_packed/{split}"
        assert cfg[k]["args"].get("training", True) is training
        assert cfg[k]["args"]["batch_size"] == base[k]["args"]["batch_size"]
    for k in ("arch", "optimizer", "metrics", "lr_scheduler", "trainer"):
        assert cfg[k] == base[k]
    with pytest.raises(FileNotFoundError, match=r"scripts/pack_images\.py"):
        PackedImageLoader(**dict(cfg["train_loader"]["args"], data_dir=str(tmp_path / "none"), device="cpu"))
