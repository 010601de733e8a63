"""The packed-image input pipeline on an MI355X: the crop + resize + flip + normalize kernel
(csrc/image_aug.hip) against the float64 reference (tests/packed_ref.py), the 64-bit image
base, PackedImageLoader's resident and staged modes, and a native ResNet-50 through Trainer."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.data import PackedImageLoader  # noqa: E402
from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

HS, WS = 40, 56
NAN_BITS = 0x7FC1  # a bf16 NaN: every output element must be overwritten

# (box, S, what it covers); case 4 runs unflipped and flipped
CASES = [
    ((0, 0, 40, 56, 0), 32),    # 1 full frame, anisotropic downscale
    ((3, 5, 17, 29, 1), 32),    # 2 odd box, interior, flipped
    ((39, 55, 1, 1, 0), 32),    # 3 1x1 box at the last pixel: every tap clamps, constant output
    ((4, 12, 32, 32, 0), 32),   # 4 identity scale
    ((4, 12, 32, 32, 1), 32),   # 4 ... flipped
    ((0, 0, 7, 50, 1), 32),     # 5 thin box
    ((10, 3, 20, 41, 0), 33),   # 6 upscale, odd S: the pair-store tail
]
IDX = [4, 0, 4, 2, 1, 3, 0]     # repeats, non-monotone


@pytest.fixture(scope="module")
def src():
    """9 stored images: the gathered runs read the first 5 (idx <= 4), the idx=None runs image b."""
    rng = np.random.default_rng(11)
    return torch.from_numpy(rng.integers(0, 256, size=(9, HS, WS, 3), dtype=np.uint8))


def _run(src_dev, idx, boxes, S):
    B = len(boxes)
    out = torch.full((B, S, S, 4), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    box = torch.tensor(boxes, dtype=torch.int32, device="cuda")
    idx_d = None if idx is None else torch.tensor(idx, dtype=torch.int64, device="cuda")
    no.crop_resize_normalize(src_dev, idx_d, box, out, R.MEAN, R.STD)
    torch.cuda.synchronize()
    return out.cpu()


def _check(out, src, idx, boxes, S, what):
    assert not out.view(torch.int16)[..., 3].any(), f"{what}: the pad channel must be +0 bit for bit"
    ref = R.reference(src, idx, boxes, S)
    for b, box in enumerate(boxes):
        R.assert_pixels_close(out[b, ..., :3].permute(2, 0, 1), ref[b], f"{what} box {box} S={S}")


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "idx_none"])
def test_kernel_cases_against_reference(src, with_idx):
    """Cases 1-6 as batches (one launch per output size), gathered through a repeating,
    non-monotone idx or read in place (idx None, image b)."""
    src = src[:5] if with_idx else src
    src_dev = src.cuda()
    for S in (32, 33):
        sel = [k for k, (_, s) in enumerate(CASES) if s == S]
        boxes = [CASES[k][0] for k in sel]
        idx = [IDX[k] for k in sel] if with_idx else None
        # pad the S=32 batch to 9 outputs: 9 * 512 pixel pairs with 256-lane workgroups, and at
        # S=33 an image is 561 pairs = 2 workgroups + a partial one
        if S == 32:
            boxes = boxes + [(1, 2, 30, 40, 1), (20, 30, 20, 26, 0), (0, 0, 40, 56, 1)][:9 - len(boxes)]
            idx = (idx + [3, 3, 1][:len(boxes) - len(idx)]) if with_idx else None
        else:
            # odd S in later images (rows start only 8-byte aligned there), a flipped tail, and a
            # repeating, non-monotone gather
            boxes = boxes + [(2, 7, 31, 18, 1), (0, 0, 40, 56, 1), (5, 5, 33, 33, 0), (17, 20, 9, 30, 1)]
            idx = (idx + [4, 2, 4, 1]) if with_idx else None
        out = _run(src_dev, idx, boxes, S)
        _check(out, src, idx, boxes, S, "idx" if with_idx else "idx=None")
        if S == 32:
            k = sel.index(2)  # case 3: the 1x1 box gives one value per channel
            px = out[k, ..., :3].reshape(-1, 3)
            assert (px == px[0]).all()


def test_flip_is_bitwise_flip_at_identity_scale(src):
    out = _run(src.cuda(), [2, 2], [(4, 12, 32, 32, 0), (4, 12, 32, 32, 1)], 32)
    assert torch.equal(out[1].view(torch.int16), torch.flip(out[0], dims=(1,)).view(torch.int16))
    # identity scale copies pixels: the output is the normalized source pixel rounded to bf16
    crop = src[2, 4:36, 12:44].to(torch.float64) / 255.0
    exact = ((crop - torch.tensor(R.MEAN, dtype=torch.float64)) / torch.tensor(R.STD, dtype=torch.float64))
    R.assert_pixels_close(out[0, ..., :3], exact, "identity")


def test_binding_rejects_bad_arguments(src):
    s = src.cuda()
    out = torch.empty((1, 8, 8, 4), dtype=torch.bfloat16, device="cuda")
    box = torch.tensor([[0, 0, 8, 8, 0]], dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        no.crop_resize_normalize(s.float(), None, box, out, R.MEAN, R.STD)
    with pytest.raises(AssertionError):
        no.crop_resize_normalize(s, None, box.long(), out, R.MEAN, R.STD)
    with pytest.raises(AssertionError):
        no.crop_resize_normalize(s, None, box, out[..., :3], R.MEAN, R.STD)
    with pytest.raises(AssertionError):
        no.crop_resize_normalize(s, None, box.cpu(), out, R.MEAN, R.STD)
    with pytest.raises(RuntimeError, match="crop_resize_norm"):  # Cp = 8: the kernel writes 4-channel pixels
        no.crop_resize_normalize(s, None, box, torch.empty((1, 8, 8, 8), dtype=torch.bfloat16, device="cuda"),
                                 R.MEAN, R.STD)


def test_image_base_offset_is_64_bit():
    """22 000 stored 256x256 images (4.33 GB): the last image starts past 2^32 bytes."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip("needs 6 GB of free device memory")
    n = 22000
    big = torch.empty((n, 256, 256, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    last = torch.randint(0, 256, (256, 256, 3), dtype=torch.uint8, device="cuda", generator=g)
    big[n - 1] = last
    big[0] = 77
    # the two images a base offset wrapped at 2^32 would read instead of the last one
    wrapped = ((n - 1) * 196608) % 2 ** 32 // 196608
    big[wrapped:wrapped + 2] = 200
    box = [(16, 16, 224, 224, 0)] * 2
    out = _run(big, [n - 1, 0], box, 224)
    small = torch.stack([last.cpu(), torch.full((256, 256, 3), 77, dtype=torch.uint8)])
    ref = R.reference(small, [0, 1], box, 224)
    del big
    for b in range(2):
        R.assert_pixels_close(out[b, ..., :3].permute(2, 0, 1), ref[b], f"image {b}")
    assert not out.view(torch.int16)[..., 3].any()


# ----------------------------------------------------------------------------- loader
@pytest.fixture(scope="module")
def packed64(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed64")
    images, labels = R.make_set(d, 64, HS, WS, num_classes=5, seed=21)
    return d, images, labels


def test_loader_resident_and_staged_are_bit_identical(packed64):
    d, images, labels = packed64
    kw = dict(batch_size=16, image_size=32, seed=3)
    res = PackedImageLoader(d, resident=True, **kw)
    stg = PackedImageLoader(d, resident=False, prefetch=2, **kw)
    assert res.mode == "resident" and stg.mode == "staged"
    assert PackedImageLoader(d, **kw).mode == "resident"                        # auto: 430 KB fits
    assert PackedImageLoader(d, resident_limit_gb=1e-6, **kw).mode == "staged"  # auto: over the limit
    for epoch in (0, 1):
        res.set_epoch(epoch)
        stg.set_epoch(epoch)
        br, bs = list(res), list(stg)
        assert len(br) == len(bs) == 4
        order = list(res.sampler)
        for n, ((xr, yr), (xs, ys)) in enumerate(zip(br, bs)):
            assert xr.shape == (16, 3, 32, 32) and xr.dtype == torch.bfloat16 and xr.is_cuda and yr.is_cuda
            assert getattr(xr, "pdt_nhwc_pad", None) == 4 and getattr(xs, "pdt_nhwc_pad", None) == 4
            assert xr.stride() == (32 * 32 * 4, 1, 32 * 4, 4)
            pad = no.nhwc_padded_view(xs, 4)
            assert pad is not None and not pad[:, 3:].any()
            assert torch.equal(xr.view(torch.int16), xs.view(torch.int16)) and torch.equal(yr, ys)
            idx = order[16 * n:16 * n + 16]
            assert torch.equal(yr.cpu(), torch.from_numpy(labels[idx]))
            ref = R.reference(images, idx, res.boxes(idx), 32)
            R.assert_pixels_close(xr, ref, f"epoch {epoch} batch {n}")
    assert not [t for t in threading.enumerate() if t.name.startswith("PackedImageLoader")]


def test_staged_passes_back_to_back_without_host_sync(packed64):
    """Two staged passes started one after the other while the device is still busy with work
    queued before them, and no host sync in between (what Trainer's endless loop does): the
    second pass must not gather into a pinned slot whose copy from the first is still queued.
    8 batches per pass over a 3-slot ring; every batch equals resident mode bit for bit."""
    d, _, _ = packed64
    kw = dict(batch_size=8, image_size=32, seed=9)
    res = PackedImageLoader(d, resident=True, **kw)
    want = []
    for epoch in (0, 1):
        res.set_epoch(epoch)
        want += [(x.clone(), y.clone()) for x, y in res]
    stg = PackedImageLoader(d, resident=False, prefetch=2, **kw)
    a = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    for _ in range(20):  # matmuls of ~1 ms ahead of the loader's kernels on the current stream ...
        a @ a
    got = []
    for epoch in (0, 1):
        stg.set_epoch(epoch)
        for batch in stg:
            got.append(batch)
            for _ in range(10):  # ... and a "training step" behind every batch: the device lags the host
                a @ a
    assert len(got) == len(want) == 16
    for n, ((xs, ys), (xr, yr)) in enumerate(zip(got, want)):
        assert torch.equal(xs.view(torch.int16), xr.view(torch.int16)), f"batch {n}"
        assert torch.equal(ys, yr)


def test_loader_eval_center_crop_and_partial_batch(packed64):
    d, images, labels = packed64
    for resident in (True, False):
        dl = PackedImageLoader(d, batch_size=24, training=False, image_size=32, resident=resident)
        xs, ys = zip(*list(dl))
        assert [x.shape[0] for x in xs] == [24, 24, 16]
        assert torch.equal(torch.cat(ys).cpu(), torch.from_numpy(labels))
        ref = R.reference(images, None, dl.boxes(list(range(64))), 32)
        R.assert_pixels_close(torch.cat(xs), ref, f"eval resident={resident}")


def test_staged_iterator_dropped_early_stops_its_thread(packed64):
    d, _, _ = packed64
    dl = PackedImageLoader(d, batch_size=8, image_size=32, resident=False, prefetch=1)
    it = iter(dl)
    next(it)
    assert [t for t in threading.enumerate() if t.name.startswith("PackedImageLoader")]
    del it
    for t in threading.enumerate():
        if t.name.startswith("PackedImageLoader"):
            t.join(timeout=5)
    assert not [t for t in threading.enumerate() if t.name.startswith("PackedImageLoader")]
    torch.cuda.synchronize()
    assert len(list(dl)) == 8  # the loader is reusable afterwards


def test_loader_rejects_out_of_range_index_on_the_host(packed64):
    d, _, _ = packed64
    for resident in (True, False):
        dl = PackedImageLoader(d, batch_size=8, image_size=32, resident=resident, training=False)
        dl.sampler = [0, 1, 64, 2]
        with pytest.raises(IndexError, match="out of range"):
            list(dl)
    assert not [t for t in threading.enumerate() if t.name.startswith("PackedImageLoader")]


# ----------------------------------------------------------------------------- integration
def test_trainer_native_resnet50_on_packed_images(packed64, tmp_path, monkeypatch):
    """Two training iterations and a validation pass of the native bf16 ResNet-50 fed by
    PackedImageLoader (batch 32 at 224, the geometry of tests/test_train_gpu.py)."""
    import json
    from pathlib import Path

    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.ops import fused
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    monkeypatch.setenv("PDT_AUTOTUNE", "0")  # shipped choices or the heuristic: no variant timing in a test
    d, _, _ = packed64
    root = Path(__file__).resolve().parents[1]
    cfg = json.loads((root / "config" / "resnet50_bf16_packed.json").read_text())
    cfg["arch"]["args"]["num_classes"] = 8  # the set's 5 classes; the native classifier needs N % 8 == 0
    cfg["trainer"].update(save_dir=str(tmp_path), len_epoch=2, epochs=1, verbosity=1)
    for k in ("train_loader", "valid_loader", "test_loader"):
        cfg[k]["args"].update(data_dir=str(d), batch_size=32)
    device = torch.device("cuda", torch.cuda.current_device())
    try:
        config = ConfigParser(cfg, run_id="packed")
        model = build_model(config, device)
        criterion, metrics = build_criterion_metrics(config)
        optimizer, sched = build_optimizer(config, model)
        train_loader, valid_loader = build_loader(config, "train_loader"), build_loader(config, "valid_loader")
        assert isinstance(train_loader, PackedImageLoader) and train_loader.mode == "resident"
        trainer = Trainer(model, criterion, metrics, optimizer, config=config, device=device,
                          data_loader=train_loader, valid_data_loader=valid_loader, lr_scheduler=sched,
                          len_epoch=2, autocast_dtype=autocast_dtype(config, device), channels_last=True)
        trainer._on_epoch_start(1)
        log = trainer._train_epoch(1)
    finally:
        fused.set_backend("auto")
    print(log)
    assert np.isfinite(log["loss"]) and np.isfinite(log["val_loss"])
    assert 0.0 <= log["val_accuracy"] <= 1.0
    assert torch.isfinite(model.conv1.weight.grad).all()
