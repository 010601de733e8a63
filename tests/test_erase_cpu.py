"""Random Erasing on the host (data/packed.py): the argument checks, the counter-based rectangles
and keys, erase_images_torch and the loader's torch path against the float64 reference
(tests/erase_ref.py), and the config surface. The last test seeds faults into the reference and
checks that the named check of each catches it."""
import json
import math
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import erase_ref as E  # noqa: E402
import mix_ref as M  # noqa: E402
import packed_ref as R  # noqa: E402

from pytorch_distributed_template_amd import data as module_data  # noqa: E402
from pytorch_distributed_template_amd.data import MixedTarget, PackedImageLoader  # noqa: E402
from pytorch_distributed_template_amd.data.packed import (check_erase_args, erase_images_torch,  # noqa: E402
                                                          erase_keys, random_erasing_rects, validate_erase)

ROOT = Path(__file__).resolve().parents[1]
HS, WS = 40, 56
AREA, ASPECT = (0.02, 1 / 3), (0.3, 1 / 0.3)


# ----------------------------------------------------------------------------- arguments
def test_argument_errors(tmp_path):
    check_erase_args(0.0, "pixel", 1, AREA, ASPECT)
    check_erase_args(1.0, "const", 8, (0.5, 1.0), (1.0, 1.0))
    for bad in (dict(re_prob=-0.1), dict(re_prob=1.5), dict(re_prob=float("nan")), dict(re_mode="rand"),
                dict(re_count=0), dict(re_count=9), dict(re_count=1.5), dict(re_area=(0.0, 0.3)),
                dict(re_area=(0.3, 0.1)), dict(re_area=(-0.1, 0.3)), dict(re_area=(0.1, 1.5)),
                dict(re_aspect=(0.0, 3.0)), dict(re_aspect=(3.0, 0.3)), dict(re_aspect=(-1.0, 3.0))):
        kw = dict(re_prob=0.25, re_mode="pixel", re_count=1, re_area=AREA, re_aspect=ASPECT)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_erase_args(**kw)
    R.make_set(tmp_path / "s", 4, 8, 8)
    with pytest.raises(ValueError, match="re_mode"):
        PackedImageLoader(tmp_path / "s", batch_size=2, image_size=8, device="cpu", re_prob=0.5, re_mode="noise")
    with pytest.raises(ValueError, match="re_count"):
        PackedImageLoader(tmp_path / "s", batch_size=2, image_size=8, device="cpu", re_count=9)
    with pytest.raises(ValueError):
        erase_images_torch(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, dtype=torch.int32), torch.zeros(1), "rand")


def test_validate_erase():
    ok = torch.tensor([[[0, 0, 0, 0], [0, 0, 32, 32]], [[3, 5, 3, 9], [31, 31, 32, 32]]], dtype=torch.int32)
    validate_erase(ok, 32)
    for k, bad in enumerate(([-1, 0, 4, 4], [0, -1, 4, 4], [0, 0, 33, 4], [0, 0, 4, 33], [5, 0, 4, 4], [0, 5, 4, 4])):
        r = ok.clone()
        r[k % 2, k % 2] = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(ValueError, match="erase rectangle"):
            validate_erase(r, 32)
    with pytest.raises(ValueError):
        validate_erase(torch.zeros(2, 9, 4, dtype=torch.int32), 32)
    with pytest.raises(ValueError):
        validate_erase(torch.zeros(2, 4, dtype=torch.int32), 32)


# ----------------------------------------------------------------------------- rectangles
@pytest.mark.parametrize("count", [1, 3, 8])
def test_rectangles_are_a_pure_function_of_seed_epoch_index(count):
    idx = torch.arange(500, 756)
    kw = dict(S=33, re_prob=0.6, re_count=count)
    whole = random_erasing_rects(idx, 2, 9, **kw)
    keys = erase_keys(idx, 2, 9)
    assert whole.dtype == torch.int32 and tuple(whole.shape) == (256, count, 4)
    assert keys.dtype == torch.int64 and tuple(keys.shape) == (256,) and int(keys.min()) >= 0 and int(keys.max()) < 2 ** 32
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(1))
    assert torch.equal(random_erasing_rects(idx[perm], 2, 9, **kw), whole[perm])
    assert torch.equal(erase_keys(idx[perm], 2, 9), keys[perm])
    for lo, hi in ((0, 1), (7, 20), (255, 256)):  # drawn in other batches, at other positions
        assert torch.equal(random_erasing_rects(idx[lo:hi], 2, 9, **kw), whole[lo:hi])
        assert torch.equal(erase_keys(idx[lo:hi].tolist(), 2, 9), keys[lo:hi])
    assert not torch.equal(random_erasing_rects(idx, 3, 9, **kw), whole)   # the epoch,
    assert not torch.equal(random_erasing_rects(idx, 2, 10, **kw), whole)  # the seed
    assert not torch.equal(erase_keys(idx, 3, 9), keys) and not torch.equal(erase_keys(idx, 2, 10), keys)
    assert len(set(keys.tolist())) == 256
    big = torch.tensor([5, 5 + 2 ** 32])  # the high index word counts
    assert not torch.equal(erase_keys(big[:1], 0, 0), erase_keys(big[1:], 0, 0))


@pytest.mark.parametrize("S", [8, 32, 33, 224])
@pytest.mark.parametrize("count", [1, 8])
def test_rectangles_lie_inside_the_output(S, count):
    rects = random_erasing_rects(torch.arange(4096), 1, 3, S, re_prob=1.0, re_count=count)
    validate_erase(rects, S)
    r = rects.to(torch.int64)
    h, w = r[..., 2] - r[..., 0], r[..., 3] - r[..., 1]
    assert int(h.max()) < S and int(w.max()) < S and int(h.min()) >= 0 and int(w.min()) >= 0
    empty = (h == 0) | (w == 0)
    assert not r[empty].any(), "an empty rectangle is all zeros"
    assert bool((~empty).any())
    none = random_erasing_rects(torch.arange(64), 1, 3, S, re_prob=0.0, re_count=count)
    assert not none.any()


def test_erased_share_and_areas_over_65536_indices():
    S, n, p = 224, 1 << 16, 0.25
    rects = random_erasing_rects(torch.arange(n), 0, 11, S, re_prob=p).to(torch.int64)[:, 0]
    h, w = rects[:, 2] - rects[:, 0], rects[:, 3] - rects[:, 1]
    hit = (h > 0) & (w > 0)
    share = float(hit.double().mean())
    sd = math.sqrt(p * (1 - p) / n)
    print(f"erased share {share:.5f} (re_prob {p}, 4 sd = {4 * sd:.5f})")
    assert abs(share - p) <= 4 * sd
    # h = round(sqrt(a r)), w = round(sqrt(a / r)) with a in [0.02, 1/3] S^2: (h +- 0.5)(w +- 0.5) brackets a
    hh, ww = h[hit].double(), w[hit].double()
    assert bool(((hh + 0.5) * (ww + 0.5) >= AREA[0] * S * S).all())
    assert bool(((hh - 0.5) * (ww - 0.5) <= AREA[1] * S * S).all())
    ratio = hh / ww  # and the aspect: (h +- 0.5) / (w -+ 0.5) brackets r
    assert bool(((hh + 0.5) / (ww - 0.5) >= ASPECT[0]).all()) and bool(((hh - 0.5) / (ww + 0.5) <= ASPECT[1]).all())
    assert float(ratio.min()) < 0.5 and float(ratio.max()) > 2.0
    # the corner is uniform over the positions that keep the rectangle inside
    assert int(rects[hit][:, 0].min()) == 0 and int((rects[hit][:, 2]).max()) == S
    assert int(rects[hit][:, 1].min()) == 0 and int((rects[hit][:, 3]).max()) == S
    # count > 1 divides the area
    r3 = random_erasing_rects(torch.arange(4096), 0, 11, S, re_prob=1.0, re_count=3).to(torch.int64)
    a3 = ((r3[..., 2] - r3[..., 0]).double() - 0.5) * ((r3[..., 3] - r3[..., 1]).double() - 0.5)
    assert float(a3.max()) <= AREA[1] * S * S / 3


def test_erasing_changes_no_box_flip_or_mix_parameter(tmp_path):
    R.make_set(tmp_path / "s", 10, HS, WS, seed=3)
    kw = dict(batch_size=4, image_size=32, seed=5, device="cpu", mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")
    a = PackedImageLoader(tmp_path / "s", **kw)
    b = PackedImageLoader(tmp_path / "s", re_prob=1.0, re_count=2, **kw)
    assert not a.erasing and a.erase([0, 1]) is None and b.erasing
    for epoch in (0, 3):
        idx = [7, 2, 9, 4]
        assert torch.equal(a.boxes(idx, epoch), b.boxes(idx, epoch))
        for u, v in zip(a.mix(idx, epoch), b.mix(idx, epoch)):
            assert torch.equal(u, v)
        rects, keys = b.erase(idx, epoch)
        assert torch.equal(rects, random_erasing_rects(idx, epoch, 5, 32, 1.0, 2))
        assert torch.equal(keys, erase_keys(idx, epoch, 5))


# ----------------------------------------------------------------------------- noise
def _moments(z, what):
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    assert z.size == 1 << 20
    mean, var = float(z.mean()), float(z.var())
    print(f"{what}: mean {mean:+.5f} (bound {4 / 1024:.5f}), var - 1 {var - 1:+.5f} (bound {4 * math.sqrt(2 / 2 ** 20):.5f})")
    assert abs(mean) <= 4 / 1024 and abs(var - 1) <= 4 * math.sqrt(2 / 2 ** 20)
    assert float(np.abs(z).max()) <= E.R_MAX


def test_noise_moments_over_2_20_draws():
    """2^20 draws per channel (64 keys x 128 x 128 pixels), each channel checked on its own."""
    S, B = 128, 64
    keys = erase_keys(torch.arange(B), 0, 4)
    ref = E.noise(keys.numpy(), S)
    full = torch.tensor([[[0, 0, S, S]]] * B, dtype=torch.int32)
    got = erase_images_torch(torch.zeros(B, 3, S, S), full, keys, "pixel")
    for c in range(3):
        _moments(ref[:, c], f"reference, channel {c}")
        _moments(got[:, c], f"erase_images_torch, channel {c}")
    # channels and neighbouring pixels are uncorrelated: |corr| <= 4 / sqrt(n)
    z = ref.numpy()
    for u, v in ((z[:, 0], z[:, 1]), (z[:, 1], z[:, 2]), (z[:, 0], z[:, 2]), (z[:, 0, :, :-1], z[:, 0, :, 1:])):
        assert abs(float(np.corrcoef(u.reshape(-1), v.reshape(-1))[0, 1])) <= 4 / math.sqrt(u.size)


# ----------------------------------------------------------------------------- the named checks
RECTS = [[(2, 3, 10, 12), (0, 0, 0, 0)], [(0, 0, 1, 1), (32, 32, 33, 33)], [(5, 0, 6, 33), (0, 7, 33, 8)],
         [(4, 28, 20, 33), (12, 3, 20, 29)], [(0, 0, 33, 33), (0, 0, 0, 0)], [(0, 0, 0, 0), (3, 3, 3, 9)]]
KEYS = [0xDEADBEEF, 7, 0xFFFFFFFF, 0, 7, 123456789]  # entries 1 and 4 share a key


def _views(S=33, B=6):
    g = torch.Generator().manual_seed(2)
    return torch.randn(B, 3, S, S, generator=g, dtype=torch.float64) * 0.5 + 3.0  # never 0, never a draw


def check_rectangle_placement(got, view, rects, keys, mode):
    """Exactly the pixels inside a rectangle changed."""
    inside = E.inside_any(rects, view.shape[2]).expand_as(view)
    assert torch.equal(got[~inside].double(), view[~inside].to(got.dtype).double()), "a pixel outside every rectangle changed"
    assert bool((got[inside].double() != view[inside]).all()), "a pixel inside a rectangle kept its value"


def check_right_edge_is_open(got, view, rects, keys, mode):
    """Column x1 of every non-empty rectangle that no other one covers keeps its value."""
    S = view.shape[2]
    inside = E.inside_any(rects, S)[:, 0]
    n = 0
    for b, rs in enumerate(rects):
        for y0, x0, y1, x1 in rs:
            if y0 < y1 and x0 < x1 and x1 < S:
                keep = ~inside[b, y0:y1, x1]
                n += int(keep.sum())
                assert torch.equal(got[b, :, y0:y1, x1][:, keep].double(), view[b, :, y0:y1, x1][:, keep].to(got.dtype).double()), \
                    f"column x1 = {x1} of batch entry {b} was erased"
    assert n > 0


def check_noise_follows_the_sample_key(got, view, rects, keys, mode):
    """Entries 1 and 4 share a key: where both are erased the noise is equal; and every erased
    element is the draw of its own key."""
    S = view.shape[2]
    inside = E.inside_any(rects, S).expand_as(view)
    both = inside[1] & inside[4]
    assert bool(both.any()) and torch.equal(got[1][both], got[4][both]), "same key, different noise"
    z = E.noise(keys, S)
    assert float((got[inside].double() - z[inside]).abs().max()) <= 2.0 ** -22, "not the draw of (key, oy, ox, c)"


def check_channels_are_independent(got, view, rects, keys, mode):
    inside = E.inside_any(rects, view.shape[2])[:, 0]
    px = got.permute(0, 2, 3, 1)[inside]
    assert bool((px[:, 0] != px[:, 1]).all()) and bool((px[:, 1] != px[:, 2]).all()) and bool((px[:, 0] != px[:, 2]).all())


CHECKS = {"shifted": check_rectangle_placement, "closed_right_edge": check_right_edge_is_open,
          "batch_position_key": check_noise_follows_the_sample_key, "channel_repeated": check_channels_are_independent}


@pytest.mark.parametrize("mode", ["pixel", "const"])
def test_erase_images_torch_against_reference(mode):
    view = _views()
    rects = torch.tensor(RECTS, dtype=torch.int32)
    keys = torch.tensor(KEYS, dtype=torch.int64)
    got = erase_images_torch(view.float(), rects, keys, mode)
    assert got.dtype == torch.float32 and got.shape == view.shape
    ref = E.erased(view.float().double(), RECTS, KEYS, mode)
    err = float((got.double() - ref).abs().max())
    print(f"{mode}: max |erase_images_torch - erased()| = {err:.3e}")
    assert err <= 2.0 ** -24 * E.R_MAX  # one fp32 rounding of a value below 5.77
    inside = E.inside_any(RECTS, 33).expand_as(view)
    assert torch.equal(got[~inside], view.float()[~inside])
    if mode == "const":
        assert not got[inside].view(torch.int32).any(), "+0 bit for bit"
    for name, check in CHECKS.items():
        if mode == "pixel" or name in ("shifted", "closed_right_edge"):
            check(got, view.float().double(), RECTS, KEYS, mode)


@pytest.mark.parametrize("fault", E.FAULTS)
def test_seeded_faults_are_caught_by_their_named_check(fault):
    view = _views()
    clean = E.erased(view, RECTS, KEYS, "pixel")
    CHECKS[fault](clean, view, RECTS, KEYS, "pixel")  # the clean reference passes
    broken = E.erased(view, RECTS, KEYS, "pixel", fault=fault)
    assert not torch.equal(broken, clean)
    with pytest.raises(AssertionError):
        CHECKS[fault](broken, view, RECTS, KEYS, "pixel")


# ----------------------------------------------------------------------------- loader (torch path)
def _reference_batch(images, dl, idx, epoch):
    box = dl.boxes(idx, epoch)
    mix = dl.mix(idx, epoch)
    if mix is None:
        view = R.reference(images, idx, box, dl.image_size)
    else:
        partner, w_own, rect, _ = mix
        view = M.mixed_batch(images, idx, box, partner, rect, w_own, dl.image_size)
    er = dl.erase(idx, epoch)
    return view if er is None else E.erased(view, er[0].numpy(), er[1].numpy(), dl.re_mode)


@pytest.mark.parametrize("mixing", [False, True], ids=["plain", "mixed"])
@pytest.mark.parametrize("mode", ["pixel", "const"])
def test_loader_torch_path_against_reference(tmp_path, mode, mixing):
    images, labels = R.make_set(tmp_path / "s", 10, HS, WS, seed=3)
    kw = dict(batch_size=4, image_size=32, seed=5, device="cpu")
    if mixing:
        kw.update(mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")
    dl = PackedImageLoader(tmp_path / "s", re_prob=0.7, re_mode=mode, re_count=2, **kw)
    off = PackedImageLoader(tmp_path / "s", **kw)
    assert dl.mode == "torch" and dl.erasing
    dl.set_epoch(1)
    off.set_epoch(1)
    order = list(dl.sampler)
    n_erased = 0
    for n, ((x, t), (x0, t0)) in enumerate(zip(dl, off)):
        idx = order[4 * n:4 * n + 4]
        assert x.dtype == torch.float32 and x.shape == (len(idx), 3, 32, 32)
        if mixing:  # the target is the one without erasing
            assert isinstance(t, MixedTarget) and all(torch.equal(u, v) for u, v in zip(t, t0))
        else:
            assert torch.equal(t, t0) and torch.equal(t, torch.from_numpy(labels[idx]))
        ref = _reference_batch(images, dl, idx, 1)
        inside = E.inside_any(dl.erase(idx, 1)[0].numpy(), 32).expand_as(ref)
        n_erased += int(inside.sum())
        assert torch.equal(x[~inside], x0[~inside]), "outside the rectangles the batch is the one without erasing"
        assert float((x.double() - ref).abs().max()) <= 2e-5  # fp32 against float64, as test_packed_data_cpu.py
        if mode == "const":
            assert not x[inside].view(torch.int32).any()
    assert n_erased > 0


def test_evaluation_loader_never_erases(tmp_path):
    images, _ = R.make_set(tmp_path / "s", 6, HS, WS, seed=8)
    kw = dict(batch_size=4, training=False, image_size=32, device="cpu")
    ev = PackedImageLoader(tmp_path / "s", re_prob=1.0, **kw)
    plain = PackedImageLoader(tmp_path / "s", **kw)
    assert not ev.erasing and ev.erase([0, 1, 2]) is None
    for (x, y), (x0, y0) in zip(ev, plain):
        assert torch.equal(x, x0) and torch.equal(y, y0)


def test_re_prob_zero_is_the_loader_without_the_arguments(tmp_path):
    R.make_set(tmp_path / "s", 10, HS, WS, seed=3)
    for mix in ({}, dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")):
        kw = dict(batch_size=4, image_size=32, seed=5, device="cpu", **mix)
        zero = PackedImageLoader(tmp_path / "s", re_prob=0.0, re_mode="const", re_count=3, **kw)
        none = PackedImageLoader(tmp_path / "s", **kw)
        assert not zero.erasing
        for (x, t), (x0, t0) in zip(zero, none):
            assert torch.equal(x, x0)
            assert all(torch.equal(u, v) for u, v in zip(t, t0)) if mix else torch.equal(t, t0)


# ----------------------------------------------------------------------------- config
def test_shipped_config_builds_the_erasing_loader(tmp_path):
    from pytorch_distributed_template_amd.config import ConfigParser
    cfg = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix_ema_dp_re.json").read_text())
    base = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix_ema_dp.json").read_text())
    assert cfg["train_loader"]["args"]["re_prob"] == 0.25
    for k in ("valid_loader", "test_loader"):
        assert "re_prob" not in cfg[k]["args"]
    args = dict(cfg["train_loader"]["args"])
    assert args.pop("re_prob") == 0.25 and args == base["train_loader"]["args"]
    assert {k: v for k, v in cfg.items() if k not in ("name", "train_loader")} == \
        {k: v for k, v in base.items() if k not in ("name", "train_loader")}
    R.make_set(tmp_path / "s", 6, 20, 20)
    cfg["train_loader"]["args"].update(data_dir=str(tmp_path / "s"), batch_size=4, image_size=16, device="cpu")
    cfg["trainer"]["save_dir"] = str(tmp_path / "ck")
    dl = ConfigParser(cfg, run_id="RE1").init_obj("train_loader", module_data)
    assert isinstance(dl, PackedImageLoader) and dl.erasing and dl.mixing and dl.re_prob == 0.25
    assert dl.re_mode == "pixel" and dl.re_count == 1 and dl.re_area == AREA and dl.re_aspect == ASPECT
    x, t = next(iter(dl))
    assert x.shape == (4, 3, 16, 16) and isinstance(t, MixedTarget)
