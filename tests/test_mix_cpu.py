"""Mixup / CutMix on the host: mix_params / validate_mix, PackedImageLoader's torch mode against
the float64 reference (tests/mix_ref.py), the paired-target loss on the torch path against
F.cross_entropy with the dense soft-target matrix, the shipped config and a CPU train.py run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_ref as M  # noqa: E402
import packed_ref as R  # noqa: E402

import pytorch_distributed_template_amd.data as module_data  # noqa: E402
from pytorch_distributed_template_amd.data import (MixedTarget, PackedImageLoader, mix_params,  # noqa: E402
                                                   validate_mix)
from pytorch_distributed_template_amd.models import loss as module_loss  # noqa: E402
from pytorch_distributed_template_amd.ops import fused  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
S = 32


def _eq(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- mix_params
def test_mix_params_is_a_pure_function_of_its_key():
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")
    idx = list(range(40, 56))
    a, b = mix_params(idx, 3, 7, S, **kw), mix_params(idx, 3, 7, S, **kw)
    assert _eq(a, b)
    # only the first index keys the draws; the rest of the batch does not
    assert _eq(a, mix_params([40] + list(range(100, 115)), 3, 7, S, **kw))
    assert not _eq(a, mix_params(idx, 4, 7, S, **kw))                       # another epoch
    assert not _eq(a, mix_params(list(range(41, 57)), 3, 7, S, **kw))       # another first index
    assert not _eq(a, mix_params(idx, 3, 8, S, **kw))                       # another seed
    partner, w_own, rect, lam = a
    assert partner.dtype == torch.int64 and partner.tolist() == list(range(15, -1, -1))
    assert w_own.dtype == torch.float32 and lam.dtype == torch.float32 and rect.dtype == torch.int32
    assert rect.shape == (16, 4) and w_own.shape == (16,) and lam.shape == (16,)
    assert mix_params([5], 0, 0, S, **kw)[0].tolist() == [0]                # a batch of 1 pairs with itself
    assert mix_params([5, 6, 7], 0, 0, S, **kw)[0].tolist() == [2, 1, 0]    # the middle of an odd batch too


def test_cutmix_rectangles_are_clipped_and_lam_is_the_clipped_area():
    seen_clipped = 0
    for first in range(64):
        partner, w_own, rect, lam = mix_params(list(range(first * 8, first * 8 + 8)), 0, 1, 33, cutmix_alpha=1.0,
                                               mix_mode="elem")
        validate_mix(partner, w_own, rect, lam, 33)
        r = rect.numpy().astype(np.int64)
        assert (r >= 0).all() and (r <= 33).all() and (r[:, 0] <= r[:, 2]).all() and (r[:, 1] <= r[:, 3]).all()
        area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
        assert np.array_equal(lam.numpy(), (1.0 - area / float(33 * 33)).astype(np.float32))  # exact in float32
        assert (w_own == 1).all()
        h, w = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        seen_clipped += int(((h != w) & (area > 0)).sum())  # an unclipped rectangle is a square
    assert seen_clipped > 0


def test_batch_mode_broadcasts_one_draw():
    for first in range(16):
        _, w_own, rect, lam = mix_params(list(range(first, first + 9)), 2, 5, S, mixup_alpha=0.8, cutmix_alpha=1.0)
        assert (w_own == w_own[0]).all() and (lam == lam[0]).all() and (rect == rect[0]).all()
    _, w_own, _, _ = mix_params(list(range(64)), 2, 5, S, mixup_alpha=0.8, mix_mode="elem")
    assert len(set(w_own.tolist())) > 32


def test_mix_prob_zero_and_single_methods():
    for mode in ("batch", "elem"):
        _, w_own, rect, lam = mix_params(list(range(32)), 0, 0, S, mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.0,
                                         mix_mode=mode)
        assert (w_own == 1).all() and (lam == 1).all()
        assert ((rect[:, 0] == rect[:, 2]) | (rect[:, 1] == rect[:, 3])).all()
    # only Mixup: never a rectangle, lam = w_own
    _, w_own, rect, lam = mix_params(list(range(512)), 0, 0, S, mixup_alpha=0.8, mix_mode="elem")
    assert not rect.any() and torch.equal(w_own, lam) and (w_own < 1).any()
    # only CutMix: w_own is always 1
    _, w_own, rect, lam = mix_params(list(range(512)), 0, 0, S, cutmix_alpha=1.0, mix_mode="elem")
    assert (w_own == 1).all() and rect.any() and (lam < 1).any()
    # no method at all
    _, w_own, rect, lam = mix_params(list(range(8)), 0, 0, S)
    assert (w_own == 1).all() and (lam == 1).all() and not rect.any()


def test_both_methods_occur_and_mixup_lam_is_centred():
    """4 096 seeded draws with both alphas positive. Beta(0.8, 0.8) is symmetric with variance
    1 / (4 (2 a + 1)) = 0.096: the mean of ~2 048 draws has a standard error of 0.007, so
    0.5 +- 0.05 is seven of them."""
    _, w_own, rect, lam = mix_params(list(range(4096)), 1, 2, S, mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")
    is_mixup = w_own != 1
    is_cut = (rect[:, 2] > rect[:, 0]) & (rect[:, 3] > rect[:, 1])
    assert not (is_mixup & is_cut).any()
    n_mixup, n_cut = int(is_mixup.sum()), int(is_cut.sum())
    print(f"mixup {n_mixup}, cutmix {n_cut}, mean mixup lam {float(lam[is_mixup].mean()):.4f}")
    assert 1700 < n_mixup < 2400 and n_cut > 1500
    assert abs(float(lam[is_mixup].mean()) - 0.5) <= 0.05


def test_invalid_arguments_raise(tmp_path):
    R.make_set(tmp_path / "s", 4, 20, 20)
    for bad in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1), dict(mix_prob=1.5), dict(mix_prob=-0.1),
                dict(mix_switch_prob=2), dict(mix_mode="pair")):
        with pytest.raises(ValueError):
            PackedImageLoader(tmp_path / "s", batch_size=2, image_size=16, device="cpu", **bad)
        with pytest.raises(ValueError):
            mix_params([0, 1], 0, 0, 16, **bad)


def test_validate_mix_raises_on_each_kind_of_bad_input():
    def good():
        return [torch.tensor([1, 0]), torch.tensor([1.0, 0.5]), torch.tensor([[0, 0, 4, 4], [2, 2, 2, 8]],
                                                                              dtype=torch.int32),
                torch.tensor([0.75, 0.5])]
    validate_mix(*good(), 8)
    for pos, value, what in ((2, [[0, 0, 9, 4], [0, 0, 0, 0]], "rectangle"), (2, [[-1, 0, 4, 4], [0, 0, 0, 0]], "rect"),
                             (2, [[5, 0, 4, 4], [0, 0, 0, 0]], "rect"), (2, [[0, 5, 4, 4], [0, 0, 0, 0]], "rect"),
                             (2, [[0, 0, 4, 9], [0, 0, 0, 0]], "rect"), (1, [1.5, 0.5], "w_own"),
                             (1, [-0.1, 0.5], "w_own"), (1, [float("nan"), 0.5], "w_own"), (3, [0.5, 1.01], "lam"),
                             (3, [-1.0, 0.5], "lam"), (0, [2, 0], "partner"), (0, [-1, 0], "partner")):
        args = good()
        args[pos] = torch.tensor(value, dtype=args[pos].dtype)
        with pytest.raises(ValueError, match=what):
            validate_mix(*args, 8)
    args = good()
    args[2] = args[2][:1]
    with pytest.raises(ValueError):
        validate_mix(*args, 8)


# ----------------------------------------------------------------------------- loader, torch mode
@pytest.fixture(scope="module")
def packed13(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed13")
    images, labels = R.make_set(d, 13, 40, 56, num_classes=5, seed=31)
    return d, images, labels


@pytest.mark.parametrize("batch", [4, 3])
@pytest.mark.parametrize("alphas", [(0.8, 0.0), (0.0, 1.0), (0.8, 1.0)], ids=["mixup", "cutmix", "both"])
def test_loader_torch_mode_matches_reference(packed13, batch, alphas):
    """13 images: batch 4 leaves a last batch of 1 (it pairs with itself), batch 3 has a
    self-paired middle element."""
    d, images, labels = packed13
    dl = PackedImageLoader(d, batch_size=batch, image_size=S, seed=4, device="cpu", mixup_alpha=alphas[0],
                           cutmix_alpha=alphas[1], mix_mode="elem")
    assert dl.mode == "torch" and dl.mixing
    for epoch in (0, 1):
        dl.set_epoch(epoch)
        order = list(dl.sampler)
        batches = list(dl)
        assert [x.shape[0] for x, _ in batches][-1] == 13 % batch
        for n, (x, t) in enumerate(batches):
            idx = order[batch * n:batch * n + batch]
            assert isinstance(t, MixedTarget) and x.dtype == torch.float32
            partner, w_own, rect, lam = dl.mix(idx, epoch)
            assert _eq((partner, w_own, rect, lam), mix_params(idx, epoch, 4, S, alphas[0], alphas[1], 1.0, 0.5, "elem"))
            assert t.label_a.dtype == torch.int64 and t.lam.dtype == torch.float32
            assert torch.equal(t.label_a, torch.from_numpy(labels[idx]))
            assert torch.equal(t.label_b, torch.from_numpy(labels[idx[::-1]]))  # the reversed batch's labels
            assert torch.equal(t.lam, lam)
            ref = M.mixed_batch(images, idx, dl.boxes(idx, epoch), partner, rect, w_own, S)
            R.assert_pixels_close(x, ref, f"epoch {epoch} batch {n}")


def test_loader_without_mixing_is_unchanged(packed13):
    d, _, labels = packed13
    kw = dict(batch_size=4, image_size=S, seed=4, device="cpu")
    plain = list(PackedImageLoader(d, **kw))
    for extra in (dict(mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=0.3, mix_mode="elem"),):
        dl = PackedImageLoader(d, **kw, **extra)
        assert not dl.mixing and dl.mix([0, 1]) is None
        for (x, y), (xp, yp) in zip(list(dl), plain):
            assert torch.is_tensor(y) and y.dtype == torch.int64 and torch.equal(y, yp) and torch.equal(x, xp)
    # evaluation never mixes, whatever the alphas
    ev = PackedImageLoader(d, training=False, mixup_alpha=0.8, cutmix_alpha=1.0, **kw)
    ev0 = PackedImageLoader(d, training=False, **kw)
    assert not ev.mixing
    for (x, y), (xp, yp) in zip(list(ev), list(ev0)):
        assert torch.is_tensor(y) and y.dtype == torch.int64 and torch.equal(y, yp) and torch.equal(x, xp)
    assert torch.equal(torch.cat([y for _, y in ev]), torch.from_numpy(labels))


# ----------------------------------------------------------------------------- loss, torch path
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_paired_loss_torch_path_matches_dense_soft_targets(eps):
    g = torch.Generator().manual_seed(3)
    B, V = 9, 11
    x = (torch.randn(B, V, generator=g) * 3).requires_grad_()
    a = torch.randint(0, V, (B,), generator=g)
    b = torch.randint(0, V, (B,), generator=g)
    b[0] = a[0]                      # ta == tb
    a[1], b[1] = 0, V - 1
    lam = torch.rand(B, generator=g)
    lam[2], lam[3], lam[4] = 0.0, 1.0, 0.5
    target = MixedTarget(a, b, lam)
    fn = module_loss.cross_entropy if eps == 0.0 else module_loss.label_smoothing_cross_entropy
    loss = fn(x, target) if eps == 0.0 else fn(x, target, smoothing=eps)
    loss.backward()
    x64 = x.detach().double().requires_grad_()
    ref = F.cross_entropy(x64, M.soft_targets(a, b, lam, V, eps))
    ref.backward()
    torch.testing.assert_close(loss.detach().double(), ref.detach(), rtol=1e-6, atol=0)
    # 1e-6 of the gradient's scale: entries near zero cancel (p - target)
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-6, atol=1e-6 * float(x64.grad.abs().max()))
    assert torch.equal(fused.softmax_cross_entropy(x.detach(), (a, b, lam), eps), loss.detach())  # a plain tuple too


def test_int64_target_gives_what_it_gave():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 10, generator=g)
    y = torch.randint(0, 10, (6,), generator=g)
    assert torch.equal(module_loss.cross_entropy(x, y), F.cross_entropy(x.float(), y))
    assert torch.equal(module_loss.label_smoothing_cross_entropy(x, y), F.cross_entropy(x.float(), y, label_smoothing=0.1))


# ----------------------------------------------------------------------------- config, end to end
def test_shipped_mix_config_parses(tmp_path):
    from pytorch_distributed_template_amd import models, optim
    from pytorch_distributed_template_amd.config import ConfigParser
    cfg = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix.json").read_text())
    lamb = json.loads((ROOT / "config" / "vit_b16_fp8_lamb.json").read_text())
    assert cfg["loss"] == "label_smoothing_cross_entropy" and hasattr(module_loss, cfg["loss"])
    assert cfg["optimizer"] == lamb["optimizer"] and cfg["arch"] == lamb["arch"]
    assert hasattr(models, cfg["arch"]["type"]) and hasattr(optim, cfg["optimizer"]["type"])
    args = cfg["train_loader"]["args"]
    assert cfg["train_loader"]["type"] == "PackedImageLoader" and args["mixup_alpha"] == 0.8 \
        and args["cutmix_alpha"] == 1.0
    assert cfg["valid_loader"]["args"]["training"] is False
    R.make_set(tmp_path / "s", 6, 20, 20)
    cfg["trainer"]["save_dir"] = str(tmp_path / "ck")
    for k in ("train_loader", "valid_loader"):
        cfg[k]["args"].update(data_dir=str(tmp_path / "s"), batch_size=4, image_size=16, device="cpu")
    parsed = ConfigParser(cfg, run_id="mix")
    train, valid = parsed.init_obj("train_loader", module_data), parsed.init_obj("valid_loader", module_data)
    assert train.mixing and not valid.mixing
    assert isinstance(next(iter(train))[1], MixedTarget) and torch.is_tensor(next(iter(valid))[1])


def test_train_py_cpu_with_mixing(tmp_path):
    R.make_set(tmp_path / "train", 12, 20, 20, num_classes=5, seed=1)
    R.make_set(tmp_path / "val", 6, 20, 20, num_classes=5, seed=2)
    loader = {"batch_size": 4, "image_size": 16, "device": "cpu"}
    cfg = {
        "name": "MixCPU",
        "arch": {"type": "VisionTransformer", "args": {"image_size": 16, "patch_size": 8, "embed_dim": 32, "depth": 1,
                                                       "num_heads": 2, "num_classes": 5}},
        "train_loader": {"type": "PackedImageLoader",
                         "args": dict(loader, data_dir=str(tmp_path / "train"), mixup_alpha=0.8, cutmix_alpha=1.0,
                                      mix_mode="elem")},
        "valid_loader": {"type": "PackedImageLoader",
                         "args": dict(loader, data_dir=str(tmp_path / "val"), training=False)},
        "optimizer": {"type": "SGD", "args": {"lr": 0.01}},
        "loss": "label_smoothing_cross_entropy",
        "metrics": ["accuracy"],
        "trainer": {"epochs": 2, "save_dir": str(tmp_path / "ck"), "save_period": 2, "verbosity": 2,
                    "monitor": "off", "tensorboard": False},
    }
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(cfg))
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2", PDT_RUN_ID="mix", CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "train.py", "-c", str(p), "--seed", "0"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = (tmp_path / "ck" / "MixCPU" / "train" / "mix" / "info.log").read_text()
    assert "    epoch          : 2" in log
    vals = {}
    for line in log.splitlines():
        for key in ("loss", "val_loss"):
            if f"    {key} " in line and ":" in line:
                vals[key] = float(line.rsplit(":", 1)[1])
    assert np.isfinite(vals["loss"]) and np.isfinite(vals["val_loss"]) and vals["val_loss"] > 0
