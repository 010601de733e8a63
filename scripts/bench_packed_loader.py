#!/usr/bin/env python
"""Measure the packed-image input pipeline on one MI355X (output kept as
profiles/packed_loader.txt).

    python scripts/bench_packed_loader.py [--batch 2048] [--n 32768] [--train-batch 256] [--skip-train]

1. kernel: pdt_crop_resize_norm_u8_bf16 at ``--batch`` images, 256x256 store -> 224, training
   boxes, against its byte floor -- the bf16 bytes written plus the uint8 bytes of the crop
   boxes read, at the streaming rate a device copy of the same size reaches in this run -- and
   against pdt_synth_images_bf16 at the same batch.
2. feed rate (img/s) of the resident and the staged PackedImageLoader alone over a generated
   set of ``--n`` images; staged mode split into host gather, H2D copy and kernel.
3. ResNet-50 bf16 training steps/s through Trainer with PackedImageLoader (resident) against
   SyntheticImageNetLoader: 20 timed steps after a warm-up epoch, two runs each.

4. ``--mix``: the launch with Mixup / CutMix (pdt_crop_resize_norm_mix_u8_bf16) -- no mixing,
   all-CutMix, all-Mixup -- against the plain entry point, three rounds of each for the run-to-run
   spread; and with training, ResNet-50 steps/s with a mixing loader against the same loader
   without mixing.
5. ``--erase``: the launch with Random Erasing (pdt_crop_resize_norm_erase_u8_bf16) beside the plain
   and the mixing entry points of the same build, three alternating rounds each: nothing to erase,
   re_prob 0.25 with drawn rectangles in both modes, every sample erased, and erasing on top of
   all-Mixup.

A run without a GPU fails: nothing here falls back to the CPU.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pytorch_distributed_template_amd.data import PackedImageLoader, random_resized_crop_boxes  # noqa: E402
from pytorch_distributed_template_amd.ops import native_ops  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def event_ms(fn, iters=20, warmup=3):
    """Mean device time of fn() in ms (HIP events around ``iters`` back-to-back calls)."""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def make_set(path, n, size=256, num_classes=1000, seed=0):
    rng = np.random.default_rng(seed)
    path.mkdir(parents=True, exist_ok=True)
    images = np.lib.format.open_memmap(path / "images.npy", mode="w+", dtype=np.uint8, shape=(n, size, size, 3))
    step = 1024
    for i in range(0, n, step):
        images[i:i + step] = rng.integers(0, 256, size=images[i:i + step].shape, dtype=np.uint8)
    images.flush()
    del images
    np.save(path / "labels.npy", rng.integers(0, num_classes, size=n, dtype=np.int64))
    (path / "meta.json").write_text(json.dumps({"num_classes": num_classes}))


def bench_kernel(B, dev):
    print(f"== kernel: B={B}, 256x256x3 uint8 store -> 224x224x4 bf16, RandomResizedCrop boxes")
    Hs = Ws = 256
    S = 224
    n_src = min(B, 4096)
    src = torch.randint(0, 256, (n_src, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    idx = (torch.randperm(B, device=dev) % n_src).to(torch.int64)
    box = random_resized_crop_boxes(torch.arange(B), 0, 0, Hs, Ws)
    box_d = box.to(dev)
    out = torch.empty((B, S, S, 4), dtype=torch.bfloat16, device=dev)
    t = event_ms(lambda: native_ops.crop_resize_normalize(src, idx, box_d, out, MEAN, STD))
    wr = out.numel() * 2
    rd = int((box[:, 2].long() * box[:, 3].long()).sum()) * 3
    # streaming rate of this device, now: a copy that moves as many bytes as the kernel's floor
    words = (wr + rd) // 2 // 8 * 2
    a = torch.empty(words, dtype=torch.int32, device=dev)
    b = torch.empty(words, dtype=torch.int32, device=dev)
    t_copy = event_ms(lambda: b.copy_(a))
    rate = 2 * words * 4 / (t_copy * 1e-3)
    floor = (wr + rd) / rate * 1e3
    print(f"crop_resize_norm: {t:.3f} ms   ({B / t * 1e3:,.0f} img/s)")
    print(f"bytes: {wr / 1e6:.0f} MB written + {rd / 1e6:.0f} MB of crop boxes read (full frames: "
          f"{B * Hs * Ws * 3 / 1e6:.0f} MB)")
    print(f"device copy of {2 * words * 4 / 1e6:.0f} MB (read+write): {t_copy:.3f} ms = {rate / 1e12:.2f} TB/s")
    print(f"byte floor at that rate: {floor:.3f} ms -> the kernel reaches {100 * floor / t:.0f} % of it")
    full = torch.tensor([[0, 0, Hs, Ws, 0]] * B, dtype=torch.int32, device=dev)
    t_full = event_ms(lambda: native_ops.crop_resize_normalize(src, idx, full, out, MEAN, STD))
    ident = torch.tensor([[16, 16, S, S, 0]] * B, dtype=torch.int32, device=dev)
    t_id = event_ms(lambda: native_ops.crop_resize_normalize(src, idx, ident, out, MEAN, STD))
    print(f"same launch, full-frame boxes (gather side at its largest, {B * Hs * Ws * 3 / 1e6:.0f} MB read): "
          f"{t_full:.3f} ms; identity center crop ({B * S * S * 3 / 1e6:.0f} MB read): {t_id:.3f} ms")
    fill = torch.empty_like(out)
    t_fill = event_ms(lambda: fill.zero_())
    print(f"store side alone (zero fill of the {wr / 1e6:.0f} MB output): {t_fill:.3f} ms")
    y = torch.empty(B, dtype=torch.int64, device=dev)
    gi = torch.arange(B, dtype=torch.int64, device=dev)
    t_syn = event_ms(lambda: native_ops.synthetic_images_at(out, gi, 3, 1, y, 1000))
    print(f"pdt_synth_images_bf16 at the same batch: {t_syn:.3f} ms (crop_resize_norm / synth = {t / t_syn:.2f}x)")


def bench_mix_kernel(B, dev):
    print(f"== mixing launch: B={B}, 256x256x3 uint8 store -> 224x224x4 bf16, RandomResizedCrop boxes, partner = "
          "the reversed batch")
    from pytorch_distributed_template_amd.data import mix_params
    Hs = Ws = 256
    S = 224
    n_src = min(B, 4096)
    src = torch.randint(0, 256, (n_src, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    idx = (torch.randperm(B, device=dev) % n_src).to(torch.int64)
    box = random_resized_crop_boxes(torch.arange(B), 0, 0, Hs, Ws).to(dev)
    pidx, pbox = idx.flip(0).contiguous(), box.flip(0).contiguous()
    out = torch.empty((B, S, S, 4), dtype=torch.bfloat16, device=dev)
    variants = {"plain entry point": None}
    for name, kw in (("mix entry point, no mixing", dict(mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.0)),
                     ("all CutMix (alpha 1.0)", dict(cutmix_alpha=1.0)), ("all Mixup (alpha 0.8)", dict(mixup_alpha=0.8))):
        _, w_own, rect, _ = mix_params(list(range(B)), 0, 0, S, mix_mode="elem", **kw)
        variants[name] = (rect.to(dev), w_own.to(dev))
    times = {k: [] for k in variants}
    for _ in range(3):
        for name, v in variants.items():
            if v is None:
                fn = lambda: native_ops.crop_resize_normalize(src, idx, box, out, MEAN, STD)  # noqa: E731
            else:
                fn = lambda v=v: native_ops.crop_resize_normalize_mix(src, idx, box, pidx, pbox, v[0], v[1], out,  # noqa: E731
                                                                      MEAN, STD)
            times[name].append(event_ms(fn))
    base = min(times["plain entry point"])
    for name, t in times.items():
        print(f"{name:28s}: " + ", ".join(f"{x:.3f}" for x in t) + f" ms   (best / plain best = {min(t) / base:.2f}x)")


def bench_erase_kernel(B, dev):
    print(f"== erasing launch: B={B}, 256x256x3 uint8 store -> 224x224x4 bf16, RandomResizedCrop boxes, "
          "pdt_crop_resize_norm_erase_u8_bf16 beside the plain and the mixing entry points")
    from pytorch_distributed_template_amd.data import erase_keys, mix_params, random_erasing_rects
    from pytorch_distributed_template_amd.data.packed import u32_bits
    Hs = Ws = 256
    S = 224
    n_src = min(B, 4096)
    src = torch.randint(0, 256, (n_src, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    idx = (torch.randperm(B, device=dev) % n_src).to(torch.int64)
    box = random_resized_crop_boxes(torch.arange(B), 0, 0, Hs, Ws).to(dev)
    pidx, pbox = idx.flip(0).contiguous(), box.flip(0).contiguous()
    out = torch.empty((B, S, S, 4), dtype=torch.bfloat16, device=dev)
    _, w_own, rect, _ = mix_params(list(range(B)), 0, 0, S, mix_mode="elem", mixup_alpha=0.8)
    mixed = (pidx, pbox, rect.to(dev), w_own.to(dev))
    ekey = u32_bits(erase_keys(torch.arange(B), 0, 0)).to(dev)
    rects = {p: random_erasing_rects(torch.arange(B), 0, 0, S, re_prob=p) for p in (0.0, 0.25, 1.0)}
    for p, r in rects.items():
        area = ((r[..., 2] - r[..., 0]).long() * (r[..., 3] - r[..., 1]).long()).sum().item() / (B * S * S)
        print(f"re_prob {p}: {int((r[:, 0, 2] > r[:, 0, 0]).sum())} of {B} samples erased, {100 * area:.1f} % of the pixels")
    rects = {p: r.to(dev) for p, r in rects.items()}

    def erase(p, mode, mix=None):
        return lambda: native_ops.crop_resize_normalize_erase(src, idx, box, mix, rects[p], ekey, mode, out, MEAN, STD)
    variants = {
        "plain entry point": lambda: native_ops.crop_resize_normalize(src, idx, box, out, MEAN, STD),
        "erase entry point, nothing to erase": erase(0.0, "pixel"),
        "re_prob 0.25, pixel": erase(0.25, "pixel"),
        "re_prob 0.25, const": erase(0.25, "const"),
        "every sample erased, pixel": erase(1.0, "pixel"),
        "every sample erased, const": erase(1.0, "const"),
        "mix entry point, all Mixup (alpha 0.8)": lambda: native_ops.crop_resize_normalize_mix(src, idx, box, *mixed, out,
                                                                                              MEAN, STD),
        "all Mixup, nothing to erase": erase(0.0, "pixel", mixed),
        "all Mixup, re_prob 0.25, pixel": erase(0.25, "pixel", mixed),
        "all Mixup, every sample erased, pixel": erase(1.0, "pixel", mixed),
    }
    times = {k: [] for k in variants}
    for _ in range(3):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    base = min(times["plain entry point"])
    for name, t in times.items():
        print(f"{name:40s}: " + ", ".join(f"{x:.3f}" for x in t) + f" ms   (best / plain best = {min(t) / base:.2f}x)")


def bench_train_mix(data_dir, batch, dev):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.ops import fused
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    print(f"== ResNet-50 bf16 native through Trainer, batch {batch}, label smoothing: PackedImageLoader with and "
          "without Mixup 0.8 / CutMix 1.0; 20 timed steps after a warm-up epoch")
    save = tempfile.mkdtemp(prefix="pdt_bench_")
    for run in (1, 2):
        for name, mix in (("no mixing", {}), ("mixup+cutmix", dict(mixup_alpha=0.8, cutmix_alpha=1.0))):
            cfg = json.loads((ROOT / "config" / "resnet50_bf16_packed.json").read_text())
            cfg["train_loader"]["args"].update(data_dir=str(data_dir), batch_size=batch, resident=True, **mix)
            cfg["trainer"].update(save_dir=save, verbosity=0)
            config = ConfigParser(cfg, run_id=f"mix{run}{len(mix)}")
            model = build_model(config, dev)
            criterion, metrics = build_criterion_metrics(config)
            optimizer, sched = build_optimizer(config, model)
            loader = build_loader(config, "train_loader")
            tr = Trainer(model, criterion, metrics, optimizer, config=config, device=dev, data_loader=loader,
                         valid_data_loader=None, lr_scheduler=sched, len_epoch=6,
                         autocast_dtype=autocast_dtype(config, dev), channels_last=True)
            tr._train_epoch(1)
            tr.len_epoch = 20
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            log = tr._train_epoch(2)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"run {run} {name:14s}: {20 / dt:.3f} steps/s  {20 * batch / dt:,.0f} img/s  loss {log['loss']:.3f}")
            del tr, model, optimizer, loader
            torch.cuda.empty_cache()
    fused.set_backend("auto")


def bench_feed(data_dir, B, dev):
    print(f"== feed rate: PackedImageLoader alone, batch {B}")
    for mode, resident in (("resident", True), ("staged", False)):
        dl = PackedImageLoader(data_dir, batch_size=B, resident=resident, prefetch=2, device=dev)
        t0 = time.perf_counter()
        for x, y in dl:  # first epoch: upload / ring allocation / page cache
            pass
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        rates = []
        for epoch in (1, 2):
            dl.set_epoch(epoch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for x, y in dl:
                n += x.shape[0]
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
        print(f"{mode}: first epoch {t_first:.2f} s (set-up included); then "
              + ", ".join(f"{r:,.0f}" for r in rates) + " img/s")
    # staged mode's three stages, one after the other, on one batch
    dl = PackedImageLoader(data_dir, batch_size=B, resident=False, device=dev)
    ds = dl.dataset
    idx = np.sort(np.array(list(dl.sampler)[:B], dtype=np.int64))
    pinned = torch.empty((B,) + tuple(ds.images.shape[1:]), dtype=torch.uint8, pin_memory=True)
    staged = torch.empty(pinned.shape, dtype=torch.uint8, device=dev)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        np.take(ds.images, idx, axis=0, out=pinned.numpy())
        ts.append(time.perf_counter() - t0)
    t_h2d = event_ms(lambda: staged.copy_(pinned, non_blocking=True), iters=5, warmup=1)
    box = dl.boxes(idx.tolist()).to(dev)
    kidx = torch.arange(B, dtype=torch.int64, device=dev)
    out = torch.empty((B, dl.image_size, dl.image_size, 4), dtype=torch.bfloat16, device=dev)
    t_k = event_ms(lambda: native_ops.crop_resize_normalize(staged, kidx, box, out, MEAN, STD))
    mb = pinned.numel() / 1e6
    print(f"staged, one batch of {B} ({mb:.0f} MB): host gather {min(ts) * 1e3:.1f} ms "
          f"({mb / min(ts) / 1e3:.2f} GB/s, one thread, sorted indices, page cache warm), "
          f"H2D copy {t_h2d:.1f} ms ({mb / t_h2d:.1f} GB/s), kernel {t_k:.3f} ms")
    print(f"staged ceiling from its slowest stage: {B / max(min(ts), t_h2d * 1e-3, t_k * 1e-3):,.0f} img/s")


def bench_train(data_dir, batch, dev):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.ops import fused
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    print(f"== ResNet-50 bf16 native through Trainer, batch {batch}: 20 timed steps after a warm-up epoch")
    base = json.loads((ROOT / "config" / "resnet50_bf16.json").read_text())
    packed = json.loads((ROOT / "config" / "resnet50_bf16_packed.json").read_text())
    packed["loss"] = base["loss"]  # the same loss on both sides: only the loader differs
    packed["train_loader"]["args"].update(data_dir=str(data_dir), batch_size=batch, resident=True)
    base["train_loader"]["args"].update(batch_size=batch)
    save = tempfile.mkdtemp(prefix="pdt_bench_")
    for run in (1, 2):
        for name, cfg in (("SyntheticImageNetLoader", base), ("PackedImageLoader", packed)):
            cfg["trainer"].update(save_dir=save, verbosity=0)
            config = ConfigParser(cfg, run_id=f"{name}{run}")
            model = build_model(config, dev)
            criterion, metrics = build_criterion_metrics(config)
            optimizer, sched = build_optimizer(config, model)
            loader = build_loader(config, "train_loader")
            tr = Trainer(model, criterion, metrics, optimizer, config=config, device=dev, data_loader=loader,
                         valid_data_loader=None, lr_scheduler=sched, len_epoch=6,
                         autocast_dtype=autocast_dtype(config, dev), channels_last=True)
            tr._train_epoch(1)  # warm-up: kernel variant choices, allocator, the resident upload
            tr.len_epoch = 20
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            log = tr._train_epoch(2)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"run {run} {name:24s}: {20 / dt:.3f} steps/s  {20 * batch / dt:,.0f} img/s  loss {log['loss']:.3f}")
            del tr, model, optimizer, loader
            torch.cuda.empty_cache()
    fused.set_backend("auto")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--n", type=int, default=32768, help="images in the generated set")
    ap.add_argument("--train-batch", type=int, default=256)
    ap.add_argument("--data-dir", default=None, help="an existing packed set (default: generate one)")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-feed", action="store_true")
    ap.add_argument("--mix", action="store_true", help="measure the Mixup / CutMix launch and training with it instead")
    ap.add_argument("--erase", action="store_true", help="measure the Random Erasing launch instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_packed_loader.py needs a GPU")
    native_ops.require()
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"device: {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; host CPUs used: "
          f"{os.environ.get('OMP_NUM_THREADS', 'all')}")
    if a.erase:
        bench_erase_kernel(a.batch, dev)
        return
    if a.mix:
        bench_mix_kernel(a.batch, dev)
        if not a.skip_train:
            with tempfile.TemporaryDirectory(prefix="pdt_packed_") as tmp:
                data_dir = Path(a.data_dir) if a.data_dir else Path(tmp) / "set"
                if not a.data_dir:
                    make_set(data_dir, a.n)
                bench_train_mix(data_dir, a.train_batch, dev)
        return
    bench_kernel(a.batch, dev)
    if a.skip_feed and a.skip_train:
        return
    with tempfile.TemporaryDirectory(prefix="pdt_packed_") as tmp:
        data_dir = Path(a.data_dir) if a.data_dir else Path(tmp) / "set"
        if not a.data_dir:
            t0 = time.perf_counter()
            make_set(data_dir, a.n)
            print(f"generated {a.n} random 256x256 images ({a.n * 196608 / 1e9:.1f} GB) in "
                  f"{time.perf_counter() - t0:.1f} s")
        if not a.skip_feed:
            bench_feed(data_dir, a.batch, dev)
        if not a.skip_train:
            bench_train(data_dir, a.train_batch, dev)


if __name__ == "__main__":
    main()
