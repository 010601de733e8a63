"""Trainer with a mixing PackedImageLoader on an MI355X: the native bf16 ResNet-50 (the smallest
native model the GPU Trainer tests run) on a 64-image packed set, batch 8, Mixup / CutMix on --
eagerly, and with ``trainer.hip_graph`` (the three target tensors are static graph inputs)."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.data import MixedTarget, PackedImageLoader  # noqa: E402
from pytorch_distributed_template_amd.trainer.trainer import GRAPH_WARMUP  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def packed64(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed64mix")
    R.make_set(d, 64, 40, 56, num_classes=5, seed=21)
    return d


def _trainer(data_dir, save_dir, hip_graph, run_id):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    cfg = json.loads((ROOT / "config" / "resnet50_bf16_packed.json").read_text())
    cfg["arch"]["args"]["num_classes"] = 8  # the set's 5 classes; the native classifier needs N % 8 == 0
    cfg["trainer"].update(save_dir=str(save_dir), len_epoch=3, epochs=1, verbosity=1, hip_graph=hip_graph)
    for k in ("train_loader", "valid_loader", "test_loader"):
        cfg[k]["args"].update(data_dir=str(data_dir), batch_size=8)
    cfg["train_loader"]["args"].update(mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem", seed=5)
    torch.manual_seed(0)
    device = torch.device("cuda", torch.cuda.current_device())
    config = ConfigParser(cfg, run_id=run_id)
    model = build_model(config, device)
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    train_loader, valid_loader = build_loader(config, "train_loader"), build_loader(config, "valid_loader")
    assert isinstance(train_loader, PackedImageLoader) and train_loader.mixing and not valid_loader.mixing
    return Trainer(model, criterion, metrics, optimizer, config=config, device=device, data_loader=train_loader,
                   valid_data_loader=valid_loader, lr_scheduler=sched, len_epoch=3,
                   autocast_dtype=autocast_dtype(config, device), channels_last=True)


def _steps(trainer, n):
    """n training steps driven the way _train_epoch drives them; the per-step losses."""
    losses = []
    trainer.model.train()
    trainer._on_epoch_start(1)
    for k, (data, target) in enumerate(trainer.data_loader):
        assert isinstance(target, MixedTarget)
        data, target = trainer._to_device(data, target)
        if trainer.hip_graph:
            loss = trainer._graph_step(data, target)
        else:
            loss = trainer._step_body(data, target)
        losses.append(float(loss.detach().float().item()))
        if k + 1 >= n:
            break
    return losses


def test_trainer_eager_with_mixing(packed64, tmp_path, monkeypatch):
    from pytorch_distributed_template_amd.ops import fused
    monkeypatch.setenv("PDT_AUTOTUNE", "0")  # shipped choices or the heuristic: no variant timing in a test
    try:
        trainer = _trainer(packed64, tmp_path, False, "eager")
        before = trainer.model.fc.weight.detach().clone()
        log = trainer._train_epoch(1)  # 3 steps, then validation with plain labels
    finally:
        fused.set_backend("auto")
    print(log)
    assert np.isfinite(log["loss"]) and np.isfinite(log["val_loss"]) and 0.0 <= log["val_accuracy"] <= 1.0
    assert not torch.equal(before, trainer.model.fc.weight.detach())


def test_trainer_hip_graph_with_mixing_matches_eager(packed64, tmp_path, monkeypatch):
    """GRAPH_WARMUP eager steps, the capture, 2 replays; the replayed losses against an eager run of
    the same seeded job within the rtol / atol of tests/test_hip_graph_gpu.py. Then replays
    with the weights frozen and other values in the static target buffers: the loss must follow
    ``lam`` and each label vector, so the graph reads the three target tensors as inputs."""
    from pytorch_distributed_template_amd.ops import fused
    monkeypatch.setenv("PDT_AUTOTUNE", "0")
    monkeypatch.setenv("PDT_DETERMINISTIC", "1")  # fixed kernel variants: the two runs take the same ones
    n = GRAPH_WARMUP + 2
    try:
        eager = _steps(_trainer(packed64, tmp_path / "e", False, "eager"), n)
        trainer = _trainer(packed64, tmp_path / "g", True, "graph")
        assert trainer.hip_graph
        graph = _steps(trainer, n)
        assert trainer._graph is not None and trainer._graph_eager_steps == GRAPH_WARMUP
        gx, gy, gloss = trainer._graph_io
        assert isinstance(gy, MixedTarget) and all(t.is_cuda for t in gy)
        print("eager", eager[-3:], "graph", graph[-3:])
        assert all(np.isfinite(graph)) and all(np.isfinite(eager))
        torch.testing.assert_close(torch.tensor(graph[-2:]), torch.tensor(eager[-2:]), rtol=1e-3, atol=1e-4)
        # the weights frozen (lr = 0: the replayed optimizer step adds nothing), the same images: only
        # the graph's target inputs change between the replays below
        for group in trainer.optimizer.param_groups:
            group["lr"] = 0.0
        trainer.optimizer.refresh_scalars()

        def replay():
            trainer._graph.replay()
            return float(gloss.item())
        gy.label_b.copy_((gy.label_a + 1) % 5)  # two different labels in every row
        gy.lam.fill_(0.25)
        a, a2 = replay(), replay()
        gy.lam.fill_(0.75)
        b = replay()
        print("replay at lam 0.25:", a, a2, "at lam 0.75:", b)
        assert np.isfinite(a) and abs(a - b) > 1e-3 * abs(a) and abs(a - a2) < 0.01 * abs(a - b)
        saved = gy.label_a.clone()
        gy.label_a.fill_(-1)  # a row with a label out of range contributes exactly 0
        assert replay() == 0.0
        gy.label_a.copy_(saved)
        gy.label_b.fill_(-1)
        assert replay() == 0.0
    finally:
        fused.set_backend("auto")
