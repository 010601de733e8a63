"""``trainer.ema`` on an MI355X: the native bf16 ResNet-50 (the smallest native model the GPU
Trainer tests run) at batch 16 on the synthetic loader, one epoch of ``GRAPH_WARMUP + 2`` steps
and a validation pass -- eagerly, and with ``trainer.hip_graph`` (the EMA update is captured with
the step; two replays). Both runs are made once and shared by the tests below; the last test
takes the captured run through a second epoch, all replays, and validates again."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.trainer.trainer import GRAPH_WARMUP  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
STEPS = GRAPH_WARMUP + 2
ENV = {"PDT_AUTOTUNE": "0",        # shipped choices or the heuristic: no variant timing in a test
       "PDT_DETERMINISTIC": "1"}   # fixed kernel variants: the two runs take the same ones


def _cfg(save_dir, hip_graph):
    cfg = json.loads((ROOT / "config" / "resnet50_bf16.json").read_text())
    cfg["trainer"].update(save_dir=str(save_dir), len_epoch=STEPS, epochs=1, verbosity=1, hip_graph=hip_graph,
                          ema={"decay": 0.9, "warmup": True, "validate": "both"})
    cfg["train_loader"]["args"].update(batch_size=16, num_samples=16 * STEPS)
    for k in ("valid_loader", "test_loader"):
        cfg[k]["args"].update(batch_size=16, num_samples=32)
    return cfg


def _trainer(cfg, run_id, resume=None):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_ema,
                                                          build_loader, build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    torch.manual_seed(0)
    device = torch.device("cuda", torch.cuda.current_device())
    config = ConfigParser(cfg, resume=resume, run_id=run_id)
    model = build_model(config, device)
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    ema = build_ema(config, model)
    assert ema is not None and ema.write_bf16_shadow and ema.decay == 0.9 and ema.warmup
    return Trainer(model, criterion, metrics, optimizer, config=config, device=device,
                   data_loader=build_loader(config, "train_loader"),
                   valid_data_loader=build_loader(config, "valid_loader"), lr_scheduler=sched, len_epoch=STEPS,
                   autocast_dtype=autocast_dtype(config, device), channels_last=True, ema=ema)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from pytorch_distributed_template_amd.ops import fused
    saved = {k: os.environ.get(k) for k in ENV}
    os.environ.update(ENV)
    out = {}
    try:
        for mode in ("eager", "graph"):
            tr = _trainer(_cfg(tmp_path_factory.mktemp(mode), mode == "graph"), mode)
            assert tr.hip_graph == (mode == "graph")
            tr._on_epoch_start(1)
            out[mode] = (tr, tr._train_epoch(1))
        torch.cuda.synchronize()
        yield out
    finally:
        fused.set_backend("auto")
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_eager_and_captured_averages_agree(runs):
    (eager, _), (graph, _) = runs["eager"], runs["graph"]
    assert graph._graph is not None and graph._graph_eager_steps == GRAPH_WARMUP and eager._graph is None
    assert eager.ema.num_updates == STEPS and graph.ema.num_updates == STEPS
    a, b = eager.ema.module.state_dict(), graph.ema.module.state_dict()
    moved = 0
    for (k, v), (_, m) in zip(a.items(), eager.model.state_dict().items()):
        if v.is_floating_point():
            assert torch.isfinite(b[k]).all(), k
            # as tests/test_hip_graph_gpu.py requires of the trained weights
            torch.testing.assert_close(b[k].float(), v.float(), rtol=1e-3, atol=1e-4, msg=k)
            moved += int(not torch.equal(v, m))
        else:
            assert torch.equal(b[k], v) and torch.equal(v, m), k  # num_batches_tracked is copied
    assert moved > 100  # an average, not a copy of the trained weights
    assert int(a["bn1.num_batches_tracked"]) == STEPS


def test_validation_reports_val_ema_and_casts_no_registered_weight(runs):
    from pytorch_distributed_template_amd.ops import native_ops as no
    for mode in ("eager", "graph"):
        tr, log = runs[mode]
        print(mode, log)
        for k in ("val_loss", "val_accuracy", "val_top_k_acc", "val_ema_loss", "val_ema_accuracy",
                  "val_ema_top_k_acc"):
            assert k in log and np.isfinite(log[k]), (mode, k)
        assert tr.model.training and not tr.ema.module.training
        ema = tr.ema
        params = list(ema.module.parameters())
        entries = {id(p): no._SHADOWS.get(id(p)) for p in params}
        registered = [p for p in params if id(p) in ema._shadows]
        assert len(registered) == len(params) > 100  # every ResNet-50 parameter is dense in its layout
        for p in registered:
            ent = entries[id(p)]
            assert ent is not None and ent[0] is ema._shadows[id(p)] and ent[1] == p._version, mode
        val = tr._valid_epoch(1, model=ema.module, prefix="ema_")
        assert set(val) == {"ema_loss", "ema_accuracy", "ema_top_k_acc"}
        assert val["ema_loss"] == pytest.approx(log["val_ema_loss"], rel=1e-4)
        for p in registered:
            # the forward read the shadow the update wrote: a cast (pdt_cast_f32_bf16) would have
            # replaced the entry with one holding a new tensor
            assert no._SHADOWS[id(p)] is entries[id(p)], mode
            assert no.bf16_weight(p) is ema._shadows[id(p)]
            assert torch.equal(ema._shadows[id(p)], p.detach().to(torch.bfloat16))


def test_checkpoint_round_trip_and_test_py_ema(runs, tmp_path):
    tr, log = runs["graph"]
    tr._save_checkpoint(1)
    path = tr.checkpoint_dir / "checkpoint-epoch1.pth"
    ck = torch.load(path, weights_only=True, map_location="cpu")
    assert {"state_dict_ema", "ema"} <= set(ck)
    assert ck["ema"] == {"num_updates": STEPS, "decay": 0.9, "warmup": True}
    for k, v in tr.ema.module.state_dict().items():
        assert torch.equal(ck["state_dict_ema"][k], v.cpu()), k
    saved = {k: os.environ.get(k) for k in ENV}
    os.environ.update(ENV)
    try:
        cfg = _cfg(tmp_path, False)
        cfg["trainer"]["epochs"] = 2
        resumed = _trainer(cfg, "resumed", resume=path)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert resumed.start_epoch == 2 and resumed.ema.num_updates == STEPS
    for k, v in ck["state_dict_ema"].items():
        assert torch.equal(resumed.ema.module.state_dict()[k].cpu(), v), k
    for k, v in ck["state_dict"].items():
        assert torch.equal(resumed.model.state_dict()[k].cpu(), v), k

    env = dict(os.environ, PYTHONPATH=str(ROOT), PDT_RUN_ID="t", **ENV)
    r = subprocess.run([sys.executable, "test.py", "-r", str(path), "--ema", "--backend", "native"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "'loss':" in out and "'accuracy':" in out
    loss = float(out.split("'loss':")[1].split(",")[0])
    # the test loader is the validation loader's twin: the averaged weights' validation loss
    assert loss == pytest.approx(log["val_ema_loss"], rel=1e-3)


def test_second_validation_after_replays_reads_current_weights(runs):
    """Replays rewrite the weights on the device and bump no version on the host, while the kernel
    layer caches derived weights (the stem's space-to-depth copy, padded and fp8 copies) per
    version: the validation after an epoch of replays must not read the copies the previous
    validation cached. Both validation losses of epoch 2 against fresh models loaded from the
    averaged and the trained ``state_dict`` (their caches are empty: everything is derived anew)."""
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import build_model
    tr, log1 = runs["graph"]
    done = tr.ema.num_updates
    versions = [p._version for p in tr.ema.module.parameters()]
    saved = {k: os.environ.get(k) for k in ENV}
    os.environ.update(ENV)
    try:
        tr._on_epoch_start(2)
        log2 = tr._train_epoch(2)  # STEPS replays, then both validations
        assert tr._graph_eager_steps == GRAPH_WARMUP and tr.ema.num_updates == done + STEPS
        assert all(p._version > v for p, v in zip(tr.ema.module.parameters(), versions))
        assert tr._replayed == {"model": False, "ema": False}
        for key, weights in (("val_ema_loss", tr.ema.module.state_dict()),
                             ("val_loss", tr.model.state_dict())):
            fresh = build_model(ConfigParser(_cfg(tr.checkpoint_dir, False), run_id="fresh"), tr.device)
            fresh.load_state_dict(weights)
            want = tr._valid_epoch(2, model=fresh, prefix="ema_")["ema_loss"]
            print(key, "epoch 1", log1[key], "epoch 2", log2[key], "fresh model", want)
            assert np.isfinite(want) and log2[key] == pytest.approx(want, rel=1e-4), key
            assert log2[key] != log1[key], key
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
