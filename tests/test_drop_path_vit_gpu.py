"""Stochastic depth in the ViT on an MI355X: the tiny model of tests/drop_path_ref.py (depth 3,
width 256, 4 heads, 5 tokens, batch 4; 16 classes so that the head runs on the GEMM kernels) in
bf16 and fp8 -- native against the torch path under the same (seed, step), rate 0 / eval mode
against the model without the argument, a block with every sample dropped, the class-token-pruned
last block, a captured training step replayed, and two Trainer steps from a config.

Tolerances are those of tests/test_vit_fusion_gpu.py: native against the torch path in fp32,
relative L2 error of the logits / the worst parameter gradient, 3e-2 / 8e-2 in bf16
(test_vit_native_matches_torch_fp32) and 0.1 / 0.25 in fp8 after the scaling state has settled
(test_vit_fp8_steps_track_torch_fp32); class-token pruning on against off as
test_vit_cls_prune_native_matches_full."""
import json
from pathlib import Path

import pytest
import torch

import drop_path_ref as dr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import drop_path as dp  # noqa: E402
from pytorch_distributed_template_amd.ops import fused  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda")
CLASSES = 16


def nrmerr(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def vit(fp8, **kw):
    return dr.tiny_vit(num_classes=CLASSES, fp8=fp8, **kw).to(DEV)


def batch():
    x, t = dr.tiny_batch(device=DEV)
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), t % CLASSES


def step(model, x, t):
    model.zero_grad(set_to_none=True)
    logits = model(x)
    loss = fused.softmax_cross_entropy(logits, t)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().float(), loss.detach().float(), {n: p.grad.detach().float().clone()
                                                            for n, p in model.named_parameters()}


@pytest.fixture(autouse=True)
def _backend(monkeypatch):
    monkeypatch.setenv("PDT_AUTOTUNE", "0")
    yield
    fused.set_backend("auto")


@pytest.mark.parametrize("fp8", [False, True])
def test_native_matches_torch_path_under_the_same_seed_and_step(fp8):
    m = vit(fp8, drop_path_rate=0.5, drop_path_seed=77).train()
    x, t = batch()
    errs = []
    for it in range(3 if fp8 else 1):  # fp8: the first passes seed the delayed-scaling histories
        out = {}
        for backend in ("native", "torch"):
            fused.set_backend(backend)
            with torch.no_grad():
                m.drop_path_state[1] = it  # both arms at the same step
            out[backend] = step(m, x if backend == "native" else x.float(), t)
            table = m.drop_path_table.clone()
            assert torch.equal(table.cpu(), dp.drop_path_table(77, it, m.drop_path_p, m.drop_path_inv_keep, 4)), backend
            assert m.drop_path_state.tolist() == [77, it + 1], backend
        fused.set_backend("auto")
        worst = max((nrmerr(out["native"][2][n], out["torch"][2][n]), n) for n in out["torch"][2])
        errs.append((it, nrmerr(out["native"][0], out["torch"][0]), worst))
    print("MEASURED native vs torch", "fp8" if fp8 else "bf16", errs)
    for it, el, worst in errs:
        assert el < (0.1 if fp8 else 3e-2), errs
        assert worst[0] < (0.25 if fp8 else 8e-2), errs


@pytest.mark.parametrize("fp8", [False, True])
def test_rate_zero_and_eval_mode_are_the_model_without_the_argument(fp8):
    fused.set_backend("native")
    x, t = batch()
    m0 = vit(fp8).train()
    m1 = vit(fp8, drop_path_rate=0.0, drop_path_seed=3).train()
    assert list(m1.state_dict()) == list(m0.state_dict())
    for _ in range(2):  # (fp8: the second pass takes the fused delayed-scaling route)
        a, b = step(m0, x, t), step(m1, x, t)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for n in a[2]:
            assert torch.equal(a[2][n], b[2][n]), n
    m2 = vit(fp8, drop_path_rate=0.5).eval()
    m2.load_state_dict(m0.state_dict())
    m0.eval()
    with torch.no_grad():
        assert torch.equal(m2(x), m0(x))
    assert m2.drop_path_state.tolist() == [0, 0]


def test_bf16_block_with_every_sample_dropped_is_the_model_without_its_branches():
    fused.set_backend("native")
    x, t = batch()
    m = vit(False, drop_path_rate=0.5).train()
    table = dr.explicit_table().to(DEV)
    table[2:4] = 0.0  # block 1: both branches of every sample
    m.drop_path_forced = table
    logits, loss, grads = step(m, x, t)
    for n, g in grads.items():
        if n.startswith("blocks.1."):
            assert not bool(g.any()), n
    # the same model with block 1 taken out: blocks 0 and 2 keep their tables
    cut = vit(False, drop_path_rate=0.5).train()
    cut.load_state_dict(m.state_dict())
    del cut.blocks[1]
    cut.drop_path_rates = [m.drop_path_rates[0], m.drop_path_rates[2]]
    cut.drop_path_forced = torch.cat([table[0:2], table[4:6]])
    logits_c, loss_c, grads_c = step(cut, x, t)
    assert torch.equal(logits, logits_c) and torch.equal(loss, loss_c)
    for n, g in grads_c.items():
        full = n.replace("blocks.1.", "blocks.2.") if n.startswith("blocks.1.") else n
        assert torch.equal(grads[full], g), n


@pytest.mark.parametrize("fp8", [False, True])
def test_cls_prune_on_and_off_agree_under_the_same_masks(fp8, monkeypatch):
    fused.set_backend("native")
    x, t = batch()
    m = vit(fp8, drop_path_rate=0.5).train()
    m.drop_path_forced = dr.explicit_table().to(DEV)

    def run(model, prune, warm):
        monkeypatch.setenv("PDT_VIT_CLS_PRUNE", prune)
        for mod in model.modules():  # fresh fp8 scaling state for each arm
            for a in ("_pdt_fp8_meta", "_pdt_fp8_gmeta"):
                if hasattr(mod, a):
                    delattr(mod, a)
        for _ in range(warm):
            step(model, x, t)
        return step(model, x, t)

    res = {prune: run(m, prune, 3 if fp8 else 0) for prune in ("0", "1")}
    l0, l1 = float(res["0"][1]), float(res["1"][1])
    assert abs(l1 - l0) < 2e-2 * abs(l0), (l1, l0)
    if not fp8:
        for n, g in res["0"][2].items():
            assert nrmerr(res["1"][2][n], g) < 2e-2, n
        return
    mb = vit(False, drop_path_rate=0.5).train()  # both fp8 arms against bf16 on the same weights and masks
    mb.load_state_dict(m.state_dict())
    mb.drop_path_forced = m.drop_path_forced
    ref = run(mb, "0", 0)[2]
    errs = {n: (nrmerr(res["0"][2][n], g), nrmerr(res["1"][2][n], g)) for n, g in ref.items()}
    print("MEASURED cls_prune fp8 (full, pruned) vs bf16", {n: tuple(round(v, 4) for v in e) for n, e in errs.items()})
    for n, (e_full, e_prune) in errs.items():
        assert e_full < 0.3, (n, errs)
        assert e_prune < 1.25 * e_full + 0.03, (n, errs)


@pytest.mark.parametrize("fp8", [False, True])
def test_captured_step_replays_advance_the_tables_on_the_device(fp8):
    from pytorch_distributed_template_amd.optim import FusedAdamW
    fused.set_backend("native")
    x, t = batch()
    m = vit(fp8, drop_path_rate=0.5, drop_path_seed=9).train()
    opt = FusedAdamW(m.parameters(), lr=1e-4, capturable=True)

    def body():
        opt.zero_grad(set_to_none=False)
        loss = fused.softmax_cross_entropy(m(x), t)
        loss.backward()
        opt.step()
        return loss

    warm = 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):  # eager warm-up: gradients, optimizer and fp8 scaling state exist
            body()
    torch.cuda.synchronize()
    assert m.drop_path_state.tolist() == [9, warm]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        loss = body()  # (recorded, not run)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert m.drop_path_state.tolist() == [9, warm]
    tables = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        tables.append(m.drop_path_table.cpu().clone())
        want = dp.drop_path_table(9, warm + k, m.drop_path_p, m.drop_path_inv_keep, 4)
        assert torch.equal(tables[-1], want), k
        assert m.drop_path_state.tolist() == [9, warm + k + 1]
        assert bool(torch.isfinite(loss).all())
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2])
    assert not torch.equal(tables[0], tables[2])


def test_two_trainer_steps_from_a_config_with_drop_path(tmp_path):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    cfg = json.loads((ROOT / "config" / "vit_b16_fp8.json").read_text())
    cfg["arch"]["args"].update(drop_path_rate=0.1, depth=3, embed_dim=256, num_heads=4, num_classes=CLASSES,
                               image_size=32)
    cfg["trainer"].update(save_dir=str(tmp_path), len_epoch=2, epochs=1, hip_graph=False)
    cfg["train_loader"]["args"].update(batch_size=4, num_samples=8, num_classes=CLASSES, image_size=32)
    cfg.pop("valid_loader", None)
    torch.manual_seed(0)
    config = ConfigParser(cfg, run_id="dp")
    model = build_model(config, DEV)
    assert model.drop_path_rates == pytest.approx([0.0, 0.05, 0.1])
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    tr = Trainer(model, criterion, metrics, optimizer, config=config, device=DEV,
                 data_loader=build_loader(config, "train_loader"), valid_data_loader=None, lr_scheduler=sched,
                 len_epoch=2, autocast_dtype=autocast_dtype(config, DEV), channels_last=True)
    tr._on_epoch_start(1)
    log = tr._train_epoch(1)
    torch.cuda.synchronize()
    assert log["loss"] == log["loss"] and abs(log["loss"]) < float("inf"), log
    assert model.drop_path_state.tolist() == [0, 2]
