"""Stochastic depth (drop-path) without a GPU: the torch mirror of the draw (ops/drop_path.py),
the rate schedule, and the ViT's torch path against a float64 reference that writes the scaled
residual adds out independently (tests/drop_path_ref.py)."""
import json
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import drop_path_ref as dr
from pytorch_distributed_template_amd.models.vit import VisionTransformer, ViT_B_16
from pytorch_distributed_template_amd.ops import drop_path as dp
from pytorch_distributed_template_amd.ops import fused

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------ mirror
def test_mirror_is_a_function_of_seed_and_step():
    a = dr.expected_table(11, 3, 0.5, 64, n_branches=6)
    assert torch.equal(a, dr.expected_table(11, 3, 0.5, 64, n_branches=6))
    assert not torch.equal(a, dr.expected_table(11, 4, 0.5, 64, n_branches=6))
    assert not torch.equal(a, dr.expected_table(12, 3, 0.5, 64, n_branches=6))
    assert set(a.unique().tolist()) == {0.0, 2.0}
    assert not torch.equal(a[0], a[1])  # branches draw independently


def test_mirror_does_not_depend_on_the_split_over_ranks():
    B = 37
    whole = dr.expected_table(5, 9, 0.5, 2 * B, n_branches=4)
    parts = [dr.expected_table(5, 9, 0.5, B, rank=r, n_branches=4) for r in (0, 1)]
    assert torch.equal(whole, torch.cat(parts, dim=1))
    assert not torch.equal(parts[0], parts[1])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_within_four_binomial_deviations(p):
    n = 2 ** 16
    table = dr.expected_table(2024, 0, p, n, n_branches=4)
    sd = (p * (1 - p) / n) ** 0.5
    for j in range(4):
        kept = (table[j] != 0).double().mean().item()
        assert abs(kept - (1 - p)) <= 4 * sd, (j, kept)
    assert set(table.unique().tolist()) == {0.0, float(torch.tensor(1 / (1 - p), dtype=torch.float32))}


def test_rate_schedule_is_linear_from_zero_to_the_rate():
    rates = dp.drop_path_rates(0.1, 12)
    assert rates[0] == 0.0 and rates[-1] == pytest.approx(0.1) and len(rates) == 12
    steps = [b - a for a, b in zip(rates, rates[1:])]
    assert all(s == pytest.approx(0.1 / 11) for s in steps)
    assert dp.drop_path_rates(0.3, 1) == [0.0]
    m = dr.tiny_vit(drop_path_rate=0.2)
    assert m.drop_path_rates == pytest.approx([0.0, 0.1, 0.2])
    assert m.drop_path_p.tolist() == pytest.approx([0, 0, 0.1, 0.1, 0.2, 0.2])
    with pytest.raises(ValueError):
        dp.drop_path_rates(1.0, 4)


# ------------------------------------------------------------------------------------- model
def run(model, x, t):
    model.zero_grad(set_to_none=True)
    loss = F.cross_entropy(model(x), t)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def test_eval_mode_is_the_model_without_drop_path():
    x, _ = dr.tiny_batch()
    m0, m1 = dr.tiny_vit().eval(), dr.tiny_vit(drop_path_rate=0.5).eval()
    with torch.no_grad():
        assert torch.equal(m1(x), m0(x))
    assert m1.drop_path_state.tolist() == [0, 0]  # no draw, no step


def test_rate_zero_is_the_model_without_the_argument():
    x, t = dr.tiny_batch()
    m0, m1 = dr.tiny_vit().train(), dr.tiny_vit(drop_path_rate=0.0, drop_path_seed=9).train()
    assert list(m1.state_dict()) == list(m0.state_dict())
    assert [n for n, _ in m1.named_buffers()] == [n for n, _ in m0.named_buffers()]
    (l0, g0), (l1, g1) = run(m0, x, t), run(m1, x, t)
    assert torch.equal(l0, l1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_state_dict_has_no_drop_path_keys_and_interchanges():
    m0, m1 = dr.tiny_vit(), dr.tiny_vit(seed=1, drop_path_rate=0.3, drop_path_seed=4)
    assert list(m1.state_dict()) == list(m0.state_dict())
    m1.load_state_dict(m0.state_dict())
    m0.load_state_dict(m1.state_dict())
    assert m1.drop_path_state.tolist() == [4, 0]


def test_training_forward_draws_the_mirrors_table_and_advances_the_step():
    x, _ = dr.tiny_batch()
    m = dr.tiny_vit(drop_path_rate=0.5, drop_path_seed=21).train()
    for step in range(3):
        m(x)
        want = dp.drop_path_table(21, step, m.drop_path_p, m.drop_path_inv_keep, x.shape[0])
        assert torch.equal(m.drop_path_table, want), step
        assert m.drop_path_state.tolist() == [21, step + 1]


def check_against_f64(model, table=None, cls_prune=False):
    """Loss and every gradient of the torch path (fp32) against the float64 reference; raises
    AssertionError where they differ beyond fp32 rounding."""
    x, t = dr.tiny_batch()
    table = dr.explicit_table() if table is None else table
    model.train()
    model.cls_prune = cls_prune
    model.drop_path_forced = table
    loss, grads = run(model, x, t)
    ref_loss, ref = dr.vit_f64_ref(model, x, t, table)
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-6)
    for n, g in ref.items():
        # fp32 evaluation of a 3-block model against float64: 1e-4 of the gradient's largest entry
        torch.testing.assert_close(grads[n].double(), g, rtol=1e-4, atol=1e-4 * g.abs().max().item() + 1e-9, msg=n)


@pytest.mark.parametrize("cls_prune", [False, True])
def test_torch_path_matches_float64(cls_prune):
    check_against_f64(dr.tiny_vit(drop_path_rate=0.5), cls_prune=cls_prune)


def test_all_samples_of_one_block_dropped_gives_that_block_zero_gradients():
    x, t = dr.tiny_batch()
    m = dr.tiny_vit(drop_path_rate=0.5).train()
    table = dr.explicit_table()
    table[2:4] = 0.0  # block 1, both branches, every sample
    m.drop_path_forced = table
    _, grads = run(m, x, t)
    for n, g in grads.items():
        if n.startswith("blocks.1."):
            assert not bool(g.any()), n
        elif not n.startswith("blocks."):
            assert bool(g.any()), n
    check_against_f64(m, table)


# --------------------------------------------------------------------------- seeded faults
def _faulty(kind):
    def scaled_add(y, r, scale):
        s = scale.to(y.dtype).reshape(-1, *([1] * (y.dim() - 1)))
        if kind == "no_keep_factor":      # the 1 / keep factor is missing: a plain mask
            return r + (s != 0).to(y.dtype) * y
        if kind == "row_indexed":         # the mask indexed by row instead of by sample
            rows = y.reshape(-1, y.shape[-1]).shape[0]
            sr = scale.to(y.dtype)[torch.arange(rows) % scale.numel()].reshape(*y.shape[:-1], 1)
            return r + sr * y
        if kind == "no_backward_scale":   # the scale is missing in the backward
            return r + (s * y).detach() + (y - y.detach())
        raise KeyError(kind)
    return scaled_add


@pytest.mark.parametrize("kind", ["no_backward_scale", "no_keep_factor", "row_indexed"])
def test_seeded_fault_is_rejected(kind, monkeypatch):
    m = dr.tiny_vit(drop_path_rate=0.5)
    check_against_f64(m)  # the check passes on the real code ...
    monkeypatch.setattr(dp, "scaled_add", _faulty(kind))
    with pytest.raises(AssertionError):  # ... and fails with the fault in place
        check_against_f64(m)


def test_torch_ln_add_fork_scale_defaults_and_shape_checks():
    ln = torch.nn.LayerNorm(256)
    y, r = torch.randn(4, 5, 256), torch.randn(4, 5, 256)
    s0, h0 = fused.ln_add_fork(y, r, ln)
    assert torch.equal(s0, y + r) and torch.equal(h0, ln(y + r))
    scale = torch.tensor([2.0, 0.0, 2.0, 0.0])
    yn = y.clone()
    yn[1] = float("nan")
    s, h = fused.ln_add_fork(yn, r, ln, scale=scale)
    assert torch.equal(s[1], r[1]) and torch.equal(s[3], r[3]) and torch.equal(s[0], r[0] + 2 * y[0])
    assert not bool(torch.isnan(h).any())
    with pytest.raises(ValueError):
        fused.ln_add_fork(y, r, ln, scale=scale[:3])
    with pytest.raises(ValueError):
        fused.ln_add_fork(y, r, ln, scale=scale, rows_per_sample=1)


# ---------------------------------------------------------------------------- config surface
def test_config_passes_drop_path_rate_to_the_model(tmp_path):
    cfg = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix_ema_dp.json").read_text())
    base = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix_ema.json").read_text())
    assert cfg["arch"]["args"]["drop_path_rate"] == 0.1
    assert cfg["trainer"]["ema"] == base["trainer"]["ema"] and cfg["optimizer"] == base["optimizer"]
    # through the project's parser and factory, as train.py builds the model (``arch.args``)
    from pytorch_distributed_template_amd import models
    from pytorch_distributed_template_amd.config import ConfigParser
    cfg["trainer"]["save_dir"] = str(tmp_path / "ck")
    cfg["arch"]["args"].update(depth=2, embed_dim=256, num_heads=4, image_size=32, num_classes=10)
    m = ConfigParser(cfg, run_id="DP").init_obj("arch", models)
    assert isinstance(m, ViT_B_16) and isinstance(m, VisionTransformer) and m.fp8
    assert m.drop_path_rates == pytest.approx([0.0, 0.1])
