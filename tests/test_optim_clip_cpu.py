"""``max_grad_norm`` / ``skip_nonfinite`` of FusedSGD / FusedAdam / FusedAdamW on CPU tensors (the
torch path): against ``torch.nn.utils.clip_grad_norm_`` followed by the ``torch.optim`` step of
the same name in float64, the norm's scope over param groups, declined steps, the state_dict
interchange, the config surface and ``trainer.log_grad_norm``."""
import copy
import json
import math
from pathlib import Path

import pytest
import torch

from pytorch_distributed_template_amd.optim import FusedAdam, FusedAdamW, FusedSGD

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(8, 3, 3, 3), (33, 17), (17,), (1,)]  # 795 elements
# N(0, 1) gradients times these: norms of about 14, 42, 3, 56, 8 against MAX_NORM 20
SCALES = [0.5, 1.5, 0.1, 2.0, 0.3]
MAX_NORM = 20.0
KINDS = ["sgd", "adam", "adamw"]
HP = {"sgd": dict(momentum=0.9, nesterov=True), "adam": dict(amsgrad=True), "adamw": dict()}
LRS = {"sgd": (0.1, 0.05), "adam": (1e-2, 2e-2), "adamw": (1e-2, 2e-2)}
WDS = {"sgd": (1e-3, 1e-4), "adam": (1e-2, 0.0), "adamw": (0.05, 0.01)}
FUSED = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}
TORCH = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}


def _params(dtype=torch.float32):
    gen = torch.Generator().manual_seed(5)
    return [torch.randn(s, generator=gen).to(dtype).requires_grad_(True) for s in SHAPES]


def _grads(steps=5):
    gen = torch.Generator().manual_seed(6)
    return [[torch.randn(s, generator=gen) * SCALES[i] for s in SHAPES] for i in range(steps)]


def _groups(kind, params):
    """Two groups (parameters 0, 2 and 1, 3) with their own lr and weight decay."""
    return [{"params": [params[0], params[2]], "lr": LRS[kind][0], "weight_decay": WDS[kind][0]},
            {"params": [params[1], params[3]], "lr": LRS[kind][1], "weight_decay": WDS[kind][1]}]


def _set(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.to(p.dtype).clone()


def _gnorm(grads):
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))


def _reference(kind, grad_steps, max_norm):
    """float64: clip_grad_norm_ over all parameters, then the torch.optim step."""
    params = _params(torch.float64)
    opt = TORCH[kind](_groups(kind, params), **HP[kind])
    for gs in grad_steps:
        _set(params, gs)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False)
        opt.step()
    return params, opt


def _assert_close(params, want):
    # the tolerance tests/test_optim_cpu.py holds the unclipped torch path to
    for p, q in zip(params, want):
        got, q = p.detach(), q.detach().float()
        assert torch.allclose(got, q, atol=1e-6), float((got - q).abs().max())


@pytest.mark.parametrize("kind", KINDS)
def test_clipped_step_matches_clip_grad_norm_then_torch_optim(kind):
    grads = _grads()
    norms = [_gnorm(gs) for gs in grads]
    assert sum(n > MAX_NORM for n in norms) == 2 and sum(n < MAX_NORM for n in norms) == 3  # active and not
    params = _params()
    opt = FUSED[kind](_groups(kind, params), max_grad_norm=MAX_NORM, **HP[kind])
    assert opt.whole_step_fallback and opt.grad_norm() is None
    for gs, n in zip(grads, norms):
        _set(params, gs)
        opt.step()
        got = opt.grad_norm()
        assert got.dim() == 0 and got.dtype == torch.float32
        assert abs(float(got) - n) <= 1e-6 * n  # before clipping
    want, _ = _reference(kind, grads, MAX_NORM)
    _assert_close(params, want)
    unclipped, _ = _reference(kind, grads, 0.0)
    assert not torch.allclose(want[1].float(), unclipped[1].float(), atol=1e-4)  # the clip mattered


@pytest.mark.parametrize("kind", KINDS)
def test_one_norm_spans_both_param_groups(kind):
    """Only group 1 has large gradients; group 0's are scaled by the same coefficient."""
    gen = torch.Generator().manual_seed(7)
    gs = [torch.randn(s, generator=gen) * (10.0 if i in (1, 3) else 0.01) for i, s in enumerate(SHAPES)]
    assert _gnorm([gs[0], gs[2]]) < 1.0 < _gnorm(gs)
    params = _params()
    opt = FUSED[kind](_groups(kind, params), max_grad_norm=1.0, **HP[kind])
    _set(params, gs)
    opt.step()
    want, _ = _reference(kind, [gs], 1.0)
    _assert_close(params, want)
    per_group, _ = _reference(kind, [gs], 0.0)  # group 0 alone would not be clipped at all
    assert not torch.allclose(want[0].float(), per_group[0].float(), atol=1e-5)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("clip", [0.0, MAX_NORM])
@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_step_is_declined(kind, clip, bad):
    grads = _grads(4)
    grads[1][1] = grads[1][1].clone()
    grads[1][1][5, 2] = bad
    params = _params()
    opt = FUSED[kind](_groups(kind, params), max_grad_norm=clip, skip_nonfinite=True, **HP[kind])
    assert int(opt.skipped_steps()) == 0
    for i, gs in enumerate(grads):
        before = [p.detach().clone() for p in params]
        state = copy.deepcopy(opt.state_dict()["state"])
        _set(params, gs)
        opt.step()
        if i == 1:
            assert all(torch.equal(p, b) for p, b in zip(params, before))
            after = opt.state_dict()["state"]
            assert after.keys() == state.keys()
            for k in state:
                for name, v in state[k].items():
                    assert torch.equal(torch.as_tensor(after[k][name]), torch.as_tensor(v)), (k, name)
            sk = opt.skipped_steps()
            assert sk.dim() == 0 and not sk.dtype.is_floating_point and int(sk) == 1
        else:
            assert not torch.equal(params[1], before[1])
    assert int(opt.skipped_steps()) == 1
    want, _ = _reference(kind, [grads[0], grads[2], grads[3]], clip)  # three steps, bias corrections included
    _assert_close(params, want)
    if kind != "sgd":
        assert all(float(st["step"]) == 3 for st in opt.state_dict()["state"].values())


def test_nonfinite_first_step_leaves_sgd_momentum_zero():
    """The declined step is the one that creates the momentum buffers: the next one starts them."""
    grads = _grads(3)
    grads[0][0] = grads[0][0].clone()
    grads[0][0][0, 0, 0, 0] = float("inf")
    params = _params()
    opt = FusedSGD(_groups("sgd", params), skip_nonfinite=True, **HP["sgd"])
    start = [p.detach().clone() for p in params]
    _set(params, grads[0])
    opt.step()
    assert all(torch.equal(p, s) for p, s in zip(params, start))
    assert all(not opt.state[p]["momentum_buffer"].any() for p in params)
    for gs in grads[1:]:
        _set(params, gs)
        opt.step()
    want, _ = _reference("sgd", grads[1:], 0.0)
    _assert_close(params, want)


def test_skip_nonfinite_with_dampening_raises():
    with pytest.raises(ValueError, match="dampening"):
        FusedSGD(_params(), lr=0.1, momentum=0.9, dampening=0.1, skip_nonfinite=True)
    with pytest.raises(ValueError, match="dampening"):
        FusedSGD([{"params": _params(), "dampening": 0.5}], lr=0.1, momentum=0.9, skip_nonfinite=True)
    FusedSGD(_params(), lr=0.1, momentum=0.9, dampening=0.1, max_grad_norm=1.0)  # clipping alone is fine


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_round_trip_through_torch_optim(kind):
    grads = _grads(5)
    grads[1][0] = grads[1][0].clone()
    grads[1][0][0, 0, 0, 0] = float("nan")  # one declined step on the way
    a_params = _params()
    a = FUSED[kind](_groups(kind, a_params), max_grad_norm=MAX_NORM, skip_nonfinite=True, **HP[kind])
    for gs in grads[:3]:
        _set(a_params, gs)
        a.step()
    sd = copy.deepcopy(a.state_dict())
    assert set(sd) == {"state", "param_groups"}  # the counter is not state
    assert set(sd["param_groups"][0]) <= set(TORCH[kind](_params()[:1], lr=0.1).state_dict()["param_groups"][0])
    t_params = [p.detach().clone().requires_grad_(True) for p in a_params]
    t = TORCH[kind](_groups(kind, t_params), **HP[kind])
    t.load_state_dict(sd)
    if kind == "adamw":
        assert float(t.state[t_params[1]]["step"]) == 2  # the steps actually taken
        assert torch.equal(t.state[t_params[1]]["exp_avg_sq"], a.state[a_params[1]]["exp_avg_sq"])
    else:
        assert torch.equal(t.state[t_params[1]]["momentum_buffer"], a.state[a_params[1]]["momentum_buffer"])
    # ... and back into a fresh fused optimizer, which continues like the original
    b_params = [p.detach().clone().requires_grad_(True) for p in a_params]
    b = FUSED[kind](_groups(kind, b_params), max_grad_norm=MAX_NORM, skip_nonfinite=True, **HP[kind])
    b.load_state_dict(copy.deepcopy(t.state_dict()))  # (torch loads state tensors without copying them)
    for gs in grads[3:]:
        _set(a_params, gs)
        _set(b_params, gs)
        a.step()
        b.step()
    for p, q in zip(a_params, b_params):
        assert torch.equal(p, q)
    # torch.optim continues from the checkpoint the way the float64 reference does from its own
    for gs in grads[3:]:
        _set(t_params, gs)
        torch.nn.utils.clip_grad_norm_(t_params, MAX_NORM)
        t.step()
    _assert_close(a_params, t_params)


def test_defaults_leave_the_step_as_it_was():
    """Without the options nothing of them runs: no norm, no counter, per-group fallback."""
    for kind in KINDS:
        params = _params()
        opt = FUSED[kind](_groups(kind, params), **HP[kind])
        assert opt.max_grad_norm == 0.0 and opt.skip_nonfinite is False and not opt.whole_step_fallback
        grads = _grads(2)
        for gs in grads:
            _set(params, gs)
            opt.step()
        assert opt.grad_norm() is None and opt._skipped is None and opt._glob is None
        want, _ = _reference(kind, grads, 0.0)
        _assert_close(params, want)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(_params(), max_grad_norm=-1.0)


class _Cfg(dict):
    """The two ConfigParser calls build_optimizer makes: cfg[key] and init_obj."""

    def init_obj(self, name, module, *args, **kwargs):
        spec = self[name]
        for m in (module if isinstance(module, (list, tuple)) else [module]):
            if hasattr(m, spec["type"]):
                return getattr(m, spec["type"])(*args, **{**spec["args"], **kwargs})
        raise AttributeError(spec["type"])


@pytest.mark.parametrize("name,cls", [("FusedSGD", FusedSGD), ("FusedAdam", FusedAdam), ("FusedAdamW", FusedAdamW)])
def test_build_optimizer_passes_the_new_keys(name, cls):
    from pytorch_distributed_template_amd.runtime.builder import build_optimizer
    cfg = _Cfg(optimizer={"type": name, "args": {"lr": 0.01, "max_grad_norm": 0.5, "skip_nonfinite": True}},
               trainer={"precision": "fp32"})
    opt, sched = build_optimizer(cfg, torch.nn.Linear(4, 3))
    assert type(opt) is cls and sched is None
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is True and opt.whole_step_fallback
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    opt.step()
    assert float(opt.grad_norm()) == pytest.approx(math.sqrt(15.0)) and int(opt.skipped_steps()) == 0


def test_clip_config_file():
    import inspect
    cfg = json.loads((ROOT / "config" / "vit_b16_fp8_clip.json").read_text())
    ref = json.loads((ROOT / "config" / "vit_b16_fp8.json").read_text())
    assert cfg["optimizer"]["type"] == "FusedAdamW"
    assert set(cfg["optimizer"]["args"]) <= set(inspect.signature(FusedAdamW.__init__).parameters)
    assert cfg["optimizer"]["args"] == {**ref["optimizer"]["args"], "max_grad_norm": 1.0, "skip_nonfinite": True}
    assert cfg["trainer"] == {**ref["trainer"], "log_grad_norm": True}
    for k in ref:
        if k not in ("name", "optimizer", "trainer"):
            assert cfg[k] == ref[k], k


def _mnist_trainer(tmp_path, log_grad_norm, optimizer):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (build_criterion_metrics, build_loader, build_model,
                                                          build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    cfg = json.loads((ROOT / "config" / "mnist_cpu.json").read_text())
    cfg["optimizer"] = optimizer
    cfg["trainer"].update(save_dir=str(tmp_path), epochs=1, verbosity=1, monitor="off")
    if log_grad_norm:
        cfg["trainer"]["log_grad_norm"] = True
    for k in ("train_loader", "valid_loader", "test_loader"):
        cfg[k]["args"].update(data_dir=str(tmp_path / "data"), synthetic_size=256, batch_size=64)
    torch.manual_seed(0)
    device = torch.device("cpu")
    config = ConfigParser(cfg, run_id="clip")
    model = build_model(config, device)
    criterion, metrics = build_criterion_metrics(config)
    opt, sched = build_optimizer(config, model)
    return Trainer(model, criterion, metrics, opt, config=config, device=device,
                   data_loader=build_loader(config, "train_loader"), lr_scheduler=sched)


def test_trainer_logs_grad_norm_and_skipped_steps(tmp_path):
    fused = {"type": "FusedAdam", "args": {"lr": 1e-3, "amsgrad": True, "max_grad_norm": 1.0,
                                           "skip_nonfinite": True, "write_bf16_shadow": False}}
    tr = _mnist_trainer(tmp_path / "a", True, fused)
    assert type(tr.optimizer) is FusedAdam and tr.log_grad_norm
    log = tr._train_epoch(1)
    assert math.isfinite(log["grad_norm"]) and log["grad_norm"] > 0
    assert log["skipped_steps"] == 0 and isinstance(log["skipped_steps"], int)
    assert math.isfinite(log["loss"])
    # without the key, and with an optimizer that has no norm, the log is what it was
    for i, (key, optimizer) in enumerate([(False, fused), (True, {"type": "Adam", "args": {"lr": 1e-3}})]):
        tr = _mnist_trainer(tmp_path / f"b{i}", key, optimizer)
        assert not tr.log_grad_norm
        log = tr._train_epoch(1)
        assert "grad_norm" not in log and "skipped_steps" not in log
