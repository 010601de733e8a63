"""FusedLARS / FusedLAMB on CPU tensors (the torch fallback of the gloo plumbing path) against
float64 references written from their definitions (tests/layerwise_ref.py), their state_dict
interchange with torch.optim.SGD / Adam, and the config surface."""
import copy
import json
import os
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layerwise_ref as R  # noqa: E402

from pytorch_distributed_template_amd.optim import FusedLAMB, FusedLARS  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
SHAPES = [(8, 3, 3, 3), (33, 17), (17,), (1,)]
EXTRA = [(5, 4), (6, 3)]  # the zero-gradient and the zero-weight tensor
STEPS = 4
LRS = [0.1, 0.1, 0.05, 0.025]
LAMB_LRS = [0.05, 0.05, 0.025, 0.0125]
MAX_NORM = 1.0  # the ~1000 N(0, 1) gradient elements have norm ~30: clip < 1 on every step


def _run(kind, exclude_1d, max_grad_norm):
    params, kinds, group_of = R.make_case(SHAPES, EXTRA, "cpu", seed=3)
    grads = R.make_grads(params, kinds, torch.Generator().manual_seed(4), STEPS)
    pg = R.split(params, group_of)
    if kind == "lars":
        wds = (1e-2, 1e-3)
        hp = dict(momentum=0.9, nesterov=True, trust_coefficient=0.1, eps=1e-8)
        opt = FusedLARS([{"params": pg[0], "weight_decay": wds[0]}, {"params": pg[1], "weight_decay": wds[1]}],
                        lr=LRS[0], exclude_1d=exclude_1d, max_grad_norm=max_grad_norm, **hp)
        ref = R.RefLARS(R.ref_groups(params, group_of, wds, exclude_1d), max_grad_norm=max_grad_norm, **hp)
        lrs = LRS
    else:
        wds = (0.01, 0.1)
        hp = dict(betas=(0.9, 0.999), eps=1e-6)
        opt = FusedLAMB([{"params": pg[0], "weight_decay": wds[0]}, {"params": pg[1], "weight_decay": wds[1]}],
                        lr=LAMB_LRS[0], exclude_1d=exclude_1d, max_grad_norm=max_grad_norm, **hp)
        ref = R.RefLAMB(R.ref_groups(params, group_of, wds, exclude_1d), max_grad_norm=max_grad_norm, **hp)
        lrs = LAMB_LRS
    for step in range(STEPS):
        if max_grad_norm > 0:
            assert R.clip_coef([[g.double() for g in grads[step]]], max_grad_norm) < 1
        R.set_grads(params, grads[step])
        for group in opt.param_groups:
            group["lr"] = lrs[step]
        opt.step()
        ref.step(R.split([g.double() for g in grads[step]], group_of), lrs[step])
    return params, group_of, ref


@pytest.mark.parametrize("max_grad_norm", [0.0, MAX_NORM])
@pytest.mark.parametrize("exclude_1d", [True, False])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_cpu_step_matches_fp64_reference(kind, exclude_1d, max_grad_norm):
    params, group_of, ref = _run(kind, exclude_1d, max_grad_norm)
    R.assert_matches(params, group_of, ref, rtol=1e-5, atol=1e-6)


def _pair(kind, params):
    pg = [params[:2], params[2:]]
    if kind == "lars":
        return FusedLARS([{"params": pg[0], "weight_decay": 1e-2}, {"params": pg[1], "weight_decay": 1e-3}],
                         lr=0.1, momentum=0.9, trust_coefficient=0.1, max_grad_norm=1.0)
    return FusedLAMB([{"params": pg[0], "weight_decay": 0.01}, {"params": pg[1], "weight_decay": 0.1}],
                     lr=0.05, max_grad_norm=1.0)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_state_dict_round_trip_through_torch_optim(kind):
    gen = torch.Generator().manual_seed(5)
    a_params = [torch.randn(s, generator=gen).requires_grad_(True) for s in SHAPES]
    grads = [[torch.randn(s, generator=gen) for s in SHAPES] for _ in range(5)]
    a = _pair(kind, a_params)
    for gs in grads[:3]:
        R.set_grads(a_params, gs)
        a.step()
    sd = copy.deepcopy(a.state_dict())
    # into the torch optimizer of the same state format, without the hyperparameters it does not know
    own = {"lars": ("trust_coefficient", "eps", "exclude_1d"), "lamb": ("exclude_1d",)}[kind]
    for group in sd["param_groups"]:
        for k in own:
            del group[k]
    t_params = [p.detach().clone().requires_grad_(True) for p in a_params]
    tg = [{"params": t_params[:2]}, {"params": t_params[2:]}]
    t = torch.optim.SGD(tg, lr=1.0, momentum=0.5) if kind == "lars" else torch.optim.Adam(tg, lr=1.0)
    t.load_state_dict(sd)
    assert t.param_groups[1]["weight_decay"] == a.param_groups[1]["weight_decay"]
    if kind == "lars":
        assert t.param_groups[0]["momentum"] == 0.9
        assert torch.equal(t.state[t_params[1]]["momentum_buffer"], a.state[a_params[1]]["momentum_buffer"])
    else:
        assert float(t.state[t_params[1]]["step"]) == 3
        assert torch.equal(t.state[t_params[1]]["exp_avg_sq"], a.state[a_params[1]]["exp_avg_sq"])
    # ... and back into a fresh fused optimizer, which then continues like the original, bitwise
    b_params = [p.detach().clone().requires_grad_(True) for p in a_params]
    b = _pair(kind, b_params)
    b.load_state_dict(t.state_dict())
    assert b.param_groups[0]["exclude_1d"] is True
    for gs in grads[3:]:
        R.set_grads(a_params, gs)
        R.set_grads(b_params, gs)
        a.step()
        b.step()
    for p, q in zip(a_params, b_params):
        assert torch.equal(p, q)
    if kind == "lamb":
        assert float(b.state_dict()["state"][0]["step"]) == 5


class _Cfg(dict):
    """The two ConfigParser calls build_optimizer makes: cfg[key] and init_obj."""

    def init_obj(self, name, module, *args, **kwargs):
        spec = self[name]
        for m in (module if isinstance(module, (list, tuple)) else [module]):
            if hasattr(m, spec["type"]):
                return getattr(m, spec["type"])(*args, **{**spec["args"], **kwargs})
        raise AttributeError(spec["type"])


@pytest.mark.parametrize("name,cls", [("FusedLARS", FusedLARS), ("FusedLAMB", FusedLAMB)])
@pytest.mark.parametrize("precision,hip_graph", [("fp32", False), ("bf16", True)])
def test_build_optimizer_resolves_layerwise_types(name, cls, precision, hip_graph):
    from pytorch_distributed_template_amd.runtime.builder import build_optimizer
    cfg = _Cfg(optimizer={"type": name, "args": {"lr": 0.01}}, trainer={"precision": precision, "hip_graph": hip_graph})
    opt, sched = build_optimizer(cfg, torch.nn.Linear(4, 3))
    assert type(opt) is cls and sched is None
    assert opt.write_bf16_shadow is (precision == "bf16")  # an fp32 model allocates no shadows
    assert opt.capturable is hip_graph  # harmless on CPU
    lin = opt.param_groups[0]["params"]
    for p in lin:
        p.grad = torch.ones_like(p)
    opt.step()


@pytest.mark.parametrize("path,name,base", [("config/resnet50_bf16_lars.json", "FusedLARS", "config/resnet50_bf16.json"),
                                            ("config/vit_b16_fp8_lamb.json", "FusedLAMB", "config/vit_b16_fp8.json")])
def test_layerwise_config_files(path, name, base):
    import inspect
    from pytorch_distributed_template_amd import data, models, optim
    cfg = json.loads((ROOT / path).read_text())
    assert cfg["optimizer"]["type"] == name
    cls = getattr(optim, name)
    assert set(cfg["optimizer"]["args"]) <= set(inspect.signature(cls.__init__).parameters)
    assert hasattr(models, cfg["arch"]["type"]) and hasattr(data, cfg["train_loader"]["type"])
    assert hasattr(torch.optim.lr_scheduler, cfg["lr_scheduler"]["type"])
    # a copy of the existing recipe with the optimizer swapped
    ref = json.loads((ROOT / base).read_text())
    for k in ref:
        if k not in ("name", "optimizer"):
            assert cfg[k] == ref[k], k
