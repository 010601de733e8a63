"""The weight EMA without a GPU: the references of tests/ema_ref.py (torch's fp32 ``lerp_`` stays
inside the derived bound; each seeded fault is caught), ``optim.ModelEMA``'s torch path, the
Trainer / checkpoint / ``test.py --ema`` plumbing on CPU, ``WarmupCosineLR`` and
``trainer.lr_step``."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as R  # noqa: E402

from pytorch_distributed_template_amd.optim import ModelEMA, WarmupCosineLR  # noqa: E402
from pytorch_distributed_template_amd.optim import ema as ema_mod  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CHUNK = 1024


# ---------------------------------------------------------------------------------------------
# the references: the tick mirror, the bound, the seeded faults
# ---------------------------------------------------------------------------------------------
def test_tick_mirror_values():
    sched = R.schedule(12, 0.9999, True)
    assert [float(t) for t, _, _ in sched] == list(range(1, 13))
    for k, (_, d, w) in enumerate(sched):
        assert d.dtype == np.float32 and w.dtype == np.float32
        assert d == np.float32(np.float32(1 + k) / np.float32(10 + k)) and w == np.float32(1) - d
    # the ramp reaches the cap: (1 + t) / (10 + t) >= 0.9999 from t ~ 90 000
    assert R.tick(80000, 0.9999, True)[1] == np.float32(np.float32(80001) / np.float32(80010)) < np.float32(0.9999)
    assert R.tick(100000, 0.9999, True)[1] == np.float32(0.9999)
    assert R.tick(5, 0.75, False)[1:] == (np.float32(0.75), np.float32(0.25))
    assert ema_mod.decay_step(7, 0.9999, True) == R.tick(7, 0.9999, True)


def _mirror(e, p, w):
    """The kernel's arithmetic in torch fp32 on the CPU (unfused)."""
    w = torch.tensor(float(w), dtype=torch.float32)
    return e + w * (p - e)


def _general_run(update, n=12, decay=0.9999, warmup=True, seed=3):
    """12 updates of the general family through ``update(e, p, w, d, step)`` next to the float64
    reference; the worst error-to-bound ratio over all tensors after every update."""
    gen = torch.Generator().manual_seed(seed)
    es = [torch.randn(s, generator=gen) for s in R.SIZES]
    bounds = [R.Bound(e) for e in es]
    worst = 0.0
    for step, (_, d, w) in enumerate(R.schedule(n, decay, warmup)):
        ps = [torch.randn(e.shape, generator=gen) for e in es]
        for i, (e, p) in enumerate(zip(es, ps)):
            bounds[i].update(p, w)
            es[i] = update(e, p, w, d, step)
            worst = max(worst, bounds[i].ratio(es[i]))
    return worst


def test_torch_lerp_and_the_fp32_mirror_stay_inside_the_bound():
    r_lerp = _general_run(lambda e, p, w, d, k: e.clone().lerp_(p, float(w)))
    r_mirror = _general_run(lambda e, p, w, d, k: _mirror(e, p, w))
    r_flat = _general_run(lambda e, p, w, d, k: e.clone().lerp_(p, float(w)), warmup=False)
    print("error / bound: torch lerp_", r_lerp, "fp32 mirror", r_mirror, "lerp_ without warm-up", r_flat)
    assert 0 < r_lerp <= 1 and 0 < r_mirror <= 1 and 0 < r_flat <= 1


def _drop_last(e, p, w, d, k):
    out = _mirror(e, p, w)
    if k == 5 and e.numel() > 1:
        last = min(CHUNK, e.numel()) - 1  # the last element of the tensor's first chunk
        out[last] = e[last]
    return out


def _chunk_twice(e, p, w, d, k):
    out = _mirror(e, p, w)
    if k == 5:
        n = min(CHUNK, e.numel())
        out[:n] = _mirror(out[:n], p[:n], w)
    return out


def _swapped(e, p, w, d, k):
    return _mirror(e, p, d)


@pytest.mark.parametrize("fault", [_drop_last, _chunk_twice, _swapped])
def test_seeded_faults_fall_outside_the_bound(fault):
    r = _general_run(fault)
    print(fault.__name__, "error / bound", r)
    assert r > 1


def _exact_run(update, decay, seed=5):
    gen = torch.Generator().manual_seed(seed)
    es = [R.exact_values((s,), gen) for s in R.SIZES]
    refs = [e.double() for e in es]
    for step, (_, d, w) in enumerate(R.schedule(4, decay, False)):
        for i in range(len(es)):
            p = R.exact_values(es[i].shape, gen)
            refs[i] = R.ref_update(refs[i], p, w)
            es[i] = update(es[i], p, w, d, step)
    return es, refs


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.75])
def test_exact_family_is_exact_in_fp32_and_catches_the_faults(decay):
    es, refs = _exact_run(lambda e, p, w, d, k: _mirror(e, p, w), decay)
    for e, r in zip(es, refs):
        assert torch.equal(e.double(), r)
        assert float(r.abs().max()) <= 2 ** 15
    for fault in (_drop_last, _chunk_twice, _swapped):
        if fault is _swapped and decay == 0.5:
            continue  # (w == d: the general family catches it)
        if fault is _chunk_twice and decay == 0.0:
            continue  # (w == 1: a second application changes nothing; the general family catches it)
        es, refs = _exact_run(lambda e, p, w, d, k, f=fault: f(e, p, w, d, 5 if k == 3 else -1), decay)
        assert not all(torch.equal(e.double(), r) for e, r in zip(es, refs)), fault.__name__


def test_truncated_shadow_is_caught():
    gen = torch.Generator().manual_seed(9)
    for vals in (torch.randn(4096, generator=gen), _exact_run(lambda e, p, w, d, k: _mirror(e, p, w), 0.75)[0][-1]):
        assert not torch.equal(R.bf16_trunc(vals).view(torch.int16), vals.to(torch.bfloat16).view(torch.int16))
    # and the reference shadow is round-to-nearest-even: a tie goes to the even bf16
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    assert tie.to(torch.bfloat16).tolist() == [1.0, 1.0 + 2.0 ** -6]


# ---------------------------------------------------------------------------------------------
# ModelEMA's torch path
# ---------------------------------------------------------------------------------------------
def _small_model(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                            torch.nn.Linear(4 * 6 * 6, 5))
    m.train()
    m(torch.randn(8, 3, 8, 8))  # running statistics and num_batches_tracked move off their initial values
    return m


def _perturb(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=gen))
        for name, b in model.named_buffers():
            if b.is_floating_point():
                b.add_(torch.rand(b.shape, generator=gen))
            else:
                b.add_(3)


def test_model_ema_module_is_a_frozen_eval_copy():
    model = _small_model(0)
    wrapped = torch.nn.Module()  # what DDP looks like: the model is its ``.module``
    wrapped.module = model
    ema = ModelEMA(wrapped)
    assert type(ema.module) is type(model) and ema.module is not model
    assert not ema.module.training and all(not p.requires_grad for p in ema.module.parameters())
    for (k, a), (_, b) in zip(ema.module.state_dict().items(), model.state_dict().items()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k
    assert ema.num_updates == 0


def test_decay_zero_copies_and_decay_one_keeps():
    model = _small_model(1)
    initial = {k: v.clone() for k, v in model.state_dict().items()}
    zero, one = ModelEMA(model, decay=0.0, warmup=False), ModelEMA(model, decay=1.0, warmup=False)
    for seed in (2, 3):
        _perturb(model, seed)
        zero.update(model)
        one.update(model)
    for k, v in model.state_dict().items():
        assert torch.equal(zero.module.state_dict()[k], v), k
        if v.is_floating_point():
            assert torch.equal(one.module.state_dict()[k], initial[k]), k
            assert not torch.equal(v, initial[k]), k
        else:
            assert torch.equal(one.module.state_dict()[k], v), k  # num_batches_tracked is copied
    assert zero.num_updates == one.num_updates == 2


def test_warmup_decay_sequence_equals_the_mirror_and_buffers_are_averaged(monkeypatch):
    model = _small_model(4)
    ema = ModelEMA(model, decay=0.9999, warmup=True)
    seen = []
    real = torch._foreach_lerp_

    def spy(es, ps, w):
        seen.append(w)
        return real(es, ps, w)
    monkeypatch.setattr(torch, "_foreach_lerp_", spy)
    ref = {k: R.Bound(v) for k, v in ema.module.state_dict().items() if v.is_floating_point()}
    sched = R.schedule(12, 0.9999, True)
    for step, (_, d, w) in enumerate(sched):
        _perturb(model, 10 + step)
        ema.update(model)
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                ref[k].update(v, w)
    assert seen == [float(w) for _, _, w in sched]
    assert ema.num_updates == 12
    sd = ema.module.state_dict()
    assert {"1.running_mean", "1.running_var", "1.num_batches_tracked"} <= set(sd)
    for k, b in ref.items():
        assert b.ratio(sd[k]) <= 1, (k, b.ratio(sd[k]))
        assert not torch.equal(sd[k], model.state_dict()[k]), k  # averaged, not copied
    assert torch.equal(sd["1.num_batches_tracked"], model.state_dict()["1.num_batches_tracked"])
    assert int(sd["1.num_batches_tracked"]) == 1 + 3 * 12


def test_state_dict_round_trip():
    model = _small_model(5)
    ema = ModelEMA(model, decay=0.99, warmup=True)
    for seed in (6, 7, 8):
        _perturb(model, seed)
        ema.update(model)
    state = ema.state_dict()
    assert set(state) == {"state_dict", "num_updates", "decay", "warmup"}
    assert state["num_updates"] == 3 and state["decay"] == 0.99 and state["warmup"] is True
    assert list(state["state_dict"]) == list(model.state_dict())
    assert all(type(v) is torch.Tensor and not v.requires_grad for v in state["state_dict"].values())
    saved = {k: v.clone() for k, v in state["state_dict"].items()}
    twin = ModelEMA(_small_model(99), decay=0.99, warmup=True)
    twin.load_state_dict(state)
    assert twin.num_updates == 3
    for k, v in saved.items():
        assert torch.equal(twin.module.state_dict()[k], v), k
    _perturb(model, 9)  # both continue with the fourth decay of the ramp
    ema.update(model)
    twin.update(model)
    for k, v in ema.module.state_dict().items():
        assert torch.equal(twin.module.state_dict()[k], v), k
    with pytest.raises(ValueError, match="names differ"):
        ModelEMA(torch.nn.Sequential(torch.nn.Linear(2, 2))).update(torch.nn.Linear(2, 2))


# ---------------------------------------------------------------------------------------------
# WarmupCosineLR
# ---------------------------------------------------------------------------------------------
def test_warmup_cosine_lr_closed_form_and_state_dict():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(1))], "lr": 0.5}], lr=0.2)
    W, T, a, m = 5, 25, 0.1, 0.01
    sched = WarmupCosineLR(opt, warmup_steps=W, total_steps=T, warmup_start_factor=a, min_lr_ratio=m)
    got = []
    for s in range(T + 5):
        got.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sched.step()

    def f(s):
        if s < W:
            return a + (1 - a) * s / W
        return m + (1 - m) * 0.5 * (1 + math.cos(math.pi * min(1.0, (s - W) / (T - W))))
    for s, lrs in enumerate(got):
        assert lrs == pytest.approx([0.2 * f(s), 0.5 * f(s)], rel=1e-12, abs=0), s
    assert got[0] == pytest.approx([0.02, 0.05]) and got[W] == [0.2, 0.5]
    assert got[T] == pytest.approx([0.002, 0.005]) and got[T + 4] == got[T]
    assert all(x[0] < y[0] for x, y in zip(got[:W], got[1:W + 1]))        # the ramp rises
    assert all(x[0] > y[0] for x, y in zip(got[W:T], got[W + 1:T + 1]))    # the cosine falls
    # a plain LRScheduler subclass: the base class's state_dict, and a reload continues the curve
    state = sched.state_dict()
    assert type(sched).state_dict is torch.optim.lr_scheduler.LRScheduler.state_dict
    assert state["last_epoch"] == T + 5 and state["warmup_steps"] == W and "optimizer" not in state
    opt2 = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.2)
    again = WarmupCosineLR(opt2, warmup_steps=W, total_steps=T, warmup_start_factor=a, min_lr_ratio=m)
    again.load_state_dict({**state, "last_epoch": 7, "base_lrs": [0.2], "_last_lr": [0.0]})
    opt2.step()
    again.step()
    assert opt2.param_groups[0]["lr"] == pytest.approx(0.2 * f(8), rel=1e-12)
    with pytest.raises(ValueError):
        WarmupCosineLR(opt2, warmup_steps=10, total_steps=5)


# ---------------------------------------------------------------------------------------------
# Trainer, checkpoints, test.py --ema on CPU (config/mnist_cpu.json's shape of run), on the gloo
# path: the Trainer tests run inside a 1-rank gloo process group, the model wrapped as train.py
# wraps it, so the collectives of the loop and the unwrapping of the EMA are the real ones
# ---------------------------------------------------------------------------------------------
_GROUP_ENV = ("MASTER_ADDR", "MASTER_PORT", "RANK", "LOCAL_RANK", "WORLD_SIZE")


@pytest.fixture(scope="module")
def gloo_group():
    from pytorch_distributed_template_amd.utils import dist as pdist
    saved = {k: os.environ.get(k) for k in _GROUP_ENV}
    try:
        device = pdist.init_distributed(backend="gloo", single_rank_group=True)
        assert device.type == "cpu" and torch.distributed.is_initialized()
        assert torch.distributed.get_backend() == "gloo" and pdist.get_world_size() == 1
        yield device
    finally:
        pdist.cleanup()
        for k, v in saved.items():  # (subprocesses started by later tests must not look launched)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _cfg(tmp_path, **trainer):
    cfg = json.loads((ROOT / "config" / "mnist_cpu.json").read_text())
    cfg["trainer"].update(save_dir=str(tmp_path / "saved"), epochs=2, verbosity=1, **trainer)
    cfg["train_loader"]["args"].update(synthetic_size=256, batch_size=64)
    for k in ("valid_loader", "test_loader"):
        cfg[k]["args"].update(synthetic_size=128)
    return cfg


def _trainer(cfg, run_id, resume=None):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (build_criterion_metrics, build_ema, build_loader,
                                                          build_model, build_optimizer, wrap_model)
    from pytorch_distributed_template_amd.trainer import Trainer
    assert torch.distributed.is_initialized(), "the Trainer tests run on the gloo path (fixture gloo_group)"
    torch.manual_seed(0)
    device = torch.device("cpu")
    config = ConfigParser(cfg, resume=resume, run_id=run_id)
    model = build_model(config, device)
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    ema = build_ema(config, model)
    model = wrap_model(config, model, device)  # (after build_ema, as in train.py)
    assert ema is None or ema.module is not model and type(ema.module) is type(model.module)
    return Trainer(model, criterion, metrics, optimizer, config=config, device=device,
                   data_loader=build_loader(config, "train_loader"),
                   valid_data_loader=build_loader(config, "valid_loader"), lr_scheduler=sched, ema=ema)


TODAY_CKPT = {"arch", "epoch", "state_dict", "optimizer", "monitor_best", "config", "lr_scheduler"}
TODAY_LOG = {"loss", "images_per_sec", "val_loss", "val_accuracy", "val_top_k_acc"}


def test_without_trainer_ema_nothing_changes(tmp_path, gloo_group):
    for ema_cfg in ("absent", None):
        cfg = _cfg(tmp_path)
        if ema_cfg is None:
            cfg["trainer"]["ema"] = None
        tr = _trainer(cfg, "plain")
        assert tr.ema is None and tr.valid_ema_metrics is None and tr.lr_step == "epoch"
        log = tr._train_epoch(1)
        assert set(log) == TODAY_LOG
        assert set(tr._checkpoint_state(1)) == TODAY_CKPT
        assert tr.lr_scheduler.last_epoch == 1  # one scheduler step per epoch


@pytest.mark.parametrize("validate", ["both", "ema", "model"])
def test_trainer_validates_what_ema_validate_names(tmp_path, validate, gloo_group):
    cfg = _cfg(tmp_path, ema={"decay": 0.9, "warmup": True, "validate": validate})
    tr = _trainer(cfg, "v" + validate)
    log = tr._train_epoch(1)
    plain = {"val_loss", "val_accuracy", "val_top_k_acc"}
    averaged = {"val_ema_loss", "val_ema_accuracy", "val_ema_top_k_acc"}
    want = {"loss", "images_per_sec"} | (plain if validate != "ema" else set()) | \
        (averaged if validate != "model" else set())
    assert set(log) == want
    assert tr.ema.num_updates == 4 and tr.model.training and not tr.ema.module.training
    if validate == "both":
        assert log["val_ema_loss"] != log["val_loss"] and np.isfinite(log["val_ema_loss"])


def test_build_ema_rejects_what_it_does_not_know(tmp_path):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import build_ema
    for bad in ({"validate": "best"}, {"momentum": 0.9}):
        config = ConfigParser(_cfg(tmp_path, ema=bad), run_id="bad")
        with pytest.raises(ValueError, match="trainer.ema"):
            build_ema(config, torch.nn.Linear(2, 2))


def test_checkpoint_resume_and_test_py_ema(tmp_path, gloo_group):
    cfg = _cfg(tmp_path, ema={"decay": 0.99, "warmup": True}, monitor="min val_ema_loss")
    tr = _trainer(cfg, "run1")
    tr.train()
    run = tmp_path / "saved" / "Mnist_LeNet_cpu" / "train" / "run1"
    assert (run / "model_best.pth").exists()  # the monitor found val_ema_loss
    ck = torch.load(run / "checkpoint-epoch2.pth", weights_only=True)
    assert set(ck) == TODAY_CKPT | {"state_dict_ema", "ema"}
    assert ck["ema"] == {"num_updates": 8, "decay": 0.99, "warmup": True}
    assert list(ck["state_dict_ema"]) == list(ck["state_dict"])
    assert any(not torch.equal(ck["state_dict_ema"][k], v) for k, v in ck["state_dict"].items())
    for k, v in tr.ema.module.state_dict().items():
        assert torch.equal(ck["state_dict_ema"][k], v), k

    # resume restores the average bit for bit (the EMA object exists before BaseTrainer resumes)
    cfg3 = json.loads(json.dumps(cfg))
    cfg3["trainer"]["epochs"] = 3
    tr2 = _trainer(cfg3, "run2", resume=run / "checkpoint-epoch2.pth")
    assert tr2.start_epoch == 3 and tr2.ema.num_updates == 8
    for k, v in ck["state_dict_ema"].items():
        assert torch.equal(tr2.ema.module.state_dict()[k], v), k
    for k, v in ck["state_dict"].items():
        assert torch.equal(tr2.model.module.state_dict()[k], v), k

    # a checkpoint without the two keys: the average starts from the loaded weights
    plain = {k: v for k, v in ck.items() if k not in ("state_dict_ema", "ema")}
    torch.save(plain, run / "plain.pth")
    tr3 = _trainer(cfg3, "run3", resume=run / "plain.pth")
    assert tr3.ema.num_updates == 0
    for k, v in ck["state_dict"].items():
        assert torch.equal(tr3.ema.module.state_dict()[k], v), k
    assert "holds no averaged weights" in (tmp_path / "saved" / "Mnist_LeNet_cpu" / "train" / "run3" /
                                           "info.log").read_text()

    # test.py --ema evaluates state_dict_ema; without the key it says so
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2", PDT_RUN_ID="t")
    for k in _GROUP_ENV:  # a plain ``python test.py``, not a rank of this process's group
        env.pop(k, None)
    r = subprocess.run([sys.executable, "test.py", "-r", str(run / "checkpoint-epoch2.pth"), "--ema"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "'loss':" in out and "'accuracy':" in out
    loss = float(out.split("'loss':")[1].split(",")[0])
    assert loss == pytest.approx(tr._valid_epoch(3, model=tr.ema.module, prefix="ema_")["ema_loss"], rel=1e-5)
    r = subprocess.run([sys.executable, "test.py", "-r", str(run / "plain.pth"), "--ema"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--ema: the checkpoint" in r.stderr and "holds no averaged weights" in r.stderr
    # without --ema the message about averaged weights is not used: a checkpoint without state_dict
    torch.save({k: v for k, v in plain.items() if k != "state_dict"}, run / "broken.pth")
    r = subprocess.run([sys.executable, "test.py", "-r", str(run / "broken.pth")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "KeyError: 'state_dict'" in r.stderr and "--ema" not in r.stderr


def test_lr_step_iteration_against_epoch(tmp_path, gloo_group):
    counts = {}
    for mode in ("epoch", "iteration"):
        cfg = _cfg(tmp_path, lr_step=mode)
        cfg["lr_scheduler"] = {"type": "WarmupCosineLR", "args": {"warmup_steps": 3, "total_steps": 8}}
        tr = _trainer(cfg, "lr" + mode)
        assert isinstance(tr.lr_scheduler, WarmupCosineLR)  # found in optim before torch.optim.lr_scheduler
        lrs = []
        real = tr.optimizer.step

        def step(*a, _lrs=lrs, _tr=tr, _real=real, **k):
            _lrs.append(_tr.optimizer.param_groups[0]["lr"])
            return _real(*a, **k)
        tr.optimizer.step = step
        tr._train_epoch(1)
        tr._train_epoch(2)
        counts[mode] = tr.lr_scheduler.last_epoch
        f = tr.lr_scheduler.factor
        if mode == "iteration":  # 4 iterations per epoch: optimizer step k runs at the lr of scheduler step k
            assert lrs == pytest.approx([0.001 * f(k) for k in range(8)], rel=1e-12)
        else:
            assert lrs == pytest.approx([0.001 * f(0)] * 4 + [0.001 * f(1)] * 4, rel=1e-12)
    assert counts == {"epoch": 2, "iteration": 8}
    with pytest.raises(ValueError, match="lr_step"):
        _trainer(_cfg(tmp_path, lr_step="batch"), "lrbad")


def test_the_ema_recipe_config_is_the_mix_recipe_plus_ema_and_warmup():
    base = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix.json").read_text())
    cfg = json.loads((ROOT / "config" / "vit_b16_fp8_packed_mix_ema.json").read_text())
    tr = cfg["trainer"]
    assert tr["ema"] == {"decay": 0.9999, "warmup": True, "validate": "both"} and tr["lr_step"] == "iteration"
    sched = cfg["lr_scheduler"]
    assert sched["type"] == "WarmupCosineLR" and sched["args"]["total_steps"] == tr["epochs"] * tr["len_epoch"]
    assert 0 < sched["args"]["warmup_steps"] < sched["args"]["total_steps"]
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=cfg["optimizer"]["args"]["lr"])
    WarmupCosineLR(opt, **sched["args"])
    for k in ("arch", "train_loader", "valid_loader", "test_loader", "optimizer", "loss", "metrics"):
        assert cfg[k] == base[k], k
    same = {k: v for k, v in tr.items() if k not in ("ema", "lr_step", "epochs")}
    assert same == {k: v for k, v in base["trainer"].items() if k != "epochs"}
