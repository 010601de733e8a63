"""``max_grad_norm`` / ``skip_nonfinite`` of FusedSGD / FusedAdam / FusedAdamW on an MI355X: the
guarded step kernels (csrc/optim.hip ``pdt_sgd_step3`` / ``pdt_adam_step3``) against float64
references written from the definitions, exact cases, declined steps, HIP-graph replay, the
launches of a step, and ``trainer.log_grad_norm`` under ``trainer.hip_graph``.

Tensors: sizes around the work-list chunk, one channels_last 4-D tensor, and the same set again
as views one float into a flat buffer (4-byte aligned only: the kernels' scalar path, what a
gradient in a DDP bucket slot is), in two param groups. The non-finite values are ordinary floats
in gradient tensors."""
import json
import math
import os
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402
from pytorch_distributed_template_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from pytorch_distributed_template_amd.optim import fused as fused_mod  # noqa: E402
from pytorch_distributed_template_amd.optim.fused import CHUNK  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
SIZES = [1, 3, CHUNK - 1, CHUNK, CHUNK + 5, 2 * CHUNK + 4]
SHAPE4 = (8, 4, 3, 3)
N_ALIGNED = len(SIZES) + 1
BAND = 64            # guard floats on either side of the flat buffers (a multiple of 4)
SENTINEL = 12345.0
KINDS = ["sgd", "adam", "adamw"]
FUSED = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}
HP = {"sgd": dict(momentum=0.9, nesterov=True), "adam": dict(amsgrad=True), "adamw": dict()}
LRS = {"sgd": (0.1, 0.05), "adam": (1e-3, 2e-3), "adamw": (1e-3, 2e-3)}
WDS = {"sgd": (1e-4, 1e-3), "adam": (1e-2, 0.0), "adamw": (0.05, 0.01)}
STATE = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
         "adamw": ("exp_avg", "exp_avg_sq")}
# N(0, 1) gradients times these over about 10 CHUNK elements have norms of about 0.1, 2, 0.01 and
# 0.5 times sqrt(10 CHUNK) (57, 1146, 6 and 286 at CHUNK = 32768): MAX_NORM sits between them
SCALES = [0.1, 2.0, 0.01, 0.5]
MAX_NORM = 0.25 * math.sqrt(10 * CHUNK)


def setup_module(module):
    assert no.available(), "native library must be built and loaded on GPU runs"
    no.require()


# ---------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------
def _host_tensors(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    ts = [torch.randn(n, generator=gen) * scale for n in SIZES]
    ts.append((torch.randn(SHAPE4, generator=gen) * scale).contiguous(memory_format=torch.channels_last))
    return ts + [t.clone() for t in ts]  # the aligned set, then the set that becomes views


def _flat_views(tensors):
    """``tensors`` as views into one flat buffer, the first at element ``BAND + 1``; the buffer
    has ``BAND`` sentinel floats on either side of them. Returns (views, flat)."""
    total = sum(t.numel() for t in tensors)
    flat = torch.full((total + 1 + 2 * BAND,), SENTINEL, device="cuda")
    off, out = BAND + 1, []
    for t in tensors:
        n = t.numel()
        if t.dim() == 4:
            s = t.shape
            v = flat[off:off + n].view(s[0], s[2], s[3], s[1]).permute(0, 3, 1, 2)
        else:
            v = flat[off:off + n].view(t.shape)
        v.copy_(t)
        off += n
        out.append(v)
    assert out[0].data_ptr() % 16 == 4 and off == total + 1 + BAND
    return out, flat


def _bands_intact(flat):
    return bool((flat[:BAND + 1] == SENTINEL).all()) and bool((flat[-BAND:] == SENTINEL).all())


class Case:
    """Parameters (aligned tensors, then views into a flat buffer) with static gradient buffers
    laid out the same way, in two groups (even / odd positions)."""

    def __init__(self, kind, **kw):
        host = _host_tensors(101)
        self.host = host
        aligned = [t.cuda() for t in host[:N_ALIGNED]]
        views, self.flat = _flat_views(host[N_ALIGNED:])
        self.params = [t.requires_grad_(True) for t in aligned + views]
        assert all(p.data_ptr() % 16 == 0 for p in self.params[:N_ALIGNED])
        g_aligned = [torch.zeros_like(p) for p in aligned]
        g_views, self.gflat = _flat_views([torch.zeros_like(t) for t in host[N_ALIGNED:]])
        for p, g in zip(self.params, g_aligned + g_views):
            assert g.stride() == p.stride()
            p.grad = g
        self.group_of = [i % 2 for i in range(len(self.params))]
        groups = [{"params": [p for p, g in zip(self.params, self.group_of) if g == gi], "lr": LRS[kind][gi],
                   "weight_decay": WDS[kind][gi]} for gi in (0, 1)]
        self.kind = kind
        self.opt = FUSED[kind](groups, **HP[kind], **kw)

    def set_grads(self, grads):
        for p, g in zip(self.params, grads):
            p.grad.copy_(g)

    def tensors(self):
        """Everything a step may write: parameters, state tensors, bf16 shadows, device scalars."""
        out = {f"p{i}": p.detach() for i, p in enumerate(self.params)}
        for i, p in enumerate(self.params):
            for k in STATE[self.kind]:
                out[f"{k}{i}"] = self.opt.state[p][k]
            out[f"shadow{i}"] = self.opt._shadows[id(p)]
        for gi, d in self.opt._dev.items():
            out[f"dev{gi}"] = d
        return out

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.tensors().items()}


def _assert_bitwise(got, want):
    assert got.keys() == want.keys()
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        ints = torch.int32 if a.element_size() == 4 else torch.int16
        assert torch.equal(a.contiguous().view(ints), b.contiguous().view(ints)), k


def _grad_steps(seed, scales):
    return [_host_tensors(seed + i, s) for i, s in enumerate(scales)]


class Ref:
    """float64 SGD (momentum, nesterov) / Adam (amsgrad) / AdamW from their definitions, with the
    clip coefficient from the float64 sum of squares of every gradient and the skip rule."""

    def __init__(self, kind, host, group_of, max_grad_norm, skip_nonfinite):
        self.kind, self.group_of = kind, group_of
        self.w = [t.double() for t in host]
        self.max_grad_norm, self.skip = max_grad_norm, skip_nonfinite
        self.t = 0
        self.buf = [None] * len(host)
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.vmax = [torch.zeros_like(w) for w in self.w]
        self.gnorm = None

    def step(self, grads):
        gs = [g.double() for g in grads]
        self.gnorm = math.sqrt(sum(float((g * g).sum()) for g in gs))
        if self.skip and not math.isfinite(self.gnorm):
            return
        clip = min(1.0, self.max_grad_norm / (self.gnorm + 1e-6)) if self.max_grad_norm > 0 else 1.0
        self.t += 1
        hp = HP[self.kind]
        for i, (w, g) in enumerate(zip(self.w, gs)):
            lr, wd = LRS[self.kind][self.group_of[i]], WDS[self.kind][self.group_of[i]]
            g = g * clip
            if self.kind == "sgd":
                g = g + wd * w
                self.buf[i] = g.clone() if self.buf[i] is None else hp["momentum"] * self.buf[i] + g
                self.w[i] = w - lr * (g + hp["momentum"] * self.buf[i])
                continue
            b1, b2, eps = 0.9, 0.999, 1e-8
            if self.kind == "adamw":
                w = w * (1 - lr * wd)
            else:
                g = g + wd * w
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            v = self.v[i]
            if hp.get("amsgrad"):
                v = self.vmax[i] = torch.maximum(self.vmax[i], v)
            denom = v.sqrt() / math.sqrt(1 - b2 ** self.t) + eps
            self.w[i] = w - lr / (1 - b1 ** self.t) * self.m[i] / denom


def _assert_matches_ref(case, ref):
    # the bound tests/test_optim_shared_gpu.py and tests/test_optim_layerwise_gpu.py hold the
    # unclipped native step to
    for i, (p, w) in enumerate(zip(case.params, ref.w)):
        got, want = p.detach().cpu(), w.to(torch.float32)
        err = float((got - want).abs().max())
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (i, tuple(p.shape), err)
        sh = case.opt._shadows[id(p)]
        assert no._SHADOWS[id(p)][0] is sh and torch.equal(sh, p.detach().to(torch.bfloat16)), i


# ---------------------------------------------------------------------------------------------
# against the float64 reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip_nonfinite", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_native_step_matches_fp64_reference(kind, skip_nonfinite):
    case = Case(kind, max_grad_norm=MAX_NORM, skip_nonfinite=skip_nonfinite)
    ref = Ref(kind, case.host, case.group_of, MAX_NORM, skip_nonfinite)
    clipped = []
    for gs in _grad_steps(200, SCALES[:3]):
        case.set_grads(gs)
        case.opt.step()
        ref.step(gs)
        clipped.append(ref.gnorm > MAX_NORM)
        got = case.opt.grad_norm()
        assert got.dim() == 0 and got.is_cuda
        rel = abs(got.item() - ref.gnorm) / ref.gnorm
        print(f"{kind} gnorm {ref.gnorm:.6g} rel err {rel:.2e}")
        assert rel <= 1e-5  # the tolerance of tests/test_optim_layerwise_gpu.py for the norm
    assert clipped == [False, True, False]  # the clip is active on some steps, not on others
    torch.cuda.synchronize()
    _assert_matches_ref(case, ref)
    assert _bands_intact(case.flat) and _bands_intact(case.gflat)
    assert int(case.opt.skipped_steps()) == 0


# ---------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_clip_of_exactly_one_is_bitwise_the_unclipped_step(kind):
    a = Case(kind, max_grad_norm=1e30)
    b = Case(kind)
    assert a.opt.whole_step_fallback and not b.opt.whole_step_fallback
    for gs in _grad_steps(300, SCALES[:3]):
        for c in (a, b):
            c.set_grads(gs)
            c.opt.step()
    assert float(a.opt._glob[3]) == 1.0 and b.opt._glob is None
    _assert_bitwise(a.snapshot(), b.snapshot())


@pytest.mark.parametrize("max_grad_norm,clip", [(256.0, 1.0), (64.0, 0.5), (32.0, 0.25)])
def test_power_of_two_gradients_give_exact_weights(max_grad_norm, clip):
    """16384 gradient elements of +-1: the norm is exactly 128 (and 128 + 1e-6 rounds to 128 in
    fp32), so the clip coefficient is exactly max_grad_norm / 128 and, with lr = 0.5 and small
    integer weights, every new weight is exact."""
    gen = torch.Generator().manual_seed(400)
    sizes = [4099, 1, 3, 12281]
    assert sum(sizes) == 16384
    w = [torch.randint(-8, 9, (n,), generator=gen).float() for n in sizes]
    g = [torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1 for n in sizes]
    views, flat = _flat_views(w[2:])
    params = [t.cuda().requires_grad_(True) for t in w[:2]] + [v.requires_grad_(True) for v in views]
    for p, gi in zip(params, g):
        p.grad = gi.cuda()
    opt = FusedSGD([{"params": params[::2]}, {"params": params[1::2]}], lr=0.5, max_grad_norm=max_grad_norm)
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.grad_norm()) == 128.0 and float(opt._glob[3]) == clip
    for p, wi, gi in zip(params, w, g):
        assert torch.equal(p.detach().cpu(), wi - 0.5 * clip * gi)
    assert _bands_intact(flat)


# ---------------------------------------------------------------------------------------------
# declined steps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["scalar_tail", "aligned_chunk"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_step_stores_nothing(kind, bad, where):
    case = Case(kind, max_grad_norm=MAX_NORM, skip_nonfinite=True, capturable=True)
    ref = Ref(kind, case.host, case.group_of, MAX_NORM, True)
    steps = _grad_steps(500, [SCALES[0], SCALES[1], SCALES[3]])
    if where == "scalar_tail":  # the last element in memory of the last tensor (a view: the scalar path)
        steps[1][-1][-1, -1, -1, -1] = bad
    else:                       # inside the second chunk of the aligned 2 CHUNK + 4 tensor
        assert case.params[5].numel() == 2 * CHUNK + 4 and case.params[5].data_ptr() % 16 == 0
        steps[1][5][CHUNK + 8] = bad
    case.set_grads(steps[0])
    case.opt.step()
    ref.step(steps[0])
    before = case.snapshot()
    assert all(float(before[f"dev{gi}"][1]) == (0.0 if kind == "sgd" else 1.0) for gi in (0, 1))
    case.set_grads(steps[1])
    case.opt.step()
    ref.step(steps[1])
    _assert_bitwise(case.snapshot(), before)
    assert _bands_intact(case.flat) and _bands_intact(case.gflat)
    sk = case.opt.skipped_steps()
    assert sk.dim() == 0 and sk.is_cuda and not sk.dtype.is_floating_point and int(sk) == 1
    assert not math.isfinite(float(case.opt.grad_norm()))
    # a finite step follows: the step count advanced once, not twice
    case.set_grads(steps[2])
    case.opt.step()
    ref.step(steps[2])
    torch.cuda.synchronize()
    assert ref.t == 2 and int(case.opt.skipped_steps()) == 1
    _assert_matches_ref(case, ref)
    if kind != "sgd":
        assert all(float(st["step"]) == 2 for st in case.opt.state_dict()["state"].values())


# ---------------------------------------------------------------------------------------------
# HIP-graph capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_captured_step_replays_bitwise_like_eager(kind):
    kw = dict(max_grad_norm=MAX_NORM, skip_nonfinite=True, capturable=True)
    case, twin = Case(kind, **kw), Case(kind, **kw)
    # eager warm-up, then replays: below the threshold, above it, non-finite, and a finite one again
    steps = _grad_steps(600, [SCALES[3], SCALES[0], SCALES[1], SCALES[0], SCALES[3]])
    steps[3][2][7] = float("inf")
    norms = [math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs)) for gs in steps]
    assert norms[1] < MAX_NORM < norms[2] and not math.isfinite(norms[3])
    graph = None
    for i, gs in enumerate(steps):
        for c in (case, twin):
            c.set_grads(gs)  # copied into the static gradient buffers
        twin.opt.step()
        if i == 0:  # state, tables, device scalars, the norm buffers and the counter exist before the capture
            case.opt.step()
            continue
        if graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                case.opt.step()  # (recorded, not run)
            torch.cuda.current_stream().wait_stream(side)
        case.opt.refresh_scalars()
        graph.replay()
        _assert_bitwise(case.snapshot(), twin.snapshot())
        assert torch.equal(case.opt.grad_norm(), twin.opt.grad_norm()) or i == 3
        assert int(case.opt.skipped_steps()) == int(twin.opt.skipped_steps()) == (1 if i >= 3 else 0)
    assert _bands_intact(case.flat)
    if kind != "sgd":
        assert all(float(st["step"]) == 4 for st in case.opt.state_dict()["state"].values())


# ---------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_launches_of_one_step(kind, monkeypatch):
    calls = []
    real = fused_mod._call

    def recording(entry, *args, **kw):
        calls.append(entry)
        return real(entry, *args, **kw)

    monkeypatch.setattr(fused_mod, "_call", recording)
    step2, step3 = ("sgd_step2", "sgd_step3") if kind == "sgd" else ("adam_step2", "adam_step3")
    gs = _grad_steps(700, [1.0])[0]
    for kw, want in [(dict(), [step2, step2]),  # the defaults: what a step launched before the options existed
                     (dict(max_grad_norm=1.0), ["sumsq_chunks", "norm_finalize"] * 2 + [step3] * 2),
                     (dict(skip_nonfinite=True), ["sumsq_chunks", "norm_finalize"] * 2 + [step3] * 2)]:
        case = Case(kind, **kw)
        case.set_grads(gs)
        for _ in range(2):
            del calls[:]
            case.opt.step()
            assert calls == want, kw
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# trainer.log_grad_norm under trainer.hip_graph
# ---------------------------------------------------------------------------------------------
def test_trainer_logs_grad_norm_of_replayed_steps(tmp_path):
    """The native bf16 ResNet-50 (the smallest model the graph tests of the Trainer run) at batch
    16: the warm-up steps run eagerly, two more are replays."""
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.ops import fused
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    from pytorch_distributed_template_amd.trainer.trainer import GRAPH_WARMUP
    steps = GRAPH_WARMUP + 2
    cfg = json.loads((ROOT / "config" / "resnet50_bf16.json").read_text())
    cfg["optimizer"]["args"].update(max_grad_norm=1.0, skip_nonfinite=True)
    cfg["trainer"].update(save_dir=str(tmp_path), len_epoch=steps, epochs=1, verbosity=1, hip_graph=True,
                          log_grad_norm=True)
    cfg["train_loader"]["args"].update(batch_size=16, num_samples=16 * steps)
    env = {"PDT_AUTOTUNE": "0", "PDT_DETERMINISTIC": "1"}  # no variant timing in a test
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        torch.manual_seed(0)
        device = torch.device("cuda", torch.cuda.current_device())
        config = ConfigParser(cfg, run_id="clip")
        model = build_model(config, device)
        criterion, metrics = build_criterion_metrics(config)
        optimizer, sched = build_optimizer(config, model)
        assert type(optimizer) is FusedSGD and optimizer.capturable and optimizer.max_grad_norm == 1.0
        tr = Trainer(model, criterion, metrics, optimizer, config=config, device=device,
                     data_loader=build_loader(config, "train_loader"), lr_scheduler=sched, len_epoch=steps,
                     autocast_dtype=autocast_dtype(config, device), channels_last=True)
        assert tr.hip_graph and tr.log_grad_norm
        tr._on_epoch_start(1)
        log = tr._train_epoch(1)
        torch.cuda.synchronize()
    finally:
        fused.set_backend("auto")
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print(log)
    assert tr._graph is not None and tr._graph_eager_steps == GRAPH_WARMUP
    assert math.isfinite(log["grad_norm"]) and log["grad_norm"] > 0 and math.isfinite(log["loss"])
    assert log["skipped_steps"] == 0
    # the last step was a replay: the optimizer's buffer holds that replay's norm
    assert math.isfinite(float(optimizer.grad_norm())) and int(optimizer.skipped_steps()) == 0
