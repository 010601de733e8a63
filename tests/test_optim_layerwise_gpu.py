"""The layer-wise optimizer kernels (csrc/optim_layerwise.hip) on an MI355X: the multi-tensor
L2 norm, FusedLARS / FusedLAMB against float64 references written from their definitions
(tests/layerwise_ref.py), gradient-norm clipping, the bf16 shadows, and HIP-graph replay.

Work-list chunks are shrunk to 1024 elements so that small tensors span many chunks."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layerwise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402
from pytorch_distributed_template_amd.optim import FusedLAMB, FusedLARS  # noqa: E402
from pytorch_distributed_template_amd.optim import fused as fused_mod  # noqa: E402

SHAPES = [(64, 3, 7, 7), (100, 257), (257,), (3,), (1,)]
EXTRA = [(40, 33), (33, 40)]  # the zero-gradient and the zero-weight tensor
STEPS = 4
LRS = {"lars": [0.1, 0.1, 0.05, 0.025, 0.0125], "lamb": [0.05, 0.05, 0.025, 0.0125, 0.00625]}
WDS = {"lars": (1e-2, 1e-3), "lamb": (0.01, 0.1)}
HP = {"lars": dict(momentum=0.9, nesterov=True, trust_coefficient=0.1, eps=1e-8),
      "lamb": dict(betas=(0.9, 0.999), eps=1e-6)}
MAX_NORM = 1.0  # the ~37k N(0, 1) gradient elements have norm ~190: clip < 1 on every step


def setup_module(module):
    assert no.available(), "native library must be built and loaded on GPU runs"
    no.require()


@pytest.fixture(autouse=True)
def small_chunks(monkeypatch):
    monkeypatch.setattr(fused_mod, "CHUNK", 1024)


def _unaligned_like(tensors):
    """Copies of ``tensors`` as views into one flat buffer starting at element 1."""
    flat = torch.zeros(sum(t.numel() for t in tensors) + 1, device="cuda")
    off, out = 1, []
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
    assert out[0].data_ptr() % 16 == 4  # (a later view may land on a 16-byte boundary)
    return out


# ---------------------------------------------------------------------------------------------
# multi_tensor_l2norm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unaligned", [False, True])
def test_multi_tensor_l2norm(unaligned):
    gen = torch.Generator().manual_seed(11)
    sizes = [1, 3, 1023, 1024, 1025, 4 * 1024 + 5]
    host = [torch.randn(n, generator=gen) for n in sizes]
    host.append(torch.randn(16, 8, 3, 3, generator=gen).contiguous(memory_format=torch.channels_last))
    ts = [t.cuda() for t in host]
    if unaligned:
        ts = _unaligned_like(ts)
    else:
        assert all(t.data_ptr() % 16 == 0 for t in ts)
    norms, gnorm = no.multi_tensor_l2norm(ts)
    assert norms.dtype == torch.float32 and norms.shape == (len(ts),) and norms.is_cuda
    assert gnorm.dim() == 0 and gnorm.is_cuda
    norms2, gnorm2 = no.multi_tensor_l2norm(ts)
    want = torch.tensor([float(t.double().norm()) for t in host], dtype=torch.float64)
    want_g = math.sqrt(float((want * want).sum()))
    got = norms.cpu().double()
    print("per-tensor rel err", ((got - want).abs() / want).tolist(), "global", abs(gnorm.item() - want_g) / want_g)
    assert torch.allclose(got, want, rtol=1e-5, atol=0)
    assert abs(gnorm.item() - want_g) <= 1e-5 * want_g
    assert torch.equal(norms, norms2) and torch.equal(gnorm, gnorm2)


# ---------------------------------------------------------------------------------------------
# FusedLARS / FusedLAMB against the fp64 reference
# ---------------------------------------------------------------------------------------------
def _make(kind, params, group_of, exclude_1d, max_grad_norm, **kw):
    pg = R.split(params, group_of)
    groups = [{"params": pg[0], "weight_decay": WDS[kind][0]}, {"params": pg[1], "weight_decay": WDS[kind][1]}]
    cls = FusedLARS if kind == "lars" else FusedLAMB
    return cls(groups, lr=LRS[kind][0], exclude_1d=exclude_1d, max_grad_norm=max_grad_norm, **HP[kind], **kw)


def _ref(kind, params, group_of, exclude_1d, max_grad_norm):
    groups = R.ref_groups(params, group_of, WDS[kind], exclude_1d)
    cls = R.RefLARS if kind == "lars" else R.RefLAMB
    return cls(groups, max_grad_norm=max_grad_norm, **HP[kind])


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("max_grad_norm", [0.0, MAX_NORM])
@pytest.mark.parametrize("exclude_1d", [True, False])
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_native_step_matches_fp64_reference(kind, exclude_1d, max_grad_norm, unaligned):
    params, kinds, group_of = R.make_case(SHAPES, EXTRA, "cuda", seed=21, unaligned=unaligned)
    grads = R.make_grads(params, kinds, torch.Generator().manual_seed(22), STEPS)
    if unaligned:  # gradients too, like views into a DDP bucket
        assert all(p.data_ptr() % 16 != 0 for p in params)
        for p, g in zip(params, _unaligned_like([torch.zeros_like(p) for p in params])):
            p.grad = g
    opt = _make(kind, params, group_of, exclude_1d, max_grad_norm)
    ref = _ref(kind, params, group_of, exclude_1d, max_grad_norm)
    versions = [p._version for p in params]
    for step in range(STEPS):
        if max_grad_norm > 0:
            assert R.clip_coef([[g.double() for g in grads[step]]], max_grad_norm) < 1
        R.set_grads(params, grads[step])
        for group in opt.param_groups:
            group["lr"] = LRS[kind][step]
        opt.step()
        ref.step(R.split([g.double() for g in grads[step]], group_of), LRS[kind][step])
    assert opt._plans and all(plan.nchunks > len(plan.norm_tables.key) for plan in opt._plans.values())
    R.assert_matches(params, group_of, ref, rtol=1e-5, atol=1e-6)
    # the bf16 shadow written by the step is the registered one, and versions moved
    for p, v0 in zip(params, versions):
        assert p._version > v0
        sh = no._SHADOWS[id(p)][0]
        assert sh is opt._shadows[id(p)]
        assert torch.equal(sh, p.detach().to(torch.bfloat16))
        if not unaligned:  # (views into one buffer share its version counter: each step outdates the others)
            assert no.bf16_weight(p) is sh  # current: the forward reads it without a cast


# ---------------------------------------------------------------------------------------------
# clipping
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_clipping_equals_scaled_gradients(kind):
    """max_grad_norm = 0.5 |g|: the first step is that of an unclipped optimizer fed 0.5 g."""
    a_params, kinds, group_of = R.make_case(SHAPES, EXTRA, "cuda", seed=31)
    b_params, _, _ = R.make_case(SHAPES, EXTRA, "cuda", seed=31)
    grads = R.make_grads(a_params, kinds, torch.Generator().manual_seed(32), 1)[0]
    gnorm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    a = _make(kind, a_params, group_of, True, 0.5 * gnorm)
    b = _make(kind, b_params, group_of, True, 0.0)
    R.set_grads(a_params, grads)
    R.set_grads(b_params, [0.5 * g for g in grads])
    a.step()
    b.step()
    assert abs(a.grad_norm().item() - gnorm) <= 1e-5 * gnorm
    for p, q in zip(a_params, b_params):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), (tuple(p.shape), float((p - q).abs().max()))


# ---------------------------------------------------------------------------------------------
# HIP-graph capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_captured_step_replays_bitwise_like_eager(kind):
    params, kinds, group_of = R.make_case(SHAPES, EXTRA, "cuda", seed=41)
    twins, _, _ = R.make_case(SHAPES, EXTRA, "cuda", seed=41)
    grads = R.make_grads(params, kinds, torch.Generator().manual_seed(42), 5)
    opt = _make(kind, params, group_of, True, MAX_NORM, capturable=True)
    twin = _make(kind, twins, group_of, True, MAX_NORM, capturable=True)
    graph = None
    for i in range(5):
        R.set_grads(params, grads[i])  # copied into the static gradient buffers
        R.set_grads(twins, grads[i])
        for o in (opt, twin):
            for group in o.param_groups:
                group["lr"] = LRS[kind][i]
        twin.step()
        if i < 2:  # eager warm-up: state, tables and device scalars exist before the capture
            opt.step()
            continue
        if graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                opt.step()  # (recorded, not run: the first replay is step 3)
            torch.cuda.current_stream().wait_stream(side)
        opt.refresh_scalars()
        graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(params, twins):
        assert torch.equal(p, q), (tuple(p.shape), float((p - q).abs().max()))
    if kind == "lamb":
        assert float(opt.state_dict()["state"][0]["step"]) == 5


def test_capturing_a_lars_step_that_creates_momentum_buffers_raises():
    params, kinds, group_of = R.make_case(SHAPES, EXTRA, "cuda", seed=51)
    R.set_grads(params, R.make_grads(params, kinds, torch.Generator().manual_seed(52), 1)[0])
    opt = _make("lars", params, group_of, True, 0.0, capturable=True)
    before = [p.detach().clone() for p in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="momentum buffer"):
        with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(params, before))
