"""What the five fused optimizers share (optim/fused.py ``_FusedBase``: the frame of ``step()``,
the gradient densifier, state creation, shadows, versions, ``state_dict``; csrc/optim_common.h in
the kernels), on an MI355X: one toy case stepped by every class, against ``torch.optim`` for
FusedSGD / FusedAdam / FusedAdamW and against the float64 references of tests/layerwise_ref.py
for FusedLARS / FusedLAMB.

Two param groups with their own lr and weight decay. ``(1025,)`` spans two of the 1024-element
work-list chunks and ends in a tail that is no multiple of 4. Three gradients are special: the
channels_last 4-D parameter gets an NCHW-contiguous one (the densifier re-lays it), ``(33, 40)``
gets an fp16 one (by a swap of ``grad.data``: torch refuses to assign it; the densifier casts it)
and one more parameter gets none at all (it must stay as it is, without state)."""
import copy
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layerwise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402
from pytorch_distributed_template_amd.optim import FusedAdam, FusedAdamW, FusedLAMB, FusedLARS, FusedSGD  # noqa: E402
from pytorch_distributed_template_amd.optim import fused as fused_mod  # noqa: E402

SHAPES = [(8, 4, 3, 3), (33, 40), (1025,), (3,)]
NO_GRAD_SHAPE = (5, 7)   # the parameter that never receives a gradient (last of group 0)
HALF_GRAD = 1            # index of the parameter whose gradient is fp16
GROUP_OF = [0, 1, 0, 1]
LRS = {"sgd": (0.1, 0.05), "adam": (1e-3, 2e-3), "adamw": (1e-3, 2e-3), "lars": (0.1, 0.05), "lamb": (0.05, 0.025)}
WDS = {"sgd": (1e-4, 1e-3), "adam": (1e-2, 0.0), "adamw": (0.05, 0.01), "lars": (1e-2, 1e-3), "lamb": (0.01, 0.1)}
HP = {"sgd": dict(momentum=0.9, nesterov=True), "adam": dict(amsgrad=True), "adamw": dict(),
      "lars": dict(momentum=0.9, nesterov=True, trust_coefficient=0.1, eps=1e-8),
      "lamb": dict(betas=(0.9, 0.999), eps=1e-6)}
MAX_NORM = 1.0  # the 2636 N(0, 1) gradient elements have norm ~51: LARS / LAMB clip on every step
FUSED = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW, "lars": FusedLARS, "lamb": FusedLAMB}
TORCH = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW,
         "lars": torch.optim.SGD, "lamb": torch.optim.Adam}  # the optimizer of the same state layout
OWN_KEYS = {"lars": ("trust_coefficient", "eps", "exclude_1d"), "lamb": ("exclude_1d",)}
KINDS = list(FUSED)
STEPS = 4


def setup_module(module):
    assert no.available(), "native library must be built and loaded on GPU runs"
    no.require()


@pytest.fixture(autouse=True)
def small_chunks(monkeypatch):
    monkeypatch.setattr(fused_mod, "CHUNK", 1024)


def make_params():
    """The four parameters with gradients and, last, the one without (fp32 CUDA leaves)."""
    gen = torch.Generator().manual_seed(71)
    ps = [torch.randn(s, generator=gen) for s in SHAPES + [NO_GRAD_SHAPE]]
    ps[0] = ps[0].contiguous(memory_format=torch.channels_last)
    return [p.cuda().requires_grad_(True) for p in ps]


@functools.lru_cache(maxsize=None)
def make_grads():
    """``STEPS`` lists of fp32 CPU gradients (NCHW-contiguous for the 4-D parameter; the values
    of ``HALF_GRAD``'s are fp16 numbers, so the fp16 copy the fused optimizer gets is exact)."""
    gen = torch.Generator().manual_seed(72)
    out = []
    for _ in range(STEPS):
        gs = [torch.randn(s, generator=gen) for s in SHAPES]
        gs[HALF_GRAD] = gs[HALF_GRAD].half().float()
        out.append(gs)
    return out


def set_grads(params, grads, half=False):
    """New gradient tensors, as autograd leaves them after ``zero_grad()``."""
    for i, g in enumerate(grads):
        p = params[i]
        p.grad = g.cuda()
        assert p.grad.stride() != p.stride() or i != 0
        if half and i == HALF_GRAD:
            p.grad.data = p.grad.data.half()
            assert p.grad.dtype == torch.float16 and p.dtype == torch.float32


def groups_of(kind, params):
    """Group 0: parameters 0, 2 and the one without a gradient; group 1: parameters 1, 3."""
    g0 = [params[0], params[2], params[4]]
    g1 = [params[1], params[3]]
    return [{"params": g, "lr": LRS[kind][gi], "weight_decay": WDS[kind][gi]} for gi, g in enumerate((g0, g1))]


def make_fused(kind, params, capturable):
    kw = dict(max_grad_norm=MAX_NORM) if kind in ("lars", "lamb") else {}
    return FUSED[kind](groups_of(kind, params), lr=LRS[kind][0], capturable=capturable, **HP[kind], **kw)


def make_torch(kind, params):
    hp = {k: v for k, v in HP[kind].items() if k not in OWN_KEYS.get(kind, ())}
    return TORCH[kind](groups_of(kind, params), **hp)


@functools.lru_cache(maxsize=None)
def reference(kind):
    """The four stepped parameters after ``STEPS`` steps, fp32 on the CPU: torch.optim's on the
    GPU for sgd / adam / adamw; for lars / lamb the float64 reference, one object per param group
    (each has one lr) without clipping of its own, fed the gradients times the clip coefficient
    of all of them -- what a single reference computes."""
    grads = make_grads()
    if kind in ("sgd", "adam", "adamw"):
        params = make_params()
        opt = make_torch(kind, params)
        for gs in grads:
            set_grads(params, gs)
            opt.step()
        return [p.detach().cpu() for p in params[:4]]
    params = [p.detach().cpu() for p in make_params()[:4]]
    cls = R.RefLARS if kind == "lars" else R.RefLAMB
    refs = []
    for gi in (0, 1):
        idx = [i for i in range(4) if GROUP_OF[i] == gi]
        group = {"w": [params[i].double() for i in idx], "adapt": [params[i].dim() > 1 for i in idx],
                 "weight_decay": WDS[kind][gi]}
        refs.append((idx, cls([group], max_grad_norm=0.0, **HP[kind])))
    for gs in grads:
        clip = R.clip_coef([[g.double() for g in gs]], MAX_NORM)
        assert clip < 1
        for gi, (idx, ref) in enumerate(refs):
            ref.step([[gs[i].double() * clip for i in idx]], LRS[kind][gi])
    out = [None] * 4
    for idx, ref in refs:
        for i, w in zip(idx, ref.groups[0]["w"]):
            out[i] = w.to(torch.float32)
    return out


def run_fused(kind, capturable):
    """``STEPS`` steps of the fused optimizer on the toy case; the first one through a closure."""
    params = make_params()
    opt = make_fused(kind, params, capturable)
    for step, gs in enumerate(make_grads()):
        set_grads(params, gs, half=True)
        if step == 0:
            def closure():
                assert torch.is_grad_enabled()
                return torch.tensor(1.5)
            assert float(opt.step(closure)) == 1.5
        else:
            assert opt.step() is None
    torch.cuda.synchronize()
    return params, opt


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_step_matches_reference(kind, capturable):
    start = make_params()
    versions = [p._version for p in start]
    params, opt = run_fused(kind, capturable)
    want = reference(kind)
    for i, (p, w) in enumerate(zip(params[:4], want)):
        got = p.detach().cpu()
        err = float((got - w).abs().max())
        print(f"{kind} capturable={capturable} param {i} {tuple(p.shape)}: max abs err {err:.3e}")
        assert torch.allclose(got, w, rtol=1e-5, atol=1e-6), (i, tuple(p.shape), err)
    # the parameter without a gradient: untouched, stateless, no shadow
    idle = params[4]
    assert torch.equal(idle, start[4]) and idle._version == versions[4]
    assert idle not in opt.state and id(idle) not in opt._shadows
    # versions moved, and the registered bf16 shadow is the one the step wrote
    for p, v0 in zip(params[:4], versions):
        assert p._version > v0
        sh = no._SHADOWS[id(p)][0]
        assert sh is opt._shadows[id(p)]
        assert sh.dtype == torch.bfloat16 and torch.equal(sh, p.detach().to(torch.bfloat16))
        assert no.bf16_weight(p) is sh
    # state_dict() is torch's: it loads into the torch optimizer of the same state layout
    sd = copy.deepcopy(opt.state_dict())
    for group in sd["param_groups"]:
        for k in OWN_KEYS.get(kind, ()):
            del group[k]
    clones = [p.detach().clone().requires_grad_(True) for p in params]
    t = make_torch(kind, clones)
    t.load_state_dict(sd)
    assert set(sd["state"]) == {0, 1, 3, 4}  # (positions in the groups' order: 2 is the idle one)
    for p, q in zip(params[:4], clones[:4]):
        for k, v in opt.state[p].items():
            assert torch.equal(t.state[q][k].cpu(), v.cpu()), k
        if "step" in opt.state[p]:
            assert float(t.state[q]["step"]) == STEPS


@pytest.mark.parametrize("kind,name", [("adam", "FusedAdam"), ("adamw", "FusedAdam"), ("lamb", "FusedLAMB")])
def test_capturable_changed_gradient_set_raises(kind, name):
    params = make_params()
    opt = make_fused(kind, params, True)
    grads = make_grads()
    set_grads(params, grads[0], half=True)
    opt.step()
    set_grads(params, grads[1], half=True)
    params[2].grad = None  # group 0 steps 1 parameter instead of 2
    before = [p.detach().clone() for p in params]
    with pytest.raises(RuntimeError) as exc:
        opt.step()
    assert str(exc.value) == (
        f"capturable {name}: the set of parameters with gradients changed between steps "
        "(group 0: 2 -> 1 params); the group's single device step "
        "count requires every parameter to receive a gradient on every step")
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(params, before))  # raised ahead of every launch
