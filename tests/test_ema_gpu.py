"""The weight-EMA kernel (csrc/ema.hip) and ``optim.ModelEMA``'s native path on an MI355X, against
the float64 recurrence, the fp32 tick mirror and the error bound of tests/ema_ref.py.

Averaged tensors and shadows sit in guard-banded buffers (tests/kernel_ref.py); work-list chunks
are shrunk to 1024 elements so that small tensors span many chunks. The tensor set is run
aligned (16-byte vector path) and as views starting at element 1 of a flat buffer (scalar path).

General family, worst error / bound measured on an MI355X: 0.937 in all four cases (aligned or
not, with or without shadows), printed by
``test_general_family_within_bound_and_dev_equals_the_mirror``. The bound is close by nature:
its last term is half an ulp of the result wherever the result lies just above a power of two."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as R  # noqa: E402
import kernel_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402
from pytorch_distributed_template_amd.optim import ModelEMA  # noqa: E402
from pytorch_distributed_template_amd.optim import ema as ema_mod  # noqa: E402
from pytorch_distributed_template_amd.optim import fused as fused_mod  # noqa: E402

DEV = torch.device("cuda")
SHAPES = [(n,) for n in R.SIZES] + [R.CL_SHAPE]
BF16_POISON = -1  # int16 view of the 0xFFFF kr.guarded() fills with


def setup_module(module):
    assert no.available(), "native library must be built and loaded on GPU runs"
    no.require()


@pytest.fixture(autouse=True)
def small_chunks(monkeypatch):
    monkeypatch.setattr(fused_mod, "CHUNK", 1024)


# ---------------------------------------------------------------------------------------------
# the tensor set
# ---------------------------------------------------------------------------------------------
def _views(flat, shapes, off):
    """Views of ``shapes`` into ``flat`` from element ``off`` on (4-d: channels_last strides)."""
    out = []
    for s in shapes:
        n = int(np.prod(s))
        v = flat[off:off + n]
        out.append(v.view(s[0], s[2], s[3], s[1]).permute(0, 3, 1, 2) if len(s) == 4 else v.view(s))
        off += n
    return out


class Case:
    """The averaged tensors (guard-banded), their sources and optional bf16 shadows (guard-banded),
    aligned or as views from element 1 of a flat buffer; ``shadows``: "none" | "all" | "one_null"
    (the table present, the entry of tensor 2 null)."""

    def __init__(self, shapes, host, unaligned, shadows):
        total = sum(int(np.prod(s)) for s in shapes)
        self.shapes, self.unaligned = shapes, unaligned
        if unaligned:
            self.flat = kr.guarded(total + 1, torch.float32, DEV, fill=0.0)
            self.e = _views(self.flat, shapes, 1)
            self.src = _views(torch.zeros(total + 1, device=DEV), shapes, 1)
            assert self.e[0].data_ptr() % 16 == 4 and self.src[0].data_ptr() % 16 == 4
        else:
            self.e = [_views(kr.guarded(int(np.prod(s)), torch.float32, DEV), [s], 0)[0] for s in shapes]
            self.src = [_views(torch.zeros(int(np.prod(s)), device=DEV), [s], 0)[0] for s in shapes]
            assert all(t.data_ptr() % 16 == 0 for t in self.e + self.src)
        for e, h in zip(self.e, host):
            e.copy_(h)
        self.sh = None
        if shadows != "none":
            if unaligned:
                self.sh_flat = kr.guarded(total + 1, torch.bfloat16, DEV)
                self.sh = _views(self.sh_flat, shapes, 1)
                assert self.sh[0].data_ptr() % 8 == 2
            else:
                self.sh = [_views(kr.guarded(int(np.prod(s)), torch.bfloat16, DEV), [s], 0)[0] for s in shapes]
            if shadows == "one_null":
                self.sh[2] = None
        self.plan = fused_mod._Plan(self.e, DEV)
        assert self.plan.nchunks == sum((int(np.prod(s)) + 1023) // 1024 for s in shapes)

    def dev(self, decay):
        return torch.tensor([0.0, decay, 1.0 - decay], dtype=torch.float32, device=DEV)

    def update(self, host_src, dev, decay, warmup):
        for s, h in zip(self.src, host_src):
            s.copy_(h)
        ema_mod.multi_tensor_ema_(self.plan, self.e, self.src, self.sh, dev, decay, warmup)

    def check_shadows(self):
        """Every shadow is torch's bf16 rounding of its tensor bit for bit; a null entry's tensor has none."""
        if self.sh is None:
            return
        for e, sh in zip(self.e, self.sh):
            if sh is not None:
                assert torch.equal(sh.contiguous().view(torch.int16),
                                   e.to(torch.bfloat16).contiguous().view(torch.int16)), tuple(e.shape)

    def check_guards(self, what):
        torch.cuda.synchronize()
        if self.unaligned:
            assert float(self.flat[0]) == 0.0, f"{what}: store before the first view"
            if self.sh is not None:
                assert int(self.sh_flat[:1].view(torch.int16)) == BF16_POISON, f"{what}: store before the first shadow"
        kr.check_guards(what)


def _host(shapes, make):
    out = []
    for s in shapes:
        t = make(s)
        out.append(t.contiguous(memory_format=torch.channels_last) if len(s) == 4 else t)
    return out


# ---------------------------------------------------------------------------------------------
# exact family
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadows", ["none", "all", "one_null"])
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.75])
def test_exact_family_equals_float64(decay, unaligned, shadows):
    gen = torch.Generator().manual_seed(101)
    host = _host(SHAPES, lambda s: R.exact_values(s, gen))
    case = Case(SHAPES, host, unaligned, shadows)
    refs = [h.double() for h in host]
    dev = case.dev(decay)
    for (t, d, w) in R.schedule(4, decay, False):
        src = _host(SHAPES, lambda s: R.exact_values(s, gen))
        case.update(src, dev, decay, False)
        refs = [R.ref_update(r, p, w) for r, p in zip(refs, src)]
    assert dev.cpu().numpy().view(np.int32).tolist() == np.array([t, d, w], np.float32).view(np.int32).tolist()
    for e, r in zip(case.e, refs):
        assert torch.equal(e.cpu().double(), r), (tuple(e.shape), float((e.cpu().double() - r).abs().max()))
    case.check_shadows()
    if shadows == "one_null":
        assert case.sh[2] is None and case.plan.ptr_keys["s"][2] == 0 and all(
            p != 0 for i, p in enumerate(case.plan.ptr_keys["s"]) if i != 2)
    case.check_guards(f"exact decay={decay} unaligned={unaligned} shadows={shadows}")


def test_second_trip_of_the_grid_stride_loop():
    """2049 * 1024 + 3 elements: 2050 chunks against ``grid_for``'s cap of 2048 workgroups."""
    n = 2049 * 1024 + 3
    gen = torch.Generator(device=DEV).manual_seed(7)

    def values():
        return (torch.randint(-128, 129, (n,), generator=gen, device=DEV) * 256).float()
    e = kr.guarded(n, torch.float32, DEV, fill=values())
    sh = kr.guarded(n, torch.bfloat16, DEV)
    src = values()
    ref = e.double()
    plan = fused_mod._Plan([e], DEV)
    assert plan.nchunks == 2050
    dev = torch.tensor([0.0, 0.75, 0.25], dtype=torch.float32, device=DEV)
    _, _, w = R.tick(0, 0.75, False)
    ema_mod.multi_tensor_ema_(plan, [e], [src], [sh], dev, 0.75, False)
    ref = R.ref_update(ref, src, w)
    assert torch.equal(e.double(), ref)
    assert not torch.equal(e[-1027:], src[-1027:])  # (the last two chunks were averaged, not copied)
    assert torch.equal(sh.view(torch.int16), e.to(torch.bfloat16).view(torch.int16))
    torch.cuda.synchronize()
    kr.check_guards("second trip")


# ---------------------------------------------------------------------------------------------
# general family
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadows", ["none", "all"])
@pytest.mark.parametrize("unaligned", [False, True])
def test_general_family_within_bound_and_dev_equals_the_mirror(unaligned, shadows):
    gen = torch.Generator().manual_seed(202)
    host = _host(SHAPES, lambda s: torch.randn(s, generator=gen))
    case = Case(SHAPES, host, unaligned, shadows)
    bounds = [R.Bound(h) for h in host]
    dev = case.dev(0.9999)
    worst = 0.0
    for step, (t, d, w) in enumerate(R.schedule(12, 0.9999, True)):
        src = _host(SHAPES, lambda s: torch.randn(s, generator=gen))
        case.update(src, dev, 0.9999, True)
        got = dev.cpu().numpy()
        assert got.view(np.int32).tolist() == np.array([t, d, w], np.float32).view(np.int32).tolist(), (step, got)
        for b, p, e in zip(bounds, src, case.e):
            b.update(p, w)
            worst = max(worst, b.ratio(e.cpu()))
    print(f"general family unaligned={unaligned} shadows={shadows}: worst error / bound = {worst:.4f}")
    assert 0 < worst <= 1
    case.check_shadows()
    case.check_guards(f"general unaligned={unaligned} shadows={shadows}")


@pytest.mark.parametrize("decay,warmup", [(0.0, False), (0.3, False), (0.9999, True), (1.0, False)])
@pytest.mark.parametrize("unaligned", [False, True])
def test_fixed_point_is_kept_bit_for_bit(unaligned, decay, warmup):
    gen = torch.Generator().manual_seed(303)
    host = _host(SHAPES, lambda s: torch.randn(s, generator=gen) * 1e3)
    case = Case(SHAPES, host, unaligned, "all")
    dev = case.dev(decay)
    for _ in range(3):
        case.update(host, dev, decay, warmup)  # p == e
    for e, h in zip(case.e, host):
        assert torch.equal(e.cpu().contiguous().view(torch.int32), h.contiguous().view(torch.int32)), tuple(e.shape)
    case.check_shadows()
    case.check_guards(f"fixed point decay={decay}")


def test_negative_zero_fixed_point_becomes_positive_zero_as_torch_lerp():
    """The one exception to the fixed point: e == p == -0 gives -0 + w (+0) = +0."""
    e = torch.full((5,), -0.0, device=DEV)
    p = e.clone()
    plan = fused_mod._Plan([e], DEV)
    dev = torch.tensor([0.0, 0.9, 0.1], dtype=torch.float32, device=DEV)
    ema_mod.multi_tensor_ema_(plan, [e], [p], None, dev, 0.9, False)
    want = torch.full((5,), -0.0).lerp_(torch.full((5,), -0.0), 0.1)
    assert want.view(torch.int32).tolist() == [0] * 5
    assert e.cpu().view(torch.int32).tolist() == [0] * 5


def test_null_dev_is_an_error_code():
    e, p = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    plan = fused_mod._Plan([e], DEV)
    plan.update({"e": [e], "p": [p]})
    rc = no._load().pdt_ema_update(plan.chunks.data_ptr(), plan.nchunks, plan.ptr("e"), plan.ptr("p"), None, None,
                                   0.5, 0, torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    torch.cuda.synchronize()
    assert float(e.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# ModelEMA's native path: one launch, versions, shadows, HIP-graph replay
# ---------------------------------------------------------------------------------------------
class _Model(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        ps = _host(SHAPES, lambda s: torch.randn(s, generator=gen))
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p) for p in ps])
        self.register_buffer("running", torch.randn(37, generator=gen))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))


def _rewrite(model, gen):
    with torch.no_grad():
        for p in model.ps:
            p.copy_(torch.randn(p.shape, generator=gen))
        model.running.copy_(torch.randn(37, generator=gen))
        model.count.add_(1)


def test_model_ema_native_update_versions_and_shadows():
    model = _Model(1).to(DEV)
    ema = ModelEMA(model, decay=0.5, warmup=False, write_bf16_shadow=True)
    assert ema.module.ps[-1].is_contiguous(memory_format=torch.channels_last)
    before = {k: v.clone() for k, v in ema.module.state_dict().items()}
    versions = [p._version for p in ema.module.ps]
    _rewrite(model, torch.Generator().manual_seed(2))
    ema.update(model)
    assert ema._plan is not None and ema._dev is not None and ema.num_updates == 1  # the native path ran
    for k, v in ema.module.state_dict().items():
        m = model.state_dict()[k]
        if v.is_floating_point():
            want = before[k].double() + 0.5 * (m.double() - before[k].double())
            assert torch.allclose(v.double(), want, rtol=1e-6, atol=1e-6), k  # (the kernel tests bound it)
        else:
            assert torch.equal(v, m) and int(v) == 1, k
    for p, v0 in zip(ema.module.ps, versions):
        assert p._version > v0
        sh = no._SHADOWS[id(p)][0]
        assert sh is ema._shadows[id(p)] and sh.stride() == p.stride()
        assert torch.equal(sh, p.detach().to(torch.bfloat16))
        assert no.bf16_weight(p) is sh  # current: a forward on .module reads it without a cast
    assert id(ema.module.running) not in ema._shadows  # buffers get no shadow: null entries of the table
    tables = dict(ema._plan.ptr_keys)
    ema.update(model)
    assert dict(ema._plan.ptr_keys) == tables and ema.num_updates == 2  # nothing moved: no re-upload
    # a state restore re-forms and re-registers the shadows and restores t
    state = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ema.state_dict().items()}
    state["state_dict"] = {k: v.clone() for k, v in state["state_dict"].items()}
    _rewrite(model, torch.Generator().manual_seed(3))
    ema.update(model)
    ema.load_state_dict(state)
    assert ema.num_updates == 2
    for k, v in state["state_dict"].items():
        assert torch.equal(ema.module.state_dict()[k], v), k
    for p in ema.module.ps:
        assert no.bf16_weight(p) is ema._shadows[id(p)]
        assert torch.equal(ema._shadows[id(p)], p.detach().to(torch.bfloat16))


def test_captured_update_replays_bitwise_like_eager():
    model = _Model(11).to(DEV)
    ema = ModelEMA(model, decay=0.9999, warmup=True, write_bf16_shadow=True)
    twin = ModelEMA(model, decay=0.9999, warmup=True, write_bf16_shadow=True)
    gen = torch.Generator().manual_seed(12)
    graph = None
    for i in range(7):
        _rewrite(model, gen)  # in place: the captured update reads the same addresses
        twin.update(model)
        if i < 2:  # eager warm-up: tables and device state exist before the capture
            ema.update(model)
            continue
        if graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                ema.update(model)  # (recorded, not run: the first replay is update 3)
            torch.cuda.current_stream().wait_stream(side)
        graph.replay()
    torch.cuda.synchronize()
    assert ema.num_updates == 7 and twin.num_updates == 7
    assert ema._dev.cpu().numpy().view(np.int32).tolist() == \
        np.array(R.schedule(7, 0.9999, True)[-1], np.float32).view(np.int32).tolist()
    for (k, a), (_, b) in zip(ema.module.state_dict().items(), twin.module.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(ema.module.count) == 7
    for p in ema.module.ps:
        assert torch.equal(ema._shadows[id(p)], p.detach().to(torch.bfloat16))


def test_capturing_before_any_eager_update_raises():
    model = _Model(21).to(DEV)
    ema = ModelEMA(model, decay=0.9, warmup=True)
    before = {k: v.clone() for k, v in ema.module.state_dict().items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="graph capture"):
        with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
            ema.update(model)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in ema.module.state_dict().items())
    assert ema.num_updates == 0
