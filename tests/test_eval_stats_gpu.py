"""csrc/eval_stats.hip (``pdt_eval_stats``) called directly, against the float64 reference of
tests/eval_ref.py, and ``trainer.eval_mode: "stream"`` under the Trainer on the native LeNet.

Conditions: ``rank`` and the counts equal the reference exactly (comparisons of stored values
round nothing); ``loss_rows`` gets the allowance tests/test_row_kernels_gpu.py gives
``pdt_xent_fwd``'s rows -- 4 x the measured error of PyTorch's fp32 ``F.cross_entropy`` against the
float64 reference on the same input, floored at the fp32 resolution of the case -- and NLL rows are
exact; the double accumulator equals the float64 sum of the kernel's own rows within
B * 2^-52 * sum|rows| per launch. Every output sits between guard bands."""
import json
import math
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import eval_ref as er
import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = torch.device("cuda")
BF, F32, F64, I32, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64
KINDS = [("ce", 0.0), ("ce", 0.1), ("nll", 0.0)]


def _ks(ks):
    import ctypes
    arr = (ctypes.c_int * max(len(ks), 1))(*ks)
    return arr, ctypes.addressof(arr)


class Acc:
    """Guard-banded accumulators and the running sums they must hold."""

    def __init__(self, ks):
        self.ks = tuple(ks)
        self.loss = kr.guarded(1, F64, DEV, 0)
        self.counts = kr.guarded(2 + len(self.ks), I64, DEV, 0)
        self.want_loss, self.want_abs = 0.0, 0.0
        self.want_counts = torch.zeros(2 + len(self.ks), dtype=I64)
        self.poisoned = False


def launch(x, t, kind, eps, acc, what):
    """One ``pdt_eval_stats`` on ``x`` (any row stride) into ``acc``; every per-row and accumulator
    condition of the module docstring."""
    lib = no._load()
    B, V = x.shape
    ld = x.stride(0) if B > 1 else V
    bf16 = int(x.dtype == BF)
    epsf = float(torch.tensor(eps, dtype=F32))
    rows, rank = kr.guarded(B, F32, DEV), kr.guarded(B, I32, DEV, -7)
    keep, ks_ptr = _ks(acc.ks)
    assert lib.pdt_eval_stats(no._p(x), bf16, ld, no._p(t), no.EVAL_KINDS[kind], epsf, ks_ptr, len(acc.ks),
                              no._p(rows), no._p(rank), no._p(acc.loss), no._p(acc.counts), B, V, no._s()) == 0, what
    torch.cuda.synchronize()  # (the guard bands of every buffer are read once per group: test_eval_stats)
    ref = er.eval_ref(x, t, kind, epsf, acc.ks)
    assert torch.equal(rank.to(I64), ref["rank"]), f"{what}: rank {rank.tolist()} ref {ref['rank'].tolist()}"
    want_nan = torch.isnan(ref["loss_rows"])
    assert torch.equal(torch.isnan(rows), want_nan), what + " NaN rows"
    fin, valid = ~want_nan, ref["valid"]
    assert bool((rows[~valid] == 0).all()), what + " out-of-range rows"
    if kind == "nll":
        assert torch.equal(rows[fin].double(), ref["loss_rows"][fin]), what + " nll rows"
    elif bool((fin & valid).any()):
        sel = fin & valid
        rows_t = F.cross_entropy(x.float()[sel], t[sel], label_smoothing=eps, reduction="none")
        e_ref = (kr.f64(rows_t) - ref["loss_rows"][sel]).abs().max().item()
        e_ker = (kr.f64(rows[sel]) - ref["loss_rows"][sel]).abs().max().item()
        allow = 4 * max(e_ref, kr.U * ref["loss_rows_abs"][sel].abs().max().item())
        print(f"MEASURED {what}: rows ref {e_ref:.3e} kernel {e_ker:.3e} (allow {allow:.3e}, "
              f"ratio {e_ker / allow if allow else 0.0:.3f})")
        kr.assert_close(rows[sel], ref["loss_rows"][sel], allow, what + " loss rows")
    # the accumulators: added to, never overwritten
    acc.want_counts += ref["counts"]
    assert torch.equal(acc.counts.cpu(), acc.want_counts), f"{what}: counts {acc.counts.tolist()}"
    if bool(want_nan.any()):
        acc.poisoned = True
    if acc.poisoned:
        assert math.isnan(float(acc.loss)), what
    else:
        acc.want_loss += float(rows.double().sum())
        acc.want_abs += B * 2.0 ** -52 * float(rows.double().abs().sum())
        assert abs(float(acc.loss) - acc.want_loss) <= acc.want_abs, \
            f"{what}: loss sum {float(acc.loss)!r} want {acc.want_loss!r} +- {acc.want_abs!r}"
    return ref


@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1000, 1001])
def test_eval_stats(V, B):
    """Per dtype and row stride (V: dense; V + 3: the rows' 16-byte alignment alternates, the pad
    columns hold NaN): three launches on the cross-entropy input, one per loss kind, into one pair
    of accumulators with k = (1, 3, 5); the tie, +-0 and out-of-range families into a second pair
    with k = (1, 3, 5, V, V + 7); the NaN family into a third."""
    for di, dtype in enumerate((BF, F32)):
        for pad in (0, 3):
            tag = f"V={V} B={B} {'bf16' if dtype == BF else 'fp32'} ld=V+{pad}"
            g = kr.gen(1000 * B + V + 17 * pad + di, DEV)
            a, b, c = Acc((1, 3, 5)), Acc((1, 3, 5, V, V + 7)), Acc((1, V, V + 7))
            x, t = er.family("xent", B, V, dtype, g)
            x = er.strided(x, pad)
            for kind, eps in KINDS:
                launch(x, t, kind, eps, a, f"xent {tag} {kind} eps={eps}")
            for fi, name in enumerate(("ties", "zeros", "oor")):
                kind, eps = KINDS[(fi + di + V + B) % 3]
                x, t = er.family(name, B, V, dtype, g)
                ref = launch(er.strided(x, pad), t, kind, eps, b, f"{name} {tag} {kind} eps={eps}")
                if name != "oor":  # k >= V counts every valid row
                    assert ref["counts"][5] == ref["counts"][6] == B
            x, t = er.family("nan", B, V, dtype, g)
            kind, eps = KINDS[(di + V + B) % 3]
            ref = launch(er.strided(x, pad), t, kind, eps, c, f"nan {tag} {kind} eps={eps}")
            assert ref["counts"][3] == ref["counts"][4] == B - (1 if B == 1 or V == 1 else 2)
            kr.check_guards(tag)


def test_eval_stats_refuses():
    lib = no._load()
    x = torch.zeros((4, 8), dtype=F32, device=DEV)
    t = torch.zeros(4, dtype=I64, device=DEV)
    rows, rank = torch.zeros(4, dtype=F32, device=DEV), torch.zeros(4, dtype=I32, device=DEV)
    loss, counts = torch.zeros(1, dtype=F64, device=DEV), torch.zeros(11, dtype=I64, device=DEV)
    ok = dict(logits=no._p(x), bf16=0, ld=8, target=no._p(t), kind=0, eps=0.0, ks=(1, 3), rows=no._p(rows),
              rank=no._p(rank), loss=no._p(loss), counts=no._p(counts), B=4, V=8)

    def call(**kw):
        a = dict(ok, **kw)
        keep, ptr = _ks(a["ks"])
        if a.get("null_ks"):
            ptr = None
        return lib.pdt_eval_stats(a["logits"], a["bf16"], a["ld"], a["target"], a["kind"], a["eps"], ptr,
                                  len(a["ks"]), a["rows"], a["rank"], a["loss"], a["counts"], a["B"], a["V"], no._s())

    assert call() == 0
    for bad in (dict(logits=None), dict(target=None), dict(rows=None), dict(rank=None), dict(loss=None),
                dict(counts=None), dict(null_ks=True), dict(B=0), dict(B=-1), dict(V=0), dict(ld=7),
                dict(ks=tuple(range(1, 10))), dict(ks=(1, 0)), dict(ks=(-3,)), dict(kind=2)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert counts.tolist()[:4] == [4, 0, 4, 4] and not counts[4:].any()  # only the one good launch ran


def test_wrapper_takes_a_strided_view_and_allocates():
    from pytorch_distributed_template_amd.ops import fused
    g = kr.gen(5, DEV)
    full = kr.normal((9, 1003), g, BF, std=3.0)
    x, t = full[:, 2:1002], torch.randint(0, 1000, (9,), generator=g, device=DEV)  # rows 4-byte aligned only
    loss, counts = fused.eval_stats_new((1, 5), DEV)
    for _ in range(2):
        rows, rank = fused.eval_stats_update(x, t, loss, counts, (1, 5), kind="ce", eps=0.1)
    ref = er.eval_ref(x, t, "ce", float(torch.tensor(0.1, dtype=F32)), (1, 5))
    assert rows.dtype == F32 and rank.dtype == I32 and torch.equal(rank.to(I64), ref["rank"])
    assert torch.equal(counts.cpu(), 2 * ref["counts"])
    assert float(loss) == pytest.approx(2 * float(ref["loss_sum"]), rel=1e-5)


# --------------------------------------------------------------------------- through the Trainer
def _trainer(save_dir, eval_mode, run_id):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (build_criterion_metrics, build_ema, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    cfg = json.loads((ROOT / "config" / "mnist_cpu.json").read_text())
    cfg["trainer"].update(save_dir=str(save_dir), epochs=1, verbosity=1, backend="native", eval_mode=eval_mode,
                          ema={"decay": 0.9, "validate": "both"})
    cfg["train_loader"]["args"]["synthetic_size"] = 512
    cfg["valid_loader"]["args"]["synthetic_size"] = 300
    torch.manual_seed(0)
    device = torch.device("cuda", torch.cuda.current_device())
    config = ConfigParser(cfg, run_id=run_id)
    model = build_model(config, device)
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    return Trainer(model, criterion, metrics, optimizer, config=config, device=device,
                   data_loader=build_loader(config, "train_loader"),
                   valid_data_loader=build_loader(config, "valid_loader"), lr_scheduler=sched,
                   ema=build_ema(config, model))


def test_trainer_stream_equals_gather_on_the_native_lenet(tmp_path):
    from pytorch_distributed_template_amd.ops import fused
    try:
        gt = _trainer(tmp_path, "gather", "g")
        st = _trainer(tmp_path, "stream", "s")
        st.model.load_state_dict(gt.model.state_dict())
        st.ema.module.load_state_dict(gt.ema.module.state_dict())
        with torch.no_grad():  # averaged weights that differ from the trained ones
            for p in gt.ema.module.parameters():
                p.mul_(0.5)
            for p, q in zip(st.ema.module.parameters(), gt.ema.module.parameters()):
                p.copy_(q)
        logs = {}
        for name, tr in (("gather", gt), ("stream", st)):
            logs[name] = dict(tr._valid_epoch(1))
            logs[name].update(tr._valid_epoch(1, model=tr.ema.module, prefix="ema_"))
        print(logs)
        g, s = logs["gather"], logs["stream"]
        assert list(s) == list(g) == ["loss", "accuracy", "top_k_acc", "ema_loss", "ema_accuracy", "ema_top_k_acc"]
        # fp32 log-probabilities of the same weights: argmax == rank 0 whatever the ties
        assert s["accuracy"] == g["accuracy"] and s["ema_accuracy"] == g["ema_accuracy"]
        # the k = 3 count against torch.topk rests on the inputs: no ties among the three largest
        # (nor with the fourth) of any validation row, for either set of weights
        for model in (st.model, st.ema.module):
            model.eval()
            with torch.no_grad():
                top = torch.cat([torch.topk(model(x.to(st.device)), 4, 1).values for x, _ in st.valid_data_loader])
            assert top.shape == (300, 4) and bool((top[:, :-1] > top[:, 1:]).all())
        st.model.train()
        assert s["top_k_acc"] == g["top_k_acc"] and s["ema_top_k_acc"] == g["ema_top_k_acc"]
        assert 0 < s["accuracy"] <= s["top_k_acc"] < 1
        assert s["loss"] == pytest.approx(g["loss"], rel=1e-5) and s["ema_loss"] == pytest.approx(g["ema_loss"], rel=1e-5)
        assert s["ema_loss"] != s["loss"]
        assert st.model.training and not st.ema.module.training
        st._on_epoch_start(1)
        log = st._train_epoch(1)  # an epoch's own two validation passes fill both trackers
        for k in ("val_loss", "val_accuracy", "val_top_k_acc", "val_ema_loss", "val_ema_accuracy",
                  "val_ema_top_k_acc"):
            assert k in log and math.isfinite(log[k]), (k, log)
    finally:
        fused.set_backend("auto")
