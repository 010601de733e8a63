"""Streaming validation without a GPU: the float64 reference of tests/eval_ref.py against PyTorch
and against seeded faults, the torch path of ``ops.fused.eval_stats_update`` against that
reference, and ``trainer.eval_mode: "stream"`` through the Trainer, test.py and 4 gloo ranks."""
import argparse
import importlib.util
import json
import math
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import eval_ref as er
import kernel_ref as kr
from test_dist_gloo import _init, _run

from pytorch_distributed_template_amd.ops import fused

ROOT = Path(__file__).resolve().parents[1]
CPU = torch.device("cpu")
F32, BF = torch.float32, torch.bfloat16


def gen(seed):
    return kr.gen(seed, CPU)


# ------------------------------------------------------------------ the reference's own checks
def _family_rows(B=12, V=65):
    """The NaN-free families with targets in range, rows of all of them stacked."""
    xs, ts = zip(*[er.family(n, B, V, F32, gen(7 + i)) for i, n in enumerate(("xent", "ties", "zeros"))])
    return torch.cat(xs), torch.cat(ts)


def check_argmax(ref):
    """rank == 0 iff torch.argmax returns the target (first maximum; -0 == +0)."""
    x, t = _family_rows()
    r = ref(x, t)["rank"]
    hit = torch.argmax(x.double(), 1) == t
    assert 0 < int(hit.sum()) < len(t)
    assert torch.equal(r == 0, hit), (r.tolist(), hit.tolist())


def _tie_free(B=64, V=101):
    g = gen(3)
    x = torch.randn((B, V), generator=g)
    t = torch.randint(0, V, (B,), generator=g)
    # row 0: the maximum sits in the last column and the target is the runner-up
    x[0, V - 1], x[0, 5], t[0] = 9.0, 8.0, 5
    assert all(len(set(row.tolist())) == V for row in x)  # no two equal values in a row
    return x, t


def check_topk(ref):
    """On tie-free rows ``rank < k`` is membership of torch.topk's k indices."""
    x, t = _tie_free()
    r = ref(x, t)["rank"]
    for k in (1, 3, 5, x.shape[1]):
        member = (torch.topk(x.double(), k, 1).indices == t[:, None]).any(1)
        assert torch.equal(r < k, member), k


def check_nan(ref):
    """A row with a NaN has rank V, wherever the NaN is; the clean rows keep theirs."""
    x, t = er.family("nan", 6, 10, F32, gen(5))
    clean = er.family("xent", 6, 10, F32, gen(5))[0]
    r = ref(x, t)["rank"]
    assert r[:2].tolist() == [10, 10]
    assert torch.equal(r[2:], ref(clean, t)["rank"][2:]) and int(r[2:].max()) < 10


def check_loss(ref):
    x, t = _family_rows()
    for eps in (0.0, 0.1):
        want = F.cross_entropy(x.double(), t, label_smoothing=eps, reduction="none")
        torch.testing.assert_close(ref(x, t, kind="ce", eps=eps)["loss_rows"], want, rtol=1e-13, atol=1e-13)
    logp = F.log_softmax(x.double(), 1)
    assert torch.equal(ref(logp, t, kind="nll")["loss_rows"], F.nll_loss(logp, t, reduction="none"))


CHECKS = [check_argmax, check_topk, check_nan, check_loss]


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_reference_agrees_with_pytorch(check):
    check(er.eval_ref)


@pytest.mark.parametrize("fault,check", [("ge", check_argmax), ("ties_after", check_argmax),
                                         ("nan_correct", check_nan), ("drop_last", check_topk)])
def test_seeded_fault_is_caught(fault, check):
    with pytest.raises(AssertionError):
        check(lambda *a, **k: er.eval_ref(*a, fault=fault, **k))


def test_reference_out_of_range_and_counts():
    x, t = er.family("oor", 5, 7, F32, gen(1))
    ref = er.eval_ref(x, t, ks=(1, 7, 9))
    assert ref["rank"][0] == 7 and ref["rank"][4] == 7 and ref["loss_rows"][0] == 0 and ref["loss_rows"][4] == 0
    assert ref["counts"].tolist()[:2] == [5, 2]
    assert ref["counts"][3] == ref["counts"][4] == 3  # k >= V: every valid row, never an invalid one


# ------------------------------------------------------------- torch path of eval_stats_update
KINDS = [("ce", 0.0), ("ce", 0.1), ("nll", 0.0)]


@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1000, 1001])
def test_torch_path_matches_reference(V, B):
    ks = (1, 3, 5, V, V + 7)
    for di, dtype in enumerate((BF, F32)):
        loss_sum, counts = fused.eval_stats_new(ks, CPU)
        want_sum, want_counts = 0.0, torch.zeros(2 + len(ks), dtype=torch.int64)
        for fi, name in enumerate(er.FAMILIES):
            kind, eps = KINDS[(fi + di + V + B) % 3]
            x, t = er.family(name, B, V, dtype, gen(100 * V + B + fi))
            x = er.strided(x, 3 * ((fi + di) % 2))
            if name == "nan":  # (a NaN loss would stay in the accumulator: its own pair)
                acc = fused.eval_stats_new(ks, CPU)
            else:
                acc = (loss_sum, counts)
            rows, rank = fused.eval_stats_update(x, t, *acc, ks, kind=kind, eps=eps)
            ref = er.eval_ref(x, t, kind, eps, ks)
            what = f"{name} V={V} B={B} {dtype} {kind} eps={eps}"
            assert torch.equal(rank.to(torch.int64), ref["rank"]), what
            assert torch.equal(torch.isnan(rows), torch.isnan(ref["loss_rows"])), what
            fin = ~torch.isnan(rows)
            kr.assert_close(rows[fin], ref["loss_rows"][fin], 1e-13 * ref["loss_rows_abs"][fin] + 1e-300, what)
            if name == "nan":
                assert torch.equal(acc[1], ref["counts"]), what
                assert math.isnan(float(acc[0])) == bool(torch.isnan(ref["loss_rows"]).any()), what
            else:
                want_sum += float(rows.double().sum())
                want_counts += ref["counts"]
        assert torch.equal(counts, want_counts), (V, B, dtype)  # launches add up
        assert float(loss_sum) == pytest.approx(want_sum, rel=1e-13, abs=1e-300)


def test_update_argument_checks():
    acc = fused.eval_stats_new((1,), CPU)
    x, t = torch.zeros(2, 3), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="kind"):
        fused.eval_stats_update(x, t, *acc, (1,), kind="mse")
    with pytest.raises(ValueError, match="k >= 1"):
        fused.eval_stats_update(x, t, *acc, (0,))
    with pytest.raises(ValueError, match="at most 8"):
        fused.eval_stats_update(x, t, *fused.eval_stats_new(range(1, 10), CPU), tuple(range(1, 10)))
    with pytest.raises(ValueError, match="expected"):
        fused.eval_stats_update(x[0], t, *acc, (1,))


# --------------------------------------------------------------------------- through the Trainer
def _mnist_cfg(save_dir, eval_mode=None, metrics=None, ema=False):
    cfg = json.loads((ROOT / "config" / "mnist_cpu.json").read_text())
    cfg["trainer"].update(save_dir=str(save_dir), epochs=1, verbosity=1)
    if eval_mode is not None:
        cfg["trainer"]["eval_mode"] = eval_mode
    if ema:
        cfg["trainer"]["ema"] = {"decay": 0.9}
    if metrics is not None:
        cfg["metrics"] = metrics
    cfg["train_loader"]["args"]["synthetic_size"] = 256
    for k in ("valid_loader", "test_loader"):
        cfg[k]["args"]["synthetic_size"] = 300  # batches of 128, 128, 44
    return cfg


def _trainer(cfg, run_id):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (build_criterion_metrics, build_ema, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    torch.manual_seed(0)
    config = ConfigParser(cfg, run_id=run_id)
    model = build_model(config, CPU)
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    return Trainer(model, criterion, metrics, optimizer, config=config, device=CPU,
                   data_loader=build_loader(config, "train_loader"),
                   valid_data_loader=build_loader(config, "valid_loader"), lr_scheduler=sched,
                   ema=build_ema(config, model))


def _epoch(tr):
    tr._on_epoch_start(1)
    return tr._train_epoch(1)


@pytest.fixture(scope="module")
def gathered(tmp_path_factory):
    tr = _trainer(_mnist_cfg(tmp_path_factory.mktemp("gather")), "gather")
    return tr, _epoch(tr)


def test_trainer_streamed_equals_gathered(gathered, tmp_path):
    gt, glog = gathered
    assert gt.eval_mode == "gather"  # the default
    st = _trainer(_mnist_cfg(tmp_path, "stream"), "stream")
    slog = _epoch(st)
    print("gather", glog, "\nstream", slog)
    assert list(slog) == list(glog)  # the same keys in the same order
    for a, b in zip(gt.model.parameters(), st.model.parameters()):
        assert torch.equal(a, b)  # the same seed trained the same weights
    # the property the exact comparison rests on: no ties among the three largest (nor with the
    # fourth) of any validation row -- topk's choice among equals is not specified
    st.model.eval()
    with torch.no_grad():
        top = torch.cat([torch.topk(st.model(x), 4, 1).values for x, _ in st.valid_data_loader])
    st.model.train()
    assert top.shape == (300, 4) and bool((top[:, :-1] > top[:, 1:]).all())
    assert type(slog["val_accuracy"]) is float and slog["val_accuracy"] == glog["val_accuracy"]
    assert slog["val_top_k_acc"] == glog["val_top_k_acc"]
    assert 0 < slog["val_accuracy"] <= slog["val_top_k_acc"] <= 1
    # gather mode sums fp32 batch means (the bound tests/test_row_kernels_gpu.py gives that mean)
    batch = st.valid_data_loader.batch_size
    rel = 2 * (math.ceil(batch / 256) + 10) * kr.U
    assert abs(slog["val_loss"] - glog["val_loss"]) <= rel * abs(glog["val_loss"])
    assert slog["loss"] == glog["loss"]


def _raise_gather(*a, **k):
    raise AssertionError("gather_tensors called in stream mode")


def _load_test_cli():
    spec = importlib.util.spec_from_file_location("pdt_test_cli", ROOT / "test.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stream_mode_never_gathers(gathered, tmp_path, monkeypatch):
    """Fails without the feature: the unknown key is ignored and the gather is reached."""
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.utils import dist as pdist
    _, glog = gathered
    monkeypatch.setattr(pdist, "gather_tensors", _raise_gather)
    cfg = _mnist_cfg(tmp_path, "stream", ema=True)
    tr = _trainer(cfg, "stream")
    log = _epoch(tr)
    assert {"val_loss", "val_accuracy", "val_top_k_acc", "val_ema_loss", "val_ema_accuracy",
            "val_ema_top_k_acc"} <= set(log)
    assert log["val_accuracy"] == glog["val_accuracy"]
    assert log["val_ema_loss"] != log["val_loss"] and math.isfinite(log["val_ema_loss"])
    assert tr.model.training and not tr.ema.module.training
    # test.py on the checkpoint: the test loader is the validation loader's twin
    tr._save_checkpoint(1)
    ck = tr.checkpoint_dir / "checkpoint-epoch1.pth"
    cli = _load_test_cli()
    out = cli.main(argparse.Namespace(ema=False), ConfigParser(cfg, resume=ck, run_id="t", training=False), CPU)
    assert list(out) == ["loss", "accuracy", "top_k_acc"]
    assert out["accuracy"] == log["val_accuracy"] and out["top_k_acc"] == log["val_top_k_acc"]
    assert out["loss"] == pytest.approx(log["val_loss"], rel=1e-12)
    out = cli.main(argparse.Namespace(ema=True), ConfigParser(cfg, resume=ck, run_id="t2", training=False), CPU)
    assert out["loss"] == pytest.approx(log["val_ema_loss"], rel=1e-12)


# ------------------------------------------------------------------------------------ 4 ranks
N_DIST, V_DIST = 61, 10
SHARDS = [0, 5, 6, 33, N_DIST]  # uneven: 5, 1, 27 and 28 rows


def _dist_data():
    g = gen(11)
    return torch.randn((N_DIST, V_DIST), generator=g) * 3, torch.randint(0, V_DIST, (N_DIST,), generator=g)


def _stream_eval():
    from pytorch_distributed_template_amd.models import loss as L, metric as M
    from pytorch_distributed_template_amd.trainer.streaming import StreamingEval
    return StreamingEval(L.label_smoothing_cross_entropy, [M.accuracy, M.top_k_acc, M.top5_acc], CPU)


def _w_stream(rank, world, port, q):
    try:
        pdist = _init(rank, world, port)
        x, t = _dist_data()
        ev = _stream_eval()
        for i in range(SHARDS[rank], SHARDS[rank + 1], 4):
            j = min(i + 4, SHARDS[rank + 1])
            ev.update(x[i:j], t[i:j])
        q.put((rank, ev.result("ema_")))
        pdist.cleanup()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))


def test_four_gloo_ranks_uneven_shards():
    res = _run(_w_stream, 4)
    x, t = _dist_data()
    ev = _stream_eval()
    ev.update(x, t)
    one = ev.result("ema_")
    assert list(one) == ["ema_loss", "ema_accuracy", "ema_top_k_acc", "ema_top5_acc"]
    assert one["ema_accuracy"] == (torch.argmax(x, 1) == t).sum().item() / N_DIST
    for r in range(4):
        assert list(res[r]) == list(one)
        for k in ("ema_accuracy", "ema_top_k_acc", "ema_top5_acc"):
            assert res[r][k] == one[k], (r, k)
        # float64 sums of the same 61 rows in another order
        assert abs(res[r]["ema_loss"] - one["ema_loss"]) <= N_DIST * 2.0 ** -52 * abs(one["ema_loss"])
        assert res[r] == res[0]


# -------------------------------------------------------------------- arguments and configs
def mean_rank(output, target):
    return 0.0


def test_metric_without_count_form_raises_and_names_it(tmp_path):
    from pytorch_distributed_template_amd.models import loss as L, metric as M
    from pytorch_distributed_template_amd.trainer.streaming import StreamingEval
    with pytest.raises(ValueError, match="mean_rank"):
        StreamingEval(L.nll_loss, [M.accuracy, mean_rank], CPU)
    with pytest.raises(ValueError, match="mean_rank"):
        StreamingEval(mean_rank, [M.accuracy], CPU)
    # a loss bound to another smoothing is not the registry's function: refused, not scored at 0.1
    import functools
    bound = functools.partial(L.label_smoothing_cross_entropy, smoothing=0.2)
    with pytest.raises(ValueError, match="no row-wise form"):
        StreamingEval(bound, [M.accuracy], CPU)
    with pytest.raises(ValueError, match="label_smoothing_cross_entropy"):
        StreamingEval(functools.wraps(L.label_smoothing_cross_entropy)(bound), [M.accuracy], CPU)
    from pytorch_distributed_template_amd.models import metric
    orig = metric.__dict__.get("mean_rank")
    metric.mean_rank = mean_rank
    try:
        with pytest.raises(ValueError, match="mean_rank"):
            _trainer(_mnist_cfg(tmp_path, "stream", metrics=["accuracy", "mean_rank"]), "bad")
        tr = _trainer(_mnist_cfg(tmp_path, "gather", metrics=["accuracy", "mean_rank"]), "fine")
        assert tr.eval_mode == "gather"
    finally:
        if orig is None:
            del metric.mean_rank


def test_unknown_eval_mode_raises(tmp_path):
    with pytest.raises(ValueError, match="eval_mode.*'streamed'"):
        _trainer(_mnist_cfg(tmp_path, "streamed"), "bad")


def test_out_of_range_target_raises_at_the_end_of_the_pass():
    ev = _stream_eval()
    x, t = _dist_data()
    t[17] = V_DIST
    ev.update(x[:16], t[:16])
    ev.update(x[16:], t[16:])  # no raise here: nothing is read back per batch
    with pytest.raises(ValueError, match="1 of 61 target"):
        ev.result()
    ev.reset()
    ev.update(x[:16], t[:16])
    assert ev.result()["accuracy"] == (torch.argmax(x[:16], 1) == t[:16]).sum().item() / 16


def test_mixed_target_raises():
    from pytorch_distributed_template_amd.data import MixedTarget
    ev = _stream_eval()
    x, t = _dist_data()
    with pytest.raises(ValueError, match="MixedTarget"):
        ev.update(x, MixedTarget(t, t, torch.ones(N_DIST)))


def test_registry_tables_and_top5():
    from pytorch_distributed_template_amd.models import loss as L, metric as M
    assert M.COUNT_FORMS == {"accuracy": 1, "top_k_acc": 3, "top5_acc": 5}
    assert L.EVAL_FORMS == {"cross_entropy": ("ce", 0.0), "label_smoothing_cross_entropy": ("ce", 0.1),
                            "nll_loss": ("nll", 0.0)}
    assert all(callable(getattr(M, n)) for n in M.COUNT_FORMS) and all(callable(getattr(L, n)) for n in L.EVAL_FORMS)
    x, t = _tie_free()
    assert M.top5_acc(x, t) == M.top_k_acc(x, t, 5) != M.top_k_acc(x, t)


def test_stream_config_parses(tmp_path):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import build_criterion_metrics
    from pytorch_distributed_template_amd.trainer.streaming import StreamingEval, eval_mode
    cfg = json.loads((ROOT / "config" / "resnet50_bf16_packed_stream.json").read_text())
    base = json.loads((ROOT / "config" / "resnet50_bf16_packed.json").read_text())
    assert cfg["trainer"].pop("eval_mode") == "stream" and cfg["metrics"].pop() == "top5_acc"
    assert cfg.pop("name") != base.pop("name") and cfg == base  # the packed config plus the two
    cfg = json.loads((ROOT / "config" / "resnet50_bf16_packed_stream.json").read_text())
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="p")
    assert eval_mode(config) == "stream"
    ev = StreamingEval(*build_criterion_metrics(config), CPU)
    assert (ev.kind, ev.eps, ev.ks) == ("ce", 0.1, (1, 3, 5))
