"""What the weight EMA (csrc/ema.hip, optim.ModelEMA) costs on an MI355X.

1. Launch time: the EMA launch over the parameter tensors of ResNet-50 and ViT-B/16, with and
   without bf16 shadows, and the FusedSGD step (momentum, bf16 shadows: 22 bytes per element)
   over the same tensors in the same run. ROUNDS alternating rounds; per round HIP events around
   STEPS calls after WARMUP calls give the time per call as a training loop sees it (host launch
   cost included), and a second pass attributes device time to the entry point
   (ops/native_ops.OpTimer). Achieved bytes per second = elements x bytes per element (12 for the
   EMA, 14 with the shadow, 22 for the SGD step) over the device time.
2. End to end: ResNet-50 bf16 through Trainer at batch 256 on the synthetic loader, with and
   without trainer.ema, alternately: TRAIN_STEPS timed steps after a warm-up epoch, steps/s by a
   host clock around the epoch (which ends in a device synchronise).

The table is written to profiles/ema.txt (--out). The launch part wraps every entry point for
its device-time pass, so the training part is measured in a process of its own, which appends:

    python scripts/bench_ema.py [--out FILE]
    python scripts/bench_ema.py --train [--out FILE] [--train-batch 256]
"""
import argparse
import json
import os
import sys
import tempfile
import time

if "--train" not in sys.argv:  # (the training part runs without the timing wrapper: its own process)
    os.environ["PDT_OP_TIMING"] = "1"  # (read when the library is loaded: the per-entry-point pass)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_distributed_template_amd import models  # noqa: E402
from pytorch_distributed_template_amd.ops import native_ops  # noqa: E402
from pytorch_distributed_template_amd.optim import FusedSGD  # noqa: E402
from pytorch_distributed_template_amd.optim import ema as ema_mod  # noqa: E402
from pytorch_distributed_template_amd.optim import fused as fused_mod  # noqa: E402

WARMUP, STEPS, BREAKDOWN_STEPS, ROUNDS = 20, 100, 20, 3
TRAIN_STEPS, TRAIN_ROUNDS = 20, 3


def timed(call):
    """(us per call over STEPS by HIP events, device us per call summed over the entry points)"""
    for _ in range(WARMUP):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        call()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) / STEPS * 1e3
    lib = native_ops._load()
    lib.records.clear()
    lib.enabled = True
    for _ in range(BREAKDOWN_STEPS):
        call()
    lib.enabled = False
    dev_us = sum(ms for ms, _calls, _name, _key in lib.summary(top=1000)) * 1e3 / BREAKDOWN_STEPS
    lib.records.clear()
    return us, dev_us


def ema_call(params, shadows):
    es = [p.detach().clone(memory_format=torch.preserve_format) for p in params]
    ps = [p.detach() for p in params]
    sh = [torch.empty_like(e, dtype=torch.bfloat16, memory_format=torch.preserve_format) for e in es] \
        if shadows else None
    plan = fused_mod._Plan(es, es[0].device)
    dev = torch.tensor([0.0, 0.9999, 0.0001], dtype=torch.float32, device=es[0].device)
    return lambda: ema_mod.multi_tensor_ema_(plan, es, ps, sh, dev, 0.9999, True)


def bench_launch(lines):
    lines += [f"1. launch time: {ROUNDS} alternating rounds, {STEPS} calls after {WARMUP} warm-up, HIP events "
              f"(us/call); device us per call from {BREAKDOWN_STEPS} further calls", ""]
    cases = [("ResNet-50", lambda: models.resnet50(num_classes=1000).cuda().to(memory_format=torch.channels_last)),
             ("ViT-B/16", lambda: models.vit_b_16(num_classes=1000).cuda())]
    ok = True
    for model_name, make_model in cases:
        model = make_model()
        params = [p for p in model.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        n = sum(p.numel() for p in params)
        lines.append(f"{model_name}: {len(params)} tensors, {n / 1e6:.1f} M elements")
        sgd = FusedSGD(params, lr=1e-4, momentum=0.9, weight_decay=5e-5)
        calls = [("FusedSGD step", sgd.step, 22), ("EMA", ema_call(params, False), 12),
                 ("EMA + bf16 shadow", ema_call(params, True), 14)]
        res = {name: [] for name, _, _ in calls}
        for _ in range(ROUNDS):
            for name, call, _ in calls:
                res[name].append(timed(call))
        for name, _, bpe in calls:
            us = [r[0] for r in res[name]]
            dv = [r[1] for r in res[name]]
            lines.append(f"  {name:18s} {min(us):7.1f}-{max(us):7.1f} us/call   device {min(dv):7.1f}-{max(dv):7.1f} us "
                         f"({n * bpe / (min(dv) * 1e-6) / 1e12:4.2f} TB/s at {bpe} B/element, best round)")
        for name in ("EMA", "EMA + bf16 shadow"):
            worse = max(r[1] for r in res[name]) > min(r[1] for r in res["FusedSGD step"])
            ok = ok and not worse
            lines.append(f"  {name}: slowest round's device time "
                         f"{'ABOVE' if worse else 'no longer than'} the SGD step's fastest")
        lines.append("")
        del model, params, sgd, calls
        torch.cuda.empty_cache()
    return ok


def bench_train(lines, batch):
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.ops import fused
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_ema,
                                                          build_loader, build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    lines += [f"2. ResNet-50 bf16 native through Trainer (eager steps), batch {batch}, synthetic loader: "
              f"{TRAIN_STEPS} timed steps after a warm-up epoch, {TRAIN_ROUNDS} alternating rounds", ""]
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(os.path.join(ROOT, "config", "resnet50_bf16.json")) as f:
        base = json.load(f)
    base["train_loader"]["args"].update(batch_size=batch)
    save = tempfile.mkdtemp(prefix="pdt_bench_ema_")
    res = {"without trainer.ema": [], "with trainer.ema": []}
    for run in range(TRAIN_ROUNDS):
        for name in res:
            cfg = json.loads(json.dumps(base))
            cfg["trainer"].update(save_dir=save, verbosity=0)
            if name.startswith("with "):
                cfg["trainer"]["ema"] = {"decay": 0.9999, "warmup": True}
            config = ConfigParser(cfg, run_id=f"r{run}{len(name)}")
            model = build_model(config, dev)
            criterion, metrics = build_criterion_metrics(config)
            optimizer, sched = build_optimizer(config, model)
            ema = build_ema(config, model)
            tr = Trainer(model, criterion, metrics, optimizer, config=config, device=dev,
                         data_loader=build_loader(config, "train_loader"), valid_data_loader=None,
                         lr_scheduler=sched, len_epoch=6, autocast_dtype=autocast_dtype(config, dev),
                         channels_last=True, ema=ema)
            tr._train_epoch(1)  # warm-up: kernel variant choices, allocator, the EMA's tables
            tr.len_epoch = TRAIN_STEPS
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            log = tr._train_epoch(2)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res[name].append(TRAIN_STEPS / dt)
            print(f"round {run} {name:20s}: {TRAIN_STEPS / dt:.3f} steps/s  loss {log['loss']:.3f}", flush=True)
            del tr, model, optimizer, ema
            torch.cuda.empty_cache()
    fused.set_backend("auto")
    for name, v in res.items():
        lines.append(f"  {name:20s} {min(v):6.2f}-{max(v):6.2f} steps/s   ({', '.join(f'{x:.2f}' for x in v)})")
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema.txt"))
    ap.add_argument("--train", action="store_true", help="the training part; appends to --out")
    ap.add_argument("--train-batch", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ema.py measures on the GPU"
    native_ops.require()
    lines, ok = [], True
    if not args.train:
        lines += ["weight EMA (csrc/ema.hip, optim.ModelEMA): scripts/bench_ema.py", torch.cuda.get_device_name(0), ""]
        ok = bench_launch(lines)
    else:
        bench_train(lines, args.train_batch)
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.train else "w") as f:
        f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
