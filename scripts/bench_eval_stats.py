"""What streaming validation (csrc/eval_stats.hip, trainer.eval_mode "stream") costs on an MI355X.

1. Call time of ``pdt_eval_stats`` (the row pass and the one-workgroup reduce) at V = 1000,
   B = 256 / 1024 / 2048, bf16 and fp32, next to what gather mode runs on the same tensors --
   ``pdt_xent_fwd`` + ``torch.argmax`` + ``torch.topk(5)`` -- and next to the byte floor of one read
   of the logits. ROUNDS alternating rounds; HIP events around STEPS back-to-back calls after
   WARMUP calls (the time per call as a validation loop sees it, host launch cost included).
2. One validation pass of ResNet-50 bf16 through ``Trainer._valid_epoch`` on the synthetic loader's
   validation batches, in a process of its own per measurement (``--validate MODE``): wall time by a
   host clock around passes that end in a device synchronise, and the peak allocation
   (``torch.cuda.max_memory_allocated``) of a pass over what was allocated before it. Each process
   appends one JSON line to ``--jsonl``; ``--summarise`` turns the lines into the table and checks
   that stream mode is not slower than gather mode beyond the spread of the rounds: each process is
   one round and counts with its fastest pass; the spread is the larger of the two modes' ranges of
   those per-round figures; stream fails if its median round is slower than gather's median round
   by more than that spread.

   Gather mode on the PARENT commit (the one before ``trainer.eval_mode`` existed): check that
   commit out into a directory of its own (``git worktree add DIR <commit>``), copy this script to
   ``DIR/scripts/`` and run ``--validate gather`` there with ``PDT_LIB_PATH`` naming this tree's
   ``libpdt_hip.so`` -- the gather path's kernels did not change, and the parent binds only the
   entry points its own header declares. The script then imports the parent's package (ROOT is
   taken from the script's place); a Trainer without ``eval_mode`` counts as gather. Alternate that
   command with ``--validate stream`` here, three times, all appending to one ``--jsonl``.

    python scripts/bench_eval_stats.py [--out FILE]
    python scripts/bench_eval_stats.py --validate stream|gather --label NAME --jsonl FILE
    python scripts/bench_eval_stats.py --summarise --jsonl FILE [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, STEPS, ROUNDS = 20, 200, 3
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12  # bytes/s: specified, and what a streaming copy reaches
VAL_PASSES = 3


def device_line():
    """The device as the runtime reports it (the marketing name can be generic: the architecture,
    the compute units and the memory identify an MI355X -- gfx950, 256 CUs, 288 GB)."""
    p = torch.cuda.get_device_properties(0)
    return (f"device: {p.name}, {getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs, "
            f"{p.total_memory / 2 ** 30:.0f} GiB")


def per_call_us(call):
    for _ in range(WARMUP):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3


def bench_kernel(lines):
    from pytorch_distributed_template_amd.ops import fused, native_ops
    native_ops.require()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines += [f"1. call time at V = 1000: {ROUNDS} alternating rounds, {STEPS} calls after {WARMUP} warm-up, HIP "
              "events (us/call, fastest-slowest round); eps = 0.1, k = (1, 3, 5)", ""]
    ks = (1, 3, 5)
    for dtype in (torch.bfloat16, torch.float32):
        for B in (256, 1024, 2048):
            g = torch.Generator(device=dev).manual_seed(B)
            x = (torch.randn((B, 1000), generator=g, device=dev) * 3).to(dtype)
            t = torch.randint(0, 1000, (B,), generator=g, device=dev)
            loss, counts = fused.eval_stats_new(ks, dev)
            rows = torch.empty(B, dtype=torch.float32, device=dev)
            rank = torch.empty(B, dtype=torch.int32, device=dev)

            def stream():
                native_ops.eval_stats(x, t, ks, loss, counts, kind="ce", eps=0.1, loss_rows=rows, rank=rank)

            def gather():
                with torch.no_grad():
                    native_ops.softmax_cross_entropy(x, t, 0.1)
                    torch.argmax(x, 1)
                    torch.topk(x, 5, 1)

            res = {"stream": [], "gather": []}
            for _ in range(ROUNDS):
                for name, call in (("stream", stream), ("gather", gather)):
                    res[name].append(per_call_us(call))
            nbytes = x.numel() * x.element_size()
            lines.append(f"  {str(dtype)[6:]:8s} B={B:5d}  pdt_eval_stats {min(res['stream']):6.1f}-{max(res['stream']):6.1f}"
                         f"   xent_fwd+argmax+topk {min(res['gather']):6.1f}-{max(res['gather']):6.1f}"
                         f"   one read of {nbytes / 1e6:5.2f} MB: {nbytes / HBM_PEAK * 1e6:5.2f} us at 8.0 TB/s, "
                         f"{nbytes / HBM_COPY * 1e6:5.2f} us at 6.3 TB/s")
    lines.append("")


def validate(mode, label, jsonl, samples):
    """One process: ResNet-50 bf16 native, validation passes of ``samples`` synthetic images at batch 256."""
    from pytorch_distributed_template_amd.config import ConfigParser
    from pytorch_distributed_template_amd.runtime import (autocast_dtype, build_criterion_metrics, build_loader,
                                                          build_model, build_optimizer)
    from pytorch_distributed_template_amd.trainer import Trainer
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(os.path.join(ROOT, "config", "resnet50_bf16.json")) as f:
        cfg = json.load(f)
    cfg["trainer"].update(save_dir=tempfile.mkdtemp(prefix="pdt_bench_eval_"), verbosity=0)
    if mode == "stream":
        cfg["trainer"]["eval_mode"] = "stream"
    cfg["train_loader"]["args"].update(num_samples=512)
    cfg["valid_loader"]["args"].update(num_samples=samples)
    torch.manual_seed(0)
    config = ConfigParser(cfg, run_id=label)
    model = build_model(config, dev)
    criterion, metrics = build_criterion_metrics(config)
    optimizer, sched = build_optimizer(config, model)
    tr = Trainer(model, criterion, metrics, optimizer, config=config, device=dev,
                 data_loader=build_loader(config, "train_loader"),
                 valid_data_loader=build_loader(config, "valid_loader"), lr_scheduler=sched,
                 autocast_dtype=autocast_dtype(config, dev), channels_last=True)
    assert getattr(tr, "eval_mode", "gather") == mode
    log = tr._valid_epoch(1)  # warm-up: kernel variant choices, the allocator
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    secs = []
    for _ in range(VAL_PASSES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = tr._valid_epoch(1)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    rec = dict(label=label, mode=mode, samples=samples, seconds=secs, allocated_before_mb=before / 2 ** 20,
               peak_mb=torch.cuda.max_memory_allocated() / 2 ** 20, log=log)
    print(json.dumps(rec), flush=True)
    with open(jsonl, "a") as f:
        f.write(json.dumps(rec) + "\n")


def summarise(jsonl, lines):
    recs = [json.loads(ln) for ln in open(jsonl) if ln.strip()]
    labels = []
    for r in recs:
        if r["label"] not in labels:
            labels.append(r["label"])
    lines += [f"2. one validation pass, ResNet-50 bf16 native through Trainer._valid_epoch, {recs[0]['samples']} "
              f"synthetic images at batch 256, one GPU: {VAL_PASSES} timed passes per process after a warm-up pass, "
              "processes alternating", ""]
    rounds = {}  # label -> the fastest pass of each of its processes
    for lb in labels:
        mine = [r for r in recs if r["label"] == lb]
        secs = [s for r in mine for s in r["seconds"]]
        rounds[lb] = [min(r["seconds"]) for r in mine]
        per = ", ".join(f"{s:.3f}" for s in rounds[lb])
        lines.append(f"  {lb:28s} {min(secs):.3f}-{max(secs):.3f} s/pass over all passes; fastest per round: {per}")
        lines.append(f"  {'':28s} torch.cuda.max_memory_allocated over the passes {max(r['peak_mb'] for r in mine):.1f} MB, "
                     f"{max(r['peak_mb'] - r['allocated_before_mb'] for r in mine):.1f} MB above the "
                     f"{mine[0]['allocated_before_mb']:.1f} MB allocated before them")
        lines.append(f"  {'':28s} { {k: round(v, 6) for k, v in mine[-1]['log'].items()} }")
    ok = True
    median = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    stream = [lb for lb in labels if any(r["mode"] == "stream" for r in recs if r["label"] == lb)]
    for s in stream:
        for o in labels:
            if o not in stream:
                spread = max(max(rounds[s]) - min(rounds[s]), max(rounds[o]) - min(rounds[o]))
                diff = median(rounds[s]) - median(rounds[o])
                worse = diff > spread
                ok = ok and not worse
                lines.append(f"  {s} against {o}: median round {median(rounds[s]):.3f} s against {median(rounds[o]):.3f} s "
                             f"({diff:+.3f} s), spread of the rounds {spread:.3f} s: stream is "
                             f"{'SLOWER beyond the spread' if worse else 'not slower beyond the spread'}")
    lines.append("")
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_stream.txt"))
    ap.add_argument("--validate", choices=["stream", "gather"])
    ap.add_argument("--label", default=None)
    ap.add_argument("--jsonl", default=os.path.join(tempfile.gettempdir(), "pdt_eval_stream.jsonl"))
    ap.add_argument("--samples", type=int, default=10240)
    ap.add_argument("--summarise", action="store_true")
    args = ap.parse_args()
    lines, ok, mode = [], True, "a"
    if args.summarise:
        ok = summarise(args.jsonl, lines)
    else:
        assert torch.cuda.is_available(), "bench_eval_stats.py measures on the GPU"
        if args.validate:
            validate(args.validate, args.label or args.validate, args.jsonl, args.samples)
            return 0
        lines += ["streaming validation (csrc/eval_stats.hip, trainer.eval_mode): scripts/bench_eval_stats.py",
                  device_line(), ""]
        bench_kernel(lines)
        mode = "w"
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, mode) as f:
        f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
