"""Step time of the layer-wise optimizers against their plain counterparts, on the parameter
shapes of the two flagship models (no forward / backward: the gradients are filled once):

    FusedSGD vs FusedLARS on ResNet-50,  FusedAdamW vs FusedLAMB on ViT-B/16,
    the layer-wise ones with max_grad_norm off and on.

HIP events around 100 steps after 20 warm-up steps give the step time as a training loop sees
it (host launch cost included); a second pass attributes device time to each kernel entry
point (ops/native_ops.OpTimer), which names the kernel responsible for a ratio. The table is
written to profiles/optim_layerwise.txt (--out).

    python scripts/bench_optim_layerwise.py [--out FILE]
"""
import argparse
import os
import sys

os.environ["PDT_OP_TIMING"] = "1"  # (read when the library is loaded: the per-entry-point pass)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_distributed_template_amd import models  # noqa: E402
from pytorch_distributed_template_amd.ops import native_ops  # noqa: E402
from pytorch_distributed_template_amd.optim import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD  # noqa: E402

WARMUP, STEPS, BREAKDOWN_STEPS = 20, 100, 20


def timed(opt):
    """(us per step over STEPS, {entry point: device us per step})"""
    for _ in range(WARMUP):
        opt.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        opt.step()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) / STEPS * 1e3
    lib = native_ops._load()
    lib.records.clear()
    lib.enabled = True
    for _ in range(BREAKDOWN_STEPS):
        opt.step()
    lib.enabled = False
    parts = {}
    for ms, _calls, name, _key in lib.summary(top=1000):
        parts[name] = parts.get(name, 0.0) + ms * 1e3 / BREAKDOWN_STEPS
    lib.records.clear()
    return us, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_layerwise.txt"))
    args = ap.parse_args()
    native_ops.require()
    lines = [f"optimizer step, {STEPS} steps after {WARMUP} warm-up, HIP events; device us per entry point from "
             f"{BREAKDOWN_STEPS} further steps", torch.cuda.get_device_name(0), ""]
    cases = [
        ("ResNet-50", lambda: models.resnet50(num_classes=1000).cuda().to(memory_format=torch.channels_last),
         ("FusedSGD", lambda ps: FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=5e-5), 22),
         [("FusedLARS", lambda ps: FusedLARS(ps, lr=0.1, momentum=0.9, weight_decay=5e-5), 30),
          ("FusedLARS clip", lambda ps: FusedLARS(ps, lr=0.1, momentum=0.9, weight_decay=5e-5, max_grad_norm=1.0),
           30)]),
        ("ViT-B/16", lambda: models.vit_b_16(num_classes=1000).cuda(),
         ("FusedAdamW", lambda ps: FusedAdamW(ps, lr=1e-3, weight_decay=0.05), 30),
         [("FusedLAMB", lambda ps: FusedLAMB(ps, lr=1e-3, weight_decay=0.01), 46),
          ("FusedLAMB clip", lambda ps: FusedLAMB(ps, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0), 50)]),
    ]
    for model_name, make_model, base, others in cases:
        model = make_model()
        params = [p for p in model.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        n = sum(p.numel() for p in params)
        lines.append(f"{model_name}: {len(params)} tensors, {n / 1e6:.1f} M elements")
        base_us = None
        for name, make, bytes_per_el in [base] + others:
            us, parts = timed(make(params))
            base_us = us if base_us is None else base_us
            dev_us = sum(parts.values())
            lines.append(f"  {name:15s} {us:8.1f} us/step  x{us / base_us:4.2f}   device {dev_us:8.1f} us "
                         f"({n * bytes_per_el / (dev_us * 1e-6) / 1e9:5.0f} GB/s at {bytes_per_el} B/element)")
            for k, v in sorted(parts.items(), key=lambda kv: -kv[1]):
                lines.append(f"      {k:22s} {v:8.1f} us")
        lines.append("")
        del model, params
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
