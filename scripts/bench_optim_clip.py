"""Step time of the one-launch optimizers with and without on-device gradient-norm clipping, on
the parameter shapes of the two flagship models (no forward / backward: the gradients are filled
once):

    FusedSGD on ResNet-50,  FusedAdamW on ViT-B/16 with clipping off,
    FusedAdamW on ViT-B/16 with max_grad_norm and skip_nonfinite.

HIP events around 100 steps after 20 warm-up steps give the step time as a training loop sees it
(host launch cost included); ``--rounds`` repeats the three cases in turn, which shows the
round-to-round spread. ``--root`` imports the package from another checkout (one without the
options times the first two cases only), so two trees can be timed alternately by one driver:

    python scripts/bench_optim_clip.py [--rounds N] [--root DIR] [--tag NAME]

Each line is ``tag round case us/step``; the table in profiles/optim_clip.txt is made of them.
"""
import argparse
import inspect
import os
import sys

import torch

WARMUP, STEPS = 20, 100


def timed(opt):
    for _ in range(WARMUP):
        opt.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        opt.step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from pytorch_distributed_template_amd import models
    from pytorch_distributed_template_amd.ops import native_ops
    from pytorch_distributed_template_amd.optim import FusedAdamW, FusedSGD
    native_ops.require()
    print(f"{args.tag}: {os.path.dirname(models.__file__)} on {torch.cuda.get_device_name(0)}", flush=True)
    has_clip = "max_grad_norm" in inspect.signature(FusedAdamW.__init__).parameters

    def params_of(model):
        params = [p for p in model.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        return params

    r50 = params_of(models.resnet50(num_classes=1000).cuda().to(memory_format=torch.channels_last))
    vit = params_of(models.vit_b_16(num_classes=1000).cuda())
    cases = [("resnet50_sgd", lambda: FusedSGD(r50, lr=0.1, momentum=0.9, weight_decay=5e-5)),
             ("vit_adamw", lambda: FusedAdamW(vit, lr=1e-3, weight_decay=0.05))]
    if has_clip:
        # (a norm of ~9 against 1.0: the clip is active; the gradients are finite, no step is declined)
        cases.append(("vit_adamw_clip_skip", lambda: FusedAdamW(vit, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0,
                                                                skip_nonfinite=True)))
    opts = [(name, make()) for name, make in cases]
    for rnd in range(args.rounds):
        for name, opt in opts:
            print(f"{args.tag} round {rnd} {name:20s} {timed(opt):8.1f} us/step", flush=True)


if __name__ == "__main__":
    main()
