"""Time csrc/layernorm_rows.hip (pdt_lnr_fwd, pdt_lnr_bwd) against the stock F.layer_norm forward
and backward on the same tensors (what these widths ran before the kernels existed) and against
the byte floor of the streams, at the ViT-Ti / ViT-S bs1024 shapes and a channels-last D = 96 shape.
Three alternating rounds per shape; each figure is the best round's mean over 20 calls.

    python scripts/bench_ln_rows.py
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

HBM_TBS = 8.0  # MI355X peak HBM bandwidth, TB/s: the byte floor's denominator
lib = no._load()
dev = "cuda"


def timed(fn, calls=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3  # us


for rows, D in ((1024 * 197, 192), (1024 * 197, 384), (256 * 3136, 96)):
    torch.manual_seed(0)
    x = torch.randn(rows, D, device=dev).to(torch.bfloat16)
    dy = torch.randn(rows, D, device=dev).to(torch.bfloat16)
    w, b = torch.rand(D, device=dev) + 0.5, torch.randn(D, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty(2, rows, device=dev)
    blocks = lib.pdt_lnr_bwd_blocks(rows, D)
    part = torch.empty(2 * blocks * D, device=dev)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    xs = x.clone().requires_grad_(True)
    # (the stock op takes no fp32 affine parameters with a bf16 input: it gets bf16 copies, its
    # fastest form -- under autocast it would run in fp32 behind a cast of x)
    ws, bs = w.to(torch.bfloat16).requires_grad_(True), b.to(torch.bfloat16).requires_grad_(True)
    ys = F.layer_norm(xs, (D,), ws, bs, 1e-6)

    def fwd():
        return lib.pdt_lnr_fwd(no._p(x), no._p(w), no._p(b), no._p(y), no._p(stats[0]), no._p(stats[1]), rows, D, 1e-6,
                               no._s())

    def bwd():
        return lib.pdt_lnr_bwd(no._p(dy), no._p(x), no._p(w), no._p(stats[0]), no._p(stats[1]), no._p(dx), None,
                               no._p(dg), no._p(db), no._p(part), rows, D, 0, None, None, 1, no._s())

    arms = {"fwd": fwd, "bwd": bwd, "stock fwd": lambda: F.layer_norm(xs, (D,), ws, bs, 1e-6),
            "stock bwd": lambda: torch.autograd.grad(ys, (xs, ws, bs), dy, retain_graph=True)}
    assert fwd() == 0 and bwd() == 0
    gs = arms["stock bwd"]()
    torch.cuda.synchronize()
    e_y = ((y.float() - ys.float()).norm() / ys.float().norm()).item()
    e_dx = ((dx.float() - gs[0].float()).norm() / gs[0].float().norm()).item()
    e_dg = ((dg - gs[1].float()).norm() / gs[1].float().norm()).item()
    best = {k: 1e30 for k in arms}
    for k, fn in arms.items():  # warm-up of every arm at this shape
        timed(fn, 5)
    for _ in range(3):  # alternating rounds
        for k, fn in arms.items():
            best[k] = min(best[k], timed(fn))
    floor = {"fwd": rows * D * 4 / (HBM_TBS * 1e6), "bwd": rows * D * 6 / (HBM_TBS * 1e6)}  # us; bf16 streams
    print(f"{rows}x{D} blocks={blocks}: " + "  ".join(
        f"{k} {best[k]:7.1f} us (stock {best['stock ' + k]:7.1f} us, x{best['stock ' + k] / best[k]:.2f}; "
        f"byte floor {floor[k]:6.1f} us = {100 * floor[k] / best[k]:.0f}%)" for k in ("fwd", "bwd"))
        + f"  rel err vs stock y {e_y:.1e} dx {e_dx:.1e} dg {e_dg:.1e}", flush=True)
