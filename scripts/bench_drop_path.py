"""What stochastic depth (drop-path) costs on an MI355X.

1. Kernels alone, rows = 1024 x 197, D = 768: the LayerNorm-add forward (pdt_ln_add_fwd against
   pdt_ln_add_dp_fwd) with e4m3 codes and no bf16 output, as the fp8 blocks run it, and the
   LayerNorm backward with e5m2 codes and the bias column sums (pdt_ln_bwd_f8_db against
   pdt_ln_dp_bwd), at a table of p = 0.1 drawn by pdt_drop_path_scales. ROUNDS alternating rounds,
   HIP events around STEPS calls after WARMUP calls (us per call, launch cost included).
2. The training step: ViT-B/16 at batch 1024 (--batch), fp8 and bf16, drop_path_rate 0 against
   0.1, forward + backward + FusedAdamW step, eager, on synthetic images; TRAIN_ROUNDS alternating
   rounds of TRAIN_STEPS timed steps after TRAIN_WARMUP (ms per step by HIP events).

The table is appended to profiles/drop_path.txt (--out):

    python scripts/bench_drop_path.py [--out FILE] [--batch 1024] [--kernels | --train]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_distributed_template_amd import models  # noqa: E402
from pytorch_distributed_template_amd.ops import drop_path as dp  # noqa: E402
from pytorch_distributed_template_amd.ops import fused, native_ops as no  # noqa: E402
from pytorch_distributed_template_amd.optim import FusedAdamW  # noqa: E402

WARMUP, STEPS, ROUNDS = 10, 50, 3
TRAIN_WARMUP, TRAIN_STEPS, TRAIN_ROUNDS = 6, 10, 3
DEV = torch.device("cuda")
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def bench_kernels(lines, B, T=197, D=768):
    lib = no._load()
    rows = B * T
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV).to(BF)  # noqa: E731
    y, r, dy, add = rnd(rows, D), rnd(rows, D), rnd(rows, D), rnd(rows, D)
    w, b = torch.randn(D, generator=g, device=DEV), torch.randn(D, generator=g, device=DEV)
    xs, mean, rstd = torch.empty_like(y), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    q = torch.empty((rows, D), dtype=U8, device=DEV)
    meta = no.quantize_fp8_delayed(y[:4096], None, no.E4M3)[2]
    gmeta = no.quantize_fp8_delayed(y[:4096], None, no.E5M2)[2]
    part = torch.empty(lib.pdt_ln_fwd_f8_blocks(rows) + 1, device=DEV)
    p, inv = dp.branch_constants([0.1])
    state = torch.tensor([0, 0], dtype=torch.int32, device=DEV)
    scale = no.drop_path_scales(state, p.to(DEV), inv.to(DEV), B)[0].contiguous()
    kept = float((scale != 0).float().mean())
    P, S = no._p, no._s
    blocks = lib.pdt_ln_bwd_blocks(rows)
    dx, dyb = torch.empty_like(y), torch.empty_like(y)
    dg, db, bias = torch.empty(D, device=DEV), torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    bpart = torch.empty(2 * blocks * D, device=DEV)
    qpart = torch.empty(blocks + 1, device=DEV)
    cpart = torch.empty(blocks * D + lib.pdt_reduce_rows_work(blocks, D), device=DEV)
    calls = {
        "forward  pdt_ln_add_fwd (codes only)": lambda: no._chk(lib.pdt_ln_add_fwd(
            P(y), P(r), P(xs), P(w), P(b), None, P(mean), P(rstd), rows, D, 1e-6, P(q), P(meta), P(part), P(part[-1:]),
            S()), "fwd"),
        "forward  pdt_ln_add_dp_fwd (codes only)": lambda: no._chk(lib.pdt_ln_add_dp_fwd(
            P(y), P(r), P(xs), P(w), P(b), None, P(mean), P(rstd), rows, D, 1e-6, P(q), P(meta), P(part), P(part[-1:]),
            P(scale), T, S()), "dp fwd"),
        "backward pdt_ln_bwd_f8_db": lambda: no._chk(lib.pdt_ln_bwd_f8_db(
            P(dy), P(xs), P(w), P(mean), P(rstd), P(dx), P(dg), P(db), P(bpart), rows, D, 0, P(add), P(q), P(gmeta),
            P(qpart), P(qpart[-1:]), P(cpart), P(bias), 0, S()), "bwd"),
        "backward pdt_ln_dp_bwd (codes, bias)": lambda: no._chk(lib.pdt_ln_dp_bwd(
            P(dy), P(xs), P(w), P(mean), P(rstd), P(dx), P(dyb), P(dg), P(db), P(bpart), rows, D, 0, P(add), P(scale), T,
            P(q), P(gmeta), P(qpart), P(qpart[-1:]), P(cpart), P(bias), 0, S()), "dp bwd"),
    }
    res = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            res[k].append(timed(c, WARMUP, STEPS) * 1e3)
    lines += [f"1. kernels alone: rows = {B} x {T}, D = {D}, p = 0.1 ({kept:.3f} of the samples kept), {ROUNDS} "
              f"alternating rounds of {STEPS} calls after {WARMUP} (us/call, HIP events)", ""]
    for k, v in res.items():
        lines.append(f"  {k:42s} {min(v):8.1f}-{max(v):8.1f} us   ({', '.join(f'{x:.1f}' for x in v)})")
    lines.append("")


def bench_train(lines, batch):
    fused.set_backend("native")
    lines += [f"2. ViT-B/16 training step (forward, backward, FusedAdamW; eager; synthetic images), batch {batch}: "
              f"{TRAIN_ROUNDS} alternating rounds of {TRAIN_STEPS} steps after {TRAIN_WARMUP} (ms/step, HIP events)", ""]
    x = no.synthetic_images((batch, 3, 224, 224), BF, DEV, seed=1)
    t = torch.randint(0, 1000, (batch,), device=DEV)
    for fp8 in (True, False):
        res = {0.0: [], 0.1: []}
        for _ in range(TRAIN_ROUNDS):
            for rate in res:
                torch.manual_seed(0)
                m = models.vit_b_16(num_classes=1000, fp8=fp8, drop_path_rate=rate).to(DEV).train()
                opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.05)

                def step():
                    opt.zero_grad(set_to_none=True)
                    fused.softmax_cross_entropy(m(x), t).backward()
                    opt.step()

                res[rate].append(timed(step, TRAIN_WARMUP, TRAIN_STEPS))
                print(f"{'fp8' if fp8 else 'bf16'} rate {rate}: {res[rate][-1]:.2f} ms/step", flush=True)
                del m, opt
                torch.cuda.empty_cache()
        for rate, v in res.items():
            lines.append(f"  {'fp8 ' if fp8 else 'bf16'} drop_path_rate {rate:3.1f}  {min(v):7.2f}-{max(v):7.2f} ms/step   "
                         f"({', '.join(f'{x:.2f}' for x in v)})")
    fused.set_backend("auto")
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_path.txt"))
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--kernels", action="store_true", help="part 1 only")
    ap.add_argument("--train", action="store_true", help="part 2 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_drop_path.py measures on the GPU"
    no.require()
    lines = ["stochastic depth (csrc/drop_path.hip, csrc/layernorm.hip DP): scripts/bench_drop_path.py",
             torch.cuda.get_device_name(0), ""]
    if not args.train:
        bench_kernels(lines, args.batch)
    if not args.kernels:
        bench_train(lines, args.batch)
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
