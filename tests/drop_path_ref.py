"""Float64 references for stochastic depth (drop-path), built on ``kernel_ref.ln_fwd_ref`` /
``ln_bwd_ref``, the expected scale tables from the package's torch mirror of the draw
(``ops/drop_path.py``), and the tiny ViT the model tests share."""
import copy

import torch

import kernel_ref as kr
from pytorch_distributed_template_amd.models.vit import VisionTransformer
from pytorch_distributed_template_amd.ops import drop_path as dp

F64 = torch.float64
TINY = dict(image_size=32, patch_size=16, num_classes=10, embed_dim=256, depth=3, num_heads=4)  # T = 5
TINY_B = 4
MASKS = ("all_kept", "all_dropped", "alternating", "last_dropped")


def expected_table(seed, step, p, batch, rank=0, n_branches=None):
    """The mirror's table for one rate ``p`` on every branch (or a list of per-branch rates)."""
    ps = [p] * n_branches if n_branches is not None else list(p)
    pt = torch.tensor(ps, dtype=F64)
    return dp.drop_path_table(seed, step, pt.to(torch.float32), (1.0 / (1.0 - pt)).to(torch.float32), batch, rank)


def mask_scale(kind, B, inv_keep=2.0, device=None):
    """One table row [B] (fp32) of a named mask: kept samples carry ``inv_keep``."""
    keep = {"all_kept": [True] * B, "all_dropped": [False] * B, "alternating": [b % 2 == 0 for b in range(B)],
            "last_dropped": [b != B - 1 for b in range(B)]}[kind]
    return torch.tensor([inv_keep if k else 0.0 for k in keep], dtype=torch.float32, device=device)


def row_scale(scale, rows_per_sample):
    """[B] -> [B * rows_per_sample, 1] float64: the scale of every row."""
    return kr.f64(scale).repeat_interleave(rows_per_sample)[:, None]


def xsum_ref(y, r, scale, rows_per_sample):
    """(r + scale[row // rps] * y in float64 -- r itself where the scale is 0, whatever y holds --
    and the sum of the terms' magnitudes)."""
    s = row_scale(scale, rows_per_sample)
    y64, r64 = kr.f64(y), kr.f64(r)
    kept = s != 0
    yk = torch.where(kept, y64, torch.zeros_like(y64))
    return r64 + s * yk, r64.abs() + (s * yk).abs()


def ln_add_dp_fwd_ref(y, r, scale, rows_per_sample, g, b, eps):
    """dict(xsum, xsum_abs) + ``kr.ln_fwd_ref`` of the bf16-rounded sum (what the kernel normalises)."""
    xs, xs_abs = xsum_ref(y, r, scale, rows_per_sample)
    out = kr.ln_fwd_ref(xs.to(torch.float32).to(torch.bfloat16), g, b, eps)
    out.update(xsum=xs, xsum_abs=xs_abs)
    return out


def ln_dp_bwd_ref(dy, x, g, mean, rstd, scale, rows_per_sample, addend=None):
    """``kr.ln_bwd_ref`` + ``dyb`` = scale[row // rps] * bf16(dx), 0 on dropped rows."""
    out = kr.ln_bwd_ref(dy, x, g, mean, rstd, addend)
    s = row_scale(scale, rows_per_sample)
    out["dyb"] = s * kr.f64(out["dx"].to(torch.float32).to(torch.bfloat16))
    return out


# ----------------------------------------------------------------------------------- tiny ViT
def tiny_vit(seed=0, **kw):
    torch.manual_seed(seed)
    return VisionTransformer(**{**TINY, **kw})


def tiny_batch(seed=1, B=TINY_B, device=None, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, TINY["image_size"], TINY["image_size"], generator=g)
    t = torch.randint(0, TINY["num_classes"], (B,), generator=g)
    return x.to(device=device, dtype=dtype), t.to(device)


def explicit_table(depth=TINY["depth"], B=TINY_B, rate=0.5, seed=5):
    """A table [2 * depth, B] with both kept and dropped samples on every branch of every block
    with p > 0 (block 0 keeps all, scale 1): drawn once from a torch generator."""
    g = torch.Generator().manual_seed(seed)
    rates = dp.drop_path_rates(rate, depth)
    rows = []
    for i in range(depth):
        for _ in range(2):
            keep = torch.ones(B, dtype=torch.bool)
            if rates[i] > 0:
                while keep.all() or not keep.any():
                    keep = torch.rand(B, generator=g) >= 0.5
            rows.append(torch.where(keep, torch.tensor(1.0 / (1.0 - rates[i])), torch.tensor(0.0)))
    return torch.stack(rows).to(torch.float32)


def vit_f64_ref(model, x, target, table):
    """Loss and parameter gradients (name -> float64 tensor) of ``model``'s weights in float64
    with the scaled residual adds written out here, independently of the model's forward:
    x <- x + table[2i][b] * attn(norm1(x)); x <- x + table[2i+1][b] * mlp(norm2(x))."""
    import torch.nn.functional as F
    m = copy.deepcopy(model).double()
    m.zero_grad(set_to_none=True)
    t64 = table.to(F64)
    x = x.double()
    B = x.shape[0]
    tok = m.patch_embed(x).flatten(2).transpose(1, 2)
    h = torch.cat([m.cls_token.expand(B, -1, -1), tok], dim=1) + m.pos_embed
    for i, blk in enumerate(m.blocks):
        n = blk.norm1(h)
        qkv = blk.attn.qkv(n)
        H, hd = blk.attn.num_heads, blk.attn.head_dim
        q, k, v = qkv.view(B, -1, 3, H, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1) @ v
        a = blk.attn.proj(a.transpose(1, 2).reshape(B, -1, H * hd))
        h = h + t64[2 * i][:, None, None] * a
        n = blk.norm2(h)
        f = blk.mlp.fc2(F.gelu(blk.mlp.fc1(n), approximate="tanh"))
        h = h + t64[2 * i + 1][:, None, None] * f
    logits = m.head(m.norm(h[:, 0]))
    loss = F.cross_entropy(logits, target)
    loss.backward()
    return loss.detach(), {n: p.grad.detach() for n, p in m.named_parameters()}
