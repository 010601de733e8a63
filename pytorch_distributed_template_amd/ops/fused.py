"""Fused op entry points used by the models.

Each function has two implementations:
  * ``native``: hand-written HIP/CDNA4 kernels (``csrc/*.hip``) wrapped in
    ``torch.autograd.Function``s (see ``ops/native_ops/``);
  * ``torch``: plain PyTorch ops -- used on CPU (gloo plumbing tests), as the
    fp32 reference in numerics tests, and as the "stock ROCm stack" baseline
    in ``bench.py --backend torch``.

The backend is chosen per process with :func:`set_backend` (default:
``native`` for GPU tensors when the extension is built, ``torch`` on CPU).
The reference has no fused ops at all -- it runs stock cuDNN/cuBLAS kernels
(SURVEY.md §2.6(a)).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

_BACKEND = os.environ.get("PDT_BACKEND", "auto")  # auto | native | torch


def set_backend(name: str) -> None:
    global _BACKEND
    assert name in ("auto", "native", "torch"), name
    _BACKEND = name


def get_backend() -> str:
    return _BACKEND


def use_native(x: torch.Tensor) -> bool:
    """True when ``x``'s op should run on the native HIP kernels (GPU tensor,
    backend not ``torch``, library present -- ``native`` raises if it is missing)."""
    return _use_native(x)


def _use_native(x: torch.Tensor) -> bool:
    if _BACKEND == "torch" or not x.is_cuda:
        return False
    from . import native_ops  # noqa: WPS433 (lazy: avoids loading the .so on CPU)
    if _BACKEND == "native":
        native_ops.require()
        return True
    return native_ops.available()


# ----------------------------------------------------------------------------
# reference (torch) implementations
# ----------------------------------------------------------------------------
def _torch_conv_bn_act(x, conv: nn.Conv2d, bn: nn.BatchNorm2d, residual=None, relu=True):
    # plain ops; under torch.autocast(bf16) conv runs in bf16 and BN keeps fp32 params
    y = conv(x)
    y = bn(y)
    if residual is not None:
        y = y + residual
    if relu:
        y = F.relu(y)
    return y


def conv_bn_act(x, conv: nn.Conv2d, bn: nn.BatchNorm2d, residual=None, relu: bool = True):
    """y = act(BN(conv(x)) [+ residual]) with training-mode batch statistics."""
    if _use_native(x):
        from . import native_ops
        return native_ops.conv_bn_act(x, conv, bn, residual, relu)
    return _torch_conv_bn_act(x, conv, bn, residual, relu)


def bottleneck(x, blk):
    """ResNet bottleneck block; the native path runs it as one fused autograd node."""
    if _use_native(x):
        from . import native_ops
        out = native_ops.bottleneck(x, blk)
        if out is not None:
            return out
    if blk.downsample is not None:
        identity = conv_bn_act(x, blk.downsample[0], blk.downsample[1], relu=False)
    else:
        identity = x
    out = conv_bn_act(x, blk.conv1, blk.bn1, relu=True)
    out = conv_bn_act(out, blk.conv2, blk.bn2, relu=True)
    return conv_bn_act(out, blk.conv3, blk.bn3, residual=identity, relu=True)


def bottleneck_chain(x, blocks):
    """A sequence of bottleneck blocks. Native: each block's final BN(+res)+ReLU pass is
    folded into the next block's first 1x1 GEMM (``native_ops.bottleneck_chain``)."""
    blocks = list(blocks)
    if _use_native(x):
        from . import native_ops
        x, n = native_ops.bottleneck_chain(x, blocks)
        blocks = blocks[n:]
    for blk in blocks:
        x = bottleneck(x, blk)
    return x


def conv_bn_relu_maxpool(x, conv: nn.Conv2d, bn: nn.BatchNorm2d, kernel_size=3, stride=2, padding=1):
    """max_pool2d(relu(BN(conv(x)))) -- the ResNet stem. Native: one node whose
    max-pool applies the BN affine + ReLU on the fly (no full-resolution activation)."""
    if _use_native(x):
        from . import native_ops
        out = native_ops.stem_pool(x, conv, bn, kernel_size, stride, padding)
        if out is not None:
            return out
    return max_pool2d(conv_bn_act(x, conv, bn, relu=True), kernel_size, stride, padding)


def max_pool2d(x, kernel_size=3, stride=2, padding=1):
    if _use_native(x):
        from . import native_ops
        return native_ops.max_pool2d(x, kernel_size, stride, padding)
    return F.max_pool2d(x, kernel_size, stride, padding)


def global_avg_pool(x):
    """[N,C,H,W] (any memory format) -> [N,C]."""
    if _use_native(x):
        from . import native_ops
        return native_ops.global_avg_pool(x)
    return torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)


def _torch_linear(x, fc: nn.Linear, act=None):
    if x.dtype != fc.weight.dtype and not torch.is_autocast_enabled(x.device.type):
        x = x.to(fc.weight.dtype)
    y = fc(x)
    if act == "gelu":
        y = F.gelu(y, approximate="tanh")
    elif act == "relu":
        y = F.relu(y)
    return y


def linear(x, fc: nn.Linear, act: str | None = None, fp8: bool = False, residual=None):
    """y = act(x @ W^T + b) (+ residual). ``act`` in {None, "gelu", "relu"}; ``fp8`` selects
    the e4m3 GEMM with per-tensor scaling on the native path (ignored on torch path).
    Native: the residual add runs in the GEMM epilogue."""
    if _use_native(x):
        from . import native_ops
        return native_ops.linear(x, fc, act=act, fp8=fp8, residual=residual)
    y = _torch_linear(x, fc, act)
    return y if residual is None else y + residual


def mlp(x, m: nn.Module, fp8: bool = False, residual=None):
    """fc2(gelu_tanh(fc1(x))) (+ residual) of a transformer MLP with ``fc1`` / ``fc2``.
    Native: one autograd node (GELU backward fused into fc2's data-gradient GEMM,
    bias gradients from the weight-gradient kernels, residual in fc2's epilogue)."""
    if _use_native(x):
        from . import native_ops
        return native_ops.mlp(x, m, fp8=fp8, residual=residual)
    y = _torch_linear(_torch_linear(x, m.fc1, "gelu"), m.fc2)
    return y if residual is None else y + residual


def layer_norm(x, ln: nn.LayerNorm):
    if _use_native(x):
        from . import native_ops
        return native_ops.layer_norm(x, ln)
    return ln(x)


def ln_fork(x, ln: nn.LayerNorm, fp8_for: nn.Linear | None = None, grad_fp8_for: nn.Linear | None = None):
    """(x, ln(x)) for a pre-norm residual block. Native: the residual gradient of x
    and the normalised branch's gradient are summed inside LayerNorm's backward;
    ``fp8_for`` (the fp8 layer consuming ln(x)) lets the LayerNorm kernel emit that
    layer's e4m3 input directly, and ``grad_fp8_for`` (the fp8 layer that produced x) its
    e5m2 output gradient in the backward."""
    if _use_native(x):
        from . import native_ops
        return native_ops.ln_fork(x, ln, fp8_for, grad_fp8_for)
    return x, ln(x)


def ln_add_fork(y, r, ln: nn.LayerNorm, fp8_for: nn.Linear | None = None, grad_fp8_for: nn.Linear | None = None,
                scale=None, rows_per_sample: int | None = None):
    """(y + r, ln(y + r)): :func:`ln_fork` with the block's residual add done by the native
    LayerNorm kernel (it reads y and r and writes the sum) instead of the producing GEMM's
    epilogue. ``scale`` (fp32 ``[B]``, one row of :func:`drop_path_scales`' table): stochastic
    depth -- the sum is ``r + scale[b] * y`` for sample ``b``, the leading dimension, each sample
    spanning ``rows_per_sample`` rows (default: all of a sample's rows); a sample whose scale is 0
    takes ``r`` itself."""
    if scale is not None:
        rows = y.numel() // y.shape[-1]
        if rows_per_sample is None:
            rows_per_sample = rows // max(scale.numel(), 1)
        if scale.dim() != 1 or y.shape[0] != scale.numel() or scale.numel() * rows_per_sample != rows:
            raise ValueError(f"ln_add_fork: scale {tuple(scale.shape)} x {rows_per_sample} rows per sample does not "
                             f"cover y {tuple(y.shape)}")
    if _use_native(y):
        from . import native_ops
        if scale is None:
            return native_ops.ln_add_fork(y, r, ln, fp8_for, grad_fp8_for)
        return native_ops.ln_add_fork(y, r, ln, fp8_for, grad_fp8_for, scale, rows_per_sample)
    if scale is None:
        s = y + r
    else:
        from .drop_path import scaled_add
        s = scaled_add(y, r, scale)
    return s, ln(s)


def drop_path_scales(state, p, inv_keep, batch: int, rank: int = 0):
    """Stochastic depth's per-sample branch scales for one training forward: fp32
    ``[len(p), batch]``, entry ``(j, b)`` 0 or ``inv_keep[j]``, a pure function of ``state`` =
    ``[seed, step]`` (int32, on the model's device), the branch and the global sample index
    ``rank * batch + b`` (``ops/drop_path.py``). ``state[1]`` advances by one. Native: one fill
    launch and a one-thread tick on the device, no host sync (a replayed HIP graph advances the
    counter too); torch path: the same table from the torch mirror (reads ``state`` on the host)."""
    if _use_native(state):
        from . import native_ops
        return native_ops.drop_path_scales(state, p, inv_keep, batch, rank)
    from .drop_path import drop_path_table
    seed, step = (int(v) for v in state.tolist())
    table = drop_path_table(seed, step, p, inv_keep, batch, rank, device=state.device)
    with torch.no_grad():
        state[1] = ((step + 1) & 0xFFFFFFFF) - (1 << 32 if (step + 1) & 0x80000000 else 0)
    return table


def attention(q, k, v):
    """softmax(q k^T / sqrt(d)) v for [B,H,T,d] tensors (non-causal)."""
    if _use_native(q):
        from . import native_ops
        return native_ops.attention(q, k, v)
    return F.scaled_dot_product_attention(q, k, v)


def qkv_attention(qkv, num_heads: int, fp8: bool = False, fp8_for: nn.Linear | None = None,
                  grad_fp8_for: nn.Linear | None = None):
    """Multi-head attention on a packed qkv projection [B, T, 3*H*hd] -> [B, T, H*hd].
    Native path: one fused MFMA kernel (hd = 64; ``fp8``: e4m3 score GEMM); torch path: SDPA."""
    B, T, D3 = qkv.shape
    hd = D3 // (3 * num_heads)
    if _use_native(qkv):
        from . import native_ops
        if hd == 64 and qkv.dtype == torch.bfloat16:
            return native_ops.qkv_attention(qkv, num_heads, fp8=fp8, fp8_for=fp8_for, grad_fp8_for=grad_fp8_for)
        native_ops.fallback("qkv_attention", f"head dim {hd}, {qkv.dtype} (kernel: head dim 64, bf16)")
    q, k, v = qkv.view(B, T, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(q, k, v)
    return o.transpose(1, 2).reshape(B, T, num_heads * hd)


def cls_attention(qkv, num_heads: int):
    """Attention of token 0's query only (against every key / value) on a packed qkv
    [B, T, 3*H*hd] -> [B, 1, H*hd]: what a classifier that reads token 0 needs from the last
    block. Native path: one small kernel per direction (hd = 64, T <= 256); torch path: the
    same math in fp32."""
    B, T, D3 = qkv.shape
    hd = D3 // (3 * num_heads)
    if _use_native(qkv):
        from . import native_ops
        if hd == 64 and qkv.dtype == torch.bfloat16 and T <= 256:
            return native_ops.cls_attention(qkv, num_heads)
        native_ops.fallback("cls_attention", f"head dim {hd}, {qkv.dtype}, T {T} (kernel: 64, bf16, T <= 256)")
    q, k, v = qkv.view(B, T, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(q[:, :, :1], k, v)
    return o.transpose(1, 2).reshape(B, 1, num_heads * hd)


def patch_embed(x, conv: nn.Conv2d):
    """Non-overlapping patch conv -> [B, N, D] tokens."""
    if _use_native(x):
        from . import native_ops
        return native_ops.patch_embed(x, conv)
    y = conv(x)
    return y.flatten(2).transpose(1, 2)


def embed_tokens(tok, cls_token, pos_embed):
    """[cls; tok] + pos for [B, N, D] patch tokens -> [B, N+1, D]. Native path: one pass
    writing the token buffer (no concatenated intermediate); torch path: cat + add."""
    if _use_native(tok):
        from . import native_ops
        return native_ops.embed_tokens(tok, cls_token, pos_embed)
    cls = cls_token.to(tok.dtype).expand(tok.shape[0], -1, -1)
    return torch.cat([cls, tok], dim=1) + pos_embed.to(tok.dtype)


def softmax_cross_entropy(logits, target, label_smoothing: float = 0.0):
    """Mean softmax cross-entropy (fused fwd/bwd kernel on the native path). ``target``: int64
    labels [B], or a mixed batch's ``(label_a, label_b, lam)`` (``data.MixedTarget``): row ``b``
    is ``lam[b]`` of class ``label_a[b]`` and ``1 - lam[b]`` of class ``label_b[b]``."""
    if isinstance(target, tuple):
        label_a, label_b, lam = target
        if _use_native(logits):
            from . import native_ops
            if logits.dim() == 2:
                return native_ops.softmax_cross_entropy_pair(logits, label_a, label_b, lam, label_smoothing)
            native_ops.fallback("softmax_cross_entropy", f"logits of shape {tuple(logits.shape)} (kernel: [B, V])")
        x = logits.float()
        ce_a = F.cross_entropy(x, label_a, label_smoothing=label_smoothing, reduction="none")
        ce_b = F.cross_entropy(x, label_b, label_smoothing=label_smoothing, reduction="none")
        lam = lam.to(torch.float32)
        return (lam * ce_a + (1 - lam) * ce_b).mean()
    if _use_native(logits):
        from . import native_ops
        return native_ops.softmax_cross_entropy(logits, target, label_smoothing)
    return F.cross_entropy(logits.float(), target, label_smoothing=label_smoothing)


EVAL_MAX_K = 8  # the k values one eval_stats_update takes (csrc/eval_stats.hip)


def eval_stats_new(ks, device):
    """Zeroed accumulators for :func:`eval_stats_update`: ``(loss_sum float64 [1], counts int64
    [2 + len(ks)])`` -- rows, out-of-range targets, rows correct at each ``k``."""
    return (torch.zeros(1, dtype=torch.float64, device=device),
            torch.zeros(2 + len(ks), dtype=torch.int64, device=device))


def _torch_eval_rows(logits, target, kind, eps):
    """Per-row ``(loss float64 [B], rank int64 [B])`` of csrc/eval_stats.hip's definition from
    comparisons and sums (no ``topk``): ``rank = #{j: x[j] > x[t]} + #{j < t: x[j] == x[t]}``, the
    target's position in a stable descending sort; ``V`` for a row with a NaN or a target outside
    ``[0, V)``, whose loss is 0."""
    x = logits.float() if logits.dtype != torch.float64 else logits
    B, V = x.shape
    t = target.to(torch.long).reshape(B)
    valid = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1).unsqueeze(1)
    xt = x.gather(1, tc)
    cols = torch.arange(V, device=x.device).unsqueeze(0)
    above = (x > xt).sum(1) + ((x == xt) & (cols < tc)).sum(1)
    rank = torch.where(valid & ~torch.isnan(x).any(1), above, torch.full_like(above, V))
    x64 = x.double()
    if kind == "nll":
        rows = -x64.gather(1, tc)[:, 0]
    else:
        rows = torch.logsumexp(x64, 1) - (1.0 - eps) * x64.gather(1, tc)[:, 0] - eps * x64.mean(1)
    return torch.where(valid, rows, torch.zeros_like(rows)), rank


def eval_stats_update(logits, target, loss_sum, counts, ks, kind: str = "ce", eps: float = 0.0):
    """Score one batch and ADD it into the accumulators of :func:`eval_stats_new` -- streaming
    validation: no logits kept, no host sync. ``logits`` [B, V]; ``target`` int64 [B]; ``kind``
    ``"ce"`` (cross-entropy with label smoothing ``eps``) or ``"nll"`` (``-x[t]`` on
    log-probabilities); ``ks``: up to 8 values ``k >= 1``. A row is correct at ``k`` iff its target's
    rank (see ``_torch_eval_rows``) is below ``min(k, V)``; rank 0 is exactly ``torch.argmax == t``.
    Native: one pass over the logits and a one-workgroup reduce (``pdt_eval_stats``); torch path:
    the same definition, the loss summed in float64. Returns the per-row ``(loss, rank)``."""
    ks = tuple(int(k) for k in ks)
    if kind not in ("ce", "nll"):
        raise ValueError(f'eval_stats_update: kind must be "ce" or "nll", got {kind!r}')
    if len(ks) > EVAL_MAX_K or any(k < 1 for k in ks):
        raise ValueError(f"eval_stats_update: at most {EVAL_MAX_K} values k >= 1, got {ks}")
    if logits.dim() != 2 or target.numel() != logits.shape[0]:
        raise ValueError(f"eval_stats_update: logits {tuple(logits.shape)} / target {tuple(target.shape)} "
                         "(expected [B, V] and [B])")
    if logits.shape[0] == 0:
        return logits.new_zeros(0, dtype=torch.float32), target.new_zeros(0, dtype=torch.int32)
    if _use_native(logits):
        from . import native_ops
        return native_ops.eval_stats(logits, target, ks, loss_sum, counts, kind=kind, eps=eps)
    with torch.no_grad():
        rows, rank = _torch_eval_rows(logits, target, kind, float(eps))
        V = logits.shape[1]
        loss_sum += rows.sum()
        new = [torch.tensor(rows.numel(), device=rank.device), ((target < 0) | (target >= V)).sum()]
        new += [(rank < min(k, V)).sum() for k in ks]
        counts += torch.stack(new)
    return rows, rank
