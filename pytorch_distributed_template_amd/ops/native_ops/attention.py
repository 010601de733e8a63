"""ViT attention: the fused multi-head kernels off the packed qkv projection output"""
from __future__ import annotations

import os

import torch

from .fp8 import fp8_settings
from .lib import _chk, _grad_buf, _load, _p, _s, fallback


def _attn_bwd_q8_target(ctx):
    """(owner, gmeta) when the fp8 attention backward should also write the qkv projection's
    e5m2 gradient codes and bias gradient: delayed scaling with an amax history on the
    projection (``grad_fp8_for`` = the fp8 layer whose output is this attention's only input)
    whose backward is fp8 in both GEMMs. PDT_ATTN_BWD_Q8=0: the separate cast pass."""
    owner = ctx.grad_owner
    if owner is None or os.environ.get("PDT_ATTN_BWD_Q8", "1") != "1":
        return None
    cfg = fp8_settings()
    gmeta = getattr(owner, "_pdt_fp8_gmeta", None)
    if gmeta is None or cfg["scaling"] != "delayed" or not (cfg["dgrad"] and cfg["wgrad"]):
        return None
    return owner, gmeta


class _QKVAttention(torch.autograd.Function):
    """Fused multi-head attention straight off the qkv projection output
    (csrc/attention.hip): qkv [B, T, 3*H*64] -> out [B, T, H*64] (the proj
    GEMM's input layout) with the log-sum-exp saved for the recomputing
    backward, which writes d(qkv) in the qkv layout (the qkv GEMM's dY)."""

    @staticmethod
    def forward(ctx, qkv, H, fp8=False, q8meta=None, box=None, grad_owner=None):
        B, T, D3 = qkv.shape
        assert D3 == 3 * H * 64 and qkv.dtype == torch.bfloat16, "head_dim must be 64, bf16"
        qkv = qkv.contiguous()
        out = torch.empty((B, T, H * 64), dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty((B * H, T), dtype=torch.float32, device=qkv.device)
        scale = 64 ** -0.5
        if fp8 and T <= 256 and q8meta is not None:  # + the projection GEMM's e4m3 input
            codes = torch.empty((B * T, H * 64), dtype=torch.uint8, device=qkv.device)
            part = torch.empty(B * H + 1, dtype=torch.float32, device=qkv.device)
            dq = part[-1:]
            _chk(_load().pdt_attn_fwd_f8_q8(_p(qkv), _p(out), _p(lse), B, T, H, scale, _p(codes), _p(q8meta),
                                            _p(part), _p(dq), _s()), "attn_fwd_f8_q8")
            box.append((codes, dq))
        elif fp8 and T <= 256:  # fp8 QK^T (csrc/attention_f8.hip), fp32 softmax, bf16 PV
            _chk(_load().pdt_attn_fwd_f8(_p(qkv), _p(out), _p(lse), B, T, H, scale, _s()), "attn_fwd_f8")
        elif T <= 256 and os.environ.get("PDT_ATTN_FWD32", "1") == "1":  # 32x32-tile bf16 forward
            _chk(_load().pdt_attn_fwd_tiles(_p(qkv), _p(out), _p(lse), B, T, H, scale, _s()), "attn_fwd_tiles")
        else:
            _chk(_load().pdt_attn_fwd(_p(qkv), _p(out), _p(lse), B, T, H, scale, _s()), "attn_fwd")
        ctx.save_for_backward(qkv, out, lse)
        ctx.H, ctx.scale, ctx.grad_owner, ctx.fp8 = H, scale, grad_owner, bool(fp8)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, T, _ = qkv.shape
        dout = dout.to(torch.bfloat16).contiguous()
        delta = torch.empty_like(lse)
        dqkv = torch.empty_like(qkv)
        owner = ctx.grad_owner
        gmeta = getattr(owner, "_pdt_fp8_gmeta", None) if owner is not None else None
        f8bwd = ctx.fp8 and T <= 256 and os.environ.get("PDT_FP8_ATTN_BWD", "1") == "1"
        if not f8bwd and gmeta is not None and T <= 256 and fp8_settings()["scaling"] == "delayed" and \
                os.environ.get("PDT_FP8_ATTN_Q8", "0") == "1":
            # also the e5m2 codes of d(qkv) for the qkv projection's fp8 gradient GEMMs
            codes = torch.empty((B * T, qkv.shape[2]), dtype=torch.uint8, device=qkv.device)
            part = torch.empty(2 * B * ctx.H + 1, dtype=torch.float32, device=qkv.device)
            dq = part[-1:]
            rc = _load().pdt_attn_bwd_q8(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), B, T, ctx.H,
                                         ctx.scale, _p(codes), _p(gmeta), _p(part), _p(dq), _s())
            if rc == 0:
                dqkv._pdt_f8g = (codes, dq, owner)
                return dqkv, None, None, None, None, None
        if f8bwd:
            # fused fp8 backward (csrc/attention_bwd_f8.hip): dQ, dK, dV in one kernel on e4m3 MFMA
            q8 = _attn_bwd_q8_target(ctx)
            if q8 is not None:
                # ... that also writes the qkv projection's e5m2 output gradient (its delayed
                # scale) and bias gradient; the bf16 d(qkv) is then never read (the projection's
                # backward consumes the codes and the bias gradient: _LinearF8), so it is not
                # written unless PDT_ATTN_BWD_Q8_BF16=1
                owner, gmeta = q8
                lib = _load()
                n = qkv.shape[2]
                codes = torch.empty((B * T, n), dtype=torch.uint8, device=qkv.device)
                grid = lib.pdt_attn_bwd_f8_grid(B, ctx.H)
                part = torch.empty(grid + 1, dtype=torch.float32, device=qkv.device)
                dq = part[-1:]
                colpart = torch.empty(B * n + lib.pdt_reduce_rows_work(B, n), dtype=torch.float32,
                                      device=qkv.device)
                db = _grad_buf(getattr(owner, "bias", None), (n,))
                wbf = os.environ.get("PDT_ATTN_BWD_Q8_BF16", "0") == "1"
                _chk(lib.pdt_attn_bwd_f8_q8(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv) if wbf else None, B, T,
                                            ctx.H, ctx.scale, _p(codes), _p(gmeta), _p(part), _p(dq), _p(colpart),
                                            _p(db), _s()), "attn_bwd_f8_q8")
                dqkv._pdt_f8g = (codes, dq, owner)
                dqkv._pdt_db = (db, owner)
                if not wbf:
                    dqkv._pdt_f8g_only = owner  # (the values were not written: see _LinearF8)
                return dqkv, None, None, None, None, None
            _chk(_load().pdt_attn_bwd_f8(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), B, T, ctx.H, ctx.scale,
                                         _s()), "attn_bwd_f8")
            return dqkv, None, None, None, None, None
        _chk(_load().pdt_attn_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), B, T, ctx.H,
                                  ctx.scale, _s()), "attn_bwd")
        return dqkv, None, None, None, None, None


class _ClsAttention(torch.autograd.Function):
    """Attention of token 0's query against all T keys of a packed qkv [B, T, 3*H*64]
    (csrc/attention_cls.hip): the output [B, 1, H*64] and, in backward, the full dqkv (token 0's
    q gradient, every token's k / v gradients, zeros for the other queries)."""

    @staticmethod
    def forward(ctx, qkv, H):
        B, T, D3 = qkv.shape
        qkv = qkv.contiguous()
        if qkv.data_ptr() % 16:  # the kernels read 16-B chunks
            qkv = qkv.clone()
        o = torch.empty((B, 1, D3 // 3), dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty(B * H, dtype=torch.float32, device=qkv.device)
        _chk(_load().pdt_cls_attn_fwd(_p(qkv), _p(o), _p(lse), B, T, H, _s()), "cls_attn_fwd")
        ctx.save_for_backward(qkv, o, lse)
        ctx.H = H
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        B, T, _ = qkv.shape
        do = do.to(torch.bfloat16).contiguous()
        if do.data_ptr() % 16:  # the kernel reads 16-B chunks
            do = do.clone()
        dqkv = torch.empty_like(qkv)
        _chk(_load().pdt_cls_attn_bwd(_p(qkv), _p(o), _p(do), _p(lse), _p(dqkv), B, T, ctx.H, _s()), "cls_attn_bwd")
        return dqkv, None


def cls_attention(qkv, num_heads):
    assert qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 3 * 64 * num_heads and qkv.shape[1] <= 256
    return _ClsAttention.apply(qkv, num_heads)


def qkv_attention(qkv, num_heads, fp8=False, fp8_for=None, grad_fp8_for=None):
    """softmax(q k^T / 8) v over heads of 64 for a packed [B, T, 3*H*64] qkv. ``fp8``: the
    score GEMM on e4m3 MFMA (per-head / per-tile power-of-two scales, T <= 256) and the
    fused fp8 backward (csrc/attention_bwd_f8.hip; PDT_FP8_ATTN_BWD=0: the bf16 one). ``fp8_for``: the fp8 layer consuming
    the output (the attention projection): under delayed scaling the kernel also writes
    its e4m3 input (``_pdt_f8`` on the result, as :func:`ln_fork` does); ``grad_fp8_for``:
    the fp8 layer that produced qkv -- the backward then also writes its e5m2 output
    gradient (``_pdt_f8g`` on d(qkv))."""
    meta = None
    # Default "fwd": the fp8 attention forward also writes the projection's e4m3 input codes
    # (same-box A/B, round 6 q29: 11 626 / 11 640 vs 11 546 / 11 558 img/s with the separate cast
    # pass, "0"). "1" adds the bf16 backward's d(qkv) codes (the fp8 backward writes its own:
    # _attn_bwd_q8_target); in round 4 (r4e-r4h) the then-kernels' uncoalesced code stores cost
    # more than the casts (6.32k vs 6.40k img/s), which is why this was off until round 6.
    q8 = os.environ.get("PDT_FP8_ATTN_Q8", "fwd")
    if q8 != "1":
        if not fp8:  # (the fp8 backward's epilogue writes the gradient codes: _attn_bwd_q8_target)
            grad_fp8_for = None
        if q8 != "fwd":
            fp8_for = None
    if fp8 and fp8_for is not None and fp8_settings()["scaling"] == "delayed":
        meta = getattr(fp8_for, "_pdt_fp8_meta", None)
    box: list = []
    out = _QKVAttention.apply(qkv, num_heads, bool(fp8), meta, box, grad_fp8_for if fp8 else None)
    if box:
        out._pdt_f8 = (box[0][0], box[0][1], fp8_for)
    return out


def attention(q, k, v):
    """softmax(q k^T / sqrt(64)) v for [B, H, T, 64] q / k / v on the fused attention
    kernel (packs them into the [B, T, 3*H*64] layout :func:`qkv_attention` reads)."""
    B, H, T, d = q.shape
    if d != 64 or k.shape != q.shape or v.shape != q.shape or q.dtype != torch.bfloat16:
        fallback("attention", f"q {tuple(q.shape)} {q.dtype} (kernel: head dim 64, bf16, self-attention shapes)")
        return torch.nn.functional.scaled_dot_product_attention(q, k, v)
    qkv = torch.stack([q, k, v], dim=2).permute(0, 3, 2, 1, 4).reshape(B, T, 3 * H * d)
    return qkv_attention(qkv, H).view(B, T, H, d).transpose(1, 2)
