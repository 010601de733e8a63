"""linear (bf16 MFMA GEMM with bias / relu epilogue), its fp8 variant, and the Transformer MLP"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .fp8 import (E4M3, E5M2, _fc1_keep_pre, _fc1_split, _fc1_split_forward, _fc2_dgrad_split, _fc2_dgrad_split_on,
                  _pre_bias_grad, _prequant, _quant_act, _quant_grad, _quant_grad_db, fp8_settings, fp8_weight,
                  gemm_f8, linear_wgrad_f8)
from .gemm import ACT, ACT_GELU_DUAL, ACT_GELU_GRAD, ACT_MUL, _gelu_dual, colsum, conv_nt, conv_wgrad
from .lib import _chk, _grad_buf, _load, _p, _s, fallback
from .shadows import bf16_weight, bf16_weight_t


# -----------------------------------------------------------------------------
# Plain-GEMM backward of nn.Linear (reference op: /root/reference/model/model.py:19,21):
#   dX = dY W     -> the conv_nt NT kernel on the transposed bf16 weight W^T [K][Nout]
#                    (cast+transposed once per optimizer version, cached like the bf16 shadow)
#   dW = dY^T X   -> the split-K weight-gradient kernel (both operands K-outer, read
#                    through ds_read_b64_tr_b16), fp32 output for the optimizer
# Both are hand-written kernels with their own tile-variant tuning; there is no
# library-GEMM branch.
# -----------------------------------------------------------------------------
def _linear_dgrad(dy2, w):
    Nout, K = w.shape
    Mrows = dy2.shape[0]
    wt = bf16_weight_t(w)
    dx = torch.empty((Mrows, K), dtype=torch.bfloat16, device=dy2.device)
    conv_nt(dy2, wt, dx, Hs=1, Ws=1, Cs=Nout, Nimg=Mrows, Hm=1, Wm=1, Ncol=K, K=Nout, ldb=Nout, sh=1, sw=1,
            oh0=0, ow0=0, dh=1, dw=1, nth=1, ntw=1, Ho=1, Wo=1, osh=1, osw=1, oph=0, opw=0, ldo=K)
    return dx


def _linear_wgrad(dy2, x2, w, with_bias=False, bias=None):
    """(dW fp32 [Nout][K], db fp32 [Nout] or None): db comes out of the same kernel."""
    Nout, K = w.shape
    dw = _grad_buf(w, (Nout, K), device=dy2.device)
    db = _grad_buf(bias, (Nout,), device=dy2.device) if with_bias else None
    conv_wgrad(dy2, x2, dw, M=dy2.shape[0], Mo=Nout, No=K, ldy=Nout, Hs=1, Ws=1, C=K, Hm=1, Wm=1, sh=1, sw=1,
               oh0=0, ow0=0, dh=1, dw=1, ntw=1, bias_out=db)
    return dw, db


def _linear_grads(dy2, x2, w, want_db, want_dw, bias=None):
    if want_dw:
        dw, db = _linear_wgrad(dy2, x2, w, with_bias=want_db, bias=bias)
        return dw, db
    return None, (colsum(dy2, dy2.shape[0], w.shape[0]) if want_db else None)


def _residual2d(residual, Mrows, Nout):
    if residual is None:
        return None
    r = residual.reshape(Mrows, Nout)
    assert r.dtype == torch.bfloat16, "residual stream must be bf16"
    return r.contiguous()


def _gemm_bf16(x2, wb, y, *, bias=None, act=None, aux=None, addend=None):
    """y[M, N] = x2[M, K] @ wb[N, K]^T (+bias, act) (+addend) on the conv_nt kernel."""
    Mrows, K = x2.shape
    Nout = wb.shape[0]
    conv_nt(x2, wb, y, Hs=1, Ws=1, Cs=K, Nimg=Mrows, Hm=1, Wm=1, Ncol=Nout, K=K, ldb=K, sh=1, sw=1, oh0=0,
            ow0=0, dh=1, dw=1, nth=1, ntw=1, Ho=1, Wo=1, osh=1, osw=1, oph=0, opw=0, ldo=Nout, bias=bias,
            act=act, aux=aux, addend=addend)
    return y


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b) (+ residual): the residual add rides the GEMM epilogue and
    its gradient is dy itself (no add kernels either way)."""

    @staticmethod
    def forward(ctx, x, w, b, act, residual):
        ctx.bref = b  # the bias parameter: its gradient goes to its reducer slot
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).to(torch.bfloat16).contiguous()
        Mrows, K = x2.shape
        Nout = w.shape[0]
        wb = bf16_weight(w)
        y = torch.empty((Mrows, Nout), dtype=torch.bfloat16, device=x.device)
        z = torch.empty_like(y) if act == "gelu" else None  # pre-activation for GELU backward
        bias = b.float().contiguous() if b is not None else None
        _gemm_bf16(x2, wb, y, bias=bias, act=act, aux=z, addend=_residual2d(residual, Mrows, Nout))
        ctx.save_for_backward(x2, w, y if act == "relu" else z)
        ctx.meta = (shp, act, b is not None)
        return y.reshape(*shp[:-1], Nout)

    @staticmethod
    def backward(ctx, dy):
        x2, w, saved = ctx.saved_tensors
        shp, act, has_b = ctx.meta
        only = getattr(dy, "_pdt_f8g_only", None)
        if only is not None and (only is not ctx.fc or act is not None or not ctx.fp8_dgrad or not ctx.f8w):
            # the producer (the fp8 attention backward) wrote the e5m2 codes and the bias
            # gradient but not the bf16 values this configuration would read
            raise RuntimeError("this output gradient carries fp8 codes only (PDT_ATTN_BWD_Q8); its layer needs "
                               "the bf16 values: set PDT_ATTN_BWD_Q8_BF16=1 or PDT_ATTN_BWD_Q8=0")
        lib = _load()
        st = _s()
        Nout, K = w.shape
        dy2 = dy.reshape(-1, Nout).to(torch.bfloat16).contiguous()
        if act == "relu":
            dy2 = dy2 * (saved > 0)
        elif act == "gelu":
            dz = torch.empty_like(dy2)
            _chk(lib.pdt_gelu_bwd(_p(dy2), _p(saved), _p(dz), dz.numel(), st), "gelu_bwd")
            dy2 = dz
        Mrows = dy2.shape[0]
        dx = _linear_dgrad(dy2, w).reshape(*shp[:-1], K) if ctx.needs_input_grad[0] else None
        dw, db = _linear_grads(dy2, x2, w, has_b and ctx.needs_input_grad[2], ctx.needs_input_grad[1],
                               bias=ctx.bref)
        return dx, dw, db, None, (dy if ctx.needs_input_grad[4] else None)


class _LinearF8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act, fc, residual):
        ctx.bref = b
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).to(torch.bfloat16).contiguous()
        Mrows, K = x2.shape
        Nout = w.shape[0]
        cfg = fp8_settings()
        pre = _prequant(x, fc)
        xq, dqx = pre if pre is not None else _quant_act(x2, fc)
        wq, _, dqw = fp8_weight(w)
        y = torch.empty((Mrows, Nout), dtype=torch.bfloat16, device=x.device)
        z = torch.empty_like(y) if act == "gelu" else None
        bias = b.float().contiguous() if b is not None else None
        gemm_f8(xq, wq, y, dqx, dqw, bias=bias, act=ACT[act], aux=z, addend=_residual2d(residual, Mrows, Nout))
        # fp8 weight gradient (needs the e5m2 dY codes of the fp8 data gradient): keep the
        # e4m3 input codes + their dequant scale instead of the bf16 input
        ctx.f8w = cfg["dgrad"] and cfg["wgrad"] and K % 16 == 0 and Nout % 16 == 0
        if ctx.f8w:
            ctx.xq, ctx.dqx = xq, dqx
            ctx.save_for_backward(None, w, y if act == "relu" else z)
        else:
            ctx.save_for_backward(x2, w, y if act == "relu" else z)
        ctx.meta = (shp, act, b is not None)
        ctx.fc = fc
        # e5m2 data-gradient GEMM (default on; PDT_FP8_DGRAD=0 keeps it bf16)
        ctx.fp8_dgrad = cfg["dgrad"]
        return y.reshape(*shp[:-1], Nout)

    @staticmethod
    def backward(ctx, dy):
        x2, w, saved = ctx.saved_tensors
        shp, act, has_b = ctx.meta
        only = getattr(dy, "_pdt_f8g_only", None)
        if only is not None and (only is not ctx.fc or act is not None or not ctx.fp8_dgrad or not ctx.f8w):
            # the producer (the fp8 attention backward) wrote the e5m2 codes and the bias
            # gradient but not the bf16 values this configuration would read
            raise RuntimeError("this output gradient carries fp8 codes only (PDT_ATTN_BWD_Q8); its layer needs "
                               "the bf16 values: set PDT_ATTN_BWD_Q8_BF16=1 or PDT_ATTN_BWD_Q8=0")
        lib = _load()
        Nout, K = w.shape
        dy2 = dy.reshape(-1, Nout).to(torch.bfloat16).contiguous()
        if act == "relu":
            dy2 = dy2 * (saved > 0)
        elif act == "gelu":
            dz = torch.empty_like(dy2)
            _chk(lib.pdt_gelu_bwd(_p(dy2), _p(saved), _p(dz), dz.numel(), _s()), "gelu_bwd")
            dy2 = dz
        Mrows = dy2.shape[0]
        need = ctx.needs_input_grad
        dx = None
        dyq = dqdy = None
        cast_db = None
        if ctx.fp8_dgrad and (need[0] or (ctx.f8w and need[1])):
            pre = getattr(dy, "_pdt_f8g", None) if act is None else None
            if act is None and has_b and need[2] and ctx.f8w and need[1] and (pre is None or pre[2] is not ctx.fc):
                cast_db = _quant_grad_db(dy2, ctx.fc, "_pdt_fp8_gmeta", ctx.bref)
            if cast_db is not None:
                dyq, dqdy = cast_db[0], cast_db[1]
            else:
                dyq, dqdy = _quant_grad(dy2, ctx.fc, "_pdt_fp8_gmeta", src=dy if act is None else None)
        if need[0]:
            if ctx.fp8_dgrad:
                _, wqt, dqw = fp8_weight(w)
                dx = torch.empty((Mrows, K), dtype=torch.bfloat16, device=dy.device)
                gemm_f8(dyq, wqt, dx, dqdy, dqw, fmt_a=E5M2)
            else:
                dx = _linear_dgrad(dy2, w)
            dx = dx.reshape(*shp[:-1], K)
        want_db = has_b and need[2]
        pre_db = _pre_bias_grad(dy, ctx.fc) if act is None and want_db else None
        if pre_db is None and cast_db is not None:
            pre_db = cast_db[2]
        if ctx.f8w and need[1]:
            dw, db = linear_wgrad_f8(dyq, ctx.xq, dqdy, ctx.dqx, dy16=dy2, with_bias=want_db and pre_db is None, w=w,
                                     b=ctx.bref)
            if pre_db is not None:
                db = pre_db
        elif ctx.f8w:
            dw, db = None, (colsum(dy2, Mrows, Nout) if want_db else None)
        else:
            dw, db = _linear_grads(dy2, x2, w, want_db, need[1], bias=ctx.bref)
        ctx.xq = ctx.dqx = None
        return dx, dw, db, None, None, (dy if need[5] else None)


def linear(x, fc: nn.Linear, act=None, fp8=False, residual=None):
    """act(x W^T + b) (+ residual, added in the GEMM epilogue)."""
    K = fc.in_features
    N = fc.out_features
    if K % 8 or N % 8 or act not in (None, "relu", "gelu") or (residual is not None and (
            residual.dtype != torch.bfloat16 or residual.shape[:-1] != x.shape[:-1] or residual.shape[-1] != N)):
        fallback("linear", f"{K}->{N} act={act} (needs K, N % 8 == 0, act in relu/gelu/None, bf16 residual)")
        from ..fused import _torch_linear
        y = _torch_linear(x, fc, act)
        return y if residual is None else y + residual
    if fp8 and K % 128 == 0 and N % 128 == 0:
        return _LinearF8.apply(x, fc.weight, fc.bias, act, fc, residual)
    return _Linear.apply(x, fc.weight, fc.bias, act, residual)


# -----------------------------------------------------------------------------
# Transformer MLP as one autograd node: fc1 (+bias, GELU in the epilogue, the
# pre-activation z kept as the aux output) -> fc2 (+bias, + residual in the
# epilogue). Backward: the fc2 data gradient's epilogue applies GELU'(z) (conv_nt
# act 3), so dL/dz comes out of that GEMM -- no gelu_bwd pass -- and both bias
# gradients come out of the weight-gradient kernels. fp8 (e4m3 forward operands,
# e5m2 output gradients when PDT_FP8_DGRAD=1) or bf16 GEMMs.
# -----------------------------------------------------------------------------
class _Mlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, mlp, fp8):
        ctx.brefs = (b1, b2)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).to(torch.bfloat16).contiguous()
        Mrows, K = x2.shape
        Hd, Nout = w1.shape[0], w2.shape[0]
        dev = x.device
        a = torch.empty((Mrows, Hd), dtype=torch.bfloat16, device=dev)
        z = None
        out = torch.empty((Mrows, Nout), dtype=torch.bfloat16, device=dev)
        res = _residual2d(residual, Mrows, Nout)
        bias1, bias2 = b1.float().contiguous(), b2.float().contiguous()
        cfg = fp8_settings()
        f8w = fp8 and cfg["dgrad"] and cfg["wgrad"]
        dual = _gelu_dual()
        act1 = ACT_GELU_DUAL if dual else ACT["gelu"]  # z holds gelu'(fc1 pre-activation) when dual
        act2 = ACT_MUL if dual else ACT_GELU_GRAD      # the fc2 data gradient's epilogue
        if fp8:
            pre = _prequant(x, mlp.fc1)
            xq, dqx = pre if pre is not None else _quant_act(x2, mlp.fc1)
            w1q, _, dqw1 = fp8_weight(w1)
            meta2 = getattr(mlp.fc2, "_pdt_fp8_meta", None) if cfg["scaling"] == "delayed" else None
            if meta2 is not None:  # fc1's epilogue writes fc2's e4m3 input (bf16 a only if a bf16 wgrad needs it)
                aq = torch.empty((Mrows, Hd), dtype=torch.uint8, device=dev)
                dqa = None
                if dual and _fc1_split(Mrows, Hd, K):
                    pre = f8w and _fc1_keep_pre()
                    z = None if pre else torch.empty_like(a)
                    dqa = _fc1_split_forward(xq, w1q, a, z, aq, dqx, dqw1, bias1, meta2, keep_a=not f8w)
                    if pre:  # a holds the pre-activation (its gelu lives only as the e4m3 codes)
                        z, act2 = a, ACT_GELU_GRAD
                if dqa is None:
                    z = torch.empty_like(a)
                    dqa = gemm_f8(xq, w1q, a, dqx, dqw1, bias=bias1, act=act1, aux=z, q8=(aq, meta2, E4M3, f8w))
            else:
                z = torch.empty_like(a)
                gemm_f8(xq, w1q, a, dqx, dqw1, bias=bias1, act=act1, aux=z)
                aq, dqa = _quant_act(a, mlp.fc2)
            w2q, _, dqw2 = fp8_weight(w2)
            gemm_f8(aq, w2q, out, dqa, dqw2, bias=bias2, addend=res)
        else:
            z = torch.empty_like(a)
            _gemm_bf16(x2, bf16_weight(w1), a, bias=bias1, act=act1, aux=z)
            _gemm_bf16(a, bf16_weight(w2), out, bias=bias2, addend=res)
        if f8w:  # fp8 weight gradients: the e4m3 GEMM inputs replace the bf16 ones in the saved state
            ctx.f8 = (xq, dqx, aq, dqa)
            ctx.save_for_backward(None, None, z, w1, w2)
        else:
            ctx.f8 = None
            ctx.save_for_backward(x2, a, z, w1, w2)
        ctx.shp, ctx.fp8, ctx.mlp = shp, fp8, mlp
        ctx.act2 = act2
        ctx.fp8_dgrad = fp8 and cfg["dgrad"]
        return out.reshape(*shp[:-1], Nout)

    @staticmethod
    def backward(ctx, g):
        x2, a, z, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        Mrows = z.shape[0]
        Hd, Nout = w1.shape[0], w2.shape[0]
        K = w1.shape[1]
        g2 = g.reshape(Mrows, Nout).to(torch.bfloat16).contiguous()
        dz = torch.empty((Mrows, Hd), dtype=torch.bfloat16, device=g.device)
        f8 = ctx.f8
        dzq = dqdz = pre_db1 = None
        if ctx.fp8_dgrad:
            gq, dqg = _quant_grad(g2, ctx.mlp.fc2, "_pdt_fp8_gmeta", src=g)
            _, w2qt, dqw2 = fp8_weight(w2)
            gmeta1 = getattr(ctx.mlp.fc1, "_pdt_fp8_gmeta", None) if fp8_settings()["scaling"] == "delayed" \
                else None
            if gmeta1 is not None:  # the epilogue also writes fc1's e5m2 output gradient (bf16 dz: bias grad)
                dzq = torch.empty((Mrows, Hd), dtype=torch.uint8, device=g.device)
                if f8 is not None and need[1] and need[2] and os.environ.get("PDT_F8_DB_EPI", "1") == "1":
                    # fc1's bias gradient = column sums of dz formed in this epilogue: the bf16 dz
                    # (only ever read for it) is not written at all
                    pre_db1 = _grad_buf(ctx.brefs[0], (Hd,))
                    if ctx.act2 == ACT_GELU_GRAD and _fc2_dgrad_split_on():  # z: the pre-activation
                        dqdz = _fc2_dgrad_split(gq, w2qt, dz, dqg, dqw2, z, dzq, gmeta1, pre_db1)
                    if dqdz is None:
                        dqdz = gemm_f8(gq, w2qt, dz, dqg, dqw2, fmt_a=E5M2, act=ctx.act2, addend=z,
                                       q8=(dzq, gmeta1, E5M2, True), colsum_out=pre_db1)
                else:
                    dqdz = gemm_f8(gq, w2qt, dz, dqg, dqw2, fmt_a=E5M2, act=ctx.act2, addend=z,
                                   q8=(dzq, gmeta1, E5M2, False))
            else:
                gemm_f8(gq, w2qt, dz, dqg, dqw2, fmt_a=E5M2, act=ctx.act2, addend=z)
        else:
            _gemm_bf16(g2, bf16_weight_t(w2), dz, act=ctx.act2, addend=z)  # dz = (g W2) * gelu'(z)
        pre_db2 = _pre_bias_grad(g, ctx.mlp.fc2) if need[4] else None
        if f8 is not None:
            dw2, db2 = linear_wgrad_f8(gq, f8[2], dqg, f8[3], dy16=g2, with_bias=need[4] and pre_db2 is None, w=w2,
                                       b=ctx.brefs[1]) if need[3] \
                else (None, colsum(g2, Mrows, Nout) if need[4] and pre_db2 is None else None)
            if pre_db2 is not None:
                db2 = pre_db2
        else:
            dw2, db2 = _linear_grads(g2, a, w2, need[4], need[3], bias=ctx.brefs[1])
        dx = None
        if dzq is None and ctx.fp8_dgrad and (need[0] or (f8 is not None and need[1])):
            dzq, dqdz = _quant_grad(dz, ctx.mlp.fc1, "_pdt_fp8_gmeta")
        if need[0]:
            dx = torch.empty((Mrows, K), dtype=torch.bfloat16, device=g.device)
            if ctx.fp8_dgrad:
                _, w1qt, dqw1 = fp8_weight(w1)
                gemm_f8(dzq, w1qt, dx, dqdz, dqw1, fmt_a=E5M2)
            else:
                _gemm_bf16(dz, bf16_weight_t(w1), dx)
            dx = dx.reshape(ctx.shp)
        if f8 is not None:
            dw1, db1 = linear_wgrad_f8(dzq, f8[0], dqdz, f8[1], dy16=dz, with_bias=need[2] and pre_db1 is None,
                                       w=w1, b=ctx.brefs[0]) if need[1] \
                else (None, colsum(dz, Mrows, Hd) if need[2] else None)
            if pre_db1 is not None:
                db1 = pre_db1
        else:
            dw1, db1 = _linear_grads(dz, x2, w1, need[2], need[1], bias=ctx.brefs[0])
        ctx.f8 = None
        return dx, dw1, db1, dw2, db2, (g if need[5] else None), None, None


def mlp(x, m, fp8=False, residual=None):
    """fc2(gelu(fc1(x))) (+ residual) for an Mlp module with fc1 / fc2 (ViT)."""
    fc1, fc2 = m.fc1, m.fc2
    K, Hd, N = fc1.in_features, fc1.out_features, fc2.out_features
    ok = (K % 8 == 0 and Hd % 8 == 0 and N % 8 == 0 and fc2.in_features == Hd and fc1.bias is not None
          and fc2.bias is not None and (residual is None or (residual.dtype == torch.bfloat16
                                                            and residual.shape[:-1] == x.shape[:-1]
                                                            and residual.shape[-1] == N)))
    use8 = fp8 and K % 128 == 0 and Hd % 128 == 0 and N % 128 == 0
    if not ok:
        y = linear(linear(x, fc1, act="gelu", fp8=fp8), fc2, fp8=fp8)
        return y if residual is None else y + residual
    return _Mlp.apply(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, residual, m, use8)
