"""ViT patch embedding and token assembly"""
from __future__ import annotations

import os

import torch

from .bn_unit import _Unit, _unit_dw, _unit_dx
from .conv import _fwd_geom, _fwd_nt_geom
from .gemm import colsum, conv_nt, conv_wgrad
from .lib import _cl, _empty_cl, _grad_buf, fallback
from .linear import _gemm_bf16
from .shadows import bf16_weight


class _PatchEmbed(torch.autograd.Function):
    """Non-overlapping patch conv as an implicit GEMM whose NHWC output IS the
    [B, N_patches, D] token matrix (no transpose pass)."""

    @staticmethod
    def forward(ctx, x, w, b, conv):
        N, C, H, W = x.shape
        Cs = C if C % 8 == 0 else 8
        x = x.to(torch.bfloat16)
        if Cs != C:
            x = torch.nn.functional.pad(_cl(x).permute(0, 2, 3, 1), (0, Cs - C)).permute(0, 3, 1, 2)
        x = _cl(x)
        Cout = w.shape[0]
        g = _fwd_geom(N, H, W, Cs, conv)
        wb = bf16_weight(w, pad_cin_to=Cs if Cs != C else None)
        y = _empty_cl(N, Cout, g["Ho"], g["Wo"], torch.bfloat16, x.device)
        conv_nt(x, wb, y, bias=b.float().contiguous() if b is not None else None,
                **_fwd_nt_geom(N, H, W, Cs, Cout, g))
        u = _Unit()
        u.x, u.w, u.N, u.C, u.Cs, u.H, u.W, u.Cout, u.g = x, w, N, C, Cs, H, W, Cout, g
        ctx.u = u
        ctx.has_b = b is not None
        return y.permute(0, 2, 3, 1).reshape(N, g["Ho"] * g["Wo"], Cout)

    @staticmethod
    def backward(ctx, dtok):
        u = ctx.u
        N, Cout = u.N, u.Cout
        dy = dtok.to(torch.bfloat16).reshape(N, u.g["Ho"], u.g["Wo"], Cout).permute(0, 3, 1, 2)
        dy = _cl(dy)
        dw = _unit_dw(dy, u) if ctx.needs_input_grad[1] else None
        db = None
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = colsum(dy, N * u.g["Ho"] * u.g["Wo"], Cout)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _unit_dx(dy, u)
        del ctx.u
        return dx, dw, db, None


class _PatchLinear(torch.autograd.Function):
    """Non-overlapping patch conv as patchify + plain GEMM: one strided copy forms the
    [B*N_patches, C*KH*KW] patch matrix (bf16, in the weight's own element order), then the
    bf16 GEMM (bias in its epilogue) writes the token matrix and the weight gradient + bias
    sums are one plain wgrad call on the same patch matrix. For 3-channel images this is
    K = 768 instead of the implicit GEMM's channel-padded K = 2048 (ViT-B/16), and no pad pass.
    The reference runs torch's conv (torchvision vit_b_16 ``conv_proj``)."""

    @staticmethod
    def forward(ctx, x, w, b, conv):
        N, C, H, W = x.shape
        Cout, _, KH, KW = w.shape
        nh, nw = H // KH, W // KW
        K = C * KH * KW
        kkc = w.is_contiguous(memory_format=torch.channels_last) and not w.is_contiguous()
        xv = x.view(N, C, nh, KH, nw, KW)
        pm = torch.empty((N * nh * nw, K), dtype=torch.bfloat16, device=x.device)
        if kkc:  # weight memory order (kh, kw, c)
            pm.view(N, nh, nw, KH, KW, C).copy_(xv.permute(0, 2, 4, 3, 5, 1))
            wb = bf16_weight(w).permute(0, 2, 3, 1).reshape(Cout, K)
        else:    # (c, kh, kw)
            pm.view(N, nh, nw, C, KH, KW).copy_(xv.permute(0, 2, 4, 1, 3, 5))
            wb = w.detach().reshape(Cout, K).to(torch.bfloat16).contiguous()
        y = torch.empty((N * nh * nw, Cout), dtype=torch.bfloat16, device=x.device)
        _gemm_bf16(pm, wb, y, bias=b.float().contiguous() if b is not None else None)
        ctx.save_for_backward(pm)
        ctx.meta = (w, b, kkc, N, nh * nw)
        return y.view(N, nh * nw, Cout)

    @staticmethod
    def backward(ctx, dtok):
        (pm,) = ctx.saved_tensors
        w, b, kkc, N, npatch = ctx.meta
        Cout = w.shape[0]
        K = pm.shape[1]
        want_dw, want_db = ctx.needs_input_grad[1], b is not None and ctx.needs_input_grad[2]
        dy2 = dtok.reshape(-1, Cout).to(torch.bfloat16).contiguous()
        dw = db = None
        if want_dw:
            if kkc:
                dw = _grad_buf(w, tuple(w.shape), torch.channels_last)
                dw2 = dw.permute(0, 2, 3, 1).reshape(Cout, K)
            else:
                dw = _grad_buf(w, tuple(w.shape))
                dw2 = dw.view(Cout, K)
            db = _grad_buf(b, (Cout,)) if want_db else None
            conv_wgrad(dy2, pm, dw2, M=dy2.shape[0], Mo=Cout, No=K, ldy=Cout, Hs=1, Ws=1, C=K, Hm=1, Wm=1, sh=1,
                       sw=1, oh0=0, ow0=0, dh=1, dw=1, ntw=1, bias_out=db)
            dw = dw.to(w.dtype) if dw.dtype != w.dtype else dw
        elif want_db:
            db = colsum(dy2, dy2.shape[0], Cout)
        return None, dw, db, None


class _EmbedTokens(torch.autograd.Function):
    """x[:, 0] = cls + pos[0], x[:, 1:] = tok + pos[1:] written straight into the [B, N+1, D]
    buffer (one pass over the tokens instead of torch.cat then the broadcast add). Backward:
    d_pos = sum over the batch, d_cls = d_pos[0] (cls and pos[0] add to the same token of every
    image), d_tok a view of the incoming gradient. The reference gets its token assembly from
    torchvision's vit_b_16 (class token concat + pos-embedding add)."""

    @staticmethod
    def forward(ctx, tok, cls_token, pos_embed):
        B, N, D = tok.shape
        x = torch.empty((B, N + 1, D), dtype=tok.dtype, device=tok.device)
        pos = pos_embed.detach().to(tok.dtype).reshape(N + 1, D)
        torch.add(tok, pos[1:], out=x[:, 1:])
        x[:, 0] = (cls_token.detach().reshape(D) + pos_embed.detach().reshape(N + 1, D)[0]).to(tok.dtype)
        ctx.meta = (cls_token.shape, cls_token.dtype, pos_embed.shape, pos_embed.dtype)
        return x

    @staticmethod
    def backward(ctx, dx):
        cshape, cdtype, pshape, pdtype = ctx.meta
        need_pos = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dpos = dx.sum(0, dtype=torch.float32) if need_pos else None
        dcls = dpos[0].reshape(cshape).to(cdtype) if ctx.needs_input_grad[1] else None
        dp = dpos.reshape(pshape).to(pdtype) if ctx.needs_input_grad[2] else None
        dtok = dx[:, 1:] if ctx.needs_input_grad[0] else None
        return dtok, dcls, dp


def embed_tokens(tok, cls_token, pos_embed):
    B, N, D = tok.shape
    if os.environ.get("PDT_EMBED_FUSED", "1") != "1":  # A/B switch: torch.cat + add
        return torch.cat([cls_token.to(tok.dtype).expand(B, -1, -1), tok], dim=1) + pos_embed.to(tok.dtype)
    if cls_token.numel() != D or pos_embed.numel() != (N + 1) * D:
        fallback("embed_tokens", f"cls {tuple(cls_token.shape)} pos {tuple(pos_embed.shape)} for tokens {tuple(tok.shape)}")
        return torch.cat([cls_token.to(tok.dtype).expand(B, -1, -1), tok], dim=1) + pos_embed.to(tok.dtype)
    return _EmbedTokens.apply(tok, cls_token, pos_embed)


def _patch_linear_ok(x, conv) -> bool:
    if os.environ.get("PDT_PATCH_LINEAR", "1") != "1" or x.requires_grad:
        return False
    K = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
    return K % 8 == 0 and x.dtype in (torch.bfloat16, torch.float32)


def patch_embed(x, conv):
    KH, KW = conv.kernel_size
    if (conv.stride != conv.kernel_size or conv.padding != (0, 0) or conv.out_channels % 8 or conv.groups != 1
            or conv.dilation != (1, 1) or x.dim() != 4 or x.shape[2] % KH or x.shape[3] % KW
            or (x.shape[1] % 8 and x.shape[1] > 8)):
        fallback("patch_embed", f"conv {tuple(conv.kernel_size)}/{tuple(conv.stride)} on {tuple(x.shape)} "
                                "(kernel: non-overlapping patches, bias-any, channels <= 8 or % 8 == 0)")
        y = conv(x)
        return y.flatten(2).transpose(1, 2)
    if _patch_linear_ok(x, conv):
        return _PatchLinear.apply(x, conv.weight, conv.bias, conv)
    return _PatchEmbed.apply(x, conv.weight, conv.bias, conv)
