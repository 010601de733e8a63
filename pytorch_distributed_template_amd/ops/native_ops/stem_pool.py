"""pooling, and the ResNet stem (space-to-depth conv -> BN -> ReLU -> max-pool as one node)"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import autotune
from .bn_unit import _BNArgs, _Unit, _bn_bwd, _bn_bwd_pool, _unit_dw, _unit_dx, _unit_fwd, nhwc_padded_view
from .conv import _BnbPartials, supports_conv
from .gemm import _nt_args, conv_nt, conv_stat_rows, conv_wgrad, conv_wgrad_bn, select_nt_variant
from .lib import _chk, _cl, _empty_cl, _grad_buf, _load, _p, _s, fallback
from .shadows import _same_tensor, _weak
from .tuning import NOT_APPLICABLE


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        x = _cl(x)
        N, C, H, W = x.shape
        Ho = (H + 2 * p - k) // s + 1
        Wo = (W + 2 * p - k) // s + 1
        y = _empty_cl(N, C, Ho, Wo, torch.bfloat16, x.device)
        idx = torch.empty(N * Ho * Wo * C, dtype=torch.uint8, device=x.device)
        _chk(_load().pdt_maxpool_fwd(_p(x), _p(y), _p(idx), N, H, W, C, Ho, Wo, k, s, p, _s()), "maxpool_fwd")
        ctx.save_for_backward(idx)
        ctx.meta = (N, C, H, W, Ho, Wo, k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, C, H, W, Ho, Wo, k, s, p = ctx.meta
        dy = _cl(dy.to(torch.bfloat16))
        dx = _empty_cl(N, C, H, W, torch.bfloat16, dy.device)
        _chk(_load().pdt_maxpool_bwd(_p(dy), _p(idx), _p(dx), N, H, W, C, Ho, Wo, k, s, p, _s()), "maxpool_bwd")
        return dx, None, None, None


# -----------------------------------------------------------------------------
# Space-to-depth stem. The 7x7 stride-2 conv over 3 channels, run directly, pads
# every pixel to 8 channels (5/8 of the GEMM K is zeros) and gathers 49 taps of
# 16 B. Over NHWC storage padded to 4 channels, one 16-B chunk is instead TWO
# horizontally adjacent pixels: the conv becomes 8 (kh) x 4 (kw pairs) taps of
# 8 "channels" (b, c), K = 256 instead of 392, with the stride-2 column walk
# folded into the tap offset (ow0 = -4, dw = 2: every pair starts on an even
# pixel, so it is 16-B aligned and either wholly inside or wholly outside the
# image). The kernels take the pixel stride separately (pix = 4, Cs = 8).
#   W'[co, (kh*4 + t)*8 + b*4 + c] = W[co, c, kh, 2t + b - 1]  (0 outside 7x7 / c >= C)
# -----------------------------------------------------------------------------
_S2D_W: dict = {}


def _s2d_ok(x, conv: nn.Conv2d) -> bool:
    return (tuple(conv.kernel_size) == (7, 7) and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3)
            and conv.in_channels <= 4 and x.shape[1] == conv.in_channels and x.shape[2] % 2 == 0
            and x.shape[3] % 2 == 0 and os.environ.get("PDT_STEM_S2D", "1") != "0")


def _s2d_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, 256] bf16 space-to-depth stem weight (cached per parameter version)."""
    ent = _S2D_W.get(id(w))
    if ent is not None and ent[1] == w._version and ent[2] == w.data_ptr() and _same_tensor(ent[3], w):
        return ent[0]
    Cout, C = w.shape[0], w.shape[1]
    wp = torch.nn.functional.pad(w.detach().float(), (1, 0, 0, 1, 0, 4 - C))  # [Cout, 4, 8(kh), 8(kw+1)]
    out = wp.view(Cout, 4, 8, 4, 2).permute(0, 2, 3, 4, 1).reshape(Cout, 256).to(torch.bfloat16).contiguous()
    _S2D_W[id(w)] = (out, w._version, w.data_ptr(), _weak(w))
    return out


def _s2d_unfold_grad(dw256: torch.Tensor, C: int) -> torch.Tensor:
    """[Cout, 256] fp32 space-to-depth weight gradient -> [Cout, C, 7, 7]."""
    Cout = dw256.shape[0]
    g = dw256.view(Cout, 8, 4, 2, 4).permute(0, 4, 1, 2, 3).reshape(Cout, 4, 8, 8)
    return g[:, :C, :7, 1:8]


def _s2d_geom(N, H, W, Cout):
    Ho, Wo = H // 2, W // 2
    return dict(Hs=H, Ws=W, Cs=8, Nimg=N, Hm=Ho, Wm=Wo, Ncol=Cout, K=256, ldb=256, sh=2, sw=2, oh0=-3, ow0=-4,
                dh=1, dw=2, nth=8, ntw=4, Ho=Ho, Wo=Wo, osh=1, osw=1, oph=0, opw=0, ldo=Cout, pix=4)


def _stem_halo_choice(x4, wb, y, N, H, W, Cout, a, v) -> bool:
    """Halo-patch stem kernel (csrc/stem.hip) or the generic space-to-depth GEMM (tile ``v``):
    a tuned per-geometry choice (both with their BN statistics epilogue); ``PDT_STEM_HALO=0``
    forces the generic GEMM."""
    lib = _load()
    if os.environ.get("PDT_STEM_HALO", "1") == "0" or lib.pdt_stem_fwd_rows(N, H, W, Cout) < 0:
        return False

    def setup():
        rows = lib.pdt_stem_fwd_rows(N, H, W, Cout), conv_stat_rows(N * H * W // 4, Cout, a["K"], v)
        ph, pg = (torch.empty(2 * r * Cout, dtype=torch.float32, device=x4.device) for r in rows)
        return (0, 1), lambda k: lib.pdt_stem_fwd(_p(x4), _p(wb), _p(y), _p(ph), N, H, W, Cout, _s()) if k == 1 \
            else lib.pdt_conv_nt(*_nt_args(x4, wb, y, pg, None, a, 0, v))

    return autotune.choose(autotune.stem_key(N, H, W, Cout), setup, 1) == 1


def _unit_fwd_s2d(x, w, gamma, beta, bna: _BNArgs):
    """Stem conv (space-to-depth GEMM) + BN statistics/finalize; no apply."""
    lib = _load()
    st = _s()
    N, C, H, W = x.shape
    x4 = nhwc_padded_view(x, 4)
    if x4 is None:
        x4 = _cl(torch.nn.functional.pad(_cl(x.to(torch.bfloat16)).permute(0, 2, 3, 1), (0, 4 - C))
                 .permute(0, 3, 1, 2))
    Cout = w.shape[0]
    a = _s2d_geom(N, H, W, Cout)
    Ho, Wo = a["Ho"], a["Wo"]
    M = N * Ho * Wo
    wb = _s2d_weight(w)
    y = _empty_cl(N, Cout, Ho, Wo, torch.bfloat16, x.device)
    f32 = dict(dtype=torch.float32, device=x.device)
    v = select_nt_variant(x4, wb, y, with_stats=bna.training, **a)
    halo = _stem_halo_choice(x4, wb, y, N, H, W, Cout, a, v) if bna.training else False
    if halo:  # the halo-patch stem kernel (csrc/stem.hip), statistics in its epilogue
        R = lib.pdt_stem_fwd_rows(N, H, W, Cout)
        part = torch.empty(2 * R * Cout + lib.pdt_rows_reduce_workspace(R, Cout), **f32)
        _chk(lib.pdt_stem_fwd(_p(x4), _p(wb), _p(y), _p(part), N, H, W, Cout, st), "stem_fwd")
    elif bna.training:
        R = conv_stat_rows(M, Cout, a["K"], v)
        part = torch.empty(2 * R * Cout + lib.pdt_rows_reduce_workspace(R, Cout), **f32)
        conv_nt(x4, wb, y, stats=part, variant=v, **a)
    if bna.training:
        vec = torch.empty((4, Cout), **f32)
        mean, invstd, scale, shift = vec[0], vec[1], vec[2], vec[3]
        _chk(lib.pdt_bn_finalize(_p(part), R, Cout, float(M), float(bna.eps), float(bna.momentum), _p(gamma),
                                 _p(beta), _p(mean), _p(invstd), _p(scale), _p(shift), _p(bna.rm), _p(bna.rv),
                                 _p(bna.nbt), st), "bn_finalize")
    else:
        conv_nt(x4, wb, y, variant=v, **a)
        invstd = torch.rsqrt(bna.rv.float() + bna.eps)
        mean = bna.rm.float().clone()
        scale = (gamma.float() * invstd).contiguous()
        shift = (beta.float() - mean * scale).contiguous()
    u = _Unit()
    u.x, u.w, u.gamma, u.beta, u.y = x4, w, gamma, beta, y
    u.act, u.mask, u.bnb_pre = None, None, None
    u.mean, u.invstd, u.scale, u.shift = mean, invstd, scale, shift
    g = dict(KH=7, KW=7, sh=2, sw=2, ph=3, pw=3, Ho=Ho, Wo=Wo, s2d=True)
    u.N, u.C, u.Cs, u.H, u.W, u.Cout, u.g, u.relu, u.has_res = N, C, 8, H, W, Cout, g, True, False
    return u


def _stem_wgrad_halo(u: _Unit, dA, coef, dw256, generic) -> bool:
    """The halo-patch stem weight gradient (csrc/stem.hip, the BN backward apply in its dY
    staging) into ``dw256``: variant 0 (register prefetch, 4-row bands) or 1 (all operands by
    LDS-DMA, double-buffered 2-row bands), a tuned per-geometry choice against each other and
    ``generic()`` (the generic weight-gradient path, itself tuned; key stem2w, value -1 =
    generic; ``PDT_STEM_HALO=0`` forces generic). False: not taken here (the caller runs
    ``generic``)."""
    lib = _load()
    N, H, W, Cout = u.N, u.H, u.W, u.Cout
    if os.environ.get("PDT_STEM_HALO", "1") == "0" or u.x.shape[1] != 4 or \
            lib.pdt_stem_wgrad_splits_v(N, H, W, Cout, 0) < 0:
        return False
    ws = {}

    def run_halo(v):
        splits = lib.pdt_stem_wgrad_splits_v(N, H, W, Cout, v)
        if splits < 0:
            return NOT_APPLICABLE
        if v not in ws:
            ws[v] = torch.empty(lib.pdt_wgrad_workspace(splits, Cout, 256), dtype=torch.float32, device=dA.device)
        rc = lib.pdt_stem_wgrad_v(_p(u.x), _p(dA), _p(u.y), _p(coef), _p(ws[v]), N, H, W, Cout, v, _s())
        if rc == 0:
            rc = lib.pdt_wgrad_reduce(_p(ws[v]), _p(dw256), None, None, splits, Cout, 256, 1.0, 0, _s())
        return rc

    # (one untimed generic() settles the generic path's own tuning before it is timed)
    choice = autotune.choose(autotune.stem_key(N, H, W, Cout, True), lambda: ((0, 1), run_halo), 1,
                             ref=generic, ref_value=-1, ref_first=True)
    if choice < 0:
        return False
    _chk(run_halo(choice), "stem_wgrad")
    return True


def _unit_dw_s2d(dy, u: _Unit, bn_dA=None):
    """Stem weight gradient (space-to-depth GEMM). ``bn_dA`` = (dA, k1, k2, k3): ``dy`` is
    not given (None) and the stem BN's backward apply is formed inside the weight
    gradient's dY staging when the tuner finds that faster than the element pass."""
    a = _s2d_geom(u.N, u.H, u.W, u.Cout)
    dw256 = torch.empty((u.Cout, 256), dtype=torch.float32, device=u.y.device)
    g = dict(M=u.N * a["Ho"] * a["Wo"], Mo=u.Cout, No=256, ldy=u.Cout, Hs=u.H, Ws=u.W, C=8, Hm=a["Ho"], Wm=a["Wo"],
             sh=2, sw=2, oh0=-3, ow0=-4, dh=1, dw=2, ntw=4, pix=4)
    if bn_dA is not None:
        dA, k1, k2, k3 = bn_dA
        coef = torch.stack([k1, k2, k3, u.scale, u.shift]).contiguous()
        lib = _load()
        M = u.y.numel() // u.Cout

        def apply_pass():
            dy = torch.empty_like(u.y, memory_format=torch.channels_last)
            _chk(lib.pdt_bn_bwd_apply(_p(dA), _p(u.y), None, _p(u.scale), _p(u.shift), _p(k1), _p(k2), _p(k3),
                                      _p(dy), None, M, u.Cout, 1, None, _s()), "bn_bwd_apply")
            return dy

        def run_ref():
            conv_wgrad(apply_pass(), u.x, dw256, **g)

        def generic():
            if not conv_wgrad_bn(dA, u.x, dw256, u.y, coef, run_ref, **g):
                conv_wgrad(apply_pass(), u.x, dw256, **g)

        if not _stem_wgrad_halo(u, dA, coef, dw256, generic):
            generic()
    else:
        conv_wgrad(dy, u.x, dw256, **g)
    dw = _grad_buf(u.w, tuple(u.w.shape), torch.channels_last).copy_(_s2d_unfold_grad(dw256, u.C))
    return dw.to(u.w.dtype) if dw.dtype != u.w.dtype else dw


def _pool_bwd_bnred(dout, idx, dA, u: _Unit, k, s, p):
    """Stem max-pool backward fused with the stem BN backward reduction
    (``pdt_maxpool_bwd_bnred``): writes ``dA`` and returns its BN partials as a
    ``_BnbPartials`` for ``_bn_bwd(pre=...)``, or None when not covered
    (``PDT_POOL_BNRED=0`` forces the separate passes)."""
    if os.environ.get("PDT_POOL_BNRED", "1") == "0" or (k, s, p) != (3, 2, 1) or not u.relu or u.mask is not None \
            or u.act is not None:
        return None
    lib = _load()
    N, C, H, W = u.N, u.Cout, u.g["Ho"], u.g["Wo"]
    Ho, Wo = dout.shape[2], dout.shape[3]
    blocks = min(int(os.environ.get("PDT_POOL_BNRED_BLOCKS", "8192")), N * ((H + 1) // 2))
    part = torch.empty(2 * blocks * C + lib.pdt_rows_reduce_workspace(blocks, C), dtype=torch.float32,
                       device=dout.device)
    rc = lib.pdt_maxpool_bwd_bnred(_p(dout), _p(idx), _p(dA), _p(u.y), _p(u.mean), _p(u.scale), _p(u.shift),
                                   _p(part), N, H, W, C, Ho, Wo, blocks, _s())
    if rc == NOT_APPLICABLE:
        return None
    _chk(rc, "maxpool_bwd_bnred")
    return _BnbPartials(part, blocks, u)


class _StemPool(torch.autograd.Function):
    """conv -> BN -> ReLU -> max-pool (the ResNet stem) with the BN apply folded into
    the max-pool: the full-resolution post-ReLU activation is never written or read.
    Backward: max-pool gradient -> BN backward (ReLU gate recomputed from y) -> weight
    gradient (and data gradient if the input needs one). PDT_STEM_POOL_BWD_FUSED=1 has
    the BN passes gather dA from the pool gradient and argmax instead (no
    full-resolution dA; measured no faster, so off by default)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, conv, bna, k, s, p):
        if _s2d_ok(x, conv) and not ctx.needs_input_grad[0]:
            u = _unit_fwd_s2d(x, w, gamma, beta, bna)
        else:
            _, u = _unit_fwd(x, w, gamma, beta, None, conv, True, bna, apply=False)
        N, C, H, W = u.N, u.Cout, u.g["Ho"], u.g["Wo"]
        Ho = (H + 2 * p - k) // s + 1
        Wo = (W + 2 * p - k) // s + 1
        assert u.y.shape == (N, C, H, W) and u.y.is_contiguous(memory_format=torch.channels_last)
        out = _empty_cl(N, C, Ho, Wo, torch.bfloat16, u.y.device)
        idx = torch.empty(N * Ho * Wo * C, dtype=torch.uint8, device=u.y.device)
        _chk(_load().pdt_maxpool_fwd_affine(_p(u.y), _p(out), _p(idx), _p(u.scale), _p(u.shift), N, H, W, C, Ho, Wo,
                                            k, s, p, _s()), "maxpool_fwd_affine")
        ctx.u = u
        ctx.meta = (N, C, H, W, Ho, Wo, k, s, p)
        ctx.save_for_backward(u.x, u.y, idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        u = ctx.u
        _, _, idx = ctx.saved_tensors
        N, C, H, W, Ho, Wo, k, s, p = ctx.meta
        dout = _cl(dout.to(torch.bfloat16))
        # off by default: measured equal to the composition (gathered reduce + apply 0.54 +
        # 0.66 ms vs maxpool_bwd + reduce + apply 0.44 + 0.31 + 0.46 ms at bs512, r59)
        if os.environ.get("PDT_STEM_POOL_BWD_FUSED", "0") == "1" and N * H * W * C < (1 << 34):
            dy, dgamma, dbeta = _bn_bwd_pool(dout, idx, u, k, s, p)
        else:
            dA = _empty_cl(N, C, H, W, torch.bfloat16, dout.device)
            s2d = u.g.get("s2d", False)
            fuse_red = s2d and ctx.needs_input_grad[1] and os.environ.get("PDT_STEM_WGRAD_BN", "1") == "1"
            pre = _pool_bwd_bnred(dout, idx, dA, u, k, s, p) if fuse_red else None
            if pre is None:
                _chk(_load().pdt_maxpool_bwd(_p(dout), _p(idx), _p(dA), N, H, W, C, Ho, Wo, k, s, p, _s()),
                     "maxpool_bwd")
            if fuse_red:
                # the stem's only consumer of dy is its weight gradient (no data gradient of the
                # image): the BN backward apply is formed in that GEMM's dY staging (tuned per shape)
                dgamma, dbeta, k1, k2, k3 = _bn_bwd(dA, u, False, coeffs_only=True, pre=pre)
                dw = _unit_dw_s2d(None, u, bn_dA=(dA, k1, k2, k3))
                del ctx.u
                return None, dw, dgamma, dbeta, None, None, None, None, None
            dy, _, dgamma, dbeta = _bn_bwd(dA, u, False)
        s2d = u.g.get("s2d", False)
        dx = _unit_dx(dy, u) if ctx.needs_input_grad[0] and not s2d else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = _unit_dw_s2d(dy, u) if s2d else _unit_dw(dy, u)
        del ctx.u
        return dx, dw, dgamma, dbeta, None, None, None, None, None


def stem_pool(x, conv: nn.Conv2d, bn: nn.BatchNorm2d, kernel_size=3, stride=2, padding=1):
    """max_pool2d(relu(bn(conv(x)))) as one node; None if the native path cannot run it."""
    if not supports_conv(x, conv) or conv.out_channels % 8:
        fallback("stem conv+bn+relu+maxpool", f"conv {tuple(conv.kernel_size)} on {tuple(x.shape)}")
        return None
    return _StemPool.apply(x, conv.weight, bn.weight, bn.bias, conv, _BNArgs(bn), kernel_size, stride, padding)


def max_pool2d(x, kernel_size=3, stride=2, padding=1):
    if x.dtype != torch.bfloat16 or x.shape[1] % 8:
        fallback("max_pool2d", f"{tuple(x.shape)} {x.dtype} (needs bf16, channels % 8 == 0)")
        return torch.nn.functional.max_pool2d(x, kernel_size, stride, padding)
    return _MaxPool.apply(x, kernel_size, stride, padding)


class _AvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        N, C, H, W = x.shape
        y = torch.empty((N, C), dtype=torch.bfloat16, device=x.device)
        _chk(_load().pdt_avgpool_fwd(_p(x), _p(y), N, H * W, C, _s()), "avgpool_fwd")
        ctx.meta = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = ctx.meta
        dy = dy.to(torch.bfloat16).contiguous()
        dx = _empty_cl(N, C, H, W, torch.bfloat16, dy.device)
        _chk(_load().pdt_avgpool_bwd(_p(dy), _p(dx), N, H * W, C, _s()), "avgpool_bwd")
        return dx


def global_avg_pool(x):
    if x.dtype != torch.bfloat16 or x.shape[1] % 8:
        fallback("global_avg_pool", f"{tuple(x.shape)} {x.dtype} (needs bf16, channels % 8 == 0)")
        return torch.flatten(torch.nn.functional.adaptive_avg_pool2d(x, 1), 1)
    return _AvgPool.apply(x)
