"""fused conv -> BN -> (+res) -> (ReLU): one "unit", with the BatchNorm apply and backward apply
folded into a consuming GEMM's A staging (AX)
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import autotune
from .conv import (_BnbPartials, _DGRAD_W, _conv_dgrad, _conv_forward, _conv_wgrad, _fwd_geom, _fwd_nt_geom,
                   supports_conv)
from .gemm import _AX_MAX_ELEMS, _check_addend
from .lib import _chk, _cl, _empty_cl, _grad_buf, _load, _p, _s, fallback
from .shadows import bf16_weight
from .tuning import NOT_APPLICABLE


class _BNArgs:
    """BatchNorm module state resolved for one call (training vs eval, running
    stats, num_batches_tracked handled inside the finalize kernel)."""
    __slots__ = ("training", "momentum", "eps", "rm", "rv", "nbt")

    def __init__(self, bn: nn.BatchNorm2d):
        self.training = bn.training or not bn.track_running_stats
        self.momentum = bn.momentum if bn.momentum is not None else 0.1
        self.eps = bn.eps
        self.rm = bn.running_mean if (bn.track_running_stats and bn.training) else None
        self.rv = bn.running_var if (bn.track_running_stats and bn.training) else None
        self.nbt = None
        if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
            self.nbt = bn.num_batches_tracked
            if bn.momentum is None:  # cumulative moving average needs the host-side count
                self.nbt.add_(1)
                self.momentum = 1.0 / float(self.nbt.item())
                self.nbt = None
        if not self.training:
            self.rm, self.rv = bn.running_mean, bn.running_var


class _Unit:
    """Saved state of one conv->BN->act unit between forward and backward."""
    __slots__ = ("x", "w", "gamma", "beta", "y", "act", "mask", "mean", "invstd", "scale", "shift", "N", "C", "Cs", "H",
                 "W", "Cout", "g", "relu", "has_res", "bnb_pre", "pend", "res_unit", "__weakref__")


def nhwc_padded_view(x, cp):
    """[N, cp, H, W] channels_last view of a [N, C, H, W] bf16 tensor that a loader
    built as a view into NHWC storage zero-padded to ``cp`` channels
    (``x.pdt_nhwc_pad == cp``); None when x is not such a view."""
    if getattr(x, "pdt_nhwc_pad", None) != cp or x.dtype != torch.bfloat16 or x.dim() != 4:
        return None
    N, C, H, W = x.shape
    if x.stride() != (H * W * cp, 1, W * cp, cp):
        return None
    if x.untyped_storage().nbytes() < (x.storage_offset() + N * H * W * cp) * 2:
        return None
    return torch.as_strided(x, (N, cp, H, W), (H * W * cp, 1, W * cp, cp))


def _unit_fwd(x, w, gamma, beta, residual, conv, relu, bna: _BNArgs, apply: bool = True, res_unit=None,
              src_pend=None, defer: bool = False):
    """conv -> BN (batch statistics from the conv epilogue) -> (+ residual) -> (ReLU).
    ``res_unit``: the residual is that unit's RAW conv output and its BN affine is applied
    inside this unit's BN apply (``residual`` must be ``res_unit.y``).
    ``defer``: skip the BN(+res)+ReLU element pass; the returned output buffer is still
    unwritten (``u.pend`` set) and the NEXT unit that reads it must be called with
    ``src_pend=u`` -- its 1x1 GEMM computes the apply in its A staging and writes the
    buffer (+ ReLU mask) once (``_conv_fwd_ax``), or the element pass runs first."""
    lib = _load()
    st = _s()
    N, C, H, W = x.shape
    Cs = C if C % 8 == 0 else 8
    xp = nhwc_padded_view(x, Cs) if Cs != C else None
    x = x.to(torch.bfloat16)
    if xp is not None:  # stem on a loader-padded NHWC batch: read in place
        x = xp
    elif Cs != C:  # stem: pad channels to 8 (NHWC)
        x = torch.nn.functional.pad(_cl(x).permute(0, 2, 3, 1), (0, Cs - C)).permute(0, 3, 1, 2)
    x = _cl(x)
    Cout = w.shape[0]
    g = _fwd_geom(N, H, W, Cs, conv)
    wb = bf16_weight(w, pad_cin_to=Cs if Cs != C else None)
    f32 = dict(dtype=torch.float32, device=x.device)
    M = N * g["Ho"] * g["Wo"]
    r = None
    if src_pend is not None and getattr(src_pend, "pend", None) is not None:
        assert src_pend.y.shape == x.shape and x.data_ptr() == src_pend.pend[2].data_ptr()
        r = _conv_fwd_ax(src_pend, x, wb, N, H, W, Cs, Cout, g, bna.training)
        if r is None:  # not covered by the AX tiles: the deferred element pass, then the plain GEMM
            _materialize(src_pend)
        src_pend.pend = None
    if r is None:
        r = _conv_forward(x, wb, N, H, W, Cs, Cout, g, with_stats=bna.training)
    y, _, part, R = r
    if bna.training:
        vec = torch.empty((4, Cout), **f32)
        mean, invstd, scale, shift = vec[0], vec[1], vec[2], vec[3]
        _chk(lib.pdt_bn_finalize(_p(part), R, Cout, float(M), float(bna.eps), float(bna.momentum), _p(gamma),
                                 _p(beta), _p(mean), _p(invstd), _p(scale), _p(shift), _p(bna.rm), _p(bna.rv),
                                 _p(bna.nbt), st), "bn_finalize")
    else:
        invstd = torch.rsqrt(bna.rv.float() + bna.eps)
        mean = bna.rm.float().clone()
        scale = (gamma.float() * invstd).contiguous()
        shift = (beta.float() - mean * scale).contiguous()
    assert y.numel() == M * Cout
    if not apply:  # the consumer applies the BN affine (+ReLU) itself (stem max-pool)
        u = _Unit()
        u.x, u.w, u.gamma, u.beta, u.y = x, w, gamma, beta, y
        u.act, u.mask, u.bnb_pre, u.pend, u.res_unit = None, None, None, None, None
        u.mean, u.invstd, u.scale, u.shift = mean, invstd, scale, shift
        u.N, u.C, u.Cs, u.H, u.W, u.Cout, u.g, u.relu, u.has_res = N, C, Cs, H, W, Cout, g, relu, False
        return None, u
    res = None
    if residual is not None:
        res = _cl(residual)
        assert res.dtype == torch.bfloat16 and res.shape == y.shape, (res.shape, y.shape)
    out = torch.empty_like(y, memory_format=torch.channels_last)
    # residual + ReLU: the backward's ReLU mask cannot be recomputed from y alone; keep it
    # as one bit per element instead of re-reading the bf16 output (1/16 of the bytes)
    mask = torch.empty(M * Cout // 8, dtype=torch.uint8, device=x.device) if (relu and residual is not None) \
        else None
    if res_unit is not None:
        assert residual is res_unit.y and res_unit.Cout == Cout
    u = _Unit()
    u.pend = None
    if defer and relu:
        u.pend = (res, res_unit, out)
    elif res_unit is not None:
        _chk(lib.pdt_bn_apply_res_affine(_p(y), _p(res), _p(out), _p(scale), _p(shift), _p(res_unit.scale),
                                         _p(res_unit.shift), M, Cout, int(relu), _p(mask), st), "bn_apply_res_affine")
    else:
        _chk(lib.pdt_bn_apply(_p(y), _p(res), _p(out), _p(scale), _p(shift), M, Cout, int(relu), _p(mask), st),
             "bn_apply")
    u.x, u.w, u.gamma, u.beta, u.y = x, w, gamma, beta, y
    u.act = None
    u.mask = mask
    u.res_unit = res_unit  # the downsample unit whose raw output is this unit's residual (or None)
    u.bnb_pre = None
    u.mean, u.invstd, u.scale, u.shift = mean, invstd, scale, shift
    u.N, u.C, u.Cs, u.H, u.W, u.Cout, u.g, u.relu, u.has_res = N, C, Cs, H, W, Cout, g, relu, residual is not None
    return out, u


def _bn_bwd(dA, u: _Unit, want_dres: bool, mask=None, pre: _BnbPartials | None = None, coeffs_only=False):
    """BN(+res)(+ReLU) backward: returns (dy, dres, dgamma, dbeta). ``mask`` (a ReLU bit
    mask of another unit's output) gates dA first -- the downsample branch of a bottleneck
    sees the block's ReLU exactly as the main branch does. ``pre``: the reduction was
    already done by the epilogue of the GEMM that produced dA (no reduce pass).
    ``coeffs_only``: stop before the apply pass, return (dgamma, dbeta, k1, k2, k3)."""
    lib = _load()
    st = _s()
    dA = _cl(dA.to(torch.bfloat16))
    Cout = u.Cout
    M = u.N * u.g["Ho"] * u.g["Wo"]
    f32 = dict(dtype=torch.float32, device=dA.device)
    if mask is None:
        mask = u.mask
    relu = u.relu or mask is not None
    if pre is not None:
        assert pre.unit is u
        part, blocks = pre.part, pre.R
    else:
        blocks = lib.pdt_bn_stats_blocks(M, Cout)
        part = torch.empty(2 * blocks * Cout + lib.pdt_rows_reduce_workspace(blocks, Cout), **f32)
        _chk(lib.pdt_bn_bwd_reduce(_p(dA), _p(u.y), _p(u.act), _p(u.mean), _p(u.scale), _p(u.shift), _p(part), M,
                                   Cout, int(relu), blocks, _p(mask), st), "bn_bwd_reduce")
    vec = torch.empty((3, Cout), **f32)
    k1, k2, k3 = vec[0], vec[1], vec[2]
    dgamma, dbeta = _grad_buf(u.gamma, (Cout,)), _grad_buf(u.beta, (Cout,))
    _chk(lib.pdt_bn_bwd_finalize(_p(part), blocks, Cout, float(M), _p(u.gamma), _p(u.mean), _p(u.invstd),
                                 _p(dgamma), _p(dbeta), _p(k1), _p(k2), _p(k3), 0, st), "bn_bwd_finalize")
    if coeffs_only:
        return dgamma, dbeta, k1, k2, k3
    dy = torch.empty_like(u.y, memory_format=torch.channels_last)
    dres = torch.empty_like(u.y, memory_format=torch.channels_last) if want_dres else None
    _chk(lib.pdt_bn_bwd_apply(_p(dA), _p(u.y), _p(u.act), _p(u.scale), _p(u.shift), _p(k1), _p(k2), _p(k3),
                              _p(dy), _p(dres), M, Cout, int(relu), _p(mask), st), "bn_bwd_apply")
    return dy, dres, dgamma, dbeta


def _bn_bwd_pool(dout, idx, u: _Unit, k, s, p):
    """Stem BN+ReLU backward reading dA straight from the max-pool output gradient
    and argmax (csrc/bn_act.hip ``pdt_bn_bwd_*_pool``): the full-resolution dA of
    the ``maxpool_bwd`` + ``_bn_bwd`` composition is never materialised."""
    lib = _load()
    st = _s()
    N, C, H, W = u.N, u.Cout, u.g["Ho"], u.g["Wo"]
    Ho, Wo = dout.shape[2], dout.shape[3]
    assert dout.is_contiguous(memory_format=torch.channels_last) and dout.dtype == torch.bfloat16
    assert idx.numel() == N * Ho * Wo * C and u.y.shape == (N, C, H, W)
    assert u.relu and u.act is None and u.mask is None
    M = N * H * W
    f32 = dict(dtype=torch.float32, device=dout.device)
    # the gathered reduce is latency-bound (argmax byte -> gradient load chains): far
    # more blocks in flight than the streaming reduce's 512
    rp = 256 // (C // 8)
    blocks = max(1, min(int(os.environ.get("PDT_POOL_BN_BLOCKS", "4096")), (M + rp - 1) // rp))
    part = torch.empty(2 * blocks * C + lib.pdt_rows_reduce_workspace(blocks, C), **f32)
    _chk(lib.pdt_bn_bwd_reduce_pool(_p(dout), _p(idx), _p(u.y), _p(u.mean), _p(u.scale), _p(u.shift), _p(part),
                                    N, H, W, C, Ho, Wo, k, s, p, blocks, st), "bn_bwd_reduce_pool")
    vec = torch.empty((3, C), **f32)
    k1, k2, k3 = vec[0], vec[1], vec[2]
    dgamma, dbeta = _grad_buf(u.gamma, (C,)), _grad_buf(u.beta, (C,))
    _chk(lib.pdt_bn_bwd_finalize(_p(part), blocks, C, float(M), _p(u.gamma), _p(u.mean), _p(u.invstd),
                                 _p(dgamma), _p(dbeta), _p(k1), _p(k2), _p(k3), 0, st), "bn_bwd_finalize")
    dy = torch.empty_like(u.y, memory_format=torch.channels_last)
    _chk(lib.pdt_bn_bwd_apply_pool(_p(dout), _p(idx), _p(u.y), _p(u.scale), _p(u.shift), _p(k1), _p(k2), _p(k3),
                                   _p(dy), N, H, W, C, Ho, Wo, k, s, p, st), "bn_bwd_apply_pool")
    return dy, dgamma, dbeta


def _unit_dx(dy, u: _Unit, addend=None, addend_mask=None, bnb_unit=None, bnb_mask=None, bnb_unit2=None):
    """Data gradient of unit ``u``'s conv. With ``bnb_unit`` (the unit whose output
    this gradient flows into) returns ``(dx, _BnbPartials)``."""
    wd = u.w
    if u.Cs != u.C:  # stem: dgrad against the channel-padded weight, then drop the pad
        wd = torch.nn.functional.pad(u.w.detach().float(), (0, 0, 0, 0, 0, u.Cs - u.C))
        assert addend is None and bnb_unit is None
    dx = _conv_dgrad(dy, wd, u.N, u.H, u.W, u.Cs, u.Cout, u.g, addend=addend, addend_mask=addend_mask,
                     bnb_unit=bnb_unit, bnb_mask=bnb_mask, bnb_unit2=bnb_unit2)
    return dx[:, :u.C] if u.Cs != u.C else dx


# -----------------------------------------------------------------------------
# BatchNorm apply folded into a 1x1 GEMM's A staging (csrc/conv_nt_kernel.h AXArgs):
# the BN'd tensor is produced by the GEMM that consumes it (and written once for its
# other consumers) instead of by an element pass + a re-read. PDT_FUSE_BN_AX=0 disables.
# -----------------------------------------------------------------------------
AX_VARIANTS = (0, 1, 3, 5, 6, 8, 10, 13, 15, 16, 18, 20, 23, 25, 26, 28, 30, 31)  # csrc/conv_igemm_ax.hip


def _ax_enabled() -> bool:
    return os.environ.get("PDT_FUSE_BN_AX", "1") != "0"


def _conv1_fold_enabled() -> bool:
    """bn1's backward apply in conv1's data gradient (PDT_FUSE_BN_AX1=0 disables)."""
    return os.environ.get("PDT_FUSE_BN_AX1", "1") != "0"


_NO_BNB = (None, None, None, None, None, None, 0, 0, 0)  # ``bnb`` of an AX launch without the BN-backward epilogue


def _ax_launch(lib, src, b, out, v, a, stats=None, bnb=None, ax=None):
    """One pdt_conv_nt_ax launch. ``bnb`` = (y, mean, scale, shift, mask, part, relu, row0, R) or None;
    ``ax`` = (mode, y2, c1, c2, c3, rsc, rsh, mask_in, mask_out, dst)."""
    bn = bnb if bnb is not None else _NO_BNB
    mode, y2, c1, c2, c3, rsc, rsh, mki, mko, dst = ax
    return lib.pdt_conv_nt_ax(_p(src), _p(b), _p(out), _p(stats), a["Hs"], a["Ws"], a["Cs"], a["Nimg"], a["Hm"],
                              a["Wm"], a["Ncol"], a["K"], a["ldb"], a["ldo"], int(v), _p(bn[0]), _p(bn[1]),
                              _p(bn[2]), _p(bn[3]), _p(bn[4]), _p(bn[5]), int(bn[6]), int(bn[7]), int(bn[8]),
                              int(mode), _p(y2), _p(c1), _p(c2), _p(c3), _p(rsc), _p(rsh), _p(mki), _p(mko), _p(dst),
                              _s())


def _ax2_launch(lib, src, b, out, v, a, stats=None, bnb=None, ax=None, addend=None, addend_mask=None):
    """``_ax_launch`` for any stride-1 geometry (``a`` as ``_fwd_nt_geom`` / ``_conv_dgrad`` build it);
    ``addend`` (+ ``addend_mask``): added in the fused BN-backward epilogue (modes 2 / 3)."""
    bn = bnb if bnb is not None else _NO_BNB
    mode, y2, c1, c2, c3, rsc, rsh, mki, mko, dst = ax
    return lib.pdt_conv_nt_ax3(
        _p(src), _p(b), _p(out), _p(stats), _p(addend), _p(addend_mask), a["Hs"], a["Ws"], a["Cs"], a["Nimg"], a["Hm"], a["Wm"], a["Ncol"], a["K"],
        a["ldb"], a["sh"], a["sw"], a["oh0"], a["ow0"], a["dh"], a["dw"], a["nth"], a["ntw"], a["Ho"], a["Wo"],
        a["osh"], a["osw"], a["oph"], a["opw"], a["ldo"], int(v), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]),
        _p(bn[4]), _p(bn[5]), int(bn[6]), int(bn[7]), int(bn[8]), int(mode), _p(y2), _p(c1), _p(c2), _p(c3), _p(rsc),
        _p(rsh), _p(mki), _p(mko), _p(dst), _s())


def _ax_select(key, run, run_ref=None):
    """Tile for an AX launch (tuned over the AX instantiations on first use when allowed);
    ``run(v)`` launches variant v (with the caller's scratch outputs) and returns its code.
    ``run_ref()``: the unfused alternative (element pass + the plain GEMM's tuned tile);
    when it is faster the key records ``AX_UNFUSED`` and the caller takes that path (the
    fold is a per-geometry tuning decision, not a blanket switch)."""
    return autotune.choose(key, lambda: (AX_VARIANTS, run), AX_VARIANTS[3],  # default: 128x128, one LDS stage
                           retune="PDT_RETUNE_AX", ref=run_ref)


def _conv3_dgrad_bn_bwd(dout, u3, k1, k2, k3, dy3, u2, side=None):
    """Data gradient of a bottleneck's conv3 (1x1) with bn3's backward apply folded into its A
    staging: A = dy3 = k1*gate(dout) + k2*y3 + k3 (gate: u3's ReLU bit mask), written to ``dy3``
    for the weight gradient; bn2's backward partials in the epilogue (as ``_unit_dx(...,
    bnb_unit=u2)``). Returns (da2, _BnbPartials) or None when the geometry is not covered.
    ``side`` = (ud, b1, b2, b3, dyd): a downsample block's shortcut BN backward, otherwise
    applied together with bn3's by ``pdt_bn_bwd_apply_dual``; here it runs as its own pass and
    the tuner compares (fold + that pass) against (dual pass + plain data gradient)."""
    N, Cout, H, W = u3.y.shape
    Cin = u3.C
    if u3.g["KH"] != 1 or u3.g["sh"] != 1 or u3.Cs != Cin or Cout % 64 or u2.Cout != Cin or u3.mask is None:
        return None
    lib = _load()
    wt = _DGRAD_W.get(u3.w, Cout, 1, 1, Cin, 0, 0, 1, 1, 1)
    da2 = _empty_cl(N, Cin, H, W, torch.bfloat16, dout.device)
    a = dict(Hs=H, Ws=W, Cs=Cout, Nimg=N, Hm=H, Wm=W, Ncol=Cin, K=Cout, ldb=Cout, ldo=Cin)
    M = N * H * W
    assert u2.y.shape == da2.shape and u2.y.is_contiguous(memory_format=torch.channels_last)
    ax = (2, u3.y, k1, k2, k3, None, None, u3.mask, None, dy3)

    def bnb(part, R):
        return (u2.y, u2.mean, u2.scale, u2.shift, None, part, 1, 0, R)

    def run(v):
        R = lib.pdt_conv_nt_bnb_rows(M, Cin, Cout, v)
        part = torch.empty(2 * R * Cin, dtype=torch.float32, device=dout.device)
        return _ax_launch(lib, dout, wt, da2, v, a, bnb=bnb(part, R), ax=ax)

    def side_apply():
        ud, b1, b2, b3, dyd = side
        _chk(lib.pdt_bn_bwd_apply(_p(dout), _p(ud.y), None, None, None, _p(b1), _p(b2), _p(b3), _p(dyd), None, M,
                                  Cout, 1, _p(u3.mask), _s()), "bn_bwd_apply (shortcut)")

    def run_ref():
        if side is None:
            _chk(lib.pdt_bn_bwd_apply(_p(dout), _p(u3.y), None, None, None, _p(k1), _p(k2), _p(k3), _p(dy3), None,
                                      M, Cout, 1, _p(u3.mask), _s()), "bn_bwd_apply")
        else:
            ud, b1, b2, b3, dyd = side
            _chk(lib.pdt_bn_bwd_apply_dual(_p(dout), _p(u3.mask), _p(u3.y), _p(k1), _p(k2), _p(k3), _p(dy3),
                                           _p(ud.y), _p(b1), _p(b2), _p(b3), _p(dyd), M, Cout, _s()),
                 "bn_bwd_apply_dual")
        _unit_dx(dy3, u3, bnb_unit=u2)

    def run_tuned(v):
        rc = run(v)
        if rc == 0 and side is not None:
            side_apply()
        return rc

    v = _ax_select(autotune.axb_key(H, W, Cout, N, Cin, side is not None), run_tuned, run_ref)
    if v < 0:
        return None
    R = lib.pdt_conv_nt_bnb_rows(M, Cin, Cout, v)
    part = torch.empty(2 * R * Cin + lib.pdt_rows_reduce_workspace(R, Cin), dtype=torch.float32, device=dout.device)
    rc = _ax_launch(lib, dout, wt, da2, v, a, bnb=bnb(part, R), ax=ax)
    if rc == NOT_APPLICABLE:
        return None
    _chk(rc, "conv_nt_ax (bn3 backward apply + conv3 dgrad)")
    if side is not None:
        side_apply()
    return da2, _BnbPartials(part, R, u2)


def _materialize(u: _Unit):
    """The deferred BN(+res)+ReLU element pass of unit ``u`` (see ``_unit_fwd(defer=True)``)."""
    _apply_pending(u)
    u.pend = None


def _apply_pending(u: _Unit):
    res, ru, out = u.pend
    lib = _load()
    M = u.y.numel() // u.Cout
    if ru is not None:
        _chk(lib.pdt_bn_apply_res_affine(_p(u.y), _p(res), _p(out), _p(u.scale), _p(u.shift), _p(ru.scale),
                                         _p(ru.shift), M, u.Cout, 1, _p(u.mask), _s()), "bn_apply_res_affine")
    else:
        _chk(lib.pdt_bn_apply(_p(u.y), _p(res), _p(out), _p(u.scale), _p(u.shift), M, u.Cout, 1, _p(u.mask), _s()),
             "bn_apply")


def _conv_fwd_ax(pu: _Unit, xbuf, wb, N, H, W, Cs, Cout, g, with_stats):
    """Forward stride-1 conv (1x1, or 3x3 'same') whose A operand is unit ``pu``'s deferred output
    relu(bn(pu.y) [+ res]), computed in the A staging (AX mode 1) and written to ``xbuf``
    (+ pu.mask) on the way. Returns ``_conv_forward``'s (y, M, part, R), or None when the
    geometry is not covered."""
    res, ru, _ = pu.pend
    Ho, Wo = g["Ho"], g["Wo"]
    M = N * Ho * Wo
    if g["sh"] != 1 or g["sw"] != 1 or Ho != H or Wo != W or Cs != pu.Cout or Cs % 64 or Cout % 8 or \
            N * H * W * Cs >= _AX_MAX_ELEMS or not pu.relu:
        return None
    lib = _load()
    y = _empty_cl(N, Cout, Ho, Wo, torch.bfloat16, xbuf.device)
    a = _fwd_nt_geom(N, H, W, Cs, Cout, g)
    K = a["K"]
    ax = (1, res, pu.scale, pu.shift, None, ru.scale if ru is not None else None,
          ru.shift if ru is not None else None, None, pu.mask, xbuf)

    def stats(v, tail):
        if not with_stats:
            return None, 0
        R = lib.pdt_conv_nt_stat_rows(M, Cout, K, v)
        ws = lib.pdt_rows_reduce_workspace(R, Cout) if tail else 0
        return torch.empty(2 * R * Cout + ws, dtype=torch.float32, device=xbuf.device), R

    def run(v):
        return _ax2_launch(lib, pu.y, wb, y, v, a, stats=stats(v, False)[0], ax=ax)

    def run_ref():
        _apply_pending(pu)
        _conv_forward(xbuf, wb, N, H, W, Cs, Cout, g, with_stats=with_stats)

    key = autotune.axf_key(H, W, Cs, N, Cout, res is not None, ru is not None, with_stats, g["KH"], g["KW"], g["ph"])
    v = _ax_select(key, run, run_ref)
    if v < 0:
        return None
    part, R = stats(v, True)
    rc = _ax2_launch(lib, pu.y, wb, y, v, a, stats=part, ax=ax)
    if rc == NOT_APPLICABLE:
        return None
    _chk(rc, "conv_nt_ax (deferred BN apply + conv)")
    return y, M, part, R


def _conv2_dgrad_bn_bwd(da2, u2, k1, k2, k3, dy2, u1, bnb_mask=None, addend=None, addend_mask=None):
    """Data gradient of a bottleneck's stride-1 conv2 (3x3) with bn2's backward apply folded into
    its A staging (AX mode 3: dy2 = k1*gate(da2) + k2*y2 + k3, the ReLU gate recomputed from y2
    as ``pdt_bn_bwd_apply`` does), dy2 written once (centre tap) for the weight gradient; bn1's
    backward partials in the epilogue. Returns (da1, _BnbPartials) or None (not covered / the
    element pass + plain data gradient tuned faster).
    The same fold serves conv1's data gradient (``u2`` = the block's conv1 unit, ``u1`` = the
    previous block's conv3 unit, ``bnb_mask`` = its ReLU bit mask): there the epilogue also adds
    the shortcut gradient ``addend`` (gated by ``addend_mask``), as ``_unit_dx`` does."""
    g = u2.g
    N, Cout, Ho, Wo = u2.y.shape
    Cin = u2.C
    if g["sh"] != 1 or g["sw"] != 1 or Ho != u2.H or Wo != u2.W or u2.Cs != Cin or Cout % 64 or u1.Cout != Cin or \
            u2.mask is not None or not u2.relu or N * Ho * Wo * Cout >= _AX_MAX_ELEMS:
        return None
    KH, KW, ph, pw = g["KH"], g["KW"], g["ph"], g["pw"]
    lib = _load()
    wt = _DGRAD_W.get(u2.w, Cout, KH, KW, Cin, 0, 0, 1, KH, KW)
    da1 = _empty_cl(N, Cin, u2.H, u2.W, torch.bfloat16, da2.device)
    a = dict(Hs=Ho, Ws=Wo, Cs=Cout, Nimg=N, Hm=u2.H, Wm=u2.W, Ncol=Cin, K=KH * KW * Cout, ldb=KH * KW * Cout, sh=1,
             sw=1, oh0=ph, ow0=pw, dh=-1, dw=-1, nth=KH, ntw=KW, Ho=u2.H, Wo=u2.W, osh=1, osw=1, oph=0, opw=0,
             ldo=Cin)
    M = N * u2.H * u2.W
    ax = (3, u2.y, k1, k2, k3, u2.scale, u2.shift, None, None, dy2)
    if addend is not None:
        _check_addend(addend, da1, addend_mask, Cin)
    if bnb_mask is not None:
        assert bnb_mask.dtype == torch.uint8 and bnb_mask.numel() * 8 == da1.numel()

    def bnb(part, R):
        return (u1.y, u1.mean, u1.scale, u1.shift, bnb_mask, part, 1, 0, R)

    def run(v):
        R = lib.pdt_conv_nt_bnb_rows(M, Cin, a["K"], v)
        part = torch.empty(2 * R * Cin, dtype=torch.float32, device=da2.device)
        return _ax2_launch(lib, da2, wt, da1, v, a, bnb=bnb(part, R), ax=ax, addend=addend, addend_mask=addend_mask)

    def run_ref():
        _chk(lib.pdt_bn_bwd_apply(_p(da2), _p(u2.y), None, _p(u2.scale), _p(u2.shift), _p(k1), _p(k2), _p(k3),
                                  _p(dy2), None, N * Ho * Wo, Cout, 1, None, _s()), "bn_bwd_apply")
        _unit_dx(dy2, u2, addend=addend, addend_mask=addend_mask, bnb_unit=u1, bnb_mask=bnb_mask)

    key = autotune.ax3_key(Ho, Wo, Cout, N, Cin, KH, KW, ph, addend is not None, addend_mask is not None,
                           bnb_mask is not None)
    v = _ax_select(key, run, run_ref)
    if v < 0:
        return None
    R = lib.pdt_conv_nt_bnb_rows(M, Cin, a["K"], v)
    part = torch.empty(2 * R * Cin + lib.pdt_rows_reduce_workspace(R, Cin), dtype=torch.float32, device=da2.device)
    rc = _ax2_launch(lib, da2, wt, da1, v, a, bnb=bnb(part, R), ax=ax, addend=addend, addend_mask=addend_mask)
    if rc == NOT_APPLICABLE:
        return None
    _chk(rc, "conv_nt_ax (BN backward apply + conv dgrad)")
    return da1, _BnbPartials(part, R, u1)


def _unit_dw(dy, u: _Unit):
    w = u.w
    KH, KW = u.g["KH"], u.g["KW"]
    if u.Cs == u.C and w.is_contiguous(memory_format=torch.channels_last):
        dw = _grad_buf(w, tuple(w.shape), torch.channels_last)
        _conv_wgrad(dy, u.x, u.N, u.H, u.W, u.Cs, u.Cout, u.g, dw)
    else:
        tmp = torch.empty((u.Cout, u.Cs, KH, KW), dtype=torch.float32, device=dy.device,
                          memory_format=torch.channels_last)
        _conv_wgrad(dy, u.x, u.N, u.H, u.W, u.Cs, u.Cout, u.g, tmp)
        dw = _grad_buf(w, tuple(w.shape), torch.channels_last).copy_(tmp[:, :u.C]) if u.Cs != u.C else tmp
    return dw.to(w.dtype) if dw.dtype != w.dtype else dw


class _ConvBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, residual, conv, relu, bna):
        out, u = _unit_fwd(x, w, gamma, beta, residual, conv, relu, bna)
        ctx.u = u
        ctx.save_for_backward(u.x, u.y, u.mask)  # version-checked activations
        return out

    @staticmethod
    def backward(ctx, dA):
        u = ctx.u
        dy, dres, dgamma, dbeta = _bn_bwd(dA, u, u.has_res)
        dx = _unit_dx(dy, u) if ctx.needs_input_grad[0] else None
        dw = _unit_dw(dy, u) if ctx.needs_input_grad[1] else None
        del ctx.u
        return (dx, dw, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None,
                dres, None, None, None)


def conv_bn_act(x, conv: nn.Conv2d, bn: nn.BatchNorm2d, residual=None, relu=True):
    if not supports_conv(x, conv) or (residual is not None and residual.dtype != torch.bfloat16):
        fallback("conv_bn_act", f"conv {tuple(conv.kernel_size)}/{tuple(conv.stride)} groups={conv.groups} "
                                f"bias={conv.bias is not None} on {tuple(x.shape)} {x.dtype}")
        from ..fused import _torch_conv_bn_act
        return _torch_conv_bn_act(x, conv, bn, residual, relu)
    return _ConvBNAct.apply(x, conv.weight, bn.weight, bn.bias, residual, conv, relu, _BNArgs(bn))
