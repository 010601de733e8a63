"""fused ResNet bottleneck: conv1-bn1-relu -> conv2-bn2-relu -> conv3-bn3 (+ identity
or downsample conv-bn) -> relu, with a hand-scheduled backward: the block-input
gradient is produced by ONE data-gradient GEMM whose epilogue adds the
identity / downsample branch gradient (no separate add pass).
"""
from __future__ import annotations

import os
import weakref

import torch

from .bn_unit import (_BNArgs, _ax_enabled, _bn_bwd, _conv1_fold_enabled, _conv2_dgrad_bn_bwd, _conv3_dgrad_bn_bwd,
                      _materialize, _unit_dw, _unit_dx, _unit_fwd)
from .conv import _bnb2_enabled, _bnb_enabled, supports_conv
from .lib import _chk, _cl, _load, _p, _s, fallback

# Cross-block fusion of the BatchNorm-backward reduction. Block k's output is
# block k+1's input; block k+1's backward produces that gradient with ONE dgrad
# GEMM (+ shortcut addend), so its epilogue also computes block k's bn3
# backward partials (gated by block k's ReLU bit mask). Forward records which
# unit produced each block output; backward leaves the partials on that unit,
# tagged with the gradient tensor's storage and version -- block k's backward
# uses them only if the gradient it receives is exactly that tensor.
_PRODUCERS: dict = {}


def _note_producer(out, u):
    if len(_PRODUCERS) > 64:
        for k in [k for k, e in _PRODUCERS.items() if e[0]() is None]:
            del _PRODUCERS[k]
    _PRODUCERS[out.data_ptr()] = (weakref.ref(u), tuple(out.shape), out.stride(), out._version)


def _producer_of(x):
    e = _PRODUCERS.get(x.data_ptr())
    if e is None:
        return None
    u = e[0]()
    if u is None or e[1] != tuple(x.shape) or e[2] != x.stride() or e[3] != x._version:
        return None
    return u


def _take_bnb(u, grad):
    """Partials a later block's epilogue left for unit ``u``, if ``grad`` is that output."""
    st, u.bnb_pre = u.bnb_pre, None
    if st is None or st[0] != grad.data_ptr() or st[1] != grad._version or st[2] != tuple(grad.shape):
        return None
    return st[3]


# (Weight gradients on a side HIP stream beside the data-gradient chain were an opt-in switch
# through round 5: +0.4 % / -0.3 % at bs 512 / 256, and at bs 2048 on the round-6 tree 1 163 vs
# 14 573 img/s -- the stream-recorded blocks of the 85-GiB step kept the caching allocator from
# reusing memory (profiles/bench_runs_round6.jsonl, call q04). Removed: one stream.)


class _Bottleneck(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, blk, has_ds, xpend, defer, holder, *params):
        # xpend: the previous block's unit whose output x is still unwritten (its bn3 apply is
        # computed in conv1's A staging, which writes x); conv1 therefore runs first
        fold = _ax_enabled()
        # bn1's apply+ReLU inside conv2's A staging when conv2 is stride 1 (a1 written once, at
        # the centre tap, for conv2's weight gradient); otherwise materialised before conv2
        a1, u1 = _unit_fwd(x, blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, None, blk.conv1, True,
                           _BNArgs(blk.bn1), src_pend=xpend, defer=fold)
        if has_ds:  # raw downsample conv output; its BN affine is applied inside bn3's apply
            _, ud = _unit_fwd(x, blk.downsample[0].weight, blk.downsample[1].weight, blk.downsample[1].bias, None,
                              blk.downsample[0], False, _BNArgs(blk.downsample[1]), apply=False)
            idn = ud.y
        else:
            idn, ud = _cl(x.to(torch.bfloat16)), None
        # bn2's apply+ReLU inside conv3's A staging (a2 written once, for conv3's weight gradient)
        a2, u2 = _unit_fwd(a1, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias, None, blk.conv2, True,
                           _BNArgs(blk.bn2), src_pend=u1, defer=fold)
        out, u3 = _unit_fwd(a2, blk.conv3.weight, blk.bn3.weight, blk.bn3.bias, idn, blk.conv3, True,
                            _BNArgs(blk.bn3), res_unit=ud, src_pend=u2, defer=defer and fold)
        if holder is not None:
            holder[0] = u3 if u3.pend is not None else None
        ctx.units = (u1, u2, u3, ud)
        ctx.has_ds = has_ds
        prev = _producer_of(x) if _bnb_enabled() else None
        ctx.prev = weakref.ref(prev) if prev is not None else None
        ctx.save_for_backward(u1.x, u1.y, u2.y, u3.y, u3.mask)
        _note_producer(out, u3)
        return out

    @staticmethod
    def backward(ctx, dout):
        u1, u2, u3, ud = ctx.units
        need = ctx.needs_input_grad
        dout = _cl(dout.to(torch.bfloat16))
        # bn3's backward partials from the next block's data-gradient epilogue (and, in a
        # downsample block, the shortcut BN's from the same epilogue: same gated gradient)
        pre3 = _take_bnb(u3, dout)
        pre_d = pre3.second if (pre3 is not None and pre3.second is not None and pre3.second.unit is ud) else None
        dual = ctx.has_ds and u3.mask is not None and os.environ.get("PDT_BN_DUAL_APPLY", "1") == "1"
        if dual:
            # both BN backwards fed by dout (bn3 and the shortcut's BN): coefficients first, then
            # ONE apply pass that reads dout and the ReLU mask once and writes both gradients
            dg3, db3, a1, a2, a3 = _bn_bwd(dout, u3, False, pre=pre3, coeffs_only=True)
            dgd, dbd, b1, b2, b3 = _bn_bwd(dout, ud, False, mask=u3.mask, pre=pre_d, coeffs_only=True)
            dy3 = torch.empty_like(u3.y, memory_format=torch.channels_last)
            dyd = torch.empty_like(ud.y, memory_format=torch.channels_last)
            fused3 = None
            if _bnb_enabled() and _ax_enabled():  # bn3's half in conv3's A staging (when it wins)
                fused3 = _conv3_dgrad_bn_bwd(dout, u3, a1, a2, a3, dy3, u2, side=(ud, b1, b2, b3, dyd))
            if fused3 is None:
                M3 = u3.N * u3.g["Ho"] * u3.g["Wo"]
                _chk(_load().pdt_bn_bwd_apply_dual(_p(dout), _p(u3.mask), _p(u3.y), _p(a1), _p(a2), _p(a3),
                                                   _p(dy3), _p(ud.y), _p(b1), _p(b2), _p(b3), _p(dyd), M3, u3.Cout,
                                                   _s()), "bn_bwd_apply_dual")
        else:
            fused3 = None
        fuse = _bnb_enabled()
        if not dual and fuse and _ax_enabled() and u3.mask is not None:
            # bn3's backward apply inside conv3's data-gradient A staging (dy3 written once, for
            # the weight gradient): no separate element pass, no re-read of dy3 by the dgrad
            dg3, db3, k1, k2, k3 = _bn_bwd(dout, u3, False, pre=pre3, coeffs_only=True)
            dy3 = torch.empty_like(u3.y, memory_format=torch.channels_last)
            fused3 = _conv3_dgrad_bn_bwd(dout, u3, k1, k2, k3, dy3, u2)
            if fused3 is None:  # not covered: the element pass
                _chk(_load().pdt_bn_bwd_apply(_p(dout), _p(u3.y), None, _p(u3.scale), _p(u3.shift), _p(k1), _p(k2),
                                              _p(k3), _p(dy3), None, u3.y.numel() // u3.Cout, u3.Cout, 1,
                                              _p(u3.mask), _s()), "bn_bwd_apply")
        elif not dual:
            dy3, _, dg3, db3 = _bn_bwd(dout, u3, False, pre=pre3)
        if fused3 is not None:
            da2, pre2 = fused3
        elif fuse:  # bn2 / bn1 backward reductions in the epilogues of the conv3 / conv2 dgrads
            da2, pre2 = _unit_dx(dy3, u3, bnb_unit=u2)
        else:
            da2, pre2 = _unit_dx(dy3, u3), None
        dw3 = _unit_dw(dy3, u3)
        fused2 = None
        if fuse and _ax_enabled():
            # bn2's backward apply inside conv2's data gradient (stride-1 conv2; tuned per shape)
            dg2, db2, c1, c2, c3 = _bn_bwd(da2, u2, False, pre=pre2, coeffs_only=True)
            dy2 = torch.empty_like(u2.y, memory_format=torch.channels_last)
            fused2 = _conv2_dgrad_bn_bwd(da2, u2, c1, c2, c3, dy2, u1)
            if fused2 is None:
                _chk(_load().pdt_bn_bwd_apply(_p(da2), _p(u2.y), None, _p(u2.scale), _p(u2.shift), _p(c1), _p(c2),
                                              _p(c3), _p(dy2), None, u2.y.numel() // u2.Cout, u2.Cout, 1, None,
                                              _s()), "bn_bwd_apply")
        else:
            dy2, _, dg2, db2 = _bn_bwd(da2, u2, False, pre=pre2)
        if fused2 is not None:
            da1, pre1 = fused2
        elif fuse:
            da1, pre1 = _unit_dx(dy2, u2, bnb_unit=u1)
        else:
            da1, pre1 = _unit_dx(dy2, u2), None
        dw2 = _unit_dw(dy2, u2)
        prev = ctx.prev() if ctx.prev is not None else None
        fold1 = fuse and _ax_enabled() and need[0] and prev is not None and prev.mask is not None and \
            prev.Cout == u1.C and u1.Cs == u1.C and _conv1_fold_enabled()
        if fold1:  # bn1's backward apply inside conv1's data gradient (below)
            dg1, db1, e1, e2, e3 = _bn_bwd(da1, u1, False, pre=pre1, coeffs_only=True)
            dy1 = torch.empty_like(u1.y, memory_format=torch.channels_last)
        else:
            dy1, _, dg1, db1 = _bn_bwd(da1, u1, False, pre=pre1)
        grads_ds = ()
        # shortcut gradient = dout * relu_mask(out): never materialised -- the downsample
        # BN backward gates dout with the mask itself, and an identity shortcut is added
        # (masked) by the epilogue of the block-input dgrad GEMM
        addend_mask = None
        if ctx.has_ds:
            if not dual:
                dyd, _, dgd, dbd = _bn_bwd(dout, ud, False, mask=u3.mask, pre=pre_d)
            addend = _unit_dx(dyd, ud) if need[0] else None
            dwd = _unit_dw(dyd, ud)
            grads_ds = (dwd, dgd, dbd)
        else:
            addend, addend_mask = dout, u3.mask
        dx = None
        if fold1:
            r1 = _conv2_dgrad_bn_bwd(da1, u1, e1, e2, e3, dy1, prev, bnb_mask=prev.mask, addend=addend,
                                     addend_mask=addend_mask)
            if r1 is not None:
                dx, pre = r1
                prev.bnb_pre = (dx.data_ptr(), dx._version, tuple(dx.shape), pre)
            else:  # not covered / tuned slower: the element pass, then the plain data gradient below
                _chk(_load().pdt_bn_bwd_apply(_p(da1), _p(u1.y), None, _p(u1.scale), _p(u1.shift), _p(e1), _p(e2),
                                              _p(e3), _p(dy1), None, u1.y.numel() // u1.Cout, u1.Cout, 1, None,
                                              _s()), "bn_bwd_apply")
        if dx is not None:
            pass
        elif need[0] and prev is not None and prev.mask is not None and prev.Cout == u1.C and u1.Cs == u1.C:
            # the previous block's bn3 backward partials from this epilogue (and its shortcut
            # BN's, when it is a downsample block)
            dx, pre = _unit_dx(dy1, u1, addend=addend, addend_mask=addend_mask, bnb_unit=prev, bnb_mask=prev.mask,
                               bnb_unit2=prev.res_unit if _bnb2_enabled() else None)
            prev.bnb_pre = (dx.data_ptr(), dx._version, tuple(dx.shape), pre)
        elif need[0]:
            dx = _unit_dx(dy1, u1, addend=addend, addend_mask=addend_mask)
        dw1 = _unit_dw(dy1, u1)
        del ctx.units
        return (dx, None, None, None, None, None, dw1, dg1, db1, dw2, dg2, db2, dw3, dg3, db3) + grads_ds


def _bottleneck_params(blk):
    params = [blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias,
              blk.conv3.weight, blk.bn3.weight, blk.bn3.bias]
    if blk.downsample is not None:
        params += [blk.downsample[0].weight, blk.downsample[1].weight, blk.downsample[1].bias]
    return params


def _bottleneck_ok(x, blk):
    convs = [blk.conv1, blk.conv2, blk.conv3] + ([blk.downsample[0]] if blk.downsample is not None else [])
    return x.dtype == torch.bfloat16 and all(supports_conv(x, c) for c in convs) and x.shape[1] % 8 == 0


def bottleneck(x, blk):
    if not _bottleneck_ok(x, blk):
        fallback("bottleneck", f"input {tuple(x.shape)} {x.dtype} (needs bf16, channels % 8 == 0, "
                               "plain convs)")
        return None
    return _Bottleneck.apply(x, blk, blk.downsample is not None, None, False, None, *_bottleneck_params(blk))


def bottleneck_chain(x, blocks):
    """A sequence of bottleneck blocks, one autograd node per block (DDP's per-parameter
    gradient hooks keep firing block by block), with each block's final BN(+residual)+ReLU
    element pass deferred into the NEXT block's conv1: that 1x1 GEMM computes the block
    output in its A staging and writes it (+ ReLU bit mask) once for the shortcut and the
    backward -- one full read of every block output per step saved. The deferred output is
    only ever read by the next block of this chain, which runs immediately after; the last
    block's output is materialised normally. Returns ``(y, n)``: ``blocks[:n]`` ran here
    (n < len(blocks) when block n is not covered -- the caller runs the rest)."""
    blocks = list(blocks)
    pend = None
    for i, blk in enumerate(blocks):
        if not _bottleneck_ok(x, blk):
            assert pend is None
            return x, i
        holder = [None]
        defer = i + 1 < len(blocks)
        x = _Bottleneck.apply(x, blk, blk.downsample is not None, pend, defer, holder, *_bottleneck_params(blk))
        pend = holder[0]
        if pend is not None and not _bottleneck_ok(x, blocks[i + 1]):
            _materialize(pend)
            pend = None
    assert pend is None
    return x, len(blocks)
