"""conv geometry helpers; conv forward, data gradient (with the fused BN-backward epilogue)
and weight gradient
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import autotune
from .gemm import _check_addend, _check_nt, conv_nt, conv_stat_rows, conv_wgrad, select_nt_variant
from .lib import _chk, _cl, _empty_cl, _load, _p, _s
from .tuning import NOT_APPLICABLE, _tuned


def _fwd_geom(N, H, W, Cs, conv: nn.Conv2d):
    KH, KW = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding
    Ho = (H + 2 * ph - KH) // sh + 1
    Wo = (W + 2 * pw - KW) // sw + 1
    return dict(KH=KH, KW=KW, sh=sh, sw=sw, ph=ph, pw=pw, Ho=Ho, Wo=Wo)


def supports_conv(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    if conv.groups != 1 or conv.dilation != (1, 1) or conv.bias is not None:
        return False
    if x.dim() != 4 or conv.out_channels % 8 != 0:
        return False
    N, C, H, W = x.shape
    if C % 8 != 0 and C > 8:
        return False
    sh, sw = conv.stride
    if (H % sh) or (W % sw):
        return False
    return True


def _fwd_nt_geom(N, H, W, Cs, Cout, g):
    K = g["KH"] * g["KW"] * Cs
    return dict(Hs=H, Ws=W, Cs=Cs, Nimg=N, Hm=g["Ho"], Wm=g["Wo"], Ncol=Cout, K=K, ldb=K, sh=g["sh"], sw=g["sw"],
                oh0=-g["ph"], ow0=-g["pw"], dh=1, dw=1, nth=g["KH"], ntw=g["KW"], Ho=g["Ho"], Wo=g["Wo"], osh=1,
                osw=1, oph=0, opw=0, ldo=Cout)


def _conv_forward(x, wb, N, H, W, Cs, Cout, g, with_stats=False):
    """Forward conv; returns (y, M, stats_partials or None, stats_rows)."""
    M = N * g["Ho"] * g["Wo"]
    y = _empty_cl(N, Cout, g["Ho"], g["Wo"], torch.bfloat16, x.device)
    a = _fwd_nt_geom(N, H, W, Cs, Cout, g)
    v = select_nt_variant(x, wb, y, with_stats=with_stats, **a)
    part, R = None, 0
    if with_stats:
        lib = _load()
        R = conv_stat_rows(M, Cout, a["K"], v)
        part = torch.empty(2 * R * Cout + lib.pdt_rows_reduce_workspace(R, Cout), dtype=torch.float32,
                           device=x.device)
    conv_nt(x, wb, y, stats=part, variant=v, **a)
    return y, M, part, R


class _DgradWeights:
    """Cache of the transposed, stride-phase-sliced bf16 weights the dgrad GEMMs
    consume (pdt_wt_dgrad layout), keyed per (parameter, phase). When the
    optimizer has stepped (parameter version changed), the FIRST request
    rebuilds every registered entry in ONE multi-tensor launch
    (pdt_wt_dgrad_multi) instead of one small kernel per conv and phase."""

    def __init__(self):
        self.entries = {}   # key -> [weakref(param), buf, version, job-tuple, data_ptr]
        self.table = None   # device job table (uint8) for the current entry set
        self.total = 0

    def get(self, param, Cout, KH, KW, Cin, kh0, kw0, s, nth, ntw):
        key = (id(param), param.data_ptr(), kh0, kw0, s, nth, ntw)
        ent = self.entries.get(key)
        if ent is not None and ent[0]() is param and ent[2] == param._version:
            return ent[1]
        lib = _load()
        if (ent is None or ent[0]() is not param) and len(self.entries) >= 512:
            self.entries.clear()  # device job table holds at most 512 entries
            self.table = None
        if ent is None or ent[0]() is not param:
            import weakref
            buf = torch.empty(max(Cin * nth * ntw * Cout, 8), dtype=torch.bfloat16, device=param.device)
            _chk(lib.pdt_wt_dgrad(_p(param), _p(buf), Cout, KH, KW, Cin, kh0, kw0, s, nth, ntw, _s()), "wt_dgrad")
            self.entries[key] = [weakref.ref(param), buf, param._version, (Cout, KH, KW, Cin, kh0, kw0, s, nth, ntw),
                                 param.data_ptr()]
            self.table = None
            return buf
        self._rebuild_all(lib)
        return ent[1]

    def _rebuild_all(self, lib):
        # drop entries whose parameter died or moved (their pointers must never reach the kernel)
        dead = [k for k, e in self.entries.items() if e[0]() is None or e[0]().data_ptr() != e[4]]
        for k in dead:
            del self.entries[k]
            self.table = None
        if self.table is None:
            import struct
            assert lib.pdt_wt_job_size() == 64
            blob, start = bytearray(), 0
            for ref, buf, _, j, ptr in self.entries.values():
                blob += struct.pack("<QQq10i", ptr, buf.data_ptr(), start, *j, 0)
                start += j[3] * j[7] * j[8] * j[0]
            dev = next(iter(self.entries.values()))[1].device
            self.table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
            self.total = start
        _chk(lib.pdt_wt_dgrad_multi(_p(self.table), len(self.entries), self.total, _s()), "wt_dgrad_multi")
        for ent in self.entries.values():
            ent[2] = ent[0]()._version


_DGRAD_W = _DgradWeights()


class _BnbPartials:
    """BatchNorm-backward partial sums produced by a data-gradient epilogue for one
    unit (see ``BnbArgs`` in csrc/conv_igemm.hip): [2][R][C] fp32 (+ rows_reduce tail).
    ``second``: the same epilogue's partials for a second unit fed by the same gated
    gradient (a downsample block's shortcut BN), or None."""
    __slots__ = ("part", "R", "unit", "second")

    def __init__(self, part, R, unit, second=None):
        self.part, self.R, self.unit, self.second = part, R, unit, second


def _bnb_enabled() -> bool:
    return os.environ.get("PDT_FUSE_BN_BWD", "1") != "0"


def _bnb2_enabled() -> bool:
    """A downsample block's shortcut-BN backward partials in the next block's data-gradient
    epilogue (PDT_FUSE_BN_BWD2=0: its own reduce pass over dout and the shortcut output)."""
    return os.environ.get("PDT_FUSE_BN_BWD2", "1") != "0"


def _conv_dgrad(dy, w32, N, H, W, Cin, Cout, g, addend=None, addend_mask=None, bnb_unit=None, bnb_mask=None,
                bnb_unit2=None):
    """dX [N,Cin,H,W] (+ addend) from dY [N,Cout,Ho,Wo] (stride phases, see csrc/conv_igemm.hip).

    ``bnb_unit``: the conv->BN(->ReLU) unit whose output dX is the gradient of; its
    BatchNorm-backward reduction (gated by its ReLU -- ``bnb_mask`` or recomputed
    from y) is computed in the GEMM epilogue. Returns ``(dx, _BnbPartials)`` then.
    ``bnb_unit2``: a second unit fed by the same gated gradient (``bnb_mask`` required),
    whose partials the same epilogue also produces (``_BnbPartials.second``; None where
    the tuned tile cannot)."""
    KH, KW, s_h, s_w, ph, pw = g["KH"], g["KW"], g["sh"], g["sw"], g["ph"], g["pw"]
    assert w32.shape[0] == Cout and w32.shape[1] == Cin, (tuple(w32.shape), Cout, Cin)
    assert dy.shape[1] == Cout and dy.numel() == N * Cout * g["Ho"] * g["Wo"]
    dx = _empty_cl(N, Cin, H, W, torch.bfloat16, dy.device)
    lib = _load()
    # parameters (fp32, channels_last storage) get cached phase weights; temporaries do not
    cacheable = isinstance(w32, nn.Parameter) and w32.dtype == torch.float32 and \
        w32.is_contiguous(memory_format=torch.channels_last)
    w32c = w32 if cacheable else _cl(w32.detach().float())
    launches = []
    for qh in range(s_h):
        kh0 = (qh + ph) % s_h
        nth = (KH - kh0 + s_h - 1) // s_h if kh0 < KH else 0
        oh0 = (qh + ph - kh0) // s_h
        for qw in range(s_w):
            kw0 = (qw + pw) % s_w
            ntw = (KW - kw0 + s_w - 1) // s_w if kw0 < KW else 0
            ow0 = (qw + pw - kw0) // s_w
            K = nth * ntw * Cout
            assert s_h == s_w, "dgrad weight slicing assumes square strides"
            if K > 0 and cacheable:
                wt = _DGRAD_W.get(w32, Cout, KH, KW, Cin, kh0, kw0, s_h, nth, ntw)
            else:
                wt = torch.empty(max(Cin * K, 8), dtype=torch.bfloat16, device=dy.device)
                if K > 0:
                    _chk(lib.pdt_wt_dgrad(_p(w32c), _p(wt), Cout, KH, KW, Cin, kh0, kw0, s_h, nth, ntw, _s()),
                         "wt_dgrad")
            a = dict(Hs=g["Ho"], Ws=g["Wo"], Cs=Cout, Nimg=N, Hm=H // s_h, Wm=W // s_w, Ncol=Cin,
                     K=K, ldb=max(K, 8), sh=1, sw=1, oh0=oh0, ow0=ow0, dh=-1, dw=-1, nth=nth, ntw=max(ntw, 0),
                     Ho=H, Wo=W, osh=s_h, osw=s_w, oph=qh, opw=qw, ldo=Cin)
            if bnb_unit is None:
                conv_nt(dy, wt, dx, addend=addend, addend_mask=addend_mask, **a)
            else:
                launches.append((wt, a))
    if bnb_unit is None:
        return dx
    # fused BN-backward partials: every phase launch writes its own row range
    u = bnb_unit
    assert u.Cout == Cin and u.y.numel() == dx.numel() and u.y.is_contiguous(memory_format=torch.channels_last)
    if addend is not None:
        _check_addend(addend, dx, addend_mask, Cin)
    relu = bool(u.relu or bnb_mask is not None)
    if bnb_mask is not None:
        assert bnb_mask.dtype == torch.uint8 and bnb_mask.numel() * 8 == dx.numel()

    def launch(wt, a, v, part, row0, R, part2=None):
        args = (_p(dy), _p(wt), _p(dx), _p(addend), _p(addend_mask), a["Hs"], a["Ws"], a["Cs"], a["Nimg"], a["Hm"],
                a["Wm"], a["Ncol"], a["K"], a["ldb"], a["sh"], a["sw"], a["oh0"], a["ow0"], a["dh"], a["dw"], a["nth"],
                a["ntw"], a["Ho"], a["Wo"], a["osh"], a["osw"], a["oph"], a["opw"], a["ldo"], int(v), _p(u.y),
                _p(u.mean), _p(u.scale), _p(u.shift), _p(bnb_mask), _p(part), int(relu), int(row0), int(R))
        if part2 is None:
            return lib.pdt_conv_nt_bnb(*args, _s())
        return lib.pdt_conv_nt_bnb2(*args, _p(u2.y), _p(u2.mean), _p(part2), _s())

    u2 = bnb_unit2
    if u2 is not None and (bnb_mask is None or u2.Cout != Cin or u2.y.shape != u.y.shape or
                           not u2.y.is_contiguous(memory_format=torch.channels_last)):
        u2 = None
    plan, R = [], 0
    has_add, has_mask = int(addend is not None), int(bnb_mask is not None)
    for wt, a in launches:
        _check_nt(dy, wt, dx, a)
        # with a second unit the tile is tuned with its partials (own key: the ring tiles cannot)
        v = _select_bnb_variant(lambda v, part, rows, part2, wt=wt, a=a: launch(wt, a, v, part, 0, rows, part2), a,
                                addend is not None, bnb_mask is not None, dy.device, two=u2 is not None)
        # a table / heuristic choice whose epilogue does not compile this configuration (a ring
        # tile): without the second unit if that is all it lacks, else the generic 64x128 tile
        if not lib.pdt_conv_nt_bnb_supports(v, has_add, has_mask, int(relu), int(u2 is not None)):
            if u2 is not None and lib.pdt_conv_nt_bnb_supports(v, has_add, has_mask, int(relu), 0):
                u2 = None
            else:
                v = _BNB_GENERIC_VARIANT
        rows = lib.pdt_conv_nt_bnb_rows(a["Nimg"] * a["Hm"] * a["Wm"], Cin, a["K"], v)
        plan.append((wt, a, v, R))
        R += rows
    one = 2 * R * Cin + lib.pdt_rows_reduce_workspace(R, Cin)
    if u2 is None:
        part = torch.empty(one, dtype=torch.float32, device=dy.device)
        for wt, a, v, row0 in plan:
            _chk(launch(wt, a, v, part, row0, R), "conv_nt_bnb")
        return dx, _BnbPartials(part, R, u)
    # both units' [2][R][C] blocks (+ their reduce tails) in one buffer, the second 256-B aligned
    off = (one + 63) // 64 * 64
    buf = torch.empty(off + one, dtype=torch.float32, device=dy.device)
    part, part2 = buf[:one], buf[off:]
    second = True
    for wt, a, v, row0 in plan:
        rc = launch(wt, a, v, part, row0, R, part2 if second else None)
        if rc == NOT_APPLICABLE and second:  # tuned tile without the second-unit epilogue
            second = False
            for wt_, a_, v_, row0_ in plan:  # redo every phase launch without it
                _chk(launch(wt_, a_, v_, part, row0_, R), "conv_nt_bnb")
            break
        _chk(rc, "conv_nt_bnb2")
    return dx, _BnbPartials(part, R, u, _BnbPartials(part2, R, u2) if second else None)


_BNB_GENERIC_VARIANT = 17  # 64x128 LDS tile, direct store: every BN-backward epilogue configuration


def _select_bnb_variant(launch, a, has_addend, has_mask, device, two=False):
    """Variant for a data gradient with the fused BN-backward epilogue: its own
    tuned-table key (the epilogue's extra loads / registers shift the best tile);
    ``two``: also a second unit's partials (key suffix ",2", timed with them)."""
    geom = (a["Hs"], a["Ws"], a["Cs"], a["Nimg"], a["Hm"], a["Wm"], a["Ncol"], a["K"], a["sh"], a["sw"], a["nth"],
            a["ntw"], a["osh"])
    M, Ncol, K = a["Nimg"] * a["Hm"] * a["Wm"], a["Ncol"], a["K"]

    def setup():
        lib = _load()
        ids = range(lib.pdt_conv_nt_num_variants())
        rows = max(lib.pdt_conv_nt_bnb_rows(M, Ncol, K, v) for v in ids)
        part = torch.empty(2 * rows * Ncol, dtype=torch.float32, device=device)
        part2 = torch.empty_like(part) if two else None
        return ids, lambda v: launch(v, part, lib.pdt_conv_nt_bnb_rows(M, Ncol, K, v), part2)

    def default():  # the plain data gradient's tuned tile, else the heuristic
        plain = _tuned().get(autotune.nt_key(*geom, 0, 0))
        return int(plain) if plain is not None else _load().pdt_conv_nt_resolve_variant(-1, M, Ncol, K)

    return autotune.choose(autotune.ntb_key(*geom, has_addend, has_mask, two), setup, default,
                           retune="PDT_RETUNE_WITH", first_only="PDT_NT_VARIANTS")


def _conv_wgrad(dy, x, N, H, W, Cs, Cout, g, out):
    M = N * g["Ho"] * g["Wo"]
    conv_wgrad(dy, x, out, M=M, Mo=Cout, No=g["KH"] * g["KW"] * Cs, ldy=Cout, Hs=H, Ws=W, C=Cs, Hm=g["Ho"],
               Wm=g["Wo"], sh=g["sh"], sw=g["sw"], oh0=-g["ph"], ow0=-g["pw"], dh=1, dw=1, ntw=g["KW"])
