"""raw kernel wrappers: the implicit-GEMM ``conv_nt``, the weight gradient, column sums"""
from __future__ import annotations

import ctypes
import os

import torch

from .. import autotune
from .lib import _chk, _load, _p, _s, c_int
from .tuning import AX_UNFUSED, NOT_APPLICABLE


def _nt_args(src, b, out, stats, bias, a, act, variant, addend=None, aux=None, addend_mask=None):
    return (_p(src), _p(b), _p(out), _p(stats), _p(bias), _p(addend), _p(addend_mask), a["Hs"], a["Ws"], a["Cs"], a["Nimg"], a["Hm"], a["Wm"],
            a["Ncol"], a["K"], a["ldb"], a["sh"], a["sw"], a["oh0"], a["ow0"], a["dh"], a["dw"], a["nth"], a["ntw"],
            a["Ho"], a["Wo"], a["osh"], a["osw"], a["oph"], a["opw"], a["ldo"], int(act), _p(aux), int(variant),
            int(a.get("pix", 0)), _s())


# element-count limit of the unsigned 32-bit offsets in the A-staging BN apply (AX) and the fused
# BN-backward epilogue (csrc/conv_nt_tile.inc): ResNet-152 stage-1 activations at 3072 images per
# GPU (N x 56 x 56 x 256 = 2.47e9) are inside it; the rest of the conv path indexes in 64 bits
_AX_MAX_ELEMS = 2 ** 32 - 8


def _check_nt(src, b, out, a):
    assert src.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    Cs, K, Ncol, ldo, ldb = a["Cs"], a["K"], a["Ncol"], a["ldo"], a["ldb"]
    assert Cs % 8 == 0 and K % 8 == 0 and Ncol % 8 == 0 and ldo % 8 == 0, (Cs, K, Ncol, ldo)
    assert K == a["nth"] * a["ntw"] * Cs
    # bounds: the kernel reads src[0 : Nimg*Hs*Ws*Cs], b[0 : Ncol*ldb], writes out rows < Nimg*Ho*Wo
    pix = a.get("pix", 0) or Cs  # elements per source pixel in memory
    assert pix % 4 == 0 and pix <= Cs
    assert src.numel() >= a["Nimg"] * a["Hs"] * a["Ws"] * pix, "src too small"
    assert b.numel() >= Ncol * ldb or K == 0, "B too small"
    assert out.numel() >= a["Nimg"] * a["Ho"] * a["Wo"] * ldo, "out too small"
    assert a["Hm"] * a["osh"] <= a["Ho"] and a["Wm"] * a["osw"] <= a["Wo"]
    # pixel indices are 32-bit; element offsets are 64-bit except the A-staging BN apply and the
    # BN-backward epilogue, which use unsigned 32-bit offsets (limit _AX_MAX_ELEMS, checked by the
    # library: it refuses those paths beyond it)
    assert a["Nimg"] * a["Hs"] * a["Ws"] < 2 ** 31 and a["Nimg"] * a["Ho"] * a["Wo"] < 2 ** 31


def select_nt_variant(src, b, out, *, with_stats=False, bias=None, act=0, aux=None, addend=None, **a):
    """Variant id for this geometry and epilogue (tuning it on first use when allowed)."""
    M, Ncol, K = a["Nimg"] * a["Hm"] * a["Wm"], a["Ncol"], a["K"]

    def setup():
        lib = _load()
        _check_nt(src, b, out, a)
        ids = range(lib.pdt_conv_nt_num_variants())
        # partial-stat rows depend on the variant's BM and waves-along-M: size for the largest
        rows = max(lib.pdt_conv_nt_stat_rows(M, Ncol, K, v) for v in ids)
        stats = torch.empty(2 * rows * Ncol, dtype=torch.float32, device=src.device) if with_stats else None
        tune_add = addend if act in (3, 5) else None  # acts 3 / 5 read their operand through the addend pointer
        return ids, lambda v: lib.pdt_conv_nt(*_nt_args(src, b, out, stats, bias, a, act, v, aux=aux,
                                                        addend=tune_add))

    return autotune.choose(
        autotune.nt_key(a["Hs"], a["Ws"], a["Cs"], a["Nimg"], a["Hm"], a["Wm"], Ncol, K, a["sh"], a["sw"], a["nth"],
                        a["ntw"], a["osh"], with_stats, bias is not None, a.get("pix", 0), act),
        setup, lambda: _load().pdt_conv_nt_resolve_variant(-1, M, Ncol, K),
        retune="PDT_RETUNE_WITH", first_only="PDT_NT_VARIANTS")


ACT = {None: 0, "none": 0, "relu": 1, "gelu": 2}
# epilogue ids beyond ACT: 3 = out * gelu'(addend = z); 4 = GELU whose aux output is gelu'(z)
# (not z) -- both from one tanh; 5 = out * addend (the stored derivative)
ACT_GELU_GRAD, ACT_GELU_DUAL, ACT_MUL = 3, 4, 5


def _gelu_dual() -> bool:
    """The MLP stores gelu'(z) in the fc1 epilogue (act 4) and its backward multiplies by it
    in the fc2 data-gradient epilogue (act 5) -- the derivative's tanh is not recomputed there.
    PDT_GELU_DUAL=0: store z and recompute gelu'(z) in the backward epilogue (acts 2 / 3)."""
    return os.environ.get("PDT_GELU_DUAL", "1") == "1"


def conv_nt(src, b, out, *, stats=None, bias=None, relu=False, act=None, variant=None, addend=None, aux=None,
            addend_mask=None, **a):
    """C[m, n] = sum_k A[m, k] B[n, k] (+ addend) with the implicit-GEMM gather (see csrc/conv_igemm.hip)."""
    _check_nt(src, b, out, a)
    if addend is not None:
        _check_addend(addend, out, addend_mask, a["Ncol"])
    act_id = (act if isinstance(act, int) else ACT[act]) if act is not None else (1 if relu else 0)
    if aux is not None:
        assert aux.dtype == torch.bfloat16 and aux.numel() == out.numel()
    if variant is None:
        variant = select_nt_variant(src, b, out, with_stats=stats is not None, bias=bias, act=act_id, aux=aux,
                                    addend=addend, **a)
    if addend_mask is not None:
        assert addend is not None and a["ldo"] == a["Ncol"]
    lib = _load()
    rc = lib.pdt_conv_nt(*_nt_args(src, b, out, stats, bias, a, act_id, variant, addend, aux, addend_mask))
    if rc == NOT_APPLICABLE:  # a cached variant tuned for another epilogue (e.g. the streaming 1x1 kernel)
        M = a["Nimg"] * a["Hm"] * a["Wm"]
        variant = lib.pdt_conv_nt_resolve_variant(-1, M, a["Ncol"], a["K"])
        rc = lib.pdt_conv_nt(*_nt_args(src, b, out, stats, bias, a, act_id, variant, addend, aux, addend_mask))
    _chk(rc, "conv_nt")


def _check_addend(addend, out, addend_mask, Ncol):
    assert addend.dtype == torch.bfloat16 and addend.numel() == out.numel() and addend.is_contiguous(
        memory_format=torch.channels_last if addend.dim() == 4 else torch.contiguous_format)
    if addend_mask is not None:
        assert addend_mask.dtype == torch.uint8 and addend_mask.numel() * 8 == addend.numel()


def conv_stat_rows(M, Ncol, K, variant):
    return _load().pdt_conv_nt_stat_rows(M, Ncol, K, variant)


def _wgrad_launch(lib, dy, x, out, v, scale, accumulate, a, bias_out=None, bna=None):
    """One weight-gradient launch (+ slab reduction); returns the kernel's return code
    (NOT_APPLICABLE: variant ``v`` cannot run this geometry). ``bna`` = (y, coef [5][Mo]):
    ``dy`` is dA and the BN backward apply runs in the dY staging (``pdt_conv_wgrad2``)."""
    kps = c_int(0)
    splits = lib.pdt_wgrad_plan2(a["M"], a["Mo"], a["No"], a["Hs"], a["Ws"], a["C"], v, ctypes.byref(kps))
    if splits < 0:
        return splits
    slab = torch.empty(lib.pdt_wgrad_workspace(splits, a["Mo"], a["No"]), dtype=torch.float32, device=dy.device)
    by, bc = bna if bna is not None else (None, None)
    return lib.pdt_conv_wgrad2(_p(dy), _p(x), _p(slab), _p(out), a["M"], a["Mo"], a["No"], a["ldy"], a["Hs"],
                               a["Ws"], a["C"], a["Hm"], a["Wm"], a["sh"], a["sw"], a["oh0"], a["ow0"], a["dh"],
                               a["dw"], a["ntw"], splits, kps.value, float(scale), int(accumulate), int(v),
                               int(a.get("pix", 0)), _p(bias_out), _p(by), _p(bc), _s())


WGB_VARIANTS = tuple(range(12))  # the 4-wave 1/2-stage tiles carry the BN-apply instantiation


def conv_wgrad_bn(dA, x, out, y, coef, run_ref, **a):
    """Weight gradient whose dY = k1*gate(dA) + k2*y + k3 (a BN+ReLU unit's backward apply,
    ``coef`` = [k1; k2; k3; scale; shift] fp32 [5][Mo], gate = y*scale+shift > 0) is formed
    while staging dA (``pdt_conv_wgrad2``): the apply pass and its dy tensor disappear.
    Tuned per geometry against ``run_ref()`` (the element pass + the plain weight gradient):
    returns False when that is faster (the caller runs it), True when done here."""
    lib = _load()
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() == 5 * a["Mo"]
    assert y.dtype == torch.bfloat16 and y.shape == dA.shape

    def run(v):
        return _wgrad_launch(lib, dA, x, out, v, 1.0, False, a, bna=(y, coef))

    v = autotune.choose(_wg_key(a, True), lambda: (WGB_VARIANTS, run), AX_UNFUSED, ref=run_ref)
    if v < 0:  # (tuning not allowed and no entry: not taken, and nothing stored)
        return False
    _chk(run(v), "conv_wgrad (BN backward apply)")
    return True


def _wg_key(a, bn=False):
    return autotune.wg_key(a["M"], a["Mo"], a["No"], a["Hs"], a["Ws"], a["C"], a["Hm"], a["Wm"], a["sh"], a["ntw"],
                           a.get("pix", 0), bn)


def conv_wgrad(dy, x, out, *, scale=1.0, accumulate=False, variant=None, bias_out=None, **a):
    """dW[co, tap*C + c] = sum_m dY[m, co] X_gather[m, (tap, c)] (see csrc/conv_wgrad.hip).
    ``bias_out`` (fp32 [Mo]): also sum_m dY[m, co] -- the nn.Linear bias gradient -- from the
    dY tiles the kernel stages anyway (no separate column-sum pass)."""
    M, Mo, No, ldy, C, Hm, Wm = a["M"], a["Mo"], a["No"], a["ldy"], a["C"], a["Hm"], a["Wm"]
    assert dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and out.dtype == torch.float32
    assert C % 8 == 0 and Mo % 8 == 0 and No % 8 == 0 and ldy % 8 == 0
    assert out.numel() >= Mo * No and dy.numel() >= M * ldy
    pix = a.get("pix", 0) or C  # elements per source pixel in memory
    assert pix % 4 == 0 and pix <= C
    assert M % (Hm * Wm) == 0 and x.numel() >= (M // (Hm * Wm)) * a["Hs"] * a["Ws"] * pix, "wgrad source too small"
    assert a["ntw"] >= 1 and No % C == 0
    if bias_out is not None:
        assert bias_out.dtype == torch.float32 and bias_out.numel() >= Mo and bias_out.is_contiguous()
        assert bias_out.device == dy.device, "bias gradient buffer on another device than dY"
    assert out.device == dy.device == x.device, "weight gradient operands on different devices"
    lib = _load()
    if variant is None:
        variant = autotune.choose(
            _wg_key(a), lambda: (range(lib.pdt_wgrad_num_variants()),
                                 lambda v: _wgrad_launch(lib, dy, x, out, v, scale, False, a)),
            -1, retune="PDT_RETUNE_WG")
    rc = _wgrad_launch(lib, dy, x, out, variant, scale, accumulate, a, bias_out)
    if rc == NOT_APPLICABLE:  # e.g. a tuned halo id for a geometry it does not cover: the heuristic tile
        rc = _wgrad_launch(lib, dy, x, out, -1, scale, accumulate, a, bias_out)
    _chk(rc, "conv_wgrad")


def colsum(x, R, C):
    """fp32 column sums of a bf16 [R][C] matrix (bias gradients)."""
    assert x.dtype == torch.bfloat16 and x.numel() >= R * C
    lib = _load()
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    work = torch.empty(lib.pdt_colsum_workspace(R, C), dtype=torch.float32, device=x.device)
    _chk(lib.pdt_colsum(_p(x), _p(out), _p(work), R, C, 0, _s()), "colsum")
    return out
