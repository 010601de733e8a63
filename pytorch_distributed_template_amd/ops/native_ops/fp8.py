"""FP8 linear (OCP e4m3 forward operands, e5m2 output gradients) -- csrc/fp8.hip
quantizes with per-tensor current scaling entirely on device; the GEMMs are
the block-scaled fp8 MFMA instantiation of conv_nt (csrc/conv_igemm.hip,
pdt_gemm_f8). Weight gradients stay bf16 (the wgrad kernel), as in common
fp8 training recipes.

This module holds the recipe, the casts, the fp8 GEMM and weight gradient, and the codes that
ride on tensors between ops; the autograd nodes built on them are in ``linear.py``.
"""
from __future__ import annotations

import ctypes
import os

import torch

from .. import autotune
from .lib import _chk, _chk_v, _grad_buf, _load, _p, _s, c_int
from .shadows import _same_tensor, _weak
from .tuning import _tuned

E4M3, E5M2 = 0, 1


def fp8_settings() -> dict:
    """The fp8 recipe actually in effect (read by the layers AND by bench.py's
    dtype label, so the label cannot drift from the code's defaults)."""
    return {"scaling": os.environ.get("PDT_FP8_SCALING", "delayed"),
            "dgrad": os.environ.get("PDT_FP8_DGRAD", "1") == "1",
            "attn": os.environ.get("PDT_FP8_ATTN", "1") == "1",
            "wgrad": os.environ.get("PDT_FP8_WGRAD", "1") == "1"}


def quantize_fp8(x: torch.Tensor, fmt: int = E4M3):
    """(q uint8 same shape, dq fp32[1]) with x ~= q.float() * dq (per-tensor scale)."""
    lib = _load()
    x = x.contiguous()
    assert x.dtype in (torch.bfloat16, torch.float32)
    n = x.numel()
    part = torch.empty(lib.pdt_amax_blocks(n), dtype=torch.float32, device=x.device)
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    dq = torch.empty(1, dtype=torch.float32, device=x.device)
    bf = int(x.dtype == torch.bfloat16)
    _chk(lib.pdt_amax_partial(_p(x), bf, n, _p(part), _s()), "amax")
    _chk(lib.pdt_cast_fp8(_p(x), bf, n, _p(part), fmt, _p(q), _p(dq), _s()), "cast_fp8")
    return q, dq


def quantize_fp8_delayed(x: torch.Tensor, meta: torch.Tensor | None, fmt: int = E4M3):
    """One-pass cast with delayed (amax-history) scaling; returns (q, dq, meta).

    ``meta`` is the tensor's scaling state (csrc/fp8.hip: scale, dq, amax,
    history); pass None on first use -- it is created and seeded with the
    exact amax of ``x`` (so the first step is current-scaled)."""
    lib = _load()
    x = x.contiguous()
    n = x.numel()
    bf = int(x.dtype == torch.bfloat16)
    if meta is None:
        meta = torch.zeros(lib.pdt_fp8_meta_words(), dtype=torch.float32, device=x.device)
        part = torch.empty(lib.pdt_amax_blocks(n), dtype=torch.float32, device=x.device)
        _chk(lib.pdt_amax_partial(_p(x), bf, n, _p(part), _s()), "amax")
        _chk(lib.pdt_fp8_meta_seed(_p(part), n, fmt, _p(meta), _s()), "fp8_meta_seed")
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    dq = torch.empty(1, dtype=torch.float32, device=x.device)  # this cast's dequant factor (stable)
    _chk(lib.pdt_cast_fp8_delayed(_p(x), bf, n, _p(meta), fmt, _p(q), _p(dq), _s()), "cast_fp8_delayed")
    return q, dq, meta


_F8W: dict = {}


def fp8_weight(w: torch.Tensor):
    """(wq [N][K] e4m3, wqt [K][N] e4m3, dq) of an fp32 [N][K] weight, cached per optimizer version."""
    ent = _F8W.get(id(w))
    if ent is not None and ent[0] == w._version and ent[1] == w.data_ptr() and _same_tensor(ent[3], w):
        return ent[2]
    lib = _load()
    src = w.detach().float().contiguous()
    N, K = src.shape
    part = torch.empty(lib.pdt_amax_blocks(src.numel()), dtype=torch.float32, device=w.device)
    wq = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    wqt = torch.empty((K, N), dtype=torch.uint8, device=w.device)
    dq = torch.empty(1, dtype=torch.float32, device=w.device)
    st = _s()
    _chk(lib.pdt_amax_partial(_p(src), 0, src.numel(), _p(part), st), "amax")
    # both layouts (forward [N][K], data gradient [K][N]) from one read of the fp32 weight
    _chk(lib.pdt_cast_fp8_dual(_p(src), N, K, _p(part), _p(wq), _p(wqt), _p(dq), st), "cast_fp8_dual")
    val = (wq, wqt, dq)
    _F8W[id(w)] = (w._version, w.data_ptr(), val, _weak(w))
    return val


def _fc1_split(M, Hd, K) -> bool:
    """The MLP's fp8 fc1 as a plain GEMM (+bias) followed by one pass that writes gelu'(z), the
    e4m3 codes of gelu(z) and their amax (pdt_gelu_dual_cast_fp8), instead of one GEMM with that
    epilogue fused (act 4 + fp8 side output). Off by default: the dense ring's fused epilogue
    (csrc/gemm_ring.hip) measured faster than the split (ViT-B/16 fp8 bs 1024: 9 404 vs 9 175
    img/s with the fc2 data gradient below, same box, r5b). Tuned-table key
    ``fc1split:M,Hd,K`` (1 = split); PDT_FP8_FC1_SPLIT=0/1 forces either. (The hipBLASLt A/B
    of these plain GEMMs lives in ``scripts/probe_scaled_mm.py`` / ``scripts/bench_f8.py``,
    not in the product.)"""
    env = os.environ.get("PDT_FP8_FC1_SPLIT")
    if env is not None:
        return env == "1"
    return bool(_tuned().get(f"fc1split:{M},{Hd},{K}", 0))


def _fc1_split_forward(xq, w1q, a, z, aq, dqx, dqw1, bias1, meta, keep_a):
    """a <- x W1^T + b1 (plain fp8 GEMM), then z <- gelu'(a) (z None: not formed -- the caller keeps
    the pre-activation a), aq <- e4m3(gelu(a)), and (keep_a) a <- gelu(a) in place. Returns the
    codes' dequant factor (device [1])."""
    lib = _load()
    dqa = torch.empty(1, dtype=torch.float32, device=a.device)
    gemm_f8(xq, w1q, a, dqx, dqw1, fmt_a=E4M3, bias=bias1)
    _chk(lib.pdt_gelu_dual_cast_fp8(_p(a), a.numel(), _p(meta), E4M3, _p(aq), _p(z) if z is not None else None,
                                    _p(a) if keep_a else None, _p(dqa), _s()), "gelu_dual_cast_fp8")
    return dqa


def _fc2_dgrad_split_on() -> bool:
    """The MLP's fc2 data gradient as a plain GEMM (bf16 g W2) followed by one pass that
    multiplies by gelu'(z), casts to e5m2 and sums fc1's bias gradient
    (pdt_cast_fp8_gelu_grad_cs), instead of one GEMM with that epilogue (act 3 + e5m2 + column
    sums). Off by default (the fused ring epilogue is faster, see ``_fc1_split``);
    PDT_FC2_DGRAD_SPLIT=1 turns it on."""
    return os.environ.get("PDT_FC2_DGRAD_SPLIT", "0") == "1"


def _fc2_dgrad_split(gq, w2qt, dz, dqg, dqw2, z, dzq, gmeta, db):
    """dz <- g W2 (plain fp8 GEMM), then dzq <- e5m2(dz * gelu'(z)) and db <- column sums of dz * gelu'(z).
    Returns the codes' dequant factor (device [1])."""
    lib = _load()
    rows, cols = dz.shape
    gemm_f8(gq, w2qt, dz, dqg, dqw2, fmt_a=E5M2)
    nb = lib.pdt_cast_cs_bands(rows)
    cpart = torch.empty(nb * cols + lib.pdt_reduce_rows_work(nb, cols), dtype=torch.float32, device=dz.device)
    dq = torch.empty(1, dtype=torch.float32, device=dz.device)
    _chk(lib.pdt_cast_fp8_gelu_grad_cs(_p(dz), _p(z), rows, cols, _p(gmeta), E5M2, _p(dzq), _p(dq), _p(cpart),
                                       _p(db), _s()), "cast_fp8_gelu_grad_cs")
    return dq


def _fc1_keep_pre() -> bool:
    """Split fc1 with fp8 weight gradients: keep the GEMM's own pre-activation output for the
    backward (whose fc2 data-gradient epilogue then forms gelu'(z) itself, act 3) instead of
    writing gelu'(z) in the cast pass -- one bf16 [M, 4D] store fewer per block."""
    return os.environ.get("PDT_FC1_KEEP_PRE", "1") == "1"


def gemm_f8(a, b, out, dq_a, dq_b, *, fmt_a=E4M3, bias=None, act=0, aux=None, addend=None, variant=None,
            q8=None, colsum_out=None):
    """out[M, N] (bf16) = dq_a*dq_b * a[M, K] @ b[N, K]^T (+bias, act) (+ addend); a, b uint8 fp8
    codes. ``act=3``: GELU backward, out = (a @ b^T) * gelu'(addend).

    ``q8 = (codes, meta, fmt, only)``: the epilogue also writes the fp8 codes (format fmt) of
    the output for the NEXT fp8 GEMM with that GEMM's delayed scale ``meta`` and rolls its
    amax history (no separate quantisation pass); ``only`` skips the bf16 output. Returns
    the codes' dequant factor (device [1]) in that case, else ``out``. ``colsum_out`` (with q8,
    fp32 [N]): also the column sums of the final bf16 output (written or not), formed in the
    epilogue -- the bias gradient of the layer whose output gradient this GEMM produces."""
    M, K = a.shape
    N = b.shape[0]
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and b.shape[1] == K and K % 128 == 0
    assert out.dtype == torch.bfloat16 and out.numel() == M * N and a.is_contiguous() and b.is_contiguous()
    lib = _load()
    if addend is not None:
        assert addend.dtype == torch.bfloat16 and addend.numel() == M * N and addend.is_contiguous()
    if q8 is None:
        args = lambda v: (_p(a), _p(b), _p(out), _p(bias), _p(dq_a), _p(dq_b), M, N, K, K, K, N, fmt_a, act,  # noqa
                          _p(aux), _p(addend), v, _s())
        nv = lib.pdt_gemm_f8_num_variants()
        if variant is None:
            key = autotune.f8_key(M, N, K, fmt_a, act, bias is not None, addend is not None and act == 0)
            variant = autotune.choose(key, lambda: (range(nv), lambda v: lib.pdt_gemm_f8(*args(v))), 0)
        if variant >= nv:
            variant = -1  # (a stale table entry: the built-in native choice)
        _chk_v(lib.pdt_gemm_f8(*args(variant)), "gemm_f8")
        return out
    codes, meta, qfmt, only = q8
    assert codes.dtype == torch.uint8 and codes.numel() == M * N and codes.is_contiguous()
    part = torch.empty(lib.pdt_gemm_f8_q8_part(M, N) + 1, dtype=torch.float32, device=a.device)
    dq = part[-1:]
    args = lambda v: (_p(a), _p(b), _p(out), _p(bias), _p(dq_a), _p(dq_b), M, N, K, K, K, N, fmt_a, act,  # noqa
                      _p(aux), _p(addend), v, _p(codes), _p(meta), _p(part), int(qfmt), int(only), _p(dq), _s())
    if variant is None:
        def setup():  # (tuning launches roll the history too: tune on a scratch copy of the state)
            scratch = meta.clone()
            targs = lambda v: args(v)[:17] + (_p(codes), _p(scratch)) + args(v)[19:]  # noqa: E731
            return range(lib.pdt_gemm_f8_num_variants()), lambda v: lib.pdt_gemm_f8_q8(*targs(v))

        variant = autotune.choose(autotune.f8_key(M, N, K, fmt_a, act, bias is not None, False, (int(qfmt), int(only)),
                                                  colsum_out is not None), setup, 0)
    if colsum_out is not None:
        assert colsum_out.dtype == torch.float32 and colsum_out.numel() == N and colsum_out.is_contiguous()
        if variant == 7 or variant < 0:  # the direct-store tile has no staged epilogue
            variant = 10
        ntm = -(-M // lib.pdt_gemm_f8_bm(variant))
        cpart = torch.empty(ntm * N + lib.pdt_reduce_rows_work(ntm, N), dtype=torch.float32, device=a.device)
        _chk_v(lib.pdt_gemm_f8_q8_cs(*args(variant)[:-1], _p(cpart), _s()), "gemm_f8_q8_cs")
        _chk(lib.pdt_wgrad_reduce_rows(_p(cpart), _p(colsum_out), ntm, N, 1.0, 0, _p(cpart[ntm * N:]), _s()),
             "colsum rows")
        return dq
    _chk_v(lib.pdt_gemm_f8_q8(*args(variant)), "gemm_f8_q8")
    return dq


def _wgrad_f8_launch(lib, dyq, xq, dq_dy, dq_x, dy16, dw, db, v):
    M, Mo = dyq.shape
    No = xq.shape[1]
    kps = c_int(0)
    splits = lib.pdt_wgrad_f8_plan(M, Mo, No, v, ctypes.byref(kps))
    slab = torch.empty(lib.pdt_wgrad_f8_workspace(splits, Mo, No), dtype=torch.float32, device=dyq.device)
    _chk(lib.pdt_linear_wgrad_f8(_p(dyq), _p(xq), _p(dq_dy), _p(dq_x), _p(dy16), _p(slab), _p(dw), _p(db), M, Mo, No,
                                 Mo, No, splits, kps.value, 0, int(v), _s()), "linear_wgrad_f8")


def linear_wgrad_f8(dyq, xq, dq_dy, dq_x, dy16=None, with_bias=False, variant=None, w=None, b=None):
    """(dW fp32 [Nout][K], db fp32 [Nout] or None) of nn.Linear from the fp8 codes the
    data-gradient and forward GEMMs consumed: dyq [M][Nout] e5m2, xq [M][K] e4m3, device
    dequant scales. db = column sums of the bf16 ``dy16`` (csrc/wgrad_f8.hip)."""
    M, Nout = dyq.shape
    K = xq.shape[1]
    assert dyq.dtype == torch.uint8 and xq.dtype == torch.uint8 and xq.shape[0] == M
    assert dyq.is_contiguous() and xq.is_contiguous() and Nout % 16 == 0 and K % 16 == 0
    if with_bias:
        assert dy16 is not None and dy16.dtype == torch.bfloat16 and dy16.shape == (M, Nout) and dy16.is_contiguous()
    lib = _load()
    dw = _grad_buf(w, (Nout, K)) if w is not None else torch.empty((Nout, K), dtype=torch.float32,
                                                                  device=dyq.device)
    db = (_grad_buf(b, (Nout,)) if b is not None else torch.empty(Nout, dtype=torch.float32, device=dyq.device)) \
        if with_bias else None
    if variant is None:
        variant = autotune.choose(
            autotune.wg8_key(M, Nout, K),
            lambda: (range(lib.pdt_wgrad_f8_num_variants()),
                     lambda v: _wgrad_f8_launch(lib, dyq, xq, dq_dy, dq_x, None, dw, None, v)), 0)
    _wgrad_f8_launch(lib, dyq, xq, dq_dy, dq_x, dy16 if with_bias else None, dw, db, variant)
    return dw, db


def _quant_grad_db(g2, owner, attr, bias):
    """(e5m2 codes, dequant, bias gradient) of a bf16 [rows][cols] output gradient in ONE pass
    (pdt_cast_fp8_delayed_cs: the delayed-scaling cast that also sums the columns it reads),
    or None when that path does not apply (current scaling, no history yet, PDT_CAST_DB=0)."""
    meta = getattr(owner, attr, None)
    if meta is None or fp8_settings()["scaling"] != "delayed" or os.environ.get("PDT_CAST_DB", "1") != "1":
        return None
    rows, cols = g2.shape
    if cols % 8:
        return None
    lib = _load()
    nb = lib.pdt_cast_cs_bands(rows)
    q = torch.empty((rows, cols), dtype=torch.uint8, device=g2.device)
    dq = torch.empty(1, dtype=torch.float32, device=g2.device)
    cpart = torch.empty(nb * cols + lib.pdt_reduce_rows_work(nb, cols), dtype=torch.float32, device=g2.device)
    db = _grad_buf(bias, (cols,))
    _chk(lib.pdt_cast_fp8_delayed_cs(_p(g2), rows, cols, _p(meta), E5M2, _p(q), _p(dq), _p(cpart), _p(db), _s()),
         "cast_fp8_delayed_cs")
    return q, dq, db


def _pre_bias_grad(g, owner):
    """The bias gradient of ``owner`` if the producer of its output gradient ``g`` (a LayerNorm
    backward, :func:`_ln_fork_backward`) already formed it, else None."""
    pre = getattr(g, "_pdt_db", None) if g is not None else None
    if pre is None or pre[1] is not owner:
        return None
    # dropped from ``g``: a LayerNorm's dx also feeds the residual branch, so it outlives this
    # backward, and a second reference to the bias gradient (a reducer slot view) would make
    # autograd clone it instead of adopting it as ``bias.grad`` (and the reducer copy it back)
    del g._pdt_db
    return pre[0]


def _fp8_wgrad_on() -> bool:
    return fp8_settings()["wgrad"]


def _quant_act(x2, owner, attr="_pdt_fp8_meta"):
    """e4m3 codes + dequant scale of a bf16 activation under the configured scaling
    (delayed: amax history kept on ``owner``)."""
    if fp8_settings()["scaling"] == "current":
        return quantize_fp8(x2, E4M3)
    q, dq, meta = quantize_fp8_delayed(x2, getattr(owner, attr, None), E4M3)
    setattr(owner, attr, meta)
    return q, dq


def _quant_grad(g2, owner, attr, src=None):
    """e5m2 codes + dequant scale of an output gradient for the fp8 data-gradient GEMM.
    Delayed scaling (the default) is one fused cast+amax pass with the history kept on
    ``owner``; current scaling needs a separate amax pass over the gradient first.
    ``src``: the gradient tensor as received -- if its producer (the LayerNorm backward,
    ``ln_fork(grad_fp8_for=owner)``) already wrote the codes, they are used as they are."""
    pre = getattr(src, "_pdt_f8g", None) if src is not None else None
    if pre is not None and pre[2] is owner:
        return pre[0].view(g2.shape), pre[1]
    if fp8_settings()["scaling"] == "current":
        return quantize_fp8(g2, E5M2)
    q, dq, meta = quantize_fp8_delayed(g2, getattr(owner, attr, None), E5M2)
    setattr(owner, attr, meta)
    return q, dq


def _prequant(x, owner):
    """(codes [rows, K], dq) if ``x`` carries fp8 codes made for ``owner`` (ln_fork), else None.
    A codes-only tensor (``_pdt_f8_only``: its bf16 values were never written) may be read by
    ``owner`` alone, and only through an fp8 path that keeps the codes for its weight gradient."""
    pre = getattr(x, "_pdt_f8", None)
    if getattr(x, "_pdt_f8_only", False):
        cfg = fp8_settings()
        if pre is None or pre[2] is not owner or not (cfg["dgrad"] and cfg["wgrad"]):
            raise RuntimeError("this LayerNorm output carries fp8 codes only (its bf16 values were not written) "
                               "and its consumer would read the values: set PDT_LN_CODES_ONLY=0")
    if pre is None or pre[2] is not owner:
        return None
    return pre[0], pre[1]
