"""LayerNorm (bf16 activations, fp32 affine params)"""
from __future__ import annotations

import os

import torch

from .fp8 import fp8_settings
from .lib import _chk, _grad_buf, _load, _p, _s, fallback


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, b, eps):
        ctx.refs = (g, b)  # the affine parameters: their gradients go to their reducer slots
        shp = x.shape
        D = shp[-1]
        x2 = x.reshape(-1, D).to(torch.bfloat16).contiguous()
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        stats = torch.empty((2, rows), dtype=torch.float32, device=x.device)
        gf = g.float().contiguous()
        bf = b.float().contiguous()
        _chk(_load().pdt_ln_fwd(_p(x2), _p(gf), _p(bf), _p(y), _p(stats[0]), _p(stats[1]), rows, D, float(eps),
                                _s()), "ln_fwd")
        ctx.save_for_backward(x2, gf, stats)
        ctx.shp = shp
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, gf, stats = ctx.saved_tensors
        rows, D = x2.shape
        lib = _load()
        dy2 = dy.reshape(rows, D).to(torch.bfloat16).contiguous()
        dx = torch.empty_like(x2)
        blocks = lib.pdt_ln_bwd_blocks(rows)
        part = torch.empty(2 * blocks * D, dtype=torch.float32, device=dy.device)
        dg, db = _grad_buf(ctx.refs[0], (D,)), _grad_buf(ctx.refs[1], (D,))
        _chk(lib.pdt_ln_bwd(_p(dy2), _p(x2), _p(gf), _p(stats[0]), _p(stats[1]), _p(dx), _p(dg), _p(db), _p(part),
                            rows, D, 0, None, _s()), "ln_bwd")
        return dx.reshape(ctx.shp), dg, db, None


def layer_norm(x, ln):
    D = ln.normalized_shape[-1]
    if len(ln.normalized_shape) != 1 or D not in (256, 512, 768, 1024) or not ln.elementwise_affine:
        fallback("layer_norm", f"normalized_shape {tuple(ln.normalized_shape)} (kernels: D in 256/512/768/1024, affine)")
        return ln(x)
    return _LayerNorm.apply(x, ln.weight, ln.bias, ln.eps)


class _LNFork(torch.autograd.Function):
    """(x, LayerNorm(x)) for a pre-norm residual block: the pass-through output feeds
    the block's residual add (a GEMM epilogue), so backward receives the residual
    gradient and the normalised branch's gradient together and sums them inside
    the LayerNorm backward kernel (no add pass)."""

    @staticmethod
    def forward(ctx, x, g, b, eps, f8meta, f8box, grad_owner, codes_only=False):
        ctx.refs = (g, b)
        shp = x.shape
        D = shp[-1]
        x2 = x.reshape(-1, D).contiguous()
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        stats = torch.empty((2, rows), dtype=torch.float32, device=x.device)
        gf = g.float().contiguous()
        lib = _load()
        bf = b.float().contiguous()
        if f8meta is not None:  # also emit the next fp8 GEMM's e4m3 input (delayed scale f8meta)
            q = torch.empty((rows, D), dtype=torch.uint8, device=x.device)
            part = torch.empty(lib.pdt_ln_fwd_f8_blocks(rows) + 1, dtype=torch.float32, device=x.device)
            dq = part[-1:]  # the codes' dequant factor (written by the history roll)
            # codes_only: the bf16 output is not written (y stays uninitialised; see _ln_codes_only)
            _chk(lib.pdt_ln_fwd_f8(_p(x2), _p(gf), _p(bf), None if codes_only else _p(y), _p(stats[0]),
                                   _p(stats[1]), rows, D, float(eps), _p(q), _p(f8meta), _p(part), _p(dq), _s()),
                 "ln_fwd_f8")
            f8box.append((q, dq))
        else:
            _chk(lib.pdt_ln_fwd(_p(x2), _p(gf), _p(bf), _p(y), _p(stats[0]), _p(stats[1]), rows, D, float(eps),
                                _s()), "ln_fwd")
        ctx.save_for_backward(x2, gf, stats)
        ctx.shp = shp
        ctx.grad_owner = grad_owner
        return x.view_as(x), y.reshape(shp)

    @staticmethod
    def backward(ctx, g_res, dy):
        if dy is None:
            return g_res, None, None, None, None, None, None, None
        dx, dg, db = _ln_fork_backward(ctx, g_res, dy)
        return dx, dg, db, None, None, None, None, None


def _ln_fork_backward(ctx, g_res, dy):
    """LayerNorm backward of a fork (x -> (x, LN(x))) with the residual gradient g_res summed
    in: (dx, dgamma, dbeta); dx carries the e5m2 codes for ctx.grad_owner (``_pdt_f8g``) when
    that fp8 layer's gradient history exists."""
    x2, gf, stats = ctx.saved_tensors
    rows, D = x2.shape
    lib = _load()
    dev = x2.device
    dy2 = dy.reshape(rows, D).to(torch.bfloat16).contiguous()
    add = g_res.reshape(rows, D).to(torch.bfloat16).contiguous() if g_res is not None else None
    dx = torch.empty_like(x2)
    blocks = lib.pdt_ln_bwd_blocks(rows)
    part = torch.empty(2 * blocks * D, dtype=torch.float32, device=dev)
    dg, db = _grad_buf(ctx.refs[0], (D,)), _grad_buf(ctx.refs[1], (D,))
    owner = ctx.grad_owner
    gmeta = getattr(owner, "_pdt_fp8_gmeta", None) if owner is not None else None
    if gmeta is not None and fp8_settings()["scaling"] == "delayed":
        # also the e5m2 codes of dx for the fp8 GEMM that consumes this gradient
        codes = torch.empty((rows, D), dtype=torch.uint8, device=dev)
        qpart = torch.empty(blocks + 1, dtype=torch.float32, device=dev)
        dq = qpart[-1:]
        bias = getattr(owner, "bias", None)
        if bias is not None and bias.requires_grad and os.environ.get("PDT_LN_DB", "1") == "1":
            # the producer's bias gradient = column sums of dx, formed here (the weight-gradient
            # kernel of that layer would re-read dx for them); picked up through ``_pdt_db``
            pdb = _grad_buf(bias, (D,))
            cpart = torch.empty(blocks * D + lib.pdt_reduce_rows_work(blocks, D), dtype=torch.float32, device=dev)
            _chk(lib.pdt_ln_bwd_f8_db(_p(dy2), _p(x2), _p(gf), _p(stats[0]), _p(stats[1]), _p(dx), _p(dg), _p(db),
                                      _p(part), rows, D, 0, _p(add), _p(codes), _p(gmeta), _p(qpart), _p(dq),
                                      _p(cpart), _p(pdb), 0, _s()), "ln_bwd_f8_db")
        else:
            pdb = None
            _chk(lib.pdt_ln_bwd_f8(_p(dy2), _p(x2), _p(gf), _p(stats[0]), _p(stats[1]), _p(dx), _p(dg), _p(db),
                                   _p(part), rows, D, 0, _p(add), _p(codes), _p(gmeta), _p(qpart), _p(dq), _s()),
                 "ln_bwd_f8")
        out = dx.reshape(ctx.shp)
        out._pdt_f8g = (codes, dq, owner)
        if pdb is not None:
            out._pdt_db = (pdb, owner)
        return out, dg, db
    _chk(lib.pdt_ln_bwd(_p(dy2), _p(x2), _p(gf), _p(stats[0]), _p(stats[1]), _p(dx), _p(dg), _p(db), _p(part),
                        rows, D, 0, _p(add), _s()), "ln_bwd")
    return dx.reshape(ctx.shp), dg, db


class _LNAddFork(torch.autograd.Function):
    """(s, LayerNorm(s)) with s = y + r: the pre-norm block's residual add done by the
    LayerNorm kernel (it reads y and r, writes s) instead of the epilogue of the GEMM that
    produced y -- so that GEMM is a plain ring GEMM (no residual addend in its epilogue). Backward
    as _LNFork; y and r both receive the summed gradient."""

    @staticmethod
    def forward(ctx, y, r, g, b, eps, f8meta, f8box, grad_owner, codes_only=False):
        ctx.refs = (g, b)
        shp = y.shape
        D = shp[-1]
        y2 = y.reshape(-1, D).contiguous()
        r2 = r.reshape(-1, D).to(torch.bfloat16).contiguous()
        rows = y2.shape[0]
        xs = torch.empty_like(y2)
        h = torch.empty_like(y2)
        stats = torch.empty((2, rows), dtype=torch.float32, device=y.device)
        gf, bf = g.float().contiguous(), b.float().contiguous()
        lib = _load()
        if f8meta is not None:
            q = torch.empty((rows, D), dtype=torch.uint8, device=y.device)
            part = torch.empty(lib.pdt_ln_fwd_f8_blocks(rows) + 1, dtype=torch.float32, device=y.device)
            dq = part[-1:]
            _chk(lib.pdt_ln_add_fwd(_p(y2), _p(r2), _p(xs), _p(gf), _p(bf), None if codes_only else _p(h),
                                    _p(stats[0]), _p(stats[1]), rows, D, float(eps), _p(q), _p(f8meta), _p(part),
                                    _p(dq), _s()), "ln_add_fwd_f8")
            f8box.append((q, dq))
        else:
            _chk(lib.pdt_ln_add_fwd(_p(y2), _p(r2), _p(xs), _p(gf), _p(bf), _p(h), _p(stats[0]), _p(stats[1]), rows, D,
                                    float(eps), None, None, None, None, _s()), "ln_add_fwd")
        ctx.save_for_backward(xs, gf, stats)
        ctx.shp = shp
        ctx.grad_owner = grad_owner
        return xs.reshape(shp), h.reshape(shp)

    @staticmethod
    def backward(ctx, g_res, dy):
        if dy is None:
            return g_res, g_res, None, None, None, None, None, None, None
        dx, dg, db = _ln_fork_backward(ctx, g_res, dy)
        return dx, dx, dg, db, None, None, None, None, None


class _LNAddDropFork(torch.autograd.Function):
    """_LNAddFork under stochastic depth: s = r + scale[b] * y for sample b (``rps`` rows each),
    scale[b] 0 or 1/keep. A dropped sample's rows of y are not read and s holds r there. Backward:
    r receives the summed gradient dx as in _LNAddFork, y receives dyb = scale[b] * dx (+0 where
    dropped) written by the same kernel, and the e5m2 codes / bias gradient of the layer that
    produced y (``_pdt_f8g`` / ``_pdt_db``) are formed from dyb and ride on it."""

    @staticmethod
    def forward(ctx, y, r, g, b, eps, f8meta, f8box, grad_owner, codes_only, scale, rps):
        ctx.refs = (g, b)
        shp = y.shape
        D = shp[-1]
        y2 = y.reshape(-1, D).contiguous()
        r2 = r.reshape(-1, D).to(torch.bfloat16).contiguous()
        rows = y2.shape[0]
        sc = scale.detach().float().contiguous()
        assert sc.numel() * rps == rows and sc.device == y.device, (tuple(sc.shape), rps, rows)
        xs = torch.empty_like(y2)
        h = torch.empty_like(y2)
        stats = torch.empty((2, rows), dtype=torch.float32, device=y.device)
        gf, bf = g.float().contiguous(), b.float().contiguous()
        lib = _load()
        if f8meta is not None:
            q = torch.empty((rows, D), dtype=torch.uint8, device=y.device)
            part = torch.empty(lib.pdt_ln_fwd_f8_blocks(rows) + 1, dtype=torch.float32, device=y.device)
            dq = part[-1:]
            _chk(lib.pdt_ln_add_dp_fwd(_p(y2), _p(r2), _p(xs), _p(gf), _p(bf), None if codes_only else _p(h),
                                       _p(stats[0]), _p(stats[1]), rows, D, float(eps), _p(q), _p(f8meta), _p(part),
                                       _p(dq), _p(sc), rps, _s()), "ln_add_dp_fwd_f8")
            f8box.append((q, dq))
        else:
            _chk(lib.pdt_ln_add_dp_fwd(_p(y2), _p(r2), _p(xs), _p(gf), _p(bf), _p(h), _p(stats[0]), _p(stats[1]), rows,
                                       D, float(eps), None, None, None, None, _p(sc), rps, _s()), "ln_add_dp_fwd")
        ctx.save_for_backward(xs, gf, stats, sc)
        ctx.shp = shp
        ctx.grad_owner = grad_owner
        ctx.rps = rps
        return xs.reshape(shp), h.reshape(shp)

    @staticmethod
    def backward(ctx, g_res, dy):
        none = (None,) * 7
        if dy is None:  # the normalised output fed nothing: only the add's gradients
            sc = ctx.saved_tensors[3].repeat_interleave(ctx.rps).reshape(*ctx.shp[:-1], 1)
            gy = torch.where(sc != 0, g_res.float() * sc, torch.zeros((), device=sc.device)).to(g_res.dtype)
            return (gy, g_res, None, None) + none
        dyb, dx, dg, db = _ln_drop_backward(ctx, g_res, dy)
        return (dyb, dx, dg, db) + none


def _ln_drop_backward(ctx, g_res, dy):
    """:func:`_ln_fork_backward` for _LNAddDropFork: (dyb, dx, dgamma, dbeta), the fp8 side
    outputs taken from dyb and riding on it."""
    x2, gf, stats, sc = ctx.saved_tensors
    rows, D = x2.shape
    lib = _load()
    dev = x2.device
    dy2 = dy.reshape(rows, D).to(torch.bfloat16).contiguous()
    add = g_res.reshape(rows, D).to(torch.bfloat16).contiguous() if g_res is not None else None
    dx = torch.empty_like(x2)
    dyb = torch.empty_like(x2)
    blocks = lib.pdt_ln_bwd_blocks(rows)
    part = torch.empty(2 * blocks * D, dtype=torch.float32, device=dev)
    dg, db = _grad_buf(ctx.refs[0], (D,)), _grad_buf(ctx.refs[1], (D,))
    owner = ctx.grad_owner
    gmeta = getattr(owner, "_pdt_fp8_gmeta", None) if owner is not None else None
    codes = qpart = dq = cpart = pdb = None
    if gmeta is not None and fp8_settings()["scaling"] == "delayed":
        codes = torch.empty((rows, D), dtype=torch.uint8, device=dev)
        qpart = torch.empty(blocks + 1, dtype=torch.float32, device=dev)
        dq = qpart[-1:]
        bias = getattr(owner, "bias", None)
        if bias is not None and bias.requires_grad and os.environ.get("PDT_LN_DB", "1") == "1":
            pdb = _grad_buf(bias, (D,))
            cpart = torch.empty(blocks * D + lib.pdt_reduce_rows_work(blocks, D), dtype=torch.float32, device=dev)
    else:
        gmeta = None
    _chk(lib.pdt_ln_dp_bwd(_p(dy2), _p(x2), _p(gf), _p(stats[0]), _p(stats[1]), _p(dx), _p(dyb), _p(dg), _p(db),
                           _p(part), rows, D, 0, _p(add), _p(sc), ctx.rps, _p(codes), _p(gmeta), _p(qpart), _p(dq),
                           _p(cpart), _p(pdb), 0, _s()), "ln_dp_bwd")
    out = dyb.reshape(ctx.shp)
    if codes is not None:
        out._pdt_f8g = (codes, dq, owner)
        if pdb is not None:
            out._pdt_db = (pdb, owner)
    return out, dx.reshape(ctx.shp), dg, db


def ln_add_fork(y, r, ln, fp8_for=None, grad_fp8_for=None, scale=None, rows_per_sample=None):
    """(y + r, ln(y + r)) -- :func:`ln_fork` with the residual add done by the LayerNorm kernel
    (``grad_fp8_for``: the fp8 layer that produced ``y``). ``scale`` (fp32 [samples], each 0 or
    1/keep) with ``rows_per_sample``: stochastic depth, the sum is r + scale[sample] * y, formed
    by the kernel's drop-path instantiation (see _LNAddDropFork)."""
    D = ln.normalized_shape[-1]
    if (len(ln.normalized_shape) != 1 or D not in (256, 512, 768, 1024) or not ln.elementwise_affine
            or y.dtype != torch.bfloat16 or r.shape != y.shape):
        if scale is not None:
            fallback("ln_add_fork", f"normalized_shape {tuple(ln.normalized_shape)}, {y.dtype} with a drop-path "
                                    "scale (kernels: D in 256/512/768/1024, affine, bf16)")
            from ..drop_path import scaled_add
            return ln_fork(scaled_add(y, r, scale), ln, fp8_for, grad_fp8_for)
        return ln_fork(y + r.to(y.dtype), ln, fp8_for, grad_fp8_for)
    if scale is not None:
        rows = y.numel() // D
        rps = rows // scale.numel() if rows_per_sample is None else int(rows_per_sample)
        if scale.numel() * rps != rows:
            raise ValueError(f"ln_add_fork: {scale.numel()} scales x {rps} rows per sample != {rows} rows")
        return _apply_fork(_LNAddDropFork, (y, r), ln, fp8_for, grad_fp8_for, (scale, rps))
    return _apply_fork(_LNAddFork, (y, r), ln, fp8_for, grad_fp8_for)


def drop_path_scales(state, p, inv_keep, batch, rank=0):
    """The drop-path scale table [len(p), batch] (fp32) of this forward, filled on the device from
    ``state`` = [seed, step] (int32), which then advances by one (csrc/drop_path.hip)."""
    n = p.numel()
    assert state.dtype == torch.int32 and state.numel() == 2 and state.is_contiguous()
    assert p.dtype == torch.float32 and inv_keep.dtype == torch.float32 and inv_keep.numel() == n
    assert p.is_contiguous() and inv_keep.is_contiguous() and p.device == state.device == inv_keep.device
    table = torch.empty((n, int(batch)), dtype=torch.float32, device=state.device)
    _chk(_load().pdt_drop_path_scales(_p(table), _p(state), _p(p), _p(inv_keep), n, int(batch),
                                      int(rank) * int(batch), _s()), "drop_path_scales")
    return table


def ln_fork(x, ln, fp8_for=None, grad_fp8_for=None):
    """(x, ln(x)) with the residual gradient summed in LayerNorm's backward (see _LNFork).

    ``fp8_for``: the nn.Linear that consumes ln(x) in fp8. Under delayed scaling (once
    that layer's amax history exists) the LayerNorm kernel also writes the e4m3 codes
    of its output with the layer's scale and rolls its history, and the codes ride on
    the returned tensor (``_pdt_f8``) for the fp8 GEMM to pick up -- no separate
    quantisation pass over the activation. ``grad_fp8_for``: the fp8 layer whose OUTPUT
    gradient is this fork's input gradient (the residual-stream producer): the LayerNorm
    backward then also writes that layer's e5m2 gradient codes (``_pdt_f8g``)."""
    D = ln.normalized_shape[-1]
    if (len(ln.normalized_shape) != 1 or D not in (256, 512, 768, 1024) or not ln.elementwise_affine
            or x.dtype != torch.bfloat16):
        return x, layer_norm(x, ln)
    return _apply_fork(_LNFork, (x,), ln, fp8_for, grad_fp8_for)


def _apply_fork(fn, tensors, ln, fp8_for, grad_fp8_for, extra=()):
    """``fn`` (``_LNFork`` / ``_LNAddFork`` / ``_LNAddDropFork``) on its leading ``tensors`` (and
    trailing ``extra`` arguments) with the fp8 side outputs :func:`ln_fork` describes resolved: the
    returned LayerNorm output carries its e4m3 codes (``_pdt_f8``, and ``_pdt_f8_only`` when its
    bf16 values were not written)."""
    meta = None
    if fp8_for is not None and fp8_settings()["scaling"] == "delayed" and ln.normalized_shape[-1] % 128 == 0:
        meta = getattr(fp8_for, "_pdt_fp8_meta", None)
    box: list = []
    if os.environ.get("PDT_FP8_LN_GRAD", "1") == "0":
        grad_fp8_for = None
    only = meta is not None and _ln_codes_only(fp8_for)
    xo, h = fn.apply(*tensors, ln.weight, ln.bias, ln.eps, meta, box, grad_fp8_for, only, *extra)
    if box:
        h._pdt_f8 = (box[0][0], box[0][1], fp8_for)
        if only:
            h._pdt_f8_only = True
    return xo, h


def _ln_codes_only(fp8_for) -> bool:
    """The LayerNorm output's bf16 values are not written when its consumer (the fp8 layer
    ``fp8_for``: ViT's qkv / fc1) reads only its e4m3 codes -- an fp8 forward GEMM on the
    codes, and fp8 weight gradients that keep the codes instead of the bf16 input. The
    returned tensor carries ``_pdt_f8_only``; a consumer that would read the values refuses it
    (:func:`_prequant`). PDT_LN_CODES_ONLY=0 writes them anyway."""
    cfg = fp8_settings()
    return (os.environ.get("PDT_LN_CODES_ONLY", "1") == "1" and cfg["dgrad"] and cfg["wgrad"]
            and fp8_for.in_features % 128 == 0 and fp8_for.out_features % 128 == 0)
