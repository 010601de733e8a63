"""Float64 references, error metrics, guard-banded buffers and input families for the element
and row kernels (csrc/bn_act.hip, pool.hip, layernorm.hip, xent.hip), and a bit-exact numpy float32
mirror of the fp8 casts and their scaling state (csrc/fp8.hip), and float64 references, derived
bounds and input families for the bf16 attention kernels (csrc/attention.hip, attention_cls.hip,
the bf16 forward of attention_f8.hip; last section).

Used by tests/test_kernel_ref_cpu.py (which checks this module against PyTorch's float64 CPU ops
and against seeded faults) and by the GPU tests test_bn_act_kernels_gpu.py,
test_pool_kernels_gpu.py, test_row_kernels_gpu.py, test_fp8_cast_kernels_gpu.py and
test_attention_kernels_gpu.py. A plain module: no fixtures, no pytest settings.

Every reference is a formula on float64 tensors (the fp32 op is never called and upcast). Every
reference that feeds a bounded comparison also returns ``abs_terms``: the sum of the absolute
values of the terms of its expression, which is what an fp32 evaluation's rounding error is
proportional to.

Bounds (U = 2^-24, the unit roundoff of fp32)
---------------------------------------------
* One fp32 operation on operands a, b has error <= U * |result| <= U * (|a| + |b|). An expression
  evaluated with r roundings therefore errs by at most r * U * abs_terms to first order; the
  metrics allow 2 * r * U * abs_terms (the factor 2 absorbs the (1 + U)^r growth, the rounding of
  intermediate results that exceed the final one under cancellation, and FMA contraction choosing
  a different, never larger, set of roundings). The element kernels evaluate at most four
  roundings (y*scale, +shift, r*rscale + rshift, the add), hence the default 8 * U.
* A recursive fp32 sum of n terms errs by at most (n - 1) * U * sum|x_i|; a reduction is bounded
  with ``roundings`` = the longest chain of additions any one partial goes through.
* Rounding an fp32 value v to bf16 (8 significant bits) to nearest moves it by at most half a
  bf16 ulp, 2^-9 * 2^floor(log2|v|+1) <= 2^-8 * |v|.
* Exact family: integer-valued bf16 data in [-8, 8], integer means, power-of-two scales. Every
  fp32 product and partial sum is an integer multiple of a power of two below 2^24 times that
  unit, so it is exact, the result does not depend on the summation order, and it must EQUAL the
  float64 reference. A dropped, doubled or misaddressed row or column changes the result by at
  least one unit and is caught at any size.

Attention (csrc/attention.hip, the bf16 instantiation of attention_f8.hip, attention_cls.hip)
---------------------------------------------------------------------------------------------
Section "attention" below. The references are float64 formulas on the bf16 inputs; the backward
reference is a function of the ``out`` and ``lse`` the kernel is GIVEN (the tests hand it the
forward reference's own rounded ones), so it differs from the kernel by rounding only. Scores live
in the log2 domain: c = fp32(scale) * fp32(log2 e), one fp32 product as the launchers form it, and
lse = log2 sum_k 2^(c s_k). Per query q, with s_k = sum_d q_d k_d:

* eps_s, the absolute error of a computed c*s_k - m: s_k is an fp32 MFMA accumulation of 64 exact
  bf16 products (64 roundings), then the product with c, c's own rounding, the subtraction of the
  maximum (or of lse) and one spare: (64 + 4) roundings on terms of size <= c * sum_d |q_d k_d|,
  doubled as everywhere above: eps_s = 2 (64 + 4) U c max_k sum_d |q_d k_d|. (|c s_k - m| <=
  2 c max_k sum_d |q_d k_d|, which the doubling also covers.)
* eps_p, the relative error of one probability before it is packed: an absolute error e of the
  exponent is a relative error ln2 * e of 2^x. Forward: eps_p = ln2 eps_s + 2^-22. Backward, where
  the exponent is c s - lse with lse of any size: eps_p = ln2 (eps_s + U |lse|) + 2^-22. The
  2^-22 is an ALLOWANCE of 2 ulp for the hardware exp2 (v_exp_f32 is specified to 1 ulp), not a
  derived term; it is four orders of magnitude below the 2^-8 that follows. An error of the
  maximum m itself cancels: the same computed m enters every term and the normaliser.
* 2^-8: P (and dS) are rounded to bf16 before the second GEMM (pack_p), each by at most 2^-8 of
  itself.
* out = sum_k p_k v_k / l, A_out = sum_k p_k |v_k|: the output's own rounding 2^-8 |ref|; every
  numerator term is off by 2^-8 (packing) + eps_p, the normaliser l (summed from the UNROUNDED
  fp32 exponentials) by eps_p: (2^-8 + 2 eps_p) A_out; and 8 further fp32 roundings on terms of
  A_out (the accumulation steps of one MFMA chain count once each per 32 keys and are <= 8 at
  T <= 321 together with 1/l, the product with it and the rescales by alpha of the online
  kernels), doubled: 2 * 8 * U * A_out.
* lse = m + log2 l: the exponents are off by eps_s, which moves log2 sum 2^(x_k) by at most eps_s;
  the exp2 allowance moves l by 2^-22, log2 l by 2^-22 / ln2 <= 2^-21; log2f, the final add and
  m's own rounding: 4 U |ref|; the sum l: every lane adds at most half the keys of a tile in one
  chain (16 of 64, 16 of 32, or 4 per 16-key subtile), then 2 cross-lane adds and, in the online
  kernels, 3 roundings per tile (alpha, l * alpha, + ls); adding a zero is exact. That chain has
  n <= ln2 (T - 1) inexact steps for every kernel and T, so l is off by n U and log2 l by
  n U / ln2 <= (T - 1) U. Bound: eps_s + 2^-21 + 4 U |ref| + (T - 1) U.
* dV = P^T dO: 2^-8 |ref| + sum_q (2^-8 + eps_p(q)) p_qk |dO_q| + 2 * 8 * U sum_q p_qk |dO_q|.
* dS = p (dP - delta), dP = dO . v, delta = dO . out (64-term fp32 dot products: 2 * 64 U times
  their absolute terms): E_dS = (2^-8 + eps_p) p (|dP| + |delta|) + p (128 U sum_d |dO_d v_d| +
  128 U sum_d |dO_d out_d|), the first term being the packing of dS and the error of p.
  dQ = scale dS K, dK = scale dS^T Q: 2^-8 |ref| + scale sum E_dS |K or Q| + 2 * 8 * U scale
  sum |dS| |K or Q|.
* delta of the tiled path is an fp32 output: ``assert_f32_close`` with roundings = 64.
* The class-token kernel works in fp32 throughout, natural-log domain, scale 1/8 (exact): no
  packing term, no ln2 factor (eps_p = eps_s [+ U |lse|] + 2^-22 with c = 1/8; its dot products
  are 8 FMAs and 3 lane adds, fewer than the 64 + 4 allowed), and the sums over keys (o, dq) are
  chains of CLS_CHAIN = 16 roundings: <= 8 FMAs per thread (256 keys over 32 token groups), 3
  lane adds, 3 adds over the waves, 1/l and the product with it.
* Results below 2^-126 (fp32) or 2^-133 (bf16) flush to zero; every bound above is relative to a
  sum that holds a probability >= 1/T, so this needs no term.

Exact attention families: ``onehot`` (every query selects one key by a margin of >= 150 in c*s, so
every other fp32 probability is exactly 0 and P, l are exactly 1: out, dV are rows of V, dO and
dQ = dK = 0, all exactly) and ``counting`` (Q = 0: every key weighs exactly 1 before
normalisation, so a dropped or doubled (q, k) pair moves an output by >= 1 / ceil(T / 64) of
itself, against a bound of about 2^-8).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
BF16_HALF = 2.0 ** -8   # largest half-ulp of a bf16 rounding, relative
F64 = torch.float64


def f64(t):
    return None if t is None else t.detach().to(F64)


# ------------------------------------------------------------------------------------ metrics
def _where(bad, out, ref, bound):
    i = int(bad.reshape(-1).to(torch.uint8).argmax())
    return (f"{int(bad.sum())} of {bad.numel()} elements; first at flat index {i}: "
            f"out={out.reshape(-1)[i].item()!r} ref={ref.reshape(-1)[i].item()!r} "
            f"bound={bound.reshape(-1)[i].item()!r}")


def assert_close(out, ref64, bound64, what=""):
    """|out - ref| <= bound for every element. NaN / unwritten poison in ``out`` fails."""
    assert tuple(out.shape) == tuple(ref64.shape), (what, tuple(out.shape), tuple(ref64.shape))
    o = f64(out)
    bound64 = torch.as_tensor(bound64, dtype=F64, device=ref64.device).expand_as(ref64)
    ok = (o - ref64).abs() <= bound64  # NaN compares false
    assert bool(ok.all()), f"{what}: {_where(~ok, o, ref64, bound64)}"


def bf16_bound(ref64, abs_terms64, roundings=4, extra=0.0):
    return BF16_HALF * ref64.abs() + 2 * roundings * U * abs_terms64 + extra


def assert_bf16_close(out, ref64, abs_terms64, what="", roundings=4, extra=0.0):
    """bf16 ``out`` of an fp32 evaluation: |out - ref| <= 2^-8 |ref| + 2*roundings * 2^-24 * abs_terms
    (+ ``extra``, a separately derived or measured term). Derivation: module docstring."""
    assert out.dtype == torch.bfloat16, out.dtype
    assert_close(out, ref64, bf16_bound(ref64, abs_terms64, roundings, extra), what)


def assert_f32_close(out, ref64, abs_terms64, what="", roundings=4, extra=0.0):
    """fp32 ``out``: |out - ref| <= 2*roundings * 2^-24 * abs_terms + 2^-24 |ref| (+ ``extra``); the
    last term is the rounding of a result that was formed in higher precision."""
    assert out.dtype == torch.float32, out.dtype
    assert_close(out, ref64, 2 * roundings * U * abs_terms64 + U * ref64.abs() + extra, what)


def ulp_bf16(ref64):
    """bf16 ulp at |ref|: 2^(floor(log2 |ref|) - 7)."""
    _, e = torch.frexp(ref64.abs())  # |ref| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref64), e - 8)


def rounding_bias(out, ref64):
    """(mean of sign(ref) * (out - ref) / ulp_bf16(ref) over |ref| >= 2^-10, count)."""
    o, r = f64(out).reshape(-1), ref64.reshape(-1)
    keep = r.abs() >= 2.0 ** -10
    o, r = o[keep], r[keep]
    return (torch.sign(r) * (o - r) / ulp_bf16(r)).mean().item(), int(keep.sum())


def assert_unbiased_rounding(out, ref64, what="", min_count=2 ** 20):
    """Round-to-nearest leaves a signed error uniform in +-1/2 ulp: its mean over n elements is
    0 +- 1/sqrt(12 n) (0.0003 at n = 2^20). Truncation toward zero gives -0.5. Limit: 0.02."""
    bias, n = rounding_bias(out, ref64)
    assert n >= min_count, (what, n)
    assert abs(bias) < 0.02, (what, bias, n)


def assert_exact(out, ref64, what=""):
    """``out`` equals the float64 reference (exact family). The reference must be an fp32 value
    (which the exact family guarantees); a bf16 ``out`` is compared with its one rounding."""
    assert tuple(out.shape) == tuple(ref64.shape), (what, tuple(out.shape), tuple(ref64.shape))
    r32 = ref64.to(torch.float32)
    assert bool((r32.to(F64) == ref64).all()), f"{what}: reference is not exact in fp32"
    want = r32.to(out.dtype) if out.dtype.is_floating_point else ref64.to(out.dtype)
    bad = ~(f64(out) == f64(want))
    assert not bool(bad.any()), f"{what}: {_where(bad, f64(out), f64(want), torch.zeros_like(ref64))}"


# ------------------------------------------------------------------------- guarded allocator
GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF   # bf16 0xFFFF / fp32 0xFFFFFFFF are NaNs: an element never written fails a metric
_FRONT = 256 + 16    # the view starts 16-byte aligned but not 32-byte aligned
_BACK = 256
_live = []


def default_device():
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def guarded(shape, dtype, device=None, fill=None):
    """A contiguous tensor of ``shape`` that is a view into a larger byte buffer: it starts at byte
    272 (16-byte aligned, non-zero) and has >= 256 bytes of GUARD_BYTE on each side. The view is
    pre-filled with NaN poison (or ``fill``). ``check_guards()`` verifies every band."""
    device = default_device() if device is None else device
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = item * math.prod(shape)
    raw = torch.full((_FRONT + nbytes + _BACK,), GUARD_BYTE, dtype=torch.uint8, device=device)
    inner = raw[_FRONT:_FRONT + nbytes]
    inner.fill_(POISON_BYTE)
    view = inner.view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != raw.data_ptr()
    if fill is not None:
        view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    _live.append((raw, nbytes))
    return view


def check_guards(what=""):
    """Assert that no guard band of any buffer handed out since the last call was written, then
    forget those buffers."""
    try:
        for raw, nbytes in _live:
            front, back = raw[:_FRONT], raw[_FRONT + nbytes:]
            assert bool((front == GUARD_BYTE).all()), f"{what}: store before the start of a {nbytes}-byte buffer"
            if not bool((back == GUARD_BYTE).all()):
                off = int((back != GUARD_BYTE).to(torch.uint8).argmax())
                raise AssertionError(f"{what}: store {off} bytes past the end of a {nbytes}-byte buffer")
    finally:
        _live.clear()


# ---------------------------------------------------------------------------- input families
def gen(seed, device=None):
    g = torch.Generator(device=default_device() if device is None else device)
    g.manual_seed(seed)
    return g


def ints(shape, g, lo=-8, hi=8, dtype=torch.bfloat16):
    """Exact family: integers in [lo, hi]."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=g.device).to(dtype)


def normal(shape, g, dtype=torch.bfloat16, std=1.0, mean=0.0):
    """Conditioning family: random normal data, rounded to ``dtype`` (the reference sees the rounded data)."""
    return (torch.randn(tuple(shape), generator=g, device=g.device) * std + mean).to(dtype)


def pow2(shape, g, lo=-2, hi=2):
    """Signed powers of two 2^lo .. 2^hi (fp32)."""
    e = torch.randint(lo, hi + 1, tuple(shape), generator=g, device=g.device).to(torch.float32)
    s = torch.randint(0, 2, tuple(shape), generator=g, device=g.device).to(torch.float32) * 2 - 1
    return s * torch.exp2(e)


# ------------------------------------------------------------------------- BatchNorm forward
def bn_partials(x64):
    """[M, C] -> [2][1][C] (sum, sum of squares): what a conv epilogue hands to the finalize."""
    return torch.stack([x64.sum(0, keepdim=True), (x64 * x64).sum(0, keepdim=True)])


def bn_finalize_ref(part64, count, eps, momentum=0.0, gamma=None, beta=None, running_mean=None,
                    running_var=None, num_batches_tracked=None):
    """part [2][R][C] -> dict(mean, invstd, scale, shift, running_mean, running_var, nbt); the
    running variance takes the unbiased batch variance (count / (count - 1), count > 1)."""
    s, q = part64[0].sum(0), part64[1].sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mean) if gamma is None else f64(gamma)
    b = torch.zeros_like(mean) if beta is None else f64(beta)
    scale = g * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=b - mean * scale,
               shift_abs=b.abs() + (mean * scale).abs())
    if running_mean is not None:
        unb = var * count / (count - 1) if count > 1 else var
        out["running_mean"] = (1 - momentum) * f64(running_mean) + momentum * mean
        out["running_var"] = (1 - momentum) * f64(running_var) + momentum * unb
        out["running_mean_abs"] = ((1 - momentum) * f64(running_mean)).abs() + (momentum * mean).abs()
        out["running_var_abs"] = ((1 - momentum) * f64(running_var)).abs() + (momentum * unb).abs()
    if num_batches_tracked is not None:
        out["nbt"] = int(num_batches_tracked) + 1
    return out


def bn_apply_ref(y, scale, shift, res=None, rscale=None, rshift=None, relu=False):
    """out = relu?(y*scale + shift (+ res | + res*rscale + rshift)) over [M, C] -> (out, abs_terms)."""
    y, scale, shift = f64(y), f64(scale), f64(shift)
    out = y * scale + shift
    terms = (y * scale).abs() + shift.abs()
    if res is not None:
        r = f64(res)
        if rscale is not None:
            out = out + r * f64(rscale) + f64(rshift)
            terms = terms + (r * f64(rscale)).abs() + f64(rshift).abs()
        else:
            out = out + r
            terms = terms + r.abs()
    if relu:
        out = out.clamp_min(0.0)
    return out, terms


def relu_mask_ref(out):
    """bit k of byte i = (out[8 i + k] > 0); -0.0 and +0.0 give 0."""
    bits = (out.reshape(-1, 8) > 0).to(torch.int32)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=out.device)
    return (bits * w).sum(1).to(torch.uint8)


def mask_to_gate(mask, shape):
    """inverse of relu_mask_ref: uint8 [n/8] -> bool ``shape``."""
    k = torch.arange(8, device=mask.device, dtype=torch.int32)
    return (((mask.to(torch.int32)[:, None] >> k) & 1) != 0).reshape(shape)


# ------------------------------------------------------------------------ BatchNorm backward
def bn_bwd_sums_ref(dA, y, gate, mean):
    """g = dA where gate (all of dA if gate is None): (sum g, sum g*(y - mean)) and the sums of the
    absolute values of their terms, each [C]."""
    g = f64(dA) if gate is None else f64(dA) * gate.to(F64)
    t = g * (f64(y) - f64(mean))
    return g.sum(0), t.sum(0), g.abs().sum(0), t.abs().sum(0)


def bn_bwd_finalize_ref(s, q, count, gamma, mean, invstd):
    """dgamma, dbeta and the coefficients of dy = k1*g + k2*y + k3; also |terms| of k3."""
    ist, mu = f64(invstd), f64(mean)
    g = torch.ones_like(ist) if gamma is None else f64(gamma)
    k1 = g * ist
    k2 = -g * ist ** 3 * q / count
    k3a = -g * ist * s / count
    return dict(dgamma=q * ist, dbeta=s, k1=k1, k2=k2, k3=k3a - k2 * mu, k3_abs=k3a.abs() + (k2 * mu).abs())


def bn_bwd_apply_ref(dA, y, gate, k1, k2, k3):
    """(dy, abs_terms, dres): dres is the gated dA itself."""
    g = f64(dA) if gate is None else f64(dA) * gate.to(F64)
    y, k1, k2, k3 = f64(y), f64(k1), f64(k2), f64(k3)
    return k1 * g + k2 * y + k3, (k1 * g).abs() + (k2 * y).abs() + k3.abs(), g


# ----------------------------------------------------------------------------------- pooling
def pool_out(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def maxpool_fwd_ref(x, k, s, p):
    """x [N][H][W][C] -> (y [N][Ho][Wo][C], argmax uint8 = kh*k + kw). Windows are scanned in
    (kh, kw) order and only a strictly larger value replaces the best: the first maximum wins."""
    x = f64(x)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, s, p), pool_out(W, k, s, p)
    Hp, Wp = max(H + 2 * p, (Ho - 1) * s + k), max(W + 2 * p, (Wo - 1) * s + k)
    xp = torch.full((N, Hp, Wp, C), -math.inf, dtype=F64, device=x.device)
    xp[:, p:p + H, p:p + W] = x
    best = torch.full((N, Ho, Wo, C), -math.inf, dtype=F64, device=x.device)
    idx = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    for kh in range(k):
        for kw in range(k):
            cand = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
            take = cand > best
            best = torch.where(take, cand, best)
            idx = torch.where(take, torch.full_like(idx, kh * k + kw), idx)
    return best, idx


def maxpool_bwd_ref(dy, idx, H, W, k, s, p):
    """Scatter of dy [N][Ho][Wo][C] to the argmax positions -> (dx [N][H][W][C], abs_terms)."""
    dy = f64(dy)
    N, Ho, Wo, C = dy.shape
    Hp, Wp = max(H + 2 * p, (Ho - 1) * s + k), max(W + 2 * p, (Wo - 1) * s + k)
    dx = torch.zeros((N, Hp, Wp, C), dtype=F64, device=dy.device)
    ab = torch.zeros_like(dx)
    for kh in range(k):
        for kw in range(k):
            sel = (idx == kh * k + kw).to(F64)
            dx[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] += dy * sel
            ab[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] += dy.abs() * sel
    return dx[:, p:p + H, p:p + W].contiguous(), ab[:, p:p + H, p:p + W].contiguous()


def avgpool_fwd_ref(x):
    """x [N][HW][C] -> (y [N][C], abs_terms)."""
    x = f64(x)
    return x.mean(1), x.abs().mean(1)


def avgpool_bwd_ref(dy, HW):
    """dy [N][C] -> (dx [N][HW][C], abs_terms)."""
    dx = (f64(dy) / HW)[:, None, :].expand(-1, HW, -1).contiguous()
    return dx, dx.abs()


# --------------------------------------------------------------------------------- LayerNorm
def ln_fwd_ref(x, g, b, eps):
    """x [rows][D] -> dict(mean, rstd, y, y_abs, xhat, var)."""
    x, g, b = f64(x), f64(g), f64(b)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    return dict(mean=mean[:, 0], rstd=rstd[:, 0], var=var[:, 0], xhat=xh, y=xh * g + b,
                y_abs=(x * rstd * g).abs() + (mean * rstd * g).abs() + b.abs())


def ln_bwd_ref(dy, x, g, mean, rstd, addend=None, dg0=None, db0=None):
    """LayerNorm backward from given row statistics; ``dg0`` / ``db0``: accumulate into them."""
    dy, x, g = f64(dy), f64(x), f64(g)
    mean, rstd = f64(mean)[:, None], f64(rstd)[:, None]
    xh = (x - mean) * rstd
    gy = dy * g
    m1, m2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    m1a, m2a = gy.abs().mean(1, keepdim=True), (gy * xh).abs().mean(1, keepdim=True)
    dx = rstd * (gy - m1 - xh * m2)
    dx_abs = rstd.abs() * (gy.abs() + m1.abs() + (xh * m2).abs())
    if addend is not None:
        dx, dx_abs = dx + f64(addend), dx_abs + f64(addend).abs()
    dg, db = (dy * xh).sum(0), dy.sum(0)
    dg_abs, db_abs = (dy * xh).abs().sum(0), dy.abs().sum(0)
    if dg0 is not None:
        dg, db = dg + f64(dg0), db + f64(db0)
        dg_abs, db_abs = dg_abs + f64(dg0).abs(), db_abs + f64(db0).abs()
    return dict(dx=dx, dx_abs=dx_abs, dx_mean_abs=rstd.abs() * (m1a + xh.abs() * m2a),
                dgamma=dg, dbeta=db, dgamma_abs=dg_abs, dbeta_abs=db_abs)


GELU_C = math.sqrt(2.0 / math.pi)


def gelu_tanh_ref(z):
    """0.5 z (1 + tanh(u)), u = sqrt(2/pi) (z + 0.044715 z^3)."""
    z = f64(z)
    return 0.5 * z * (1 + torch.tanh(GELU_C * (z + 0.044715 * z ** 3)))


def gelu_tanh_grad_ref(z):
    """d/dz [0.5 z (1 + tanh(u))], u = sqrt(2/pi) (z + 0.044715 z^3)."""
    z = f64(z)
    t = torch.tanh(GELU_C * (z + 0.044715 * z ** 3))
    return 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * GELU_C * (1 + 3 * 0.044715 * z * z)


# ----------------------------------------------------------------------------- cross-entropy
def xent_ref(logits, target, eps, gout=1.0):
    """Mean-reduced cross-entropy with label smoothing over [B][V] ->
    dict(lse, loss_rows, loss, dlogits); dlogits = gout/B * (softmax - (1-eps) onehot - eps/V)."""
    x = f64(logits)
    B, V = x.shape
    m = x.max(1, keepdim=True).values
    lse = (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))[:, 0]
    xt = x.gather(1, target.view(-1, 1))[:, 0]
    rows = lse - (1 - eps) * xt - eps * x.mean(1)
    onehot = torch.zeros_like(x).scatter_(1, target.view(-1, 1), 1.0)
    p = torch.exp(x - lse[:, None])
    return dict(lse=lse, loss_rows=rows, loss=rows.sum() / B, softmax=p,
                loss_rows_abs=lse.abs() + ((1 - eps) * xt).abs() + eps * x.abs().mean(1),
                dlogits=gout / B * (p - (1 - eps) * onehot - eps / V),
                dlogits_abs=abs(gout) / B * (p + (1 - eps) * onehot + eps / V))


def colsum_ref(x, out0=None):
    """x [R][C] -> (column sums [C] (+ out0), abs_terms)."""
    x = f64(x)
    s, a = x.sum(0), x.abs().sum(0)
    if out0 is not None:
        s, a = s + f64(out0), a + f64(out0).abs()
    return s, a


# ------------------------------------------------------------- exact-family inputs (shared)
# tests/test_kernel_ref_cpu.py checks on the CPU that an fp32 evaluation of each of these equals
# the float64 reference; the GPU tests feed the same generators to the kernels.
def exact_partials(R, C, g):
    """BatchNorm partial sums [2][R][C] fp32: integer sums in [-8, 8], integer sums of squares in
    [8, 16] (so the variance is positive at count = 16 R). |sum| <= 16 * 2049 << 2^24."""
    return torch.stack([ints((R, C), g, dtype=torch.float32), ints((R, C), g, 8, 16, dtype=torch.float32)])


def exact_bn_bwd_inputs(M, C, g):
    """dA, y: integers in [-8, 8] (bf16); mean: integers in [-2, 2]. |g (y - mean)| <= 80, so a
    sum over M <= 2^17 rows stays below 2^24."""
    assert M <= 2 ** 17
    return ints((M, C), g), ints((M, C), g), ints((C,), g, -2, 2, dtype=torch.float32)


def exact_ln_bwd_inputs(rows, D, g):
    """dy, x, addend: integers in [-8, 8]; gamma: +-2^-1..2^1; mean: integers in [-2, 2]; rstd:
    1/2 or 1. xhat is a multiple of 1/2 below 10, dy*xhat a multiple of 1/2 below 80 (rows <= 2^16:
    sums < 2^24 halves), and every term of dx a multiple of 1/(8 D) below 1640 (D <= 1024:
    < 2^24 units)."""
    assert rows <= 2 ** 16 and D <= 1024
    return dict(dy=ints((rows, D), g), x=ints((rows, D), g), addend=ints((rows, D), g),
                gamma=pow2((D,), g, -1, 1), mean=ints((rows,), g, -2, 2, dtype=torch.float32),
                rstd=torch.exp2(-ints((rows,), g, 0, 1, dtype=torch.float32)))


# ------------------------------------------------------------------------- fp8 quantization
# csrc/fp8.hip, mirrored operation by operation in numpy float32: one correctly rounded divide
# (scale = FMAX / amax), one multiply (x * scale), the clamp to +-FMAX and one round to nearest
# even. Each of these is a single IEEE operation, so the mirror is exact and the GPU tests compare
# codes, dq, partials and the scaling state with equality. No library fp8 cast is used here:
# fp8_encode works on the bits of the float32 pattern, fp8_decode from the format's formula.
FP8_FMAX = (448.0, 57344.0)      # fmt 0 = OCP e4m3fn (no infinity), 1 = OCP e5m2
FP8_MAX_CODE = (0x7E, 0x7B)
_FP8_MBITS = (3, 2)
_FP8_EMIN = (-6, -14)            # exponent of the smallest normal
FP8_META_WORDS = 21
FP8_HIST = 16


def _np32(x):
    """float32 numpy array of a tensor (any device, bf16 or fp32), an array or a scalar."""
    if torch.is_tensor(x):
        x = x.detach().to(torch.float32).cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def fp8_encode(v32, fmt):
    """float32 array -> uint8 OCP fp8 codes: fminf(fmaxf(v, -FMAX), FMAX), then round to nearest
    even (into the subnormal range too), the sign of zero kept. NaN goes where that clamp sends it:
    fmaxf(NaN, -FMAX) = -FMAX, so to the -FMAX code whatever its sign bit."""
    v32 = _np32(v32)
    M, emin = _FP8_MBITS[fmt], _FP8_EMIN[fmt]
    bits = v32.view(np.uint32).astype(np.uint64)
    sign = (bits >> np.uint64(31)) << np.uint64(7)
    mag = bits & np.uint64(0x7FFFFFFF)
    nan = mag > np.uint64(0x7F800000)
    fmax_bits = np.uint64(np.array(FP8_FMAX[fmt], dtype=np.float32).view(np.uint32))
    mag = np.minimum(mag, fmax_bits)                      # the clamp (infinity included)
    e = (mag >> np.uint64(23)).astype(np.int64) - 127     # (fp32 subnormals: e = -127, far below half
    sig = (mag & np.uint64(0x7FFFFF)) | np.uint64(1 << 23)  # the smallest code, they round to 0)
    et = np.maximum(e, emin)                              # exponent of the target binade
    shift = np.minimum(23 - M + (et - e), 40).astype(np.uint64)
    k = sig >> shift
    rem = sig & ((np.uint64(1) << shift) - np.uint64(1))
    half = np.uint64(1) << (shift - np.uint64(1))
    up = (rem > half) | ((rem == half) & ((k & np.uint64(1)) == np.uint64(1)))
    k = k + up.astype(np.uint64)
    # normal: k in [2^M, 2^(M+1)] -> ((e - emin + 1) << M) + k - 2^M; subnormal: the code is k itself
    code = ((et - emin).astype(np.uint64) << np.uint64(M)) + k
    code = np.where(mag == 0, np.uint64(0), code) | sign
    code = np.where(nan, np.uint64(0x80 | FP8_MAX_CODE[fmt]), code)
    return code.astype(np.uint8)


def _fp8_table(fmt):
    M, emin = _FP8_MBITS[fmt], _FP8_EMIN[fmt]
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        eb, m = (c & 0x7F) >> M, c & ((1 << M) - 1)
        if fmt == 0 and (c & 0x7F) == 0x7F:
            v = math.nan
        elif fmt == 1 and eb == 31:
            v = math.inf if m == 0 else math.nan
        elif eb == 0:
            v = m * 2.0 ** (emin - M)
        else:
            v = (1 + m / 2.0 ** M) * 2.0 ** (eb - 1 + emin)
        t[c] = -v if c & 0x80 else v
    return t


_FP8_TABLE = (_fp8_table(0), _fp8_table(1))


def fp8_decode(codes, fmt):
    """uint8 codes -> float64 values (NaN / inf codes included), from the format's formula."""
    if torch.is_tensor(codes):
        codes = codes.detach().cpu().numpy()
    return _FP8_TABLE[fmt][np.asarray(codes, dtype=np.uint8)]


def fp8_finite_codes(fmt):
    """Every code with a finite value, both signs (254 for e4m3fn, 248 for e5m2)."""
    return np.array([c for c in range(256) if (c & 0x7F) <= FP8_MAX_CODE[fmt]], dtype=np.uint8)


def fp8_midpoints(fmt):
    """float64 midpoints between adjacent non-negative values, from 0 | smallest subnormal up to
    the one below FMAX, and the codes on either side. All are exact in float32."""
    lo = np.arange(0, FP8_MAX_CODE[fmt], dtype=np.uint8)
    return (fp8_decode(lo, fmt) + fp8_decode(lo + 1, fmt)) / 2, lo, lo + 1


def fp8_scale(amax32, fmt):
    """scale_from: float32(FMAX) / amax if amax > 0 else 1, one float32 divide."""
    a = np.float32(amax32)
    with np.errstate(all="ignore"):
        return np.float32(FP8_FMAX[fmt]) / a if a > 0 else np.float32(1)


def fp8_dq(s32):
    with np.errstate(all="ignore"):
        return np.float32(1) / np.float32(s32)


def fp8_cast_ref(x, s32, fmt):
    """codes of float32(x) * float32(s), the multiply in float32."""
    with np.errstate(all="ignore"):
        return fp8_encode(_np32(x) * np.float32(s32), fmt)


def fp8_amax(x):
    """max |x| as the kernels form it: fmaxf from 0, which drops NaN."""
    a = np.abs(_np32(x)).reshape(-1)
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def fp8_amax_partials(x, nblk):
    """pdt_amax_partial's index map: block b reduces elements [2048 (b + k nblk), + 2048), k = 0, 1, ..."""
    a = np.abs(_np32(x)).reshape(-1)
    a = np.where(np.isnan(a), np.float32(0), a)
    chunks = -(-a.size // 2048)
    rounds = -(-chunks // nblk)
    pad = np.zeros(rounds * nblk * 2048, dtype=np.float32)
    pad[:a.size] = a
    return pad.reshape(rounds, nblk, 2048).max(axis=(0, 2))


def _f32_bits(v):
    return int(np.array(v, dtype=np.float32).view(np.uint32))


class fp8_meta_ref:
    """The 21-word delayed-scaling state of csrc/fp8.hip in plain Python: [0] scale in use, [1] dq
    of the last cast, [2] amax of the running cast (bits), [3] unused, [4] history index (integer),
    [5 .. 21) amax history. seed / roll / roll_partial are the three kernels that write it."""

    def __init__(self, fmt, words=None):
        self.fmt = fmt
        self.scale, self.dq, self.amax, self.unused, self.idx = np.float32(0), np.float32(0), np.float32(0), 0, 0
        self.hist = [np.float32(0)] * FP8_HIST
        if words is not None:
            w = np.asarray(words, dtype=np.uint32)
            f = w.view(np.float32)
            self.scale, self.dq, self.amax = f[0], f[1], f[2]
            self.unused, self.idx = int(w[3]), int(w[4])
            self.hist = [f[5 + i] for i in range(FP8_HIST)]

    def seed(self, amax32):
        self.hist = [np.float32(0)] * FP8_HIST
        self.hist[0] = np.float32(amax32)
        self.idx, self.amax, self.unused = 1, np.float32(0), 0
        self.scale = fp8_scale(amax32, self.fmt)
        self.dq = fp8_dq(self.scale)

    def roll(self, amax32):
        """One delayed cast of a tensor with this amax: returns (scale it was cast with, dq_out)."""
        used, dq = self.scale, fp8_dq(self.scale)
        cur = np.float32(max(np.float32(amax32), self.amax))  # atomicMax onto the slot's content
        self.hist[self.idx % FP8_HIST] = cur
        self.idx += 1
        h = np.float32(0)
        for v in self.hist:
            h = v if v > h else h  # fmaxf from 0
        self.dq = dq
        self.scale = fp8_scale(h, self.fmt)
        self.amax = np.float32(0)
        return used, dq

    def roll_partial(self, partials):
        """pdt_fp8_meta_roll_partial: the amax is the largest partial or the slot, whichever is larger."""
        return self.roll(fp8_amax(partials))

    def words(self):
        """The state as 21 uint32 words, for a bitwise comparison with the device's."""
        w = [_f32_bits(self.scale), _f32_bits(self.dq), _f32_bits(self.amax), self.unused, self.idx & 0xFFFFFFFF]
        return np.array(w + [_f32_bits(v) for v in self.hist], dtype=np.uint32)


def meta_words(meta):
    """A device meta tensor (21 fp32 words) as uint32 numpy words."""
    return meta.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).copy()


def assert_same_bits(out, ref, what=""):
    """Bitwise equality of two arrays / tensors of the same item size (codes, float32 words):
    zero mismatches, and NaNs compare by pattern."""
    def raw(t):
        if torch.is_tensor(t):
            t = t.detach().cpu().contiguous()
            t = t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).numpy()
        t = np.ascontiguousarray(t)
        return t.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.itemsize])
    o, r = raw(out), raw(ref)
    assert o.shape == r.shape, (what, o.shape, r.shape)
    bad = o != r
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ; first at flat index {i}: "
                             f"out=0x{int(o.reshape(-1)[i]):x} ref=0x{int(r.reshape(-1)[i]):x}")


def fp8_exhaustive_inputs(fmt, s32):
    """(bf16 bit patterns int16 tensor, float32 array) for the exhaustive rounding test at scale s:
    every bf16 pattern that is not a NaN (+-inf and both zeros kept); and the same values as float32
    followed by, for every code midpoint m (and FMAX plus half a step) and both signs, float32(m / s)
    and its two float32 neighbours. At a power-of-two s these are exact ties and one ulp either side."""
    pat = np.arange(65536, dtype=np.uint32)
    pat = pat[~(((pat & 0x7F80) == 0x7F80) & ((pat & 0x7F) != 0))]
    as32 = (pat << 16).astype(np.uint32).view(np.float32)
    mids, _, _ = fp8_midpoints(fmt)
    top = FP8_FMAX[fmt] + (FP8_FMAX[fmt] - fp8_decode(np.uint8(FP8_MAX_CODE[fmt] - 1), fmt)) / 2
    m = (np.append(mids, top) / np.float64(np.float32(s32))).astype(np.float32)
    near = np.concatenate([np.nextafter(m, np.float32(0)), m, np.nextafter(m, np.float32(np.inf))])
    x32 = np.concatenate([as32, near, -near]).astype(np.float32)
    return torch.from_numpy(pat.astype(np.uint16).view(np.int16).copy()), x32


def fp8_boundary_check(codes, prod64, absx64, s32, allow, fmt, what=""):
    """The condition on codes of a product x * f(z) whose fp32 factor f is only known to within
    ``allow`` of the float64 one: a code may differ from fp8_cast_ref(float32(prod64), s) only by
    one step, and only where prod64 * s lies within allow * |x| * s of a rounding boundary (a
    midpoint between adjacent values, or 0 between the two zeros). Returns the number of codes that differ."""
    if torch.is_tensor(codes):
        codes = codes.detach().cpu().numpy()
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    p = np.asarray(prod64, dtype=np.float64).reshape(-1)
    ax = np.asarray(absx64, dtype=np.float64).reshape(-1)
    s = np.float64(np.float32(s32))
    ref = fp8_cast_ref(p.astype(np.float32), s32, fmt).reshape(-1)
    diff = codes != ref
    if diff.any():
        # (0 is a boundary too: it separates the codes of -0 and +0, which count as adjacent)
        mids = np.sort(np.concatenate([fp8_midpoints(fmt)[0], [0.0], -fp8_midpoints(fmt)[0]]))
        t = p * s
        j = np.clip(np.searchsorted(mids, t), 1, mids.size - 1)
        dist = np.minimum(np.abs(t - mids[j - 1]), np.abs(t - mids[j]))
        near = dist <= allow * ax * s

        def order(c):  # signed position of a code among the values
            c = c.astype(np.int64)
            return np.where(c & 0x80, -(c & 0x7F), c & 0x7F)
        step = np.abs(order(codes) - order(ref)) <= 1
        bad = diff & ~(near & step)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what}: {int(bad.sum())} codes differ away from a rounding boundary or by more "
                                 f"than a step; first at {i}: out=0x{codes[i]:02x} ref=0x{ref[i]:02x} "
                                 f"product*s={t[i]!r} distance={dist[i]!r} allowed={allow * ax[i] * s!r}")
    return int(diff.sum())


FP8_PLANT = 17.25


def fp8_cast_inputs(n, bf16, seed, fmt=0):
    """float32 array for the current-scaling cast tests: normal data of std 3 with |x| < 16 (so a
    planted +-17.25 is the amax), bf16-representable when ``bf16``. A product of a bf16 value by
    FMAX / 17.25 never comes within an fp32 ulp of a tie, so on bf16 data x / dq and x * s give the
    same codes; the fp32 data of n >= 2047 therefore carries, from index 64 on and with alternating
    signs, float32(m / s) and its two neighbours for every code midpoint m below 15.5 s."""
    x = (torch.randn(n, generator=gen(seed, torch.device("cpu"))) * 3).clamp(-15.5, 15.5)
    if bf16:
        return x.to(torch.bfloat16).float().numpy()
    x = x.numpy()
    if n >= 2047:
        s = fp8_scale(FP8_PLANT, fmt)
        m = (fp8_midpoints(fmt)[0] / np.float64(s)).astype(np.float32)
        m = m[m < 15.5]
        near = np.stack([np.nextafter(m, np.float32(0)), m, np.nextafter(m, np.float32(np.inf))], 1).reshape(-1)
        near[1::2] *= -1
        assert 64 + near.size <= 2040
        x[64:64 + near.size] = near
    return x


def fp8_script():
    """(amax of the seeding tensor, amaxes of the 40 delayed casts that follow): every value is a
    bf16 number. The seed (4) is larger than every ordinary step (<= 3), step 2 is a spike (64) and
    step 9 an all-zero tensor: the scale must forget the seed 16 rolls after it and the spike
    exactly 16 steps after it entered."""
    steps = [0.75 + 0.25 * ((3 * k) % 10) for k in range(40)]
    steps[2], steps[9] = 64.0, 0.0
    return 4.0, steps


def fp8_boundary_scale(allow, xmax, fmt):
    """The scale for fp8_boundary_check's cases: the condition allows one step, so the uncertainty
    allow * |x| * s must stay below half the smallest step of the format (2^-10 for e4m3, 2^-17 for
    e5m2). The largest power of two that keeps it there, times 7/8 so that it is no power of two,
    and at most FMAX / 5."""
    half_step = 2.0 ** (_FP8_EMIN[fmt] - _FP8_MBITS[fmt] - 1)
    p = 2.0 ** math.floor(math.log2(half_step / (allow * xmax)))
    return np.float32(min(p * 0.875, FP8_FMAX[fmt] / 5))


# --------------------------------------------------------------------------------- attention
# csrc/attention.hip, the bf16 instantiation of csrc/attention_f8.hip (pdt_attn_fwd_tiles) and
# csrc/attention_cls.hip. qkv is [B][T][3][H][64], out / dout [B][T][H*64], lse / delta [B*H][T].
# Bounds: module docstring, "Attention".
LN2 = math.log(2.0)
SCORE_ROUNDINGS = 64 + 4     # eps_s
EXP2_ALLOW = 2.0 ** -22      # 2 ulp for the hardware exp2 (an allowance)
LSE_EXP2 = 2.0 ** -21        # >= EXP2_ALLOW / ln2
ACC_ROUNDINGS = 8            # fp32 roundings of an accumulator after the second GEMM
DOT_ROUNDINGS = 64           # dP, delta: 64-term fp32 dot products
CLS_CHAIN = 16               # the class-token kernel's sums over keys
ONEHOT_GAP = 150.0


def attn_c(scale):
    """scale * log2(e) as the launchers form it: one fp32 product of two fp32 numbers."""
    return float(np.float32(scale) * np.float32(1.4426950408889634))


def attn_heads(qkv, H):
    """[B][T][3*H*64] -> float64 q, k, v, each [B][H][T][64]."""
    B, T, _ = qkv.shape
    q, k, v = f64(qkv).view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    return q, k, v


def attn_rows(x, H):
    """[B][T][H*64] -> float64 [B][H][T][64]."""
    B, T, _ = x.shape
    return f64(x).view(B, T, H, 64).transpose(1, 2)


def attn_flat(x):
    """[B][H][T][64] -> [B][T][H*64]."""
    B, H, T, _ = x.shape
    return x.transpose(1, 2).reshape(B, T, H * 64)


def _attn_pack3(dq, dk, dv):
    """three [B][H][T][64] -> [B][T][3*H*64]."""
    B, H, T, _ = dq.shape
    return torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * 64)


def _top_gap(cs):
    """Smallest distance over all queries between the largest and the second largest of cs[..., :]."""
    if cs.shape[-1] < 2:
        return math.inf
    top = cs.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def attn_fwd_ref(qkv, H, scale):
    """dict(out [B][T][H*64], lse [B*H][T] (log2 domain of the scaled scores), A_out = sum_k p_k |v_k|,
    sabs [B*H][T] = max_k sum_d |q_d k_d|, eps_s, out_bound, lse_bound, gap = the smallest margin in
    c*s between a query's best and second-best key)."""
    q, k, v = attn_heads(qkv, H)
    B, _, T, _ = q.shape
    c = attn_c(scale)
    cs = c * (q @ k.transpose(-1, -2))
    m = cs.max(-1, keepdim=True).values
    e = torch.exp2(cs - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    lse = (m + torch.log2(l)).reshape(B * H, T)
    out, A = attn_flat(P @ v), attn_flat(P @ v.abs())
    sabs = (q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values   # [B][H][T][1]
    eps_s = 2 * SCORE_ROUNDINGS * U * c * sabs
    eps_p = attn_flat((LN2 * eps_s + EXP2_ALLOW).expand(B, H, T, 64))
    return dict(out=out, lse=lse, A_out=A, sabs=sabs.reshape(B * H, T), eps_s=eps_s.reshape(B * H, T), c=c,
                gap=_top_gap(cs),
                out_bound=BF16_HALF * out.abs() + (BF16_HALF + 2 * eps_p) * A + 2 * ACC_ROUNDINGS * U * A,
                lse_bound=eps_s.reshape(B * H, T) + LSE_EXP2 + 4 * U * lse.abs() + (T - 1) * U)


def attn_bwd_ref(qkv, out, dout, lse, H, scale):
    """The backward as a function of what the kernel is given (``out`` bf16, ``lse`` fp32):
    P = exp2(c S - lse), dP = dO V^T, delta = rowsum(dO o out), dS = P o (dP - delta),
    dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO -> dict(dqkv [B][T][3*H*64], dqkv_bound,
    delta [B*H][T], delta_abs)."""
    q, k, v = attn_heads(qkv, H)
    B, _, T, _ = q.shape
    o, do = attn_rows(out, H), attn_rows(dout, H)
    L = f64(lse).view(B, H, T, 1)
    c, sc = attn_c(scale), float(np.float32(scale))
    kt, vt = k.transpose(-1, -2), v.transpose(-1, -2)
    P = torch.exp2(c * (q @ kt) - L)
    dP = do @ vt
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ, dK, dV = sc * (dS @ k), sc * (dS.transpose(-1, -2) @ q), P.transpose(-1, -2) @ do
    eps_s = 2 * SCORE_ROUNDINGS * U * c * (q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values
    eps_p = LN2 * (eps_s + U * L.abs()) + EXP2_ALLOW                            # per query [B][H][T][1]
    delta_abs = (do * o).abs().sum(-1, keepdim=True)
    E = (BF16_HALF + eps_p) * P * (dP.abs() + delta.abs()) + \
        P * (2 * DOT_ROUNDINGS * U * (do.abs() @ vt.abs()) + 2 * DOT_ROUNDINGS * U * delta_abs)
    acc = 2 * ACC_ROUNDINGS * U
    bV = BF16_HALF * dV.abs() + ((BF16_HALF + eps_p) * P).transpose(-1, -2) @ do.abs() + \
        acc * (P.transpose(-1, -2) @ do.abs())
    bQ = BF16_HALF * dQ.abs() + sc * (E @ k.abs()) + acc * sc * (dS.abs() @ k.abs())
    bK = BF16_HALF * dK.abs() + sc * (E.transpose(-1, -2) @ q.abs()) + acc * sc * (dS.abs().transpose(-1, -2) @ q.abs())
    return dict(dqkv=_attn_pack3(dQ, dK, dV), dqkv_bound=_attn_pack3(bQ, bK, bV),
                delta=delta.reshape(B * H, T), delta_abs=delta_abs.reshape(B * H, T))


def attn_cls_ref(qkv, H, dout=None, o=None, lse=None):
    """Token 0's query against all keys (header of csrc/attention_cls.hip): natural-log domain,
    scale 1/8, fp32 throughout. Forward: dict(out [B][H*64], lse [B*H], out_bound, lse_bound, gap).
    With ``dout`` [B][H*64] and the ``o`` (bf16) and ``lse`` (fp32) the kernel is given, also
    dqkv [B][T][3*H*64] and dqkv_bound (dq of every token but 0: exactly 0, bound 0)."""
    q, k, v = attn_heads(qkv, H)
    B, _, T, _ = q.shape
    q0 = q[:, :, :1]
    kt = k.transpose(-1, -2)
    s = 0.125 * (q0 @ kt)                                                        # [B][H][1][T]
    eps_s = 2 * SCORE_ROUNDINGS * U * 0.125 * (q0.abs() @ kt.abs()).max(-1, keepdim=True).values
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    L = (m + torch.log(l)).reshape(B * H)
    out, A = (P @ v).reshape(B, H * 64), (P @ v.abs()).reshape(B, H * 64)
    eps_p = (eps_s + EXP2_ALLOW).expand(B, H, 1, 64).reshape(B, H * 64)
    ref = dict(out=out, lse=L, gap=_top_gap(s) / LN2,
               out_bound=BF16_HALF * out.abs() + 2 * eps_p * A + 2 * CLS_CHAIN * U * A,
               lse_bound=eps_s.reshape(B * H) + LSE_EXP2 + 4 * U * L.abs() + (T - 1) * U)
    if dout is None:
        return ref
    do, og = f64(dout).view(B, H, 1, 64), f64(o).view(B, H, 1, 64)
    Lg = f64(lse).view(B, H, 1, 1)
    P = torch.exp(s - Lg)
    dP = do @ v.transpose(-1, -2)                                                # [B][H][1][T]
    delta = (do * og).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    eps_p = eps_s + U * Lg.abs() + EXP2_ALLOW
    E = eps_p * P * (dP.abs() + delta.abs()) + \
        P * (2 * DOT_ROUNDINGS * U * (do.abs() @ v.abs().transpose(-1, -2)) +
             2 * DOT_ROUNDINGS * U * (do * og).abs().sum(-1, keepdim=True))
    acc = 2 * ACC_ROUNDINGS * U
    dQ, bQ = torch.zeros_like(q), torch.zeros_like(q)
    dQ[:, :, :1] = 0.125 * (dS @ k)
    bQ[:, :, :1] = BF16_HALF * dQ[:, :, :1].abs() + 0.125 * (E @ k.abs()) + 2 * CLS_CHAIN * U * 0.125 * (dS.abs() @ k.abs())
    dSt, Et, Pt = dS.transpose(-1, -2), E.transpose(-1, -2), P.transpose(-1, -2)  # [B][H][T][1]
    dK = 0.125 * dSt * q0
    bK = BF16_HALF * dK.abs() + 0.125 * Et * q0.abs() + acc * 0.125 * dSt.abs() * q0.abs()
    dV = Pt * do
    bV = BF16_HALF * dV.abs() + (eps_p * P).transpose(-1, -2) * do.abs() + acc * Pt * do.abs()
    ref.update(dqkv=_attn_pack3(dQ, dK, dV), dqkv_bound=_attn_pack3(bQ, bK, bV))
    return ref


ATTN_FAMILIES = ("onehot", "counting", "negative", "normal", "peaked")


def attn_inputs(family, B, T, H, seed, device=None):
    """dict(qkv bf16 [B][T][3*H*64], dout bf16 [B][T][H*64], sel) of one input family; every
    (batch, head) gets different data.

    onehot    K rows random +-8, Q[q] = 2 K[sel[q]] for a random permutation sel per (b, h) with
              sel[0] = T - 1 and sel[T - 1] = 0 forced ("onehot0": sel[0] = 0, sel[T - 1] = T - 1),
              V and dO integers in [-8, 8]. Raw selected score 64 * 128 = 8192; ``sel`` [B][H][T].
    counting  Q = 0, K random integers, V[k] = 8 onehot((k + 5 bh) mod 64), dO[q] = 8 onehot((q + 11 bh)
              mod 64) with bh = b H + h: out[q][d] = 8 n_d / T.
    negative  K = |N(0,1)|, Q = -|N(0,1)|: every score far below the 0 of a padded (zero) key.
    normal    N(0, 1.5^2), the regime of the older tests; dO N(0,1).
    peaked    as normal with Q of std 4: probabilities span > 2^30 in a row, maxima anywhere."""
    device = default_device() if device is None else device
    g = gen(seed, device)
    shape = (B, H, T, 64)
    sel = None

    def rnd(std):
        return torch.randn(shape, generator=g, device=device) * std

    if family in ("onehot", "onehot0"):
        k = (torch.randint(0, 2, shape, generator=g, device=device) * 16 - 8).to(torch.float32)
        sel = torch.empty((B, H, T), dtype=torch.long, device=device)
        for i in range(B * H):
            s = torch.arange(T, device=device)
            if T > 2:
                s[1:T - 1] = 1 + torch.randperm(T - 2, generator=g, device=device)
            if family == "onehot" and T > 1:
                s[0], s[T - 1] = T - 1, 0
            sel[i // H, i % H] = s
        q = 2 * torch.gather(k, 2, sel[..., None].expand(shape))
        v, do = ints(shape, g, dtype=torch.float32), ints(shape, g, dtype=torch.float32)
    elif family == "counting":
        q, k = torch.zeros(shape, device=device), ints(shape, g, dtype=torch.float32)
        bh = torch.arange(B * H, device=device).view(B, H, 1)
        t = torch.arange(T, device=device).view(1, 1, T)
        v = 8.0 * torch.nn.functional.one_hot((t + 5 * bh) % 64, 64)
        do = 8.0 * torch.nn.functional.one_hot((t + 11 * bh) % 64, 64)
    elif family == "negative":
        q, k, v, do = -rnd(1.0).abs(), rnd(1.0).abs(), rnd(1.0), rnd(1.0)
    elif family == "normal":
        q, k, v, do = rnd(1.5), rnd(1.5), rnd(1.5), rnd(1.0)
    elif family == "peaked":
        q, k, v, do = rnd(4.0), rnd(1.5), rnd(1.5), rnd(1.0)
    else:
        raise ValueError(family)
    return dict(family=family, qkv=_attn_pack3(q, k, v).to(torch.bfloat16).contiguous(),
                dout=attn_flat(do.to(torch.float32)).to(torch.bfloat16).contiguous(), sel=sel)


def attn_onehot_expect(inp, H):
    """What the onehot family must give exactly: out[q] = V[sel[q]], and with that out and the
    reference lse, dV[k] = dO[sel^-1[k]] and dQ = dK = 0 -> (out [B][T][H*64], dqkv [B][T][3*H*64])."""
    _, _, v = attn_heads(inp["qkv"], H)
    do = attn_rows(inp["dout"], H)
    idx = inp["sel"][..., None].expand(v.shape)
    out = torch.gather(v, 2, idx)
    dv = torch.zeros_like(v).scatter_(2, idx, do)
    return attn_flat(out), _attn_pack3(torch.zeros_like(v), torch.zeros_like(v), dv)


def attn_check_fwd(inp, ref, out, lse, H, what=""):
    """Every element of out and lse. onehot: out exactly, lse within 4 U |ref| (the gap condition is
    asserted on the reference first); every other family: the derived bounds."""
    if inp["family"] == "onehot":
        assert ref["gap"] >= ONEHOT_GAP, (what, ref["gap"])
        assert_exact(out, attn_onehot_expect(inp, H)[0], what + " out")
        assert_close(lse, ref["lse"], 4 * U * ref["lse"].abs(), what + " lse")
    else:
        assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
        assert_close(out, ref["out"], ref["out_bound"], what + " out")
        assert_close(lse, ref["lse"], ref["lse_bound"], what + " lse")


def attn_check_bwd(inp, bref, dqkv, H, what="", delta=None):
    """Every element of d(qkv) (and of delta, where the path writes it) against ``attn_bwd_ref``
    evaluated on the forward reference's rounded out and lse; onehot: exactly."""
    if inp["family"] == "onehot":
        assert_exact(dqkv, attn_onehot_expect(inp, H)[1], what + " dqkv")
    else:
        assert dqkv.dtype == torch.bfloat16
        assert_close(dqkv, bref["dqkv"], bref["dqkv_bound"], what + " dqkv")
    if delta is not None:
        assert_f32_close(delta, bref["delta"], bref["delta_abs"], what + " delta", roundings=DOT_ROUNDINGS)


# the sequence lengths of tests/test_attention_kernels_gpu.py (also walked on the CPU: the onehot gap)
ATTN_B, ATTN_H, ATTN_SCALE = 2, 3, 0.125
ATTN_T_FWD_SEQ = tuple(sorted({16 * n - d for n in range(1, 17) for d in (0, 15)} | {5, 197}))
ATTN_T_TILES = tuple(sorted({32 * n - d for n in range(1, 9) for d in (0, 31)} | {197}))
ATTN_T_TILED = (257, 320, 321)         # as dispatched
ATTN_T_TILED_FORCED = (1, 63, 64, 65, 129)
ATTN_T_BWD_SEQ = tuple(sorted({16 * n - d for n in (1, 2, 7, 8, 9, 13, 16) for d in (0, 15)} | {5}))
ATTN_T_CLS = (1, 7, 31, 32, 33, 64, 197, 256)
ATTN_T_ALL = tuple(sorted(set(ATTN_T_FWD_SEQ + ATTN_T_TILES + ATTN_T_TILED + ATTN_T_TILED_FORCED + ATTN_T_BWD_SEQ +
                              ATTN_T_CLS)))


def attn_seed(family, T):
    return 1000 * (ATTN_FAMILIES + ("onehot0",)).index(family) + T


def attn_cls_onehot_expect(inp, H):
    """Class token, onehot families: out[b][h] = V[sel[b][h][0]], lse = 8192 / 8, dV of that key =
    dO of token 0 and every other gradient 0 -> (out [B][H*64], dqkv [B][T][3*H*64])."""
    _, _, v = attn_heads(inp["qkv"], H)
    B, _, T, _ = v.shape
    do = attn_rows(inp["dout"], H)[:, :, :1]
    idx = inp["sel"][:, :, :1, None].expand(B, H, 1, 64)
    dv = torch.zeros_like(v).scatter_(2, idx, do)
    return torch.gather(v, 2, idx).reshape(B, H * 64), _attn_pack3(torch.zeros_like(v), torch.zeros_like(v), dv)


def attn_check_cls_fwd(inp, ref, out, lse, H, what=""):
    if inp["family"] in ("onehot", "onehot0"):
        assert ref["gap"] >= ONEHOT_GAP, (what, ref["gap"])
        assert_exact(out, attn_cls_onehot_expect(inp, H)[0], what + " out")
        assert_close(lse, torch.full_like(ref["lse"], 1024.0), 4 * U * 1024.0, what + " lse")
    else:
        assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
        assert_close(out, ref["out"], ref["out_bound"], what + " out")
        assert_close(lse, ref["lse"], ref["lse_bound"], what + " lse")


def attn_check_cls_bwd(inp, ref, dqkv, H, what=""):
    """Every element of d(qkv): dq of every token but 0 has bound 0 (and NaN poison fails)."""
    if inp["family"] in ("onehot", "onehot0"):
        assert_exact(dqkv, attn_cls_onehot_expect(inp, H)[1], what + " dqkv")
    else:
        assert dqkv.dtype == torch.bfloat16
        assert_close(dqkv, ref["dqkv"], ref["dqkv_bound"], what + " dqkv")
