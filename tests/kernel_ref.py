"""Float64 references, error metrics, guard-banded buffers and input families for the element
and row kernels (csrc/bn_act.hip, pool.hip, layernorm.hip, xent.hip).

Used by tests/test_kernel_ref_cpu.py (which checks this module against PyTorch's float64 CPU ops
and against seeded faults) and by the GPU tests test_bn_act_kernels_gpu.py,
test_pool_kernels_gpu.py and test_row_kernels_gpu.py. A plain module: no fixtures, no pytest
settings.

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
"""
import math

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
