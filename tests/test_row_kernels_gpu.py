"""csrc/layernorm.hip (bf16 forward / backward, GELU backward) and csrc/xent.hip (cross-entropy,
column sums) against float64 references (tests/kernel_ref.py), at every dispatched width and at
the row counts where the block geometry changes. Outputs and workspaces are guard-banded.

Transcendental kernels (cross-entropy: __expf / __logf; GELU backward: exp + rcp tanh) have no
derivable ulp bound. Their allowance is measured at run time, never from the kernel: E_ref, the
largest error of PyTorch's own fp32 GPU op (torch.logsumexp, F.cross_entropy and its autograd,
the autograd of F.gelu(approximate="tanh")) against the float64 reference on the same inputs,
and the kernel is allowed 4 x E_ref (fast intrinsics are specified at a few ulp where libm is at
1-2) plus the derived bf16 half-ulp where its output is bf16. E_ref is floored at one fp32 unit
roundoff of the case's largest |reference|: an fp32 result cannot be expected to carry less than
its own representation error, and on a one-row case the library's error can be 0 by luck. Each
test prints a ``MEASURED`` line with the reference op's and the kernel's error."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
LN_EPS = float(torch.tensor(1e-6, dtype=F32))


def G(shape, dtype, fill=None):
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def emax(a, ref64):
    return (kr.f64(a) - ref64).abs().max().item()


def allowance(e_ref, ref64):
    """4 x the reference op's error, floored at the fp32 resolution of the case (module docstring)."""
    return 4 * max(e_ref, kr.U * ref64.abs().max().item())


# --------------------------------------------------------------------------------- LayerNorm
LN_CASES = [(D, r) for D in (256, 512, 768, 1024) for r in (1, 3, 4, 5, 63, 64, 65, 197)] + [(256, 32769)]


@pytest.mark.parametrize("D,rows", LN_CASES)
def test_ln_fwd(D, rows):
    lib = no._load()
    g = kr.gen(D + rows)
    x = kr.normal((rows, D), g, std=2.0, mean=1.0)
    if rows >= 3:
        x[1] = 3.0  # constant row: var = 0, rstd = 1/sqrt(eps), y = bias
        x[2] = kr.normal((D,), g, mean=100.0)  # mean 100, std 1 (bf16 steps of 0.5)
    w, b = kr.normal((D,), g, F32), kr.normal((D,), g, F32)
    y, mean, rstd = G((rows, D), BF), G(rows, F32), G(rows, F32)
    what = f"ln_fwd D={D} rows={rows}"
    assert lib.pdt_ln_fwd(no._p(x), no._p(w), no._p(b), no._p(y), no._p(mean), no._p(rstd), rows, D, LN_EPS,
                          no._s()) == 0, what
    done(what)
    ref = kr.ln_fwd_ref(x, w, b, LN_EPS)
    # the row sum: 4 D/256 adds per lane, 6 wave steps, the rounded 1/D and its product
    L = 4 * (D // 256) + 8
    em = 2 * L * kr.U * kr.f64(x).abs().mean(1)
    kr.assert_close(mean, ref["mean"], em + kr.U * ref["mean"].abs(), what + " mean")
    # var: the same chain over d^2 (each two roundings more); the mean's error enters at second
    # order (sum (x - mean) = 0); rsqrt and the eps fma: 4 U
    dvar = 2 * (L + 3) * kr.U * ref["var"] + em ** 2
    rrel = 0.5 * dvar / (ref["var"] + LN_EPS) + 4 * kr.U
    kr.assert_close(rstd, ref["rstd"], ref["rstd"] * rrel, what + " rstd")
    ga = kr.f64(w).abs()
    extra = (em * ref["rstd"])[:, None] * ga + (ref["xhat"] * kr.f64(w)).abs() * rrel[:, None]
    kr.assert_bf16_close(y, ref["y"], ref["y_abs"], what, extra=extra)
    if rows >= 3:
        assert abs(rstd[1].item() * math.sqrt(LN_EPS) - 1) < 1e-6, what
        if D != 768:  # D a power of two: the constant row's mean is exact, so y is the bias itself
            assert torch.equal(y[1], b.to(BF)), what
        # two-pass variance at mean 100: rstd is as accurate as at mean 0
        assert abs(rstd[2].item() / ref["rstd"][2].item() - 1) < 1e-5, what


@pytest.mark.parametrize("D,rows", LN_CASES)
def test_ln_bwd(D, rows):
    lib = no._load()
    g = kr.gen(3 * D + rows)
    blocks = lib.pdt_ln_bwd_blocks(rows)
    rpb = 64 if rows <= 32768 else 128
    assert blocks == max(1, math.ceil(rows / rpb))
    for family, acc, use_add in [("exact", 0, False), ("exact", 1, True), ("normal", 0, True), ("normal", 1, False)]:
        what = f"ln_bwd D={D} rows={rows} {family} acc={acc} addend={use_add}"
        if family == "exact":
            d = kr.exact_ln_bwd_inputs(rows, D, g)
        else:
            d = dict(dy=kr.normal((rows, D), g), x=kr.normal((rows, D), g, std=2.0, mean=1.0),
                     addend=kr.normal((rows, D), g), gamma=kr.normal((D,), g, F32),
                     mean=kr.normal((rows,), g, F32, 0.5, 1.0), rstd=torch.rand(rows, generator=g, device=DEV) + 0.25)
        add = d["addend"] if use_add else None
        dg0, db0 = kr.ints((D,), g, dtype=F32), kr.ints((D,), g, dtype=F32)
        dx, part = G((rows, D), BF), G(2 * blocks * D, F32)
        dg, db = G(D, F32, dg0 if acc else None), G(D, F32, db0 if acc else None)
        rc = lib.pdt_ln_bwd(no._p(d["dy"]), no._p(d["x"]), no._p(d["gamma"]), no._p(d["mean"]), no._p(d["rstd"]),
                            no._p(dx), no._p(dg), no._p(db), no._p(part), rows, D, acc, no._p(add), no._s())
        assert rc == 0, what
        done(what)
        ref = kr.ln_bwd_ref(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], add, dg0 if acc else None,
                            db0 if acc else None)
        L = 4 * (D // 256) + 8  # row means: as in the forward
        if family == "exact":
            kr.assert_exact(dg, ref["dgamma"], what + " dgamma")
            kr.assert_exact(db, ref["dbeta"], what + " dbeta")
            if D != 768:
                kr.assert_exact(dx, ref["dx"], what + " dx")
        kr.assert_bf16_close(dx, ref["dx"], ref["dx_abs"], what + " dx", roundings=6,
                             extra=2 * L * kr.U * ref["dx_mean_abs"])
        # column sums: a wave's rows, 4 waves, then colsum_f32 (16 row groups); dy * xhat: 3 roundings
        Lc = math.ceil(min(rows, rpb) / 4) + 4 + math.ceil(blocks / 16) + 16 + 3 + acc
        kr.assert_f32_close(dg, ref["dgamma"], ref["dgamma_abs"], what + " dgamma", roundings=Lc)
        kr.assert_f32_close(db, ref["dbeta"], ref["dbeta_abs"], what + " dbeta", roundings=Lc)


def test_ln_refuses_other_widths():
    lib = no._load()
    x = torch.zeros(4, 384, dtype=BF, device=DEV)
    w = torch.zeros(384, device=DEV)
    y, mean, rstd = G((4, 384), BF, 1.0), G(4, F32, 1.0), G(4, F32, 1.0)
    part, dg, db = G(2 * 384, F32, 1.0), G(384, F32, 1.0), G(384, F32, 1.0)
    assert lib.pdt_ln_fwd(no._p(x), no._p(w), no._p(w), no._p(y), no._p(mean), no._p(rstd), 4, 384, LN_EPS,
                          no._s()) == -1
    assert lib.pdt_ln_bwd(no._p(x), no._p(x), no._p(w), no._p(mean), no._p(rstd), no._p(y), no._p(dg), no._p(db),
                          no._p(part), 4, 384, 0, None, no._s()) == -1
    # the fp8 / residual-add entry points: nothing launched either (codes, scaling state, partials)
    xsum, q = G((4, 384), BF, 1.0), G((4, 384), torch.uint8, 1)
    meta, qpart, dq = G(lib.pdt_fp8_meta_words(), F32, 1.0), G(4, F32, 1.0), G(1, F32, 1.0)
    cpart, bias = G(384 + lib.pdt_reduce_rows_work(1, 384), F32, 1.0), G(384, F32, 1.0)
    assert lib.pdt_ln_fwd_f8(no._p(x), no._p(w), no._p(w), no._p(y), no._p(mean), no._p(rstd), 4, 384, LN_EPS,
                             no._p(q), no._p(meta), no._p(qpart), no._p(dq), no._s()) == -1
    for codes in (None, q):
        m, p, d = (no._p(meta), no._p(qpart), no._p(dq)) if codes is not None else (None, None, None)
        assert lib.pdt_ln_add_fwd(no._p(x), no._p(x), no._p(xsum), no._p(w), no._p(w), no._p(y), no._p(mean),
                                  no._p(rstd), 4, 384, LN_EPS, no._p(codes), m, p, d, no._s()) == -1
    bwd = (no._p(x), no._p(x), no._p(w), no._p(mean), no._p(rstd), no._p(y), no._p(dg), no._p(db), no._p(part), 4, 384,
           0, None, no._p(q), no._p(meta), no._p(qpart), no._p(dq))
    assert lib.pdt_ln_bwd_f8(*bwd, no._s()) == -1
    assert lib.pdt_ln_bwd_f8_db(*bwd, no._p(cpart), no._p(bias), 0, no._s()) == -1
    done("refused")
    for t in (y, mean, rstd, part, dg, db, xsum, q, meta, qpart, dq, cpart, bias):
        assert bool((t == 1).all())


# ------------------------------------------------------------------------------ GELU backward
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (8192 * 256 + 3)])
def test_gelu_bwd(n):
    """Allowance: 4 x the error of the autograd of F.gelu(approximate="tanh") in fp32 (module docstring)."""
    lib = no._load()
    g = kr.gen(n)
    z = kr.normal((n,), g, std=3.0)
    z[:7] = torch.tensor([0.0, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0], device=DEV).to(BF)
    dy = kr.normal((n,), g)
    dz = G(n, BF)
    assert lib.pdt_gelu_bwd(no._p(dy), no._p(z), no._p(dz), n, no._s()) == 0
    done(f"gelu_bwd n={n}")
    ref = kr.f64(dy) * kr.gelu_tanh_grad_ref(z)
    zz = z.float().requires_grad_()
    F.gelu(zz, approximate="tanh").backward(dy.float())
    e_ref = emax(zz.grad, ref)
    allow = allowance(e_ref, ref)
    e_k = ((kr.f64(dz) - ref).abs() - kr.BF16_HALF * ref.abs()).clamp_min(0).max().item()
    print(f"MEASURED gelu_bwd n={n}: reference op max err {e_ref:.3e}, allowance {allow:.3e}, "
          f"kernel max err beyond the bf16 half-ulp {e_k:.3e}")
    kr.assert_bf16_close(dz, ref, ref.abs(), f"gelu_bwd n={n}", roundings=0, extra=allow)
    assert lib.pdt_gelu_bwd(no._p(dy), no._p(z), no._p(dz), 12, no._s()) == -1


# ------------------------------------------------------------------------------ cross-entropy
def xent_inputs(B, V, bf16, g):
    x = kr.normal((B, V), g, BF if bf16 else F32, std=3.0)
    t = torch.randint(0, V, (B,), generator=g, device=DEV)
    x[0, 0], t[0] = 20.0, 0  # the maximum in the first column
    if B > 1:
        x[1, V - 1], t[1] = 20.0, V - 1  # ... and in the last
    if B > 2:
        x[2] = 1.5  # all equal
    if B > 3:  # magnitude 80: exp overflows unless the maximum is subtracted
        x[3] = (torch.randint(0, 2, (V,), generator=g, device=DEV).to(x.dtype) * 2 - 1) * 80
    return x, t


@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("V", [2, 10, 63, 64, 65, 1000, 1001])
def test_xent(V, B):
    """Allowances: 4 x the error of torch.logsumexp / F.cross_entropy / its autograd in fp32 (module docstring).

    Finding (first run: 31 cases failed at 4 x, all at the target column of a peaked row with eps = 0,
    e.g. V=10 B=1: dlogits 0.0 for -4.41e-07): xent_bwd_kernel forms the softmax as
    __expf(x - lse) from the fp32 lse it is handed, where PyTorch differentiates log_softmax
    (x - max - log(sum)). An lse of 20.0000003 is stored as 20.0 (fp32 spacing 1.9e-6 there), so p
    carries the relative error |delta lse| <= U |lse|, and at the target of a confident row
    d = p - 1 cancels to that error. This is the conditioning of the stored quantity, not a wrong
    instruction: removing it needs (max, log-sum) stored separately, a change of the kernel's
    interface. The factor 4 is kept; the bound adds the PROPAGATION of what the lse is already
    allowed, |g|/B * p * (a_lse + 4 U |x - lse|) (the second term: the subtraction and the
    exp2 argument scaling). It is an absolute error below 1e-6 * |g| / B on a gradient entry."""
    lib = no._load()
    g = kr.gen(1000 * B + V)
    for bf16 in (1, 0):
        for eps in (0.0, 0.1):
            what = f"xent V={V} B={B} bf16={bf16} eps={eps}"
            epsf = float(torch.tensor(eps, dtype=F32))
            x, t = xent_inputs(B, V, bf16, g)
            gout = torch.tensor([1.7], device=DEV)
            lse, rows, loss, dl = G(B, F32), G(B, F32), G(1, F32), G((B, V), BF)
            assert lib.pdt_xent_fwd(no._p(x), bf16, no._p(t), no._p(lse), no._p(rows), no._p(loss), B, V, epsf,
                                    no._s()) == 0, what
            done(what)
            assert lib.pdt_xent_bwd(no._p(x), bf16, no._p(t), no._p(lse), no._p(gout), no._p(dl), B, V, epsf,
                                    no._s()) == 0, what
            done(what + " bwd")
            ref = kr.xent_ref(x, t, epsf, gout=float(gout.item()))
            # PyTorch's fp32 ops on the same inputs
            xx = x.float().requires_grad_()
            rows_t = F.cross_entropy(xx, t, label_smoothing=eps, reduction="none")
            loss_t = rows_t.mean()
            (loss_t * gout[0]).backward()
            e_lse = emax(torch.logsumexp(x.float(), 1), ref["lse"])
            e_rows, e_loss = emax(rows_t.detach(), ref["loss_rows"]), emax(loss_t.detach(), ref["loss"])
            e_dl = emax(xx.grad, ref["dlogits"])
            a_lse = allowance(e_lse, ref["lse"])
            a_rows = allowance(e_rows, ref["loss_rows_abs"])
            a_dl = allowance(e_dl, ref["dlogits"])
            k_dl = ((kr.f64(dl) - ref["dlogits"]).abs() - kr.BF16_HALF * ref["dlogits"].abs()).clamp_min(0).max().item()
            print(f"MEASURED {what}: lse ref {e_lse:.3e} kernel {emax(lse, ref['lse']):.3e} (allow {a_lse:.3e}); "
                  f"rows ref {e_rows:.3e} kernel {emax(rows, ref['loss_rows']):.3e} (allow {a_rows:.3e}); "
                  f"mean ref {e_loss:.3e} kernel {emax(loss[0], ref['loss']):.3e}; "
                  f"dlogits ref {e_dl:.3e} kernel beyond bf16 half-ulp {k_dl:.3e} (allow {a_dl:.3e})")
            kr.assert_close(lse, ref["lse"], a_lse, what + " lse")
            kr.assert_close(rows, ref["loss_rows"], a_rows, what + " loss rows")
            # the mean of the kernel's own rows: their error, the reference op's for a mean, and a
            # sum of ceil(B/256) + 8 adds and the 1/B product
            mabs = ref["loss_rows"].abs().mean().item()
            a_mean = a_rows + allowance(e_loss, ref["loss"]) + 2 * (math.ceil(B / 256) + 10) * kr.U * mabs
            kr.assert_close(loss[0], ref["loss"], a_mean, what + " mean loss")
            prop = abs(gout.item()) / B * ref["softmax"] * (
                a_lse + 4 * kr.U * (kr.f64(x) - ref["lse"][:, None]).abs())  # (docstring: the lse's own error)
            kr.assert_bf16_close(dl, ref["dlogits"], ref["dlogits_abs"], what + " dlogits", roundings=0,
                                 extra=a_dl + prop)
            # softmax - target distribution sums to 0: each stored entry is off by at most half a
            # bf16 ulp of the row's largest entry
            big = kr.f64(dl).abs().max(1).values
            assert bool((kr.f64(dl).sum(1).abs() <= V * 0.5 * kr.ulp_bf16(big) + prop.sum(1)).all()), what + " row sums"
            assert torch.isfinite(lse).all() and torch.isfinite(dl.float()).all(), what


# -------------------------------------------------------------------------------- column sums
COLSUM = [(R, C) for C in (8, 1000, 2304, 3072, 10, 1001) for R in (1, 3, 33, 4097, 16417) if R * C * 2 <= 33e6]


@pytest.mark.parametrize("R,C", COLSUM)
def test_colsum(R, C):
    lib = no._load()
    g = kr.gen(R + C)
    vec = C % 8 == 0
    Gr = max(1, min(512 if vec else 128, math.ceil(R / 32)))
    ws = lib.pdt_colsum_workspace(R, C)
    assert ws == Gr * C
    for family in ("exact", "normal"):
        for acc in (0, 1):
            what = f"colsum R={R} C={C} {family} acc={acc}"
            x = kr.ints((R, C), g) if family == "exact" else kr.normal((R, C), g, mean=0.25)
            o0 = kr.ints((C,), g, dtype=F32)
            out, work = G(C, F32, o0 if acc else None), G(ws, F32)
            assert lib.pdt_colsum(no._p(x), no._p(out), no._p(work), R, C, acc, no._s()) == 0, what
            done(what)
            ref, ab = kr.colsum_ref(x, o0 if acc else None)
            if family == "exact":
                kr.assert_exact(out, ref, what)
            else:
                # stage 1: a thread's rows, then the block's LDS adds; stage 2: G/4 partials + 3
                rp = max(1, 256 // min(C // 8, 256)) if vec else 4
                L = math.ceil(R / (Gr * rp)) + rp + math.ceil(Gr / 4) + 3 + acc
                kr.assert_f32_close(out, ref, ab, what, roundings=L)
