"""tests/kernel_ref.py checked without a GPU:

* every float64 reference against PyTorch's own float64 CPU op at 1e-12 relative;
* every metric rejects a seeded fault and accepts a faithful fp32 emulation of the kernel
  (torch fp32 on the CPU, output cast to bf16);
* every exact-family input really is exact: its fp32 emulation equals the float64 reference;
* the fp8 mirror (fp8_encode / fp8_decode / fp8_meta_ref) against PyTorch's CPU float8 cast on every
  bf16 pattern, and the inputs of tests/test_fp8_cast_kernels_gpu.py against seeded faults;
* the attention references against float64 autograd, an fp32 emulation of the kernels' algorithm
  (online softmax over key tiles, bf16-packed P and dS) inside every derived bound for every input
  family, nine seeded faults each rejected by a named family, and the onehot family's margin at
  every sequence length of tests/test_attention_kernels_gpu.py.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr

CPU = torch.device("cpu")
BF = torch.bfloat16


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def g(seed):
    return kr.gen(seed, CPU)


def trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (the seeded rounding fault)."""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


# ------------------------------------------------------------ references against torch fp64
@pytest.mark.parametrize("relu", [False, True])
def test_bn_refs_match_torch(relu):
    gg = g(0)
    N, C, H = 5, 24, 6
    x = (torch.randn(N, C, H, H, generator=gg, dtype=kr.F64) * 1.5 + 0.3).requires_grad_()
    w = (torch.rand(C, generator=gg, dtype=kr.F64) + 0.5).requires_grad_()
    b = torch.randn(C, generator=gg, dtype=kr.F64).requires_grad_()
    rm, rv = torch.randn(C, generator=gg, dtype=kr.F64), torch.rand(C, generator=gg, dtype=kr.F64) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    dA = torch.randn(N, C, H, H, generator=gg, dtype=kr.F64)
    out = F.batch_norm(x, rm, rv, w, b, training=True, momentum=0.1, eps=1e-5)
    if relu:
        out = F.relu(out)
    (out * dA).sum().backward()

    def rows(t):  # NCHW -> [M][C]
        return t.detach().permute(0, 2, 3, 1).reshape(-1, C)

    M = N * H * H
    x2 = rows(x)
    fin = kr.bn_finalize_ref(kr.bn_partials(x2), M, 1e-5, 0.1, w, b, rm0, rv0, 7)
    assert fin["nbt"] == 8
    assert rel(fin["running_mean"], rm) < 1e-12 and rel(fin["running_var"], rv) < 1e-12
    o, terms = kr.bn_apply_ref(x2, fin["scale"], fin["shift"], relu=relu)
    assert rel(o, rows(out)) < 1e-12
    assert bool((terms >= o.abs() - 1e-12).all())
    gate = (o > 0) if relu else None
    s, q, _, _ = kr.bn_bwd_sums_ref(rows(dA), x2, gate, fin["mean"])
    bw = kr.bn_bwd_finalize_ref(s, q, M, w, fin["mean"], fin["invstd"])
    assert rel(bw["dgamma"], w.grad) < 1e-12 and rel(bw["dbeta"], b.grad) < 1e-12
    dy, _, dres = kr.bn_bwd_apply_ref(rows(dA), x2, gate, bw["k1"], bw["k2"], bw["k3"])
    assert rel(dy, rows(x.grad)) < 1e-11  # (two cancellations deep: 1e-11 of max |dx|)
    assert torch.equal(dres, rows(dA) * (gate.to(kr.F64) if relu else 1.0))


def test_bn_apply_ref_residual_forms():
    gg = g(1)
    y, r = torch.randn(9, 8, generator=gg, dtype=kr.F64), torch.randn(9, 8, generator=gg, dtype=kr.F64)
    sc, sh, rs, rb = (torch.randn(8, generator=gg, dtype=kr.F64) for _ in range(4))
    o, t = kr.bn_apply_ref(y, sc, sh, r, relu=True)
    assert rel(o, F.relu(y * sc + sh + r)) < 1e-12 and bool((t >= o).all())
    o, t = kr.bn_apply_ref(y, sc, sh, r, rs, rb)
    assert rel(o, y * sc + sh + (r * rs + rb)) < 1e-12


def test_relu_mask_ref_bits_and_zeros():
    out = torch.tensor([1.0, -1.0, 0.0, -0.0, 2.0, 0.0, -3.0, 5.0] + [0.0] * 7 + [1.0], dtype=kr.F64)
    m = kr.relu_mask_ref(out)
    assert m.tolist() == [1 | 16 | 128, 128]
    assert torch.equal(kr.mask_to_gate(m, (16,)), out > 0)


@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (3, 1, 1), (3, 2, 0), (3, 2, 1), (2, 3, 0), (5, 3, 2)])
@pytest.mark.parametrize("H,W", [(5, 7), (8, 9)])
@pytest.mark.parametrize("ties", [False, True])
def test_maxpool_refs_match_torch(k, s, p, H, W, ties):
    gg = g(2)
    N, C = 2, 8
    x = torch.randn(N, H, W, C, generator=gg, dtype=kr.F64)
    if ties:  # ReLU-like: ~60 % exact zeros
        x = (x - 0.25).clamp_min(0.0)
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    y_t, flat = F.max_pool2d(xn, k, s, p, return_indices=True)
    y, idx = kr.maxpool_fwd_ref(x, k, s, p)
    Ho, Wo = y.shape[1:3]
    assert (Ho, Wo) == tuple(y_t.shape[2:])
    assert torch.equal(y, y_t.detach().permute(0, 2, 3, 1))
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    kh, kw = flat // W - (oh * s - p), flat % W - (ow * s - p)
    assert torch.equal(idx.to(torch.int64), (kh * k + kw).permute(0, 2, 3, 1))
    dy = torch.randn(N, Ho, Wo, C, generator=gg, dtype=kr.F64)
    (y_t * dy.permute(0, 3, 1, 2)).sum().backward()
    dx, ab = kr.maxpool_bwd_ref(dy, idx, H, W, k, s, p)
    assert rel(dx, xn.grad.permute(0, 2, 3, 1)) < 1e-12
    assert bool((ab >= dx.abs() - 1e-12).all())


def test_maxpool_ref_1x1_and_uncovered_pixels():
    x = torch.tensor([[[[3.0]]]], dtype=kr.F64)
    y, idx = kr.maxpool_fwd_ref(x, 3, 2, 1)
    assert y.item() == 3.0 and idx.item() == 4
    # k < s: input rows / columns 2 (mod 3) lie in no window
    x = torch.randn(1, 5, 7, 8, generator=g(3), dtype=kr.F64)
    y, idx = kr.maxpool_fwd_ref(x, 2, 3, 0)
    dx, _ = kr.maxpool_bwd_ref(torch.ones_like(y), idx, 5, 7, 2, 3, 0)
    assert dx[:, 2].abs().sum() == 0 and dx[:, :, 2].abs().sum() == 0 and dx[:, :, 5].abs().sum() == 0
    assert dx.sum() == y.numel()


def test_avgpool_refs_match_torch():
    x = torch.randn(3, 50, 24, generator=g(4), dtype=kr.F64)
    xn = x.permute(0, 2, 1).reshape(3, 24, 5, 10).contiguous().requires_grad_()
    y_t = F.adaptive_avg_pool2d(xn, 1)
    y, _ = kr.avgpool_fwd_ref(x)
    assert rel(y, y_t.detach().reshape(3, 24)) < 1e-12
    dy = torch.randn(3, 24, generator=g(5), dtype=kr.F64)
    (y_t.reshape(3, 24) * dy).sum().backward()
    dx, _ = kr.avgpool_bwd_ref(dy, 50)
    assert rel(dx, xn.grad.reshape(3, 24, 50).permute(0, 2, 1)) < 1e-12


@pytest.mark.parametrize("D", [256, 768])
def test_layernorm_refs_match_torch(D):
    gg = g(6)
    x = (torch.randn(7, D, generator=gg, dtype=kr.F64) * 2 + 1).requires_grad_()
    w = torch.randn(D, generator=gg, dtype=kr.F64).requires_grad_()
    b = torch.randn(D, generator=gg, dtype=kr.F64).requires_grad_()
    dy, add = torch.randn(7, D, generator=gg, dtype=kr.F64), torch.randn(7, D, generator=gg, dtype=kr.F64)
    y_t = F.layer_norm(x, (D,), w, b, 1e-6)
    (y_t * dy).sum().backward()
    fw = kr.ln_fwd_ref(x, w, b, 1e-6)
    assert rel(fw["y"], y_t.detach()) < 1e-12
    dg0, db0 = torch.randn(D, generator=gg, dtype=kr.F64), torch.randn(D, generator=gg, dtype=kr.F64)
    bw = kr.ln_bwd_ref(dy, x, w, fw["mean"], fw["rstd"])
    assert rel(bw["dx"], x.grad) < 1e-12 and rel(bw["dgamma"], w.grad) < 1e-12 and rel(bw["dbeta"], b.grad) < 1e-12
    bw2 = kr.ln_bwd_ref(dy, x, w, fw["mean"], fw["rstd"], add, dg0, db0)
    assert rel(bw2["dx"], x.grad + add) < 1e-12
    assert rel(bw2["dgamma"], w.grad + dg0) < 1e-12 and rel(bw2["dbeta"], b.grad + db0) < 1e-12


def test_gelu_grad_ref_matches_torch():
    z = torch.cat([torch.tensor([0.0, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0], dtype=kr.F64),
                   torch.randn(1000, generator=g(7), dtype=kr.F64) * 2]).requires_grad_()
    F.gelu(z, approximate="tanh").sum().backward()
    assert rel(kr.gelu_tanh_grad_ref(z), z.grad) < 1e-12


@pytest.mark.parametrize("V", [2, 63, 1001])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_xent_ref_matches_torch(V, eps):
    gg = g(8)
    B = 5
    x = (torch.randn(B, V, generator=gg, dtype=kr.F64) * 3).requires_grad_()
    t = torch.randint(0, V, (B,), generator=gg)
    t[0], t[1] = 0, V - 1
    loss = F.cross_entropy(x, t, label_smoothing=eps)
    (loss * 1.7).backward()
    r = kr.xent_ref(x, t, eps, gout=1.7)
    assert rel(r["lse"], torch.logsumexp(x.detach(), 1)) < 1e-12
    assert rel(r["loss"], loss.detach()) < 1e-12
    assert rel(r["loss_rows"], F.cross_entropy(x.detach(), t, label_smoothing=eps, reduction="none")) < 1e-12
    assert rel(r["dlogits"], x.grad) < 1e-12


def test_colsum_ref():
    x = torch.randn(33, 10, generator=g(9), dtype=kr.F64)
    o0 = torch.randn(10, generator=g(10), dtype=kr.F64)
    s, a = kr.colsum_ref(x, o0)
    assert rel(s, x.sum(0) + o0) < 1e-12 and bool((a >= s.abs()).all())


# ------------------------------------------------------- fp32 emulations of the kernels (CPU)
def emu_bn_apply(y, sc, sh, res=None, relu=False):
    o = y.float() * sc + sh
    if res is not None:
        o = o + res.float()
    return o.clamp_min(0.0) if relu else o


def emu_bn_bwd_sums(dA, y, mean, drop=None):
    gq, t = dA.float(), dA.float() * (y.float() - mean)
    if drop is not None:
        keep = torch.ones(dA.shape[0], dtype=torch.bool)
        keep[drop] = False
        gq, t = gq[keep], t[keep]
    return gq.sum(0), t.sum(0)


def emu_ln_bwd(d, addend=True):
    dy, x, gm = d["dy"].float(), d["x"].float(), d["gamma"]
    D = x.shape[1]
    xh = (x - d["mean"][:, None]) * d["rstd"][:, None]
    gy = dy * gm
    m1, m2 = gy.sum(1, keepdim=True) * (1.0 / D), (gy * xh).sum(1, keepdim=True) * (1.0 / D)
    dx = d["rstd"][:, None] * (gy - m1 - xh * m2)
    if addend:
        dx = dx + d["addend"].float()
    return dx.to(BF), (dy * xh).sum(0), dy.sum(0)


def emu_maxpool(x, k, s, p, last_wins=False):
    """fp32 window scan in the kernel's order; ``last_wins``: the seeded tie-break fault."""
    N, H, W, C = x.shape
    Ho, Wo = kr.pool_out(H, k, s, p), kr.pool_out(W, k, s, p)
    best = torch.full((N, Ho, Wo, C), float("-inf"))
    idx = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8)
    for oh in range(Ho):
        for ow in range(Wo):
            for kh in range(k):
                for kw in range(k):
                    ih, iw = oh * s - p + kh, ow * s - p + kw
                    if 0 <= ih < H and 0 <= iw < W:
                        v = x[:, ih, iw].float()
                        take = (v >= best[:, oh, ow]) if last_wins else (v > best[:, oh, ow])
                        best[:, oh, ow] = torch.where(take, v, best[:, oh, ow])
                        idx[:, oh, ow] = torch.where(take, torch.full_like(idx[:, oh, ow], kh * k + kw),
                                                     idx[:, oh, ow])
    return best.to(BF), idx


# ---------------------------------------------------------- the exact family really is exact
def test_exact_family_bn():
    gg = g(20)
    for R, C in [(1, 8), (257, 24), (2049, 72)]:
        part = kr.exact_partials(R, C, gg)
        # the fp32 sums are exact; the mean (a quotient by 16 R) is then one rounding of the fp64 value
        kr.assert_exact(part[0].sum(0), kr.f64(part)[0].sum(0), "sum")
        kr.assert_exact(part[1].sum(0), kr.f64(part)[1].sum(0), "sum of squares")
        fin = kr.bn_finalize_ref(kr.f64(part), 16.0 * R, 1e-5)
        assert torch.equal((part[0].sum(0).double() / (16.0 * R)).float(), fin["mean"].float())
    dA, y, mean = kr.exact_bn_bwd_inputs(40001, 24, gg)
    s, q, _, _ = kr.bn_bwd_sums_ref(dA, y, None, mean)
    es, eq = emu_bn_bwd_sums(dA, y, mean)
    kr.assert_exact(es, s, "sum g")
    kr.assert_exact(eq, q, "sum g (y - mean)")
    gate = y > 0
    s, q, _, _ = kr.bn_bwd_sums_ref(dA, y, gate, mean)
    es, eq = emu_bn_bwd_sums(dA * gate, y, mean)
    kr.assert_exact(es, s, "gated sum g")
    kr.assert_exact(eq, q, "gated sum g (y - mean)")


def test_exact_family_pool_and_colsum():
    gg = g(21)
    x = kr.ints((5, 16, 72), gg)
    y, _ = kr.avgpool_fwd_ref(x)
    kr.assert_exact((x.float().sum(1) * (1.0 / 16)).to(BF), y, "avgpool fwd")
    dy = kr.ints((5, 72), gg)
    dx, _ = kr.avgpool_bwd_ref(dy, 16)
    kr.assert_exact((dy.float() * (1.0 / 16))[:, None, :].expand(-1, 16, -1).to(BF), dx, "avgpool bwd")
    x = kr.ints((16417, 10), gg)
    s, _ = kr.colsum_ref(x, kr.f64(kr.ints((10,), gg, dtype=torch.float32)))
    # (the same generator state cannot be replayed: accumulate into zeros instead)
    s0, _ = kr.colsum_ref(x)
    kr.assert_exact(x.float().sum(0), s0, "colsum")
    xs = kr.ints((2, 8, 9, 8), gg)
    yv, idx = kr.maxpool_fwd_ref(xs, 3, 1, 1)
    dyi = kr.ints(tuple(yv.shape), gg)
    dxr, _ = kr.maxpool_bwd_ref(dyi, idx, 8, 9, 3, 1, 1)
    kr.assert_exact(dxr.to(torch.float32).to(BF), dxr, "maxpool bwd: up to 9 integers <= 8 fit bf16")
    del s


@pytest.mark.parametrize("D", [256, 512, 768, 1024])
def test_exact_family_layernorm_bwd(D):
    d = kr.exact_ln_bwd_inputs(197, D, g(22))
    ref = kr.ln_bwd_ref(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], d["addend"])
    dx, dg, db = emu_ln_bwd(d)
    kr.assert_exact(dg, ref["dgamma"], "dgamma")
    kr.assert_exact(db, ref["dbeta"], "dbeta")
    if D != 768:  # 1/768 is not a power of two: the row means round
        kr.assert_exact(dx, ref["dx"], "dx")
    else:
        kr.assert_bf16_close(dx, ref["dx"], ref["dx_abs"], "dx", extra=2 * 20 * kr.U * ref["dx_mean_abs"])


# ------------------------------------------------- metrics: accept the faithful, reject faults
def _apply_case(M=4160, C=256):
    gg = g(30)
    y, r = kr.normal((M, C), gg), kr.normal((M, C), gg)
    sc, sh = torch.rand(C, generator=gg) + 0.5, torch.randn(C, generator=gg) * 0.5
    ref, terms = kr.bn_apply_ref(y, sc, sh, r)
    return emu_bn_apply(y, sc, sh, r), ref, terms


def test_rounding_metrics_accept_rne_reject_truncation():
    o32, ref, terms = _apply_case()
    assert ref.numel() >= 2 ** 20
    kr.assert_bf16_close(o32.to(BF), ref, terms, "rne")
    kr.assert_unbiased_rounding(o32.to(BF), ref, "rne")
    bias, _ = kr.rounding_bias(o32.to(BF), ref)
    assert abs(bias) < 0.002
    with pytest.raises(AssertionError):
        kr.assert_unbiased_rounding(trunc_bf16(o32), ref, "trunc")
    bias, _ = kr.rounding_bias(trunc_bf16(o32), ref)
    assert -0.52 < bias < -0.48
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(trunc_bf16(o32), ref, terms, "trunc")
    with pytest.raises(AssertionError):  # too few elements to judge a bias
        kr.assert_unbiased_rounding(o32.to(BF)[:100], ref[:100], "short")


def test_exact_metric_rejects_one_dropped_row_of_40000():
    dA, y, mean = kr.exact_bn_bwd_inputs(40000, 8, g(31))
    dA[12345] = 1  # (a row that certainly contributes)
    s, q, _, _ = kr.bn_bwd_sums_ref(dA, y, None, mean)
    es, eq = emu_bn_bwd_sums(dA, y, mean)
    kr.assert_exact(es, s)
    kr.assert_exact(eq, q)
    es, eq = emu_bn_bwd_sums(dA, y, mean, drop=12345)
    with pytest.raises(AssertionError):
        kr.assert_exact(es, s)
    # ... which a Frobenius-norm tolerance cannot see
    assert ((es.double() - s).norm() / s.norm()).item() < 2e-2


def test_unwritten_last_row_is_rejected():
    o32, ref, terms = _apply_case(64, 8)
    out = kr.guarded(o32.shape, BF, CPU)
    out.copy_(o32.to(BF))
    kr.assert_bf16_close(out, ref, terms, "all rows")
    kr.check_guards()
    out = kr.guarded(o32.shape, BF, CPU)
    out[:-1].copy_(o32.to(BF)[:-1])
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(out, ref, terms, "last row unwritten")
    with pytest.raises(AssertionError):
        kr.assert_exact(out, kr.f64(o32.to(BF)), "last row unwritten")
    kr.check_guards()


def test_mask_metric_rejects_one_flipped_bit():
    o32, _, _ = _apply_case(64, 8)
    out = o32.to(BF).clamp_min(0)
    want = kr.relu_mask_ref(out)
    kr.assert_exact(want.clone(), want, "mask")
    bad = want.clone()
    bad[17] ^= 4
    with pytest.raises(AssertionError):
        kr.assert_exact(bad, want, "mask")


def test_argmax_metric_rejects_last_maximum():
    for x in (torch.full((1, 5, 7, 8), 2.0).to(BF), (kr.normal((1, 5, 7, 8), g(32)).float() - 0.25).clamp_min(0).to(BF)):
        y, idx = kr.maxpool_fwd_ref(x, 3, 2, 1)
        ey, eidx = emu_maxpool(x, 3, 2, 1)
        kr.assert_exact(ey, y, "values")
        kr.assert_exact(eidx, idx, "argmax")
        ey, eidx = emu_maxpool(x, 3, 2, 1, last_wins=True)
        kr.assert_exact(ey, y, "values are the same whichever maximum is taken")
        with pytest.raises(AssertionError):
            kr.assert_exact(eidx, idx, "argmax")


def test_guard_band_catches_store_past_the_end():
    for dtype, shape in [(BF, (37, 24)), (torch.float32, (2, 3, 10)), (torch.uint8, (5,))]:
        t = kr.guarded(shape, dtype, CPU)
        assert t.data_ptr() % 16 == 0 and t.is_contiguous() and tuple(t.shape) == shape
        t.fill_(1)
        kr.check_guards()
        t = kr.guarded(shape, dtype, CPU)
        raw, nbytes = kr._live[-1]
        assert raw.numel() - nbytes >= 512 and t.data_ptr() - raw.data_ptr() >= 256
        raw[kr._FRONT + nbytes + 16] = 0  # one store 16 bytes past the end
        with pytest.raises(AssertionError):
            kr.check_guards()
        t = kr.guarded(shape, dtype, CPU)
        kr._live[-1][0][kr._FRONT - 1] = 0  # one byte before the start
        with pytest.raises(AssertionError):
            kr.check_guards()
        assert kr._live == []


def test_loss_mean_metric_rejects_b_plus_one():
    gg = g(33)
    B, V = 257, 1000
    x = kr.normal((B, V), gg, torch.float32, std=3.0)
    t = torch.randint(0, V, (B,), generator=gg)
    r = kr.xent_ref(x, t, 0.1)
    rows32 = F.cross_entropy(x, t, label_smoothing=0.1, reduction="none")
    row_err = (rows32.double() - r["loss_rows"]).abs().max().item()
    good = (rows32.sum() * (1.0 / B)).reshape(())
    bad = (rows32.sum() * (1.0 / (B + 1))).reshape(())
    kr.assert_f32_close(good, r["loss"], r["loss_rows"].abs().mean(), "mean", roundings=12, extra=row_err)
    with pytest.raises(AssertionError):
        kr.assert_f32_close(bad, r["loss"], r["loss_rows"].abs().mean(), "mean", roundings=12, extra=row_err)


def test_bf16_close_accepts_emulations_of_each_family():
    gg = g(34)
    # LayerNorm forward, with a row of mean 100 / std 1 and a constant row
    D = 768
    x = kr.normal((6, D), gg)
    x[1] = kr.normal((D,), gg, mean=100.0)
    x[2] = 3.0
    w, b = torch.randn(D, generator=gg), torch.randn(D, generator=gg)
    fw = kr.ln_fwd_ref(x, w, b, 1e-6)
    xf = x.float()
    mean = xf.mean(1, keepdim=True)
    rstd = torch.rsqrt(((xf - mean) ** 2).mean(1, keepdim=True) + 1e-6)
    y = ((xf - mean) * rstd * w + b).to(BF)
    kr.assert_bf16_close(y, fw["y"], fw["y_abs"], "ln fwd", roundings=20)
    assert abs(fw["rstd"][2].item() - 1e3) < 1e-6 and torch.equal(y[2].float(), b.to(BF).float())
    # max-pool backward, random gradients
    xs = kr.normal((2, 8, 9, 8), gg)
    yv, idx = kr.maxpool_fwd_ref(xs, 3, 1, 1)
    dy = kr.normal(tuple(yv.shape), gg)
    dx, ab = kr.maxpool_bwd_ref(dy, idx, 8, 9, 3, 1, 1)
    kr.assert_bf16_close(dx.to(torch.float32).to(BF), dx, ab, "pool bwd")


# ----------------------------------------------------------------------- fp8 quantization
FP8_DT = (torch.float8_e4m3fn, torch.float8_e5m2)
FMTS = [0, 1]


def torch_codes(x32, fmt):
    """PyTorch's CPU cast of the clamped values (the library cast fp8_encode is independent of)."""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32))
    return t.clamp(-kr.FP8_FMAX[fmt], kr.FP8_FMAX[fmt]).to(FP8_DT[fmt]).view(torch.uint8).numpy()


def faulty_encode(v32, fmt, fault):
    """fp8_encode with one seeded fault, by search in the table of values (float64):
    'trunc' rounds toward zero, 'away' rounds ties away from zero, 'noclamp' lets values past FMAX
    overflow (NaN code of e4m3fn, infinity code of e5m2), 'fmax240' clamps at 240."""
    v = np.asarray(v32, dtype=np.float32).astype(np.float64)
    vals = kr.fp8_decode(np.arange(kr.FP8_MAX_CODE[fmt] + 1, dtype=np.uint8), fmt)
    fmax = 240.0 if fault == "fmax240" else kr.FP8_FMAX[fmt]
    a = np.abs(v)
    over = a > fmax + (vals[-1] - vals[-2]) / 2 if fault == "noclamp" else np.zeros(a.shape, dtype=bool)
    a = np.minimum(a, fmax)
    lo = np.clip(np.searchsorted(vals, a, side="right") - 1, 0, vals.size - 1)
    hi = np.minimum(lo + 1, vals.size - 1)
    mid = (vals[lo] + vals[hi]) / 2
    if fault == "trunc":
        up = np.zeros(a.shape, dtype=bool)
    elif fault == "away":
        up = a >= mid
    else:
        up = (a > mid) | ((a == mid) & (lo % 2 == 1))
    code = np.where(up & (hi > lo), hi, lo)
    code = np.where(over, 0x7F if fmt == 0 else 0x7C, code)
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_decode_encode_identity_and_table(fmt):
    codes = kr.fp8_finite_codes(fmt)
    assert codes.size == (254 if fmt == 0 else 248)
    vals = kr.fp8_decode(codes, fmt)
    assert np.isfinite(vals).all() and np.abs(vals).max() == kr.FP8_FMAX[fmt]
    assert kr.fp8_decode(np.uint8(kr.FP8_MAX_CODE[fmt]), fmt) == kr.FP8_FMAX[fmt]
    kr.assert_same_bits(kr.fp8_encode(vals.astype(np.float32), fmt), codes, "decode . encode")
    assert kr.fp8_encode(np.float32([0.0, -0.0]), fmt).tolist() == [0x00, 0x80]
    # the formula's table against the library's, all 256 codes (NaN codes as NaN)
    lib = torch.arange(256, dtype=torch.uint8).view(FP8_DT[fmt]).double().numpy()
    mine = kr.fp8_decode(np.arange(256, dtype=np.uint8), fmt)
    assert ((lib == mine) | (np.isnan(lib) & np.isnan(mine))).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_encode_midpoints_go_to_even(fmt):
    mids, lo, hi = kr.fp8_midpoints(fmt)
    m32 = mids.astype(np.float32)
    assert (m32.astype(np.float64) == mids).all() and mids[0] == kr.fp8_decode(np.uint8(1), fmt) / 2
    even = np.where(lo % 2 == 0, lo, hi)
    below, above = np.nextafter(m32, np.float32(0)), np.nextafter(m32, np.float32(np.inf))
    for sgn, bit in ((1, 0), (-1, 0x80)):
        kr.assert_same_bits(kr.fp8_encode(sgn * m32, fmt), even | bit, "tie")
        kr.assert_same_bits(kr.fp8_encode(sgn * below, fmt), lo | bit, "one ulp below a tie")
        kr.assert_same_bits(kr.fp8_encode(sgn * above, fmt), hi | bit, "one ulp above a tie")


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_encode_saturates(fmt):
    fmax = np.float32(kr.FP8_FMAX[fmt])
    big = np.float32([np.nextafter(fmax, np.float32(np.inf)), fmax * 1.07, fmax * 2, 3e38, np.inf])
    assert (kr.fp8_encode(big, fmt) == kr.FP8_MAX_CODE[fmt]).all()
    assert (kr.fp8_encode(-big, fmt) == (0x80 | kr.FP8_MAX_CODE[fmt])).all()
    # the clamp as the kernel writes it, fminf(fmaxf(NaN, -FMAX), FMAX), gives -FMAX
    assert (kr.fp8_encode(np.float32([np.nan, -np.nan]), fmt) == (0x80 | kr.FP8_MAX_CODE[fmt])).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_encode_matches_torch_cpu_cast(fmt):
    pat, _ = kr.fp8_exhaustive_inputs(fmt, 1.0)
    assert pat.numel() == 65536 - 2 * 127
    xb = pat.view(BF).float().numpy()
    kr.assert_same_bits(kr.fp8_encode(xb, fmt), torch_codes(xb, fmt), "all bf16 patterns")
    gg = g(40 + fmt)
    x = torch.randn(400000, generator=gg) * torch.exp2(torch.rand(400000, generator=gg) * 37 - 20)
    assert x.abs().min() < 2.0 ** -19 and x.abs().max() > 2.0 ** 16
    kr.assert_same_bits(kr.fp8_encode(x, fmt), torch_codes(x.numpy(), fmt), "random fp32")
    for s in (2.0 ** -3, 448.0 / 17, 57344.0 / 3):
        _, x32 = kr.fp8_exhaustive_inputs(fmt, s)
        with np.errstate(all="ignore"):
            v = x32 * np.float32(s)
        kr.assert_same_bits(kr.fp8_cast_ref(x32, s, fmt), torch_codes(v, fmt), f"exhaustive set at s={s}")


def test_fp8_scale_and_meta_ref():
    assert kr.fp8_scale(0.0, 0) == 1 and kr.fp8_scale(np.inf, 1) == 0 and kr.fp8_dq(np.float32(0)) == np.inf
    assert kr.fp8_scale(17.0, 0) == np.float32(448) / np.float32(17)
    m = kr.fp8_meta_ref(1)
    m.seed(4.0)
    assert m.idx == 1 and m.scale == np.float32(14336) and m.dq == np.float32(1 / 14336) and m.hist[0] == 4
    used, dq = m.roll(64.0)
    assert used == np.float32(14336) and dq == m.dq and m.hist[1] == 64 and m.scale == np.float32(896) and m.idx == 2
    w = m.words()
    assert w.dtype == np.uint32 and w.size == kr.FP8_META_WORDS and w[4] == 2 and w[2] == 0
    kr.assert_same_bits(kr.fp8_meta_ref(1, w).words(), w, "round trip")
    m.amax = np.float32(100)  # a preset slot above the cast's amax wins
    m.roll_partial(np.float32([1, 3, 2]))
    assert m.hist[2] == 100 and m.amax == 0
    # the partial index map: block b of nblk takes 2048-element chunks b, b + nblk, ...
    x = np.zeros(3 * 2048 + 5, dtype=np.float32)
    x[0], x[2048], x[2 * 2048 + 7], x[-1] = -1, 2, -3, 4
    assert kr.fp8_amax_partials(x, 4).tolist() == [1, 2, 3, 4]
    assert kr.fp8_amax_partials(x, 2).tolist() == [3, 4] and kr.fp8_amax(x) == 4


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fault", ["trunc", "away", "noclamp", "fmax240"])
def test_fp8_exhaustive_set_rejects_rounding_and_clamp_faults(fmt, fault):
    """The inputs of the GPU rounding test, at each of its scales, under code equality."""
    for s in (1.0, 2.0 ** -3, 2.0 ** 5, 448.0 / 17, 57344.0 / 3):
        pat, x32 = kr.fp8_exhaustive_inputs(fmt, s)
        for x in (pat.view(BF).float().numpy(), x32):
            with np.errstate(all="ignore"):
                v = x * np.float32(s)
            ref = kr.fp8_cast_ref(x, s, fmt)
            fin = ~np.isnan(v)
            kr.assert_same_bits(faulty_encode(v[fin], fmt, "none"), ref[fin], "the emulation without a fault")
            if fault == "fmax240" and fmt == 1:
                continue  # (240 is an e4m3 maximum; e5m2 has no such neighbour format)
            if fault == "away" and s not in (1.0, 2.0 ** -3, 2.0 ** 5):
                continue  # (a product by 448/17 or 57344/3 need not land on a tie: the power-of-two scales hold them)
            with pytest.raises(AssertionError):
                kr.assert_same_bits(faulty_encode(v[fin], fmt, fault), ref[fin], fault)
    if fault == "away":  # ties are the only difference, and the bf16 patterns at s = 1 hold them
        x = kr.fp8_exhaustive_inputs(fmt, 1.0)[0].view(BF).float().numpy()
        bad = faulty_encode(x, fmt, fault) != kr.fp8_cast_ref(x, 1.0, fmt)
        mids = kr.fp8_midpoints(fmt)[0]
        assert bad.any() and np.isin(np.abs(x[bad]).astype(np.float64), mids).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_cast_inputs_reject_divide_by_dq(fmt):
    """x / dq is not x * s: the fp32 inputs of the current-scaling cast test hold values whose
    product lies an ulp from a tie, where the two differ (in few codes: a ratio test passes it)."""
    x = kr.fp8_cast_inputs(2049, 0, 7, fmt).copy()
    x[-1] = -kr.FP8_PLANT
    s = kr.fp8_scale(kr.fp8_amax(x), fmt)
    assert s == np.float32(kr.FP8_FMAX[fmt]) / np.float32(kr.FP8_PLANT)
    ref = kr.fp8_cast_ref(x, s, fmt)
    div = kr.fp8_encode(x / kr.fp8_dq(s), fmt)
    same = (div == ref).mean()
    assert 0.9 < same < 1.0, same
    with pytest.raises(AssertionError):
        kr.assert_same_bits(div, ref, "x / dq")
    _, x32 = kr.fp8_exhaustive_inputs(fmt, 57344.0 / 3)  # ... and so do those of the rounding test
    s = np.float32(57344.0 / 3)
    with np.errstate(all="ignore"):
        assert (kr.fp8_encode(x32 / kr.fp8_dq(s), fmt) != kr.fp8_cast_ref(x32, s, fmt)).any()


def test_fp8_code_equality_rejects_stale_tail_and_shifted_group():
    x = kr.fp8_cast_inputs(2049, 1, 8)
    ref = kr.fp8_cast_ref(x, 448.0 / 17, 0)
    out = kr.guarded(2049, torch.uint8, CPU)
    out.copy_(torch.from_numpy(ref))
    kr.assert_same_bits(out, ref, "all written")
    out[-1] = kr.POISON_BYTE  # the scalar tail's one byte left as it was
    assert ref[-1] != kr.POISON_BYTE
    with pytest.raises(AssertionError):
        kr.assert_same_bits(out, ref, "stale tail byte")
    kr.check_guards()
    R, C = 65, 63
    w = kr.fp8_cast_inputs(R * C, 0, 9).reshape(R, C)
    q = kr.fp8_cast_ref(w, 448.0 / 16, 0)
    qt = np.ascontiguousarray(q.T)
    kr.assert_same_bits(torch.from_numpy(qt.copy()), q.T, "transpose")
    bad = qt.copy()
    bad[62, 60:64] = qt[62, 61:65]  # the last column's last whole 4-row group, one row late
    assert (bad != qt).any()
    with pytest.raises(AssertionError):
        kr.assert_same_bits(bad, q.T, "shifted 4-row group")


class _sticky_slot0(kr.fp8_meta_ref):
    """The seeded history fault: the ring wraps over slots 1 .. 15 and never overwrites slot 0."""

    def roll(self, amax32):
        real, self.idx = self.idx, (self.idx if self.idx < kr.FP8_HIST else 1 + (self.idx - 1) % (kr.FP8_HIST - 1))
        out = super().roll(amax32)
        self.idx = real + 1
        return out


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_script_forgets_seed_and_spike(fmt):
    seed, steps = kr.fp8_script()
    assert len(steps) == 40 and steps[2] == max(steps) and 0.0 in steps and seed > sorted(steps)[-2]
    assert all(float(torch.tensor(a).to(BF)) == a for a in steps + [seed])
    good, bad = kr.fp8_meta_ref(fmt), _sticky_slot0(fmt)
    good.seed(seed)
    bad.seed(seed)
    fmax = np.float32(kr.FP8_FMAX[fmt])
    first_diff = None
    for k, a in enumerate(steps):
        good.roll(a)
        bad.roll(a)
        if 2 <= k <= 17:
            assert good.scale == fmax / np.float32(64), k  # the spike rules for exactly 16 steps
        if k == 18:
            assert good.scale == fmax / np.float32(max(steps[3:19])), k
        if first_diff is None and (good.words() != bad.words()).any():
            first_diff = k
    assert good.idx == 41  # two wraps of the 16-slot ring
    assert first_diff == 15, first_diff  # the roll that should overwrite slot 0 (the seed)
    assert bad.scale == fmax / np.float32(seed) and good.scale > bad.scale  # ... and it never forgets it


@pytest.mark.parametrize("fmt", FMTS)
def test_fp8_boundary_condition_holds_for_an_fp32_gelu_grad(fmt):
    """The GELU-gradient cast's condition (kr.fp8_boundary_check), on the CPU: codes of an fp32
    x * gelu'(z) stay within it, with the allowance measured as the GPU test measures it; codes one
    step off away from a boundary, or two steps off, do not."""
    gg = g(50 + fmt)
    z = kr.normal((129 * 1032,), gg, std=2.0)
    x = kr.ints((129 * 1032,), gg)
    d64 = kr.gelu_tanh_grad_ref(z)
    zz = z.float().requires_grad_()
    F.gelu(zz, approximate="tanh").sum().backward()
    e_ref = (zz.grad.double() - d64).abs().max().item()
    allow = 4 * max(e_ref, kr.U * d64.abs().max().item())
    s = kr.fp8_boundary_scale(allow, 8, fmt)
    codes = kr.fp8_cast_ref((x.float() * zz.grad).numpy(), s, fmt)
    p64, ax = (kr.f64(x) * d64).numpy(), kr.f64(x).abs().numpy()
    ndiff = kr.fp8_boundary_check(codes, p64, ax, s, allow, fmt, "fp32 gelu'")
    print(f"MEASURED fp8 boundary check fmt={fmt}: allowance {allow:.3e}, {ndiff} of {codes.size} codes differ")
    # (nearly all of them are -0 for +0 at z < -5, where gelu' is below the fp32 op's absolute error)
    assert ndiff < codes.size * 1e-2
    ref = kr.fp8_cast_ref(p64.astype(np.float32), s, fmt)
    i = int(np.flatnonzero((ref & 0x7F > 8) & (ref & 0x7F < kr.FP8_MAX_CODE[fmt] - 2))[0])
    for delta in (1, 2):
        bad = ref.copy()
        bad[i] += delta
        with pytest.raises(AssertionError):
            kr.fp8_boundary_check(bad, p64, ax, s, 0.0 if delta == 1 else 1.0, fmt, "seeded")


# ------------------------------------------------------------------------------------ attention
AB, AH, ASC = kr.ATTN_B, kr.ATTN_H, kr.ATTN_SCALE
EMU_T = [5, 65, 197, 321]


def _attn_case(family, T):
    inp = kr.attn_inputs(family, AB, T, AH, kr.attn_seed(family, T), CPU)
    fwd = kr.attn_fwd_ref(inp["qkv"], AH, ASC)
    out_r, lse_r = fwd["out"].to(BF), fwd["lse"].to(torch.float32)
    return inp, fwd, out_r, lse_r, kr.attn_bwd_ref(inp["qkv"], out_r, inp["dout"], lse_r, AH, ASC)


_attn_cases = {}


def attn_case(family, T):
    if (family, T) not in _attn_cases:
        _attn_cases[family, T] = _attn_case(family, T)
    return _attn_cases[family, T]


def test_attn_refs_match_torch_autograd():
    """attn_fwd_ref / attn_bwd_ref / attn_cls_ref against float64 autograd attention. The backward
    references take the unrounded O and the fp64 lse here, where their definition (delta from the
    given out, P from the given lse) coincides with the derivative."""
    B, T, H = 2, 37, 3
    gg = g(60)
    x = (torch.randn(B, T, 3 * H * 64, generator=gg, dtype=kr.F64) * 1.5).requires_grad_()
    dout = torch.randn(B, T, H * 64, generator=gg, dtype=kr.F64)
    q, k, v = x.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, H * 64)
    (o * dout).sum().backward()
    f = kr.attn_fwd_ref(x, H, 0.125)
    # (c is an fp32 product: it differs from 0.125 log2(e) by < 2^-24 relative, |c s| < 400 here)
    assert rel(f["out"], o.detach()) < 1e-4
    lse2 = torch.logsumexp(s.detach(), -1).reshape(B * H, T) / kr.LN2
    assert rel(f["lse"], lse2) < 1e-7
    assert bool((f["A_out"] >= f["out"].abs() - 1e-12).all()) and bool((f["out_bound"] > 0).all())
    # with c exactly 0.125 log2(e) the formulas agree to 1e-12
    c0 = kr.attn_c
    try:
        kr.attn_c = lambda scale: scale / kr.LN2
        f = kr.attn_fwd_ref(x, H, 0.125)
        assert rel(f["out"], o.detach()) < 1e-12 and rel(f["lse"], lse2) < 1e-12
        b = kr.attn_bwd_ref(x, f["out"], dout, f["lse"], H, 0.125)
        assert rel(b["dqkv"], x.grad) < 1e-12
        assert rel(b["delta"], (dout * o.detach()).view(B, T, H, 64).sum(-1).permute(0, 2, 1).reshape(B * H, T)) < 1e-12
        assert bool((b["dqkv_bound"] >= 0).all())
    finally:
        kr.attn_c = c0
    # class token: the same attention, gradient flowing into token 0's output only
    x2 = x.detach().clone().requires_grad_()
    q, k, v = x2.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q[:, :, :1] @ k.transpose(-1, -2)) * 0.125
    o0 = (torch.softmax(s, -1) @ v).reshape(B, H * 64)
    (o0 * dout[:, 0]).sum().backward()
    cf = kr.attn_cls_ref(x2, H)
    assert rel(cf["out"], o0.detach()) < 1e-12
    assert rel(cf["lse"], torch.logsumexp(s.detach(), -1).reshape(B * H)) < 1e-12
    cb = kr.attn_cls_ref(x2, H, dout[:, 0], cf["out"], cf["lse"])
    assert rel(cb["dqkv"], x2.grad) < 1e-12
    dq = cb["dqkv"].view(B, T, 3, H * 64)[:, 1:, 0]
    assert bool((dq == 0).all()) and bool((cb["dqkv_bound"].view(B, T, 3, H * 64)[:, 1:, 0] == 0).all())


@pytest.mark.parametrize("T", kr.ATTN_T_ALL)
def test_attn_onehot_gap_and_exactness(T):
    """The onehot family at every T of the GPU file: every other key lies >= 150 below the selected
    one in c*s (fp32 exp2 gives exactly 0), and the float64 references agree with the closed forms
    V[sel], dO[sel^-1], 0 to far below an fp32 denormal."""
    for fam in ("onehot", "onehot0"):
        inp = kr.attn_inputs(fam, AB, T, AH, kr.attn_seed(fam, T), CPU)
        sel = inp["sel"]
        assert int(sel[0, 0, 0]) == (T - 1 if fam == "onehot" else 0) and int(sel[1, 2, T - 1]) == (0 if fam == "onehot" else T - 1)
        assert bool((sel.sort(-1).values == torch.arange(T)).all())
        f = kr.attn_fwd_ref(inp["qkv"], AH, ASC)
        assert f["gap"] >= kr.ONEHOT_GAP, f["gap"]
        assert kr.attn_cls_ref(inp["qkv"], AH)["gap"] >= kr.ONEHOT_GAP
        out, dqkv = kr.attn_onehot_expect(inp, AH)
        assert (f["out"] - out).abs().max().item() < 1e-100
        assert bool((f["lse"] == f["c"] * 8192).all())
        b = kr.attn_bwd_ref(inp["qkv"], f["out"].to(BF), inp["dout"], f["lse"].to(torch.float32), AH, ASC)
        assert (b["dqkv"] - dqkv).abs().max().item() < 1e-100
    if T > 1:
        assert not torch.equal(sel[0, 0], sel[0, 1]) or T < 4


def _heads32(x, H):
    return [t.float() for t in kr.attn_heads(x, H)]


def emulate_attn_fwd(inp, tile=64, fault=None):
    """fp32 emulation of the kernels' algorithm: online softmax over ``tile`` keys with rescaling,
    P packed to bf16 for the PV product, l summed from the unrounded exponentials, fp32
    accumulation -> (out bf16 [B][T][H*64], lse fp32 [B*H][T]). ``fault``: one seeded fault."""
    q, k, v = _heads32(inp["qkv"], AH)
    B, H, T, _ = q.shape
    c = torch.tensor(kr.attn_c(ASC), dtype=torch.float32)
    Tp = -(-T // tile) * tile
    k, v = F.pad(k, (0, 0, 0, Tp - T)), F.pad(v, (0, 0, 0, Tp - T))
    if fault == "swap_v":
        j = T // 2
        v[:, :, [j, j + 1 if j + 1 < T else j - 1]] = v[:, :, [j + 1 if j + 1 < T else j - 1, j]]
    m = torch.full((B, H, T, 1), -math.inf)
    l, o = torch.zeros(B, H, T, 1), torch.zeros(B, H, T, 64)
    for k0 in range(0, Tp, tile):
        s = (q @ k[:, :, k0:k0 + tile].transpose(-1, -2)) * c
        key = torch.arange(k0, k0 + tile)
        valid = key < (T + 1 if fault == "unmasked" else T)
        if fault == "skip_key":
            valid = valid & (key != T // 2)
        s = torch.where(valid, s, torch.tensor(-math.inf))
        mn = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp2(m - mn)
        e = torch.exp2(s - mn)
        pb = e.to(BF).float()
        l = l * alpha + (pb if fault == "l_from_bf16" else e).sum(-1, keepdim=True)
        if fault != "no_rescale":
            o = o * alpha
        o = o + pb @ v[:, :, k0:k0 + tile]
        m = mn
    lse = m + torch.log2(l)
    if fault == "lse_natural":
        lse = lse * kr.LN2
    lse = lse.reshape(B, H, T)
    if fault == "lse_bh_swapped":  # stored at [h * B + b]
        lse = lse.transpose(0, 1)
    return kr.attn_flat(o / l).to(BF), lse.reshape(B * H, T).contiguous()


def emulate_attn_bwd(inp, out, lse, fault=None):
    """fp32 emulation of the recomputing backward: P and dS packed to bf16 before the second
    GEMMs, fp32 accumulation -> dqkv bf16 [B][T][3*H*64]."""
    q, k, v = _heads32(inp["qkv"], AH)
    B, H, T, _ = q.shape
    o, do = kr.attn_rows(out, AH).float(), kr.attn_rows(inp["dout"], AH).float()
    c = torch.tensor(kr.attn_c(ASC), dtype=torch.float32)
    P = torch.exp2((q @ k.transpose(-1, -2)) * c - lse.view(B, H, T, 1))
    delta = (do * o).sum(-1, keepdim=True)
    if fault == "delta_wrong_row":
        delta = delta.roll(1, 2)
    dS = P * (do @ v.transpose(-1, -2) - delta)
    Pb, dSb = P.to(BF).float(), dS.to(BF).float()
    sc = 1.0 if fault == "dk_no_scale" else ASC
    return kr._attn_pack3((dSb @ k) * ASC, (dSb.transpose(-1, -2) @ q) * sc, Pb.transpose(-1, -2) @ do).to(BF)


@pytest.mark.parametrize("T", EMU_T)
@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
def test_attn_emulation_within_bounds(family, T):
    """The unmodified fp32 emulation passes every family within the derived bounds (tiles of 64 and
    of 32 keys, and the whole sequence at once): the references alone stay inside them."""
    inp, fwd, out_r, lse_r, bwd = attn_case(family, T)
    for tile in (64, 32, 512):
        out, lse = emulate_attn_fwd(inp, tile)
        kr.attn_check_fwd(inp, fwd, out, lse, AH, f"{family} T={T} tile={tile}")
    kr.attn_check_bwd(inp, bwd, emulate_attn_bwd(inp, out_r, lse_r), AH, f"{family} T={T}")
    if family == "counting":  # the closed form: 8 n_d / T
        n = torch.zeros(AB, AH, 64, dtype=kr.F64)
        for b in range(AB):
            for h in range(AH):
                n[b, h] = torch.bincount((torch.arange(T) + 5 * (b * AH + h)) % 64, minlength=64)
        assert rel(fwd["out"].view(AB, T, AH, 64)[:, 3], 8 * n / T) < 1e-12


def _rejects(check):
    try:
        check()
    except AssertionError:
        return True
    return False


# fault -> (forward or backward, the family named to reject it, the T at which it does)
ATTN_FAULTS = {
    "unmasked": ("fwd", "negative", 65),         # the padded key's score 0 beats every real one
    "skip_key": ("fwd", "onehot", 65),           # the query that selects it gets another row (NaN: none)
    "swap_v": ("fwd", "onehot", 65),
    "no_rescale": ("fwd", "onehot", 65),         # query 0 selects key T - 1: the maximum arrives last
    "l_from_bf16": ("fwd", "negative", 5),       # lse moves by ~2^-9 / sqrt(T), the bound is ~1e-4
    "lse_natural": ("fwd", "counting", 65),
    "lse_bh_swapped": ("fwd", "normal", 65),     # (onehot and counting have the same lse in every head)
    "dk_no_scale": ("bwd", "normal", 65),
    "delta_wrong_row": ("bwd", "onehot", 65),    # dP - delta no longer cancels: dQ, dK != 0
}


@pytest.mark.parametrize("fault", sorted(ATTN_FAULTS))
def test_attn_seeded_fault_is_rejected(fault):
    """Each fault, seeded alone into the emulation, is rejected by the family named for it."""
    kind, family, T = ATTN_FAULTS[fault]
    inp, fwd, out_r, lse_r, bwd = attn_case(family, T)
    if kind == "fwd":
        out, lse = emulate_attn_fwd(inp, 64, fault)
        assert _rejects(lambda: kr.attn_check_fwd(inp, fwd, out, lse, AH, fault))
        kr.attn_check_fwd(inp, fwd, *emulate_attn_fwd(inp, 64), AH, fault)
    else:
        assert _rejects(lambda: kr.attn_check_bwd(inp, bwd, emulate_attn_bwd(inp, out_r, lse_r, fault), AH, fault))
        kr.attn_check_bwd(inp, bwd, emulate_attn_bwd(inp, out_r, lse_r), AH, fault)


def emulate_cls(inp, o=None, lse=None):
    """fp32 evaluation of the class-token attention: forward (o is None) -> (out bf16 [B][H*64],
    lse fp32 [B*H]); backward from the given o and lse -> dqkv bf16 [B][T][3*H*64]."""
    q, k, v = _heads32(inp["qkv"], AH)
    B, H, T, _ = q.shape
    q0 = q[:, :, :1] * 0.125
    s = q0 @ k.transpose(-1, -2)
    if o is None:
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        return ((e / l) @ v).reshape(B, H * 64).to(BF), (m + torch.log(l)).reshape(B * H)
    do = inp["dout"][:, 0].float().view(B, H, 1, 64)
    P = torch.exp(s - lse.view(B, H, 1, 1))
    dS = P * (do @ v.transpose(-1, -2) - (do * o.float().view(B, H, 1, 64)).sum(-1, keepdim=True))
    dq = torch.zeros_like(q)
    dq[:, :, :1] = (dS @ k) * 0.125
    return kr._attn_pack3(dq, dS.transpose(-1, -2) * q0, P.transpose(-1, -2) * do).to(BF)


def test_attn_cls_emulation_and_faults():
    """The class-token checks accept an fp32 evaluation and reject an unwritten dq row, a dq of
    another token that is not 0, and a log2-domain lse."""
    for family in ("onehot", "onehot0", "counting", "negative", "normal"):
        for T in (1, 33, 197):
            what = f"{family} T={T}"
            inp = kr.attn_inputs(family, AB, T, AH, kr.attn_seed(family, T), CPU)
            f = kr.attn_cls_ref(inp["qkv"], AH)
            out, lse = emulate_cls(inp)
            kr.attn_check_cls_fwd(inp, f, out, lse, AH, what)
            o_r, lse_r = f["out"].to(BF), f["lse"].to(torch.float32)
            r = kr.attn_cls_ref(inp["qkv"], AH, inp["dout"][:, 0], o_r, lse_r)
            good = emulate_cls(inp, o_r, lse_r)
            kr.attn_check_cls_bwd(inp, r, good, AH, what)
            if T > 1:
                bad = good.clone()
                bad.view(AB, T, 3, AH * 64)[1, T - 1, 0, 5] = float("nan")
                assert _rejects(lambda: kr.attn_check_cls_bwd(inp, r, bad, AH, "poison"))
                bad = good.clone()
                bad.view(AB, T, 3, AH * 64)[0, 1, 0, 0] = 2.0 ** -100
                assert _rejects(lambda: kr.attn_check_cls_bwd(inp, r, bad, AH, "nonzero"))
                assert _rejects(lambda: kr.attn_check_cls_fwd(inp, f, out, lse / kr.LN2, AH, "log2 lse"))
