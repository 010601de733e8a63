"""The stochastic-depth kernels, called directly: pdt_drop_path_scales (csrc/drop_path.hip)
against the torch mirror of the draw, and the drop-path instantiations of the LayerNorm kernels
(pdt_ln_add_dp_fwd / pdt_ln_dp_bwd, csrc/layernorm.hip) against their existing siblings bit for
bit and against float64 (tests/drop_path_ref.py). Row counts are no multiple of the 4 waves of a
block, and a block straddles a sample boundary at 197 rows per sample. Outputs are guard-banded.

Bounds: the forward's are those of tests/test_row_kernels_gpu.py::test_ln_fwd, restated here with
the kernel's own bf16 sum as the LayerNorm's input, plus one fused multiply-add and the bf16
rounding for the sum itself; the bias gradient's on random data is the relative 1e-3 of
tests/test_vit_launch_dispatch_gpu.py::test_ln_backward_entry_points_agree."""
import pytest
import torch

import drop_path_ref as dr
import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
LN_EPS = float(torch.tensor(1e-6, dtype=F32))
WIDTHS = (256, 512, 768, 1024)
SHAPES = ((3, 5), (2, 197), (5, 1))  # (samples, rows per sample)


def G(shape, dtype, fill=None):
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def seeded_meta(shape, g, fmt):
    return no.quantize_fp8_delayed(kr.normal(shape, g), None, fmt)[2]


# ------------------------------------------------------------------------------- scale table
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_branches", [1, 24])
def test_scale_table_matches_the_mirror_and_the_step_advances(B, n_branches):
    lib = no._load()
    seed, step0 = 1234 + B, 7
    for p in (0.0, 0.1, 0.5):
        what = f"drop_path_scales B={B} n={n_branches} p={p}"
        pt = torch.full((n_branches,), p, dtype=torch.float64)
        p32, inv32 = pt.to(F32).to(DEV), (1.0 / (1.0 - pt)).to(F32).to(DEV)
        state = G(2, I32, torch.tensor([seed, step0], dtype=I32))
        for k, rank in ((0, 0), (1, 3)):  # two consecutive calls: steps s and s + 1
            table = G((n_branches, B), F32)
            assert lib.pdt_drop_path_scales(no._p(table), no._p(state), no._p(p32), no._p(inv32), n_branches, B,
                                            rank * B, no._s()) == 0, what
            torch.cuda.synchronize()
            want = dr.expected_table(seed, step0 + k, p, B, rank, n_branches)
            assert torch.equal(table.cpu(), want), (what, k)
            assert state.tolist() == [seed, step0 + k + 1], what
            if p == 0.0:
                assert bool((table == 1.0).all()), what
        done(what)


def test_scale_table_refuses_bad_arguments():
    lib = no._load()
    t, s, p = G((2, 4), F32, 3.0), G(2, I32, 0), G(2, F32, 0.5)
    for args in ((None, no._p(s), no._p(p), no._p(p), 2, 4), (no._p(t), None, no._p(p), no._p(p), 2, 4),
                 (no._p(t), no._p(s), no._p(p), no._p(p), 0, 4), (no._p(t), no._p(s), no._p(p), no._p(p), 2, 0)):
        assert lib.pdt_drop_path_scales(*args, 0, no._s()) == -1
    done("refused")
    assert bool((t == 3.0).all()) and s.tolist() == [0, 0]


# ----------------------------------------------------------------------------------- forward
def dp_fwd(lib, y, r, w, b, scale, rps, what, meta0=None, codes_only=False):
    rows, D = r.shape
    xsum, h, mean, rstd = G((rows, D), BF), G((rows, D), BF), G(rows, F32), G(rows, F32)
    q = part = dq = meta = None
    if meta0 is not None:
        q, part = G((rows, D), U8), G(lib.pdt_ln_fwd_f8_blocks(rows), F32)
        dq, meta = G(1, F32), G(meta0.shape, F32, meta0)
    assert lib.pdt_ln_add_dp_fwd(no._p(y), no._p(r), no._p(xsum), no._p(w), no._p(b), None if codes_only else no._p(h),
                                 no._p(mean), no._p(rstd), rows, D, LN_EPS, no._p(q), no._p(meta), no._p(part),
                                 no._p(dq), no._p(scale), rps, no._s()) == 0, what
    return dict(xsum=xsum, h=h, mean=mean, rstd=rstd, q=q, dq=dq, meta=meta)


def add_fwd(lib, y, r, w, b, what, meta0=None):
    rows, D = r.shape
    xsum, h, mean, rstd = G((rows, D), BF), G((rows, D), BF), G(rows, F32), G(rows, F32)
    q = part = dq = meta = None
    if meta0 is not None:
        q, part = G((rows, D), U8), G(lib.pdt_ln_fwd_f8_blocks(rows), F32)
        dq, meta = G(1, F32), G(meta0.shape, F32, meta0)
    assert lib.pdt_ln_add_fwd(no._p(y), no._p(r), no._p(xsum), no._p(w), no._p(b), no._p(h), no._p(mean), no._p(rstd),
                              rows, D, LN_EPS, no._p(q), no._p(meta), no._p(part), no._p(dq), no._s()) == 0, what
    return dict(xsum=xsum, h=h, mean=mean, rstd=rstd, q=q, dq=dq, meta=meta)


def ln_fwd_f8(lib, x, w, b, meta0, what):
    rows, D = x.shape
    h, mean, rstd = G((rows, D), BF), G(rows, F32), G(rows, F32)
    q, part = G((rows, D), U8), G(lib.pdt_ln_fwd_f8_blocks(rows), F32)
    dq, meta = G(1, F32), G(meta0.shape, F32, meta0)
    assert lib.pdt_ln_fwd_f8(no._p(x), no._p(w), no._p(b), no._p(h), no._p(mean), no._p(rstd), rows, D, LN_EPS,
                             no._p(q), no._p(meta), no._p(part), no._p(dq), no._s()) == 0, what
    return dict(h=h, mean=mean, rstd=rstd, q=q, dq=dq, meta=meta)


@pytest.mark.parametrize("B,rps", SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_table_of_ones_is_the_plain_add(D, B, rps):
    lib = no._load()
    rows = B * rps
    g = kr.gen(13 * D + rows)
    what = f"ln_add_dp_fwd ones D={D} B={B} rps={rps}"
    y, r = kr.normal((rows, D), g, std=2.0, mean=1.0), kr.normal((rows, D), g)
    w, b = kr.normal((D,), g, F32), kr.normal((D,), g, F32)
    ones = torch.ones(B, dtype=F32, device=DEV)
    for meta0 in (None, seeded_meta((rows, D), g, no.E4M3)):
        a = dp_fwd(lib, y, r, w, b, ones, rps, what, meta0)
        ref = add_fwd(lib, y, r, w, b, what, meta0)
        done(what)
        for k in ("xsum", "h", "mean", "rstd") + (("q", "dq", "meta") if meta0 is not None else ()):
            assert torch.equal(a[k], ref[k]), (what, k, meta0 is not None)


@pytest.mark.parametrize("B,rps", SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_masks(D, B, rps):
    lib = no._load()
    rows = B * rps
    g = kr.gen(17 * D + rows)
    w, b = kr.normal((D,), g, F32), kr.normal((D,), g, F32)
    meta0 = seeded_meta((rows, D), g, no.E4M3)
    L = 4 * (D // 256) + 8
    for mask in dr.MASKS:
        what = f"ln_add_dp_fwd D={D} B={B} rps={rps} {mask}"
        scale = dr.mask_scale(mask, B, 2.0, DEV)
        rowkeep = (scale != 0).repeat_interleave(rps)
        # integers, scale 2: the sum is exact
        yi, ri = kr.ints((rows, D), g), kr.ints((rows, D), g)
        out = dp_fwd(lib, yi, ri, w, b, scale, rps, what)
        done(what + " ints")
        kr.assert_exact(out["xsum"], dr.xsum_ref(yi, ri, scale, rps)[0], what + " xsum (ints)")
        # dropped samples: y is NaN there; xsum holds r's bits and nothing is NaN
        yn, rn = kr.normal((rows, D), g, std=2.0, mean=1.0), kr.normal((rows, D), g)
        yn[~rowkeep] = float("nan")
        if not bool(rowkeep.all()):  # bits that an add of 0 would change, in the first dropped row
            rn[int((~rowkeep).to(torch.uint8).argmax()), :4] = torch.tensor([-0.0, 0.0, -1e-40, 1e-40], dtype=BF, device=DEV)
        out = dp_fwd(lib, yn, rn, w, b, scale, rps, what, meta0)
        only = dp_fwd(lib, yn, rn, w, b, scale, rps, what, meta0, codes_only=True)
        of8 = ln_fwd_f8(lib, out["xsum"], w, b, meta0, what)
        done(what + " normal")
        assert torch.equal(out["xsum"][~rowkeep].view(torch.int16), rn[~rowkeep].view(torch.int16)), what
        for k in ("xsum", "h", "mean", "rstd"):
            assert not bool(torch.isnan(out[k]).any()), (what, k)
        # the codes and the rolled scaling state: pdt_ln_fwd_f8 of the kernel's own sum
        for k in ("h", "mean", "rstd", "q", "dq", "meta"):
            assert torch.equal(out[k], of8[k]), (what, k)
        for k in ("xsum", "mean", "rstd", "q", "dq", "meta"):  # codes only: y == nullptr
            assert torch.equal(only[k], out[k]), (what, k, "codes only")
        # against float64 (test_ln_fwd's bounds, the LayerNorm's input being the bf16 sum)
        ref = dr.ln_add_dp_fwd_ref(yn, rn, scale, rps, w, b, LN_EPS)
        kr.assert_bf16_close(out["xsum"], ref["xsum"], ref["xsum_abs"], what + " xsum")
        xs = kr.f64(out["xsum"])
        ref = kr.ln_fwd_ref(out["xsum"], w, b, LN_EPS)
        em = 2 * L * kr.U * xs.abs().mean(1)
        kr.assert_close(out["mean"], ref["mean"], em + kr.U * ref["mean"].abs(), what + " mean")
        dvar = 2 * (L + 3) * kr.U * ref["var"] + em ** 2
        rrel = 0.5 * dvar / (ref["var"] + LN_EPS) + 4 * kr.U
        kr.assert_close(out["rstd"], ref["rstd"], ref["rstd"] * rrel, what + " rstd")
        ga = kr.f64(w).abs()
        extra = (em * ref["rstd"])[:, None] * ga + (ref["xhat"] * kr.f64(w)).abs() * rrel[:, None]
        kr.assert_bf16_close(out["h"], ref["y"], ref["y_abs"], what + " y", extra=extra)


def test_forward_refuses_bad_arguments():
    lib = no._load()
    x = torch.zeros(4, 256, dtype=BF, device=DEV)
    w, s = torch.zeros(256, device=DEV), torch.ones(4, device=DEV)
    xsum, y, mean, rstd = G((4, 256), BF, 1.0), G((4, 256), BF, 1.0), G(4, F32, 1.0), G(4, F32, 1.0)
    args = [no._p(x), no._p(x), no._p(xsum), no._p(w), no._p(w), no._p(y), no._p(mean), no._p(rstd), 4, 256, LN_EPS, None,
            None, None, None]
    assert lib.pdt_ln_add_dp_fwd(*args, None, 1, no._s()) == -1       # no scale
    assert lib.pdt_ln_add_dp_fwd(*args, no._p(s), 0, no._s()) == -1   # no rows per sample
    args[9] = 384
    assert lib.pdt_ln_add_dp_fwd(*args, no._p(s), 1, no._s()) == -1   # width outside the kernels'
    done("refused")
    for t in (xsum, y, mean, rstd):
        assert bool((t == 1.0).all())


# ---------------------------------------------------------------------------------- backward
def dp_bwd(lib, d, add, scale, rps, what, gmeta0=None, with_bias=False):
    rows, D = d["x"].shape
    blocks = lib.pdt_ln_bwd_blocks(rows)
    dx, dyb, dg, db, part = G((rows, D), BF), G((rows, D), BF), G(D, F32), G(D, F32), G(2 * blocks * D, F32)
    q8 = gmeta = qpart = dq = cpart = bias = None
    if gmeta0 is not None:
        q8, gmeta, qpart, dq = G((rows, D), U8), G(gmeta0.shape, F32, gmeta0), G(blocks, F32), G(1, F32)
        if with_bias:
            cpart, bias = G(blocks * D + lib.pdt_reduce_rows_work(blocks, D), F32), G(D, F32)
    assert lib.pdt_ln_dp_bwd(no._p(d["dy"]), no._p(d["x"]), no._p(d["gamma"]), no._p(d["mean"]), no._p(d["rstd"]),
                             no._p(dx), no._p(dyb), no._p(dg), no._p(db), no._p(part), rows, D, 0, no._p(add),
                             no._p(scale), rps, no._p(q8), no._p(gmeta), no._p(qpart), no._p(dq), no._p(cpart),
                             no._p(bias), 0, no._s()) == 0, what
    return dict(dx=dx, dyb=dyb, dg=dg, db=db, q8=q8, gmeta=gmeta, dq=dq, bias=bias)


def plain_bwd(lib, d, add, what):
    rows, D = d["x"].shape
    blocks = lib.pdt_ln_bwd_blocks(rows)
    dx, dg, db, part = G((rows, D), BF), G(D, F32), G(D, F32), G(2 * blocks * D, F32)
    assert lib.pdt_ln_bwd(no._p(d["dy"]), no._p(d["x"]), no._p(d["gamma"]), no._p(d["mean"]), no._p(d["rstd"]),
                          no._p(dx), no._p(dg), no._p(db), no._p(part), rows, D, 0, no._p(add), no._s()) == 0, what
    return dict(dx=dx, dg=dg, db=db)


@pytest.mark.parametrize("B,rps", SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_backward_masks(D, B, rps):
    lib = no._load()
    rows = B * rps
    g = kr.gen(19 * D + rows)
    gmeta0 = seeded_meta((rows, D), g, no.E5M2)
    families = {
        "exact": kr.exact_ln_bwd_inputs(rows, D, g),
        "normal": dict(dy=kr.normal((rows, D), g), x=kr.normal((rows, D), g, std=2.0, mean=1.0),
                       addend=kr.normal((rows, D), g), gamma=kr.normal((D,), g, F32),
                       mean=kr.normal((rows,), g, F32, 0.5, 1.0), rstd=torch.rand(rows, generator=g, device=DEV) + 0.25)}
    for mask in dr.MASKS:
        for family, d in families.items():
            # exact family: scale 2 keeps every product exact; normal: 1 / (1 - 0.1)
            scale = dr.mask_scale(mask, B, 2.0 if family == "exact" else float(torch.tensor(1 / 0.9, dtype=F32)), DEV)
            srow = scale.repeat_interleave(rps)[:, None]
            for add in (None, d["addend"]):
                what = f"ln_dp_bwd D={D} B={B} rps={rps} {mask} {family} addend={add is not None}"
                ref = plain_bwd(lib, d, add, what)
                a = dp_bwd(lib, d, add, scale, rps, what)
                f8 = dp_bwd(lib, d, add, scale, rps, what, gmeta0)
                f8b = dp_bwd(lib, d, add, scale, rps, what, gmeta0, with_bias=True)
                done(what)
                want = torch.where(srow != 0, ref["dx"].float() * srow, torch.zeros((), device=DEV)).to(BF)
                for o in (a, f8, f8b):
                    for k in ("dx", "dg", "db"):
                        assert torch.equal(o[k], ref[k]), (what, k)
                    assert torch.equal(o["dyb"].view(torch.int16), want.view(torch.int16)), what + " dyb"
                dropped = (srow == 0).expand_as(want)
                assert bool((a["dyb"].view(torch.int16)[dropped] == 0).all()), what + ": +0 on dropped samples"
                # the codes, the dequant factor and the rolled history: the e5m2 cast of dyb
                q_ref, dq_ref, meta_ref = no.quantize_fp8_delayed(a["dyb"], gmeta0.clone(), no.E5M2)
                torch.cuda.synchronize()
                for o in (f8, f8b):
                    assert torch.equal(o["q8"], q_ref) and torch.equal(o["dq"], dq_ref), what + " codes"
                    assert torch.equal(o["gmeta"], meta_ref), what + " history"
                # the producer's bias gradient: column sums of dyb as stored
                cs = kr.f64(a["dyb"]).sum(0)
                err = ((kr.f64(f8b["bias"]) - cs).norm() / cs.norm().clamp_min(1e-6)).item()
                assert err < 1e-3, (what, err)
                # and against float64: dyb within a bf16 rounding of scale * dx as stored
                r64 = dr.ln_dp_bwd_ref(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], scale, rps, add)
                prod = kr.f64(srow) * kr.f64(a["dx"])  # (one fp32 rounding of the product, then the bf16 one)
                kr.assert_close(a["dyb"], prod, (kr.BF16_HALF + 2 * kr.U) * prod.abs(), what + " dyb (f64)")
                if family == "exact" and D != 768:
                    kr.assert_exact(a["dyb"], r64["dyb"], what + " dyb (exact)")
        # integer-valued gradients (dy = 0: dx is the addend itself), scale 2: the bias gradient is exact
        what = f"ln_dp_bwd D={D} B={B} rps={rps} {mask} integer dx"
        d = dict(families["exact"], dy=torch.zeros((rows, D), dtype=BF, device=DEV))
        scale = dr.mask_scale(mask, B, 2.0, DEV)
        o = dp_bwd(lib, d, d["addend"], scale, rps, what, gmeta0, with_bias=True)
        done(what)
        assert torch.equal(o["dx"], d["addend"]), what
        want64 = dr.row_scale(scale, rps) * kr.f64(d["addend"])
        kr.assert_exact(o["dyb"], want64, what + " dyb")
        kr.assert_exact(o["bias"], want64.sum(0), what + " bias")


def test_backward_refuses_bad_arguments():
    lib = no._load()
    x = torch.zeros(4, 256, dtype=BF, device=DEV)
    w, s = torch.zeros(256, device=DEV), torch.ones(4, device=DEV)
    dx, dyb, dg, db, part = G((4, 256), BF, 1.0), G((4, 256), BF, 1.0), G(256, F32, 1.0), G(256, F32, 1.0), G(512, F32, 1.0)
    q8, cpart = G((4, 256), U8, 1), G(256 + lib.pdt_reduce_rows_work(1, 256), F32, 1.0)

    def call(dyb_p, scale_p, rps, q8_p=None, meta_p=None, cpart_p=None, D=256):
        return lib.pdt_ln_dp_bwd(no._p(x), no._p(x), no._p(w), no._p(dg), no._p(dg), no._p(dx), dyb_p, no._p(dg), no._p(db),
                                 no._p(part), 4, D, 0, None, scale_p, rps, q8_p, meta_p, meta_p, meta_p, cpart_p, None, 0,
                                 no._s())

    assert call(None, no._p(s), 1) == -1            # no branch gradient buffer
    assert call(no._p(dyb), None, 1) == -1          # no scale
    assert call(no._p(dyb), no._p(s), 0) == -1      # no rows per sample
    assert call(no._p(dyb), no._p(s), 1, no._p(q8)) == -1                    # codes without their state
    assert call(no._p(dyb), no._p(s), 1, None, None, no._p(cpart)) == -1     # column sums without codes
    assert call(no._p(dyb), no._p(s), 1, D=384) == -1
    done("refused")
    for t in (dx, dyb, db, part, cpart):
        assert bool((t == 1.0).all())
    assert bool((q8 == 1).all())
