"""Every instantiation the LayerNorm (csrc/layernorm.hip) and fp8 attention forward
(csrc/attention_f8.hip) entry points dispatch to, each checked bit for bit against a sibling entry
point that reaches the same arithmetic through another template argument:

* pdt_attn_fwd_f8_q8 against pdt_attn_fwd_f8 (O, LSE) and the separate delayed-scaling cast of O
  (codes, dequant factor, rolled history), at both ends of every 32-key tile count of the 4-wave
  (T <= 128) and 8-wave (T > 128) ladders, and on the 4-wave fp8-PV ladder above 128;
* pdt_ln_fwd_f8 / pdt_ln_add_fwd against pdt_ln_fwd, pdt_ln_bwd_f8 / pdt_ln_bwd_f8_db against
  pdt_ln_bwd, at every width and at one row, one full block of 4 rows and one row past it.

Outputs are guard-banded (tests/kernel_ref.py)."""
import pytest
import torch

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
LN_EPS = float(torch.tensor(1e-6, dtype=F32))


def G(shape, dtype, fill=None):
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def seeded_meta(shape, g, fmt, std=1.0):
    """The delayed-scaling state of a GEMM operand that has seen one tensor of ``shape``."""
    return no.quantize_fp8_delayed(kr.normal(shape, g, std=std), None, fmt)[2]


# --------------------------------------------------------------------- fp8 attention forward
ATTN_B, ATTN_H = 2, 2
ATTN_T = sorted({32 * k - 31 for k in range(1, 9)} | {32 * k for k in range(1, 9)} | {197})


def check_attn_fwd_q8(T):
    lib = no._load()
    B, H = ATTN_B, ATTN_H
    g = kr.gen(1000 + T)
    what = f"attn_fwd_f8_q8 T={T}"
    qkv = kr.normal((B, T, 3 * H * 64), g, std=1.5)
    meta0 = seeded_meta((B * T, H * 64), g, no.E4M3)
    out, lse = G((B, T, H * 64), BF), G((B * H, T), F32)
    assert lib.pdt_attn_fwd_f8(no._p(qkv), no._p(out), no._p(lse), B, T, H, 0.125, no._s()) == 0, what
    out8, lse8 = G((B, T, H * 64), BF), G((B * H, T), F32)
    codes, part, dq, meta = G((B * T, H * 64), U8), G(B * H, F32), G(1, F32), G(meta0.shape, F32, meta0)
    assert lib.pdt_attn_fwd_f8_q8(no._p(qkv), no._p(out8), no._p(lse8), B, T, H, 0.125, no._p(codes), no._p(meta),
                                  no._p(part), no._p(dq), no._s()) == 0, what
    done(what)
    assert torch.equal(out8, out) and torch.equal(lse8, lse), what
    q_ref, dq_ref, meta_ref = no.quantize_fp8_delayed(out.reshape(-1, H * 64), meta0.clone(), no.E4M3)
    torch.cuda.synchronize()
    assert torch.equal(codes, q_ref), what
    assert torch.equal(dq, dq_ref), what
    assert torch.equal(meta, meta_ref), what


@pytest.mark.parametrize("T", ATTN_T)
def test_attn_fwd_f8_q8_every_tile_count(T):
    check_attn_fwd_q8(T)


@pytest.mark.parametrize("T", [129, 160, 197, 256])
def test_attn_fwd_f8_q8_fp8_pv_above_128(T):
    """pdt_attn_set_pv8(1): the 4-wave kernels with the PV GEMM on e4m3, at 5..8 key tiles."""
    lib = no._load()
    lib.pdt_attn_set_pv8(1)
    try:
        check_attn_fwd_q8(T)
    finally:
        lib.pdt_attn_set_pv8(0)


# --------------------------------------------------------------------------------- LayerNorm
LN_CASES = [(D, rows) for D in (256, 512, 768, 1024) for rows in (1, 4, 5)]


def ln_fwd(lib, x, w, b, what):
    rows, D = x.shape
    y, mean, rstd = G((rows, D), BF), G(rows, F32), G(rows, F32)
    assert lib.pdt_ln_fwd(no._p(x), no._p(w), no._p(b), no._p(y), no._p(mean), no._p(rstd), rows, D, LN_EPS,
                          no._s()) == 0, what
    return y, mean, rstd


def ln_fwd_f8(lib, x, w, b, meta0, what):
    rows, D = x.shape
    y, mean, rstd = G((rows, D), BF), G(rows, F32), G(rows, F32)
    q, part = G((rows, D), U8), G(lib.pdt_ln_fwd_f8_blocks(rows), F32)
    dq, meta = G(1, F32), G(meta0.shape, F32, meta0)
    assert lib.pdt_ln_fwd_f8(no._p(x), no._p(w), no._p(b), no._p(y), no._p(mean), no._p(rstd), rows, D, LN_EPS,
                             no._p(q), no._p(meta), no._p(part), no._p(dq), no._s()) == 0, what
    return y, mean, rstd, q, dq, meta


@pytest.mark.parametrize("D,rows", LN_CASES)
def test_ln_forward_entry_points_agree(D, rows):
    lib = no._load()
    g = kr.gen(7 * D + rows)
    what = f"ln forward D={D} rows={rows}"
    x, r = kr.normal((rows, D), g, std=2.0, mean=1.0), kr.normal((rows, D), g)
    w, b = kr.normal((D,), g, F32), kr.normal((D,), g, F32)
    meta0 = seeded_meta((rows, D), g, no.E4M3)
    # pdt_ln_fwd_f8 == pdt_ln_fwd
    y, mean, rstd = ln_fwd(lib, x, w, b, what)
    y8, mean8, rstd8, _, _, _ = ln_fwd_f8(lib, x, w, b, meta0, what)
    done(what)
    assert torch.equal(y8, y) and torch.equal(mean8, mean) and torch.equal(rstd8, rstd), what
    # pdt_ln_add_fwd without codes: xsum = bf16(x + r), normalised as pdt_ln_fwd does
    xsum, ya, meana, rstda = G((rows, D), BF), G((rows, D), BF), G(rows, F32), G(rows, F32)
    assert lib.pdt_ln_add_fwd(no._p(x), no._p(r), no._p(xsum), no._p(w), no._p(b), no._p(ya), no._p(meana),
                              no._p(rstda), rows, D, LN_EPS, None, None, None, None, no._s()) == 0, what
    done(what + " add")
    assert torch.equal(xsum, (x.float() + r.float()).to(BF)), what
    ys, means, rstds = ln_fwd(lib, xsum, w, b, what)
    done(what + " of xsum")
    assert torch.equal(ya, ys) and torch.equal(meana, means) and torch.equal(rstda, rstds), what
    # pdt_ln_add_fwd with codes == pdt_ln_fwd_f8 of xsum from the same scaling state
    xsum2, yq, meanq, rstdq = G((rows, D), BF), G((rows, D), BF), G(rows, F32), G(rows, F32)
    q, part = G((rows, D), U8), G(lib.pdt_ln_fwd_f8_blocks(rows), F32)
    dq, meta = G(1, F32), G(meta0.shape, F32, meta0)
    assert lib.pdt_ln_add_fwd(no._p(x), no._p(r), no._p(xsum2), no._p(w), no._p(b), no._p(yq), no._p(meanq),
                              no._p(rstdq), rows, D, LN_EPS, no._p(q), no._p(meta), no._p(part), no._p(dq),
                              no._s()) == 0, what
    _, _, _, q_ref, dq_ref, meta_ref = ln_fwd_f8(lib, xsum, w, b, meta0, what)
    done(what + " add with codes")
    assert torch.equal(xsum2, xsum), what
    assert torch.equal(q, q_ref) and torch.equal(dq, dq_ref) and torch.equal(meta, meta_ref), what


@pytest.mark.parametrize("D,rows", LN_CASES)
def test_ln_backward_entry_points_agree(D, rows):
    lib = no._load()
    g = kr.gen(11 * D + rows)
    x, dy, addend = kr.normal((rows, D), g, std=2.0, mean=1.0), kr.normal((rows, D), g), kr.normal((rows, D), g)
    w, b = kr.normal((D,), g, F32), kr.normal((D,), g, F32)
    _, mean, rstd = ln_fwd(lib, x, w, b, "ln backward: forward statistics")
    gmeta0 = seeded_meta((rows, D), g, no.E5M2)
    blocks = lib.pdt_ln_bwd_blocks(rows)
    for add in (None, addend):
        what = f"ln backward D={D} rows={rows} addend={add is not None}"
        common = (no._p(dy), no._p(x), no._p(w), no._p(mean), no._p(rstd))

        def outs():
            return G((rows, D), BF), G(D, F32), G(D, F32), G(2 * blocks * D, F32)

        def codes():
            return G((rows, D), U8), G(gmeta0.shape, F32, gmeta0), G(blocks, F32), G(1, F32)

        dx, dg, db, part = outs()
        assert lib.pdt_ln_bwd(*common, no._p(dx), no._p(dg), no._p(db), no._p(part), rows, D, 0, no._p(add),
                              no._s()) == 0, what
        dx8, dg8, db8, part8 = outs()
        q8, gmeta, qpart, dq = codes()
        assert lib.pdt_ln_bwd_f8(*common, no._p(dx8), no._p(dg8), no._p(db8), no._p(part8), rows, D, 0, no._p(add),
                                 no._p(q8), no._p(gmeta), no._p(qpart), no._p(dq), no._s()) == 0, what
        dxb, dgb, dbb, partb = outs()
        q8b, gmetab, qpartb, dqb = codes()
        cpart = G(blocks * D + lib.pdt_reduce_rows_work(blocks, D), F32)
        bias = G(D, F32)
        assert lib.pdt_ln_bwd_f8_db(*common, no._p(dxb), no._p(dgb), no._p(dbb), no._p(partb), rows, D, 0, no._p(add),
                                    no._p(q8b), no._p(gmetab), no._p(qpartb), no._p(dqb), no._p(cpart), no._p(bias),
                                    0, no._s()) == 0, what
        done(what)
        assert torch.equal(dx8, dx) and torch.equal(dg8, dg) and torch.equal(db8, db), what + " (f8)"
        assert torch.equal(dxb, dx) and torch.equal(dgb, dg) and torch.equal(dbb, db), what + " (f8_db)"
        # the bias gradient: column sums of dx as stored; the allowance of the bias gradients in
        # tests/test_vit_fusion_gpu.py::test_ln_backward_bias_grads_match_wgrad_bias
        ref = kr.f64(dx).sum(0)
        err = ((kr.f64(bias) - ref).norm() / ref.norm().clamp_min(1e-6)).item()
        assert err < 1e-3, (what, err)
