"""csrc/fp8.hip called entry point by entry point (amax reduction, current- and delayed-scaled
casts, the transposing weight cast, the GELU casts, the history rolls) against the bit-exact
mirror in tests/kernel_ref.py.

A cast is one correctly rounded fp32 divide (scale = FMAX / amax), one fp32 multiply, a clamp and
one round to nearest even, so codes, dq, amax partials and the 21-word scaling state are compared
with equality: zero mismatches. Only the two GELU entry points carry a transcendental (exp2 + rcp);
what follows it is still exact (the codes are those of the bf16 gelu the kernel wrote), and the
transcendental itself gets the measured allowance of test_row_kernels_gpu.py: 4 x the error of
PyTorch's own fp32 op against float64, floored at one fp32 roundoff, printed on a MEASURED line.
Every output is guard-banded.

NaN inputs (pinned by test_cast_delayed_nan_inputs): a NaN gets the -FMAX code, because the clamp
is fminf(fmaxf(NaN, -FMAX), FMAX), and is left out of the amax, because fmaxf drops it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
FMTS = [0, 1]


def G(shape, dtype, fill=None):
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def dev(x32, bf16=0):
    """numpy float32 -> device tensor (bf16: the values are bf16 numbers already)."""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DEV)
    return t.to(BF) if bf16 else t


def G_meta(words):
    """Guarded 21-word state from uint32 words (None: poison) -> (fp32 view for the kernels)."""
    fill = None if words is None else torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy())
    return G(kr.FP8_META_WORDS, I32, fill).view(F32)


def hand_meta(fmt, scale, idx=5, slot_amax=0.0):
    """A hand-built state: the given scale, a junk dq, history 0.5, 0.25, 0.5, ... and the index."""
    m = kr.fp8_meta_ref(fmt)
    m.scale, m.dq, m.amax, m.idx = np.float32(scale), np.float32(123.0), np.float32(slot_amax), idx
    m.hist = [np.float32(0.5 if i % 2 == 0 else 0.25) for i in range(kr.FP8_HIST)]
    return m


def allowance(e_ref, ref64):
    return 4 * max(e_ref, kr.U * ref64.abs().max().item())


# ------------------------------------------------------------- pdt_amax_partial + pdt_cast_fp8
N_CASES = [1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 5, 1024 * 2048, 1024 * 2048 + 2048 + 3]


def _cast_base(n, bf16, fmt):
    """(inputs, their codes at the scale FMAX / 17.25): computed once for all positions of the amax."""
    x = kr.fp8_cast_inputs(n, bf16, n % 1000 + bf16, fmt)
    return x, kr.fp8_cast_ref(x, kr.fp8_scale(kr.FP8_PLANT, fmt), fmt)


def run_cast(lib, x32, bf16, fmt, what):
    n = x32.size
    nb = lib.pdt_amax_blocks(n)
    assert nb == min(1024, max(1, -(-n // 2048))), what
    x = dev(x32, bf16)
    partial, q, dq = G(nb, F32), G(n, U8), G(1, F32)
    assert lib.pdt_amax_partial(no._p(x), bf16, n, no._p(partial), no._s()) == 0, what
    assert lib.pdt_cast_fp8(no._p(x), bf16, n, no._p(partial), fmt, no._p(q), no._p(dq), no._s()) == 0, what
    done(what)
    return partial, q, dq


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("bf16", [1, 0])
@pytest.mark.parametrize("n", N_CASES)
def test_amax_partial_and_cast(n, bf16, fmt):
    """n = 1024 * 2048 is the first n with 1024 partials (block_amax's 4-way loop); the last n
    reaches the grid-stride second trip and a scalar tail on it. The amax is planted at index 0,
    at n - 1 (in the scalar tail where n % 8 != 0), at the start of the last block and on the
    second trip; the fp32 inputs hold values an ulp either side of a tie (kr.fp8_cast_inputs)."""
    lib = no._load()
    base, base_codes = _cast_base(n, bf16, fmt)
    nb = lib.pdt_amax_blocks(n)
    s = kr.fp8_scale(kr.FP8_PLANT, fmt)
    spots = {0, n - 1, (nb - 1) * 2048}
    if n > nb * 2048:
        spots |= {nb * 2048, nb * 2048 + 2047}
    for k, pos in enumerate(sorted(spots)):
        what = f"cast n={n} bf16={bf16} fmt={fmt} amax at {pos}"
        x32 = base.copy()
        x32[pos] = kr.FP8_PLANT if k % 2 else -kr.FP8_PLANT
        partial, q, dq = run_cast(lib, x32, bf16, fmt, what)
        assert kr.fp8_amax(x32) == np.float32(kr.FP8_PLANT)
        kr.assert_same_bits(partial, kr.fp8_amax_partials(x32, nb), what + " partial")
        kr.assert_same_bits(dq, np.array([kr.fp8_dq(s)], dtype=np.float32), what + " dq")
        ref = base_codes.copy()
        ref[pos] = kr.fp8_cast_ref(x32[pos:pos + 1], s, fmt)[0]
        assert ref[pos] == (0x00 if k % 2 else 0x80) | kr.FP8_MAX_CODE[fmt]
        kr.assert_same_bits(q, ref, what + " codes")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("bf16", [1, 0])
def test_cast_all_zero_and_single_negative(bf16, fmt):
    lib = no._load()
    n = 2049
    partial, q, dq = run_cast(lib, np.zeros(n, dtype=np.float32), bf16, fmt, "all zero")
    assert bool((partial == 0).all()) and dq.item() == 1.0 and bool((q == 0).all())
    x32 = np.zeros(n, dtype=np.float32)
    x32[1030] = -3.0
    partial, q, dq = run_cast(lib, x32, bf16, fmt, "one negative value")
    s = kr.fp8_scale(3.0, fmt)
    kr.assert_same_bits(partial, np.float32([3.0, 0.0]), "one negative value: partial")
    kr.assert_same_bits(dq, np.array([kr.fp8_dq(s)], dtype=np.float32), "one negative value: dq")
    kr.assert_same_bits(q, kr.fp8_cast_ref(x32, s, fmt), "one negative value: codes")
    assert q[1030].item() == 0x80 | kr.FP8_MAX_CODE[fmt] and int((q != 0).sum()) == 1


# ----------------------------------------------------- pdt_cast_fp8_delayed: rounding, exhaustively
def run_delayed(lib, x, bf16, model, fmt, what, x32=None):
    """One delayed cast from the model's state: codes, the whole state and dq_out must equal the
    mirror's. ``x32``: the values as numpy float32 (default: read back from x)."""
    n = x.numel()
    meta, q, dq = G_meta(model.words()), G(n, U8), G(1, F32)
    assert lib.pdt_cast_fp8_delayed(no._p(x), bf16, n, no._p(meta), fmt, no._p(q), no._p(dq), no._s()) == 0, what
    done(what)
    x32 = kr._np32(x) if x32 is None else x32
    used, dq_ref = model.roll(kr.fp8_amax(x32))
    kr.assert_same_bits(q, kr.fp8_cast_ref(x32, used, fmt), what + " codes")
    kr.assert_same_bits(kr.meta_words(meta), model.words(), what + " meta")
    kr.assert_same_bits(dq, np.array([dq_ref], dtype=np.float32), what + " dq_out")
    return meta, q


SCALES = [1.0, 2.0 ** -3, 2.0 ** 5, 448.0 / 17, 57344.0 / 3]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scale", SCALES)
def test_cast_delayed_every_bf16_pattern_and_every_tie(scale, fmt):
    """All 65 282 bf16 patterns that are no NaN (+-inf, both zeros, subnormals), the same as fp32
    and fp32 values one ulp either side of every code midpoint, under a hand-set (stale) scale:
    ties, subnormal codes, saturation, -0, inf -> FMAX. The amax is inf there: the history slot
    holds it, the next scale is FMAX / inf = 0, and meta[1] = dq_out = 1 / the old scale."""
    lib = no._load()
    pat, x32 = kr.fp8_exhaustive_inputs(fmt, scale)
    for bf16, x in ((1, pat.to(DEV).view(BF)), (0, dev(x32))):
        what = f"delayed exhaustive fmt={fmt} scale={scale} bf16={bf16}"
        model = hand_meta(fmt, scale)
        meta, q = run_delayed(lib, x, bf16, model, fmt, what)
        w = kr.meta_words(meta)
        assert w[2] == 0 and w[4] == 6, what
        assert w.view(np.float32)[5 + 5] == np.inf and w.view(np.float32)[0] == 0, what
        assert w.view(np.float32)[1] == np.float32(1) / np.float32(scale), what
        # spot checks that do not go through the mirror: -0 and the infinities
        vals = kr._np32(x)
        codes = q.cpu().numpy()
        top = kr.FP8_MAX_CODE[fmt]
        assert (codes[np.isposinf(vals)] == top).all() and (codes[np.isneginf(vals)] == 0x80 | top).all(), what
        zero = vals == 0
        assert (codes[zero] == np.where(np.signbit(vals[zero]), 0x80, 0)).all(), what


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("bf16", [1, 0])
def test_cast_delayed_nan_inputs(bf16, fmt):
    """Quiet and signalling NaNs of either sign, in a vector chunk and in the scalar tail: each gets
    the -FMAX code (fminf(fmaxf(NaN, -FMAX), FMAX)) and none reaches the amax (fmaxf drops it)."""
    lib = no._load()
    n = 2049 + 4
    x32 = kr.fp8_cast_inputs(n, bf16, 3, fmt).copy()
    bits = x32.view(np.uint32)
    where = [3, 4, 1029, n - 1]
    for i, b in zip(where, (0x7FC00000, 0xFFC00000, 0x7F810000, 0xFF810000)):
        bits[i] = b
    x = torch.from_numpy(x32.view(np.int32).copy()).to(DEV).view(F32)
    if bf16:  # the same NaN patterns as bf16 (a float conversion would quiet them)
        x = (x.view(I32) >> 16).to(torch.int16).view(BF)
    assert bool(torch.isnan(x.float()).sum() == 4)
    model = hand_meta(fmt, 7.0)
    meta, q = run_delayed(lib, x, bf16, model, fmt, f"NaN inputs bf16={bf16} fmt={fmt}", x32=x32)
    assert q[where].tolist() == [0x80 | kr.FP8_MAX_CODE[fmt]] * 4
    amax = meta[5 + 5].item()
    assert amax == np.abs(x32[~np.isnan(x32)]).max() and math.isfinite(amax)


# ------------------------------------------------------------------------------ state machine
@pytest.mark.parametrize("fmt", FMTS)
def test_delayed_scaling_state_machine(fmt):
    """pdt_fp8_meta_seed, then 40 delayed casts of n = 2049 whose amaxes follow kr.fp8_script (a
    spike at step 2, a zero tensor at step 9): after every step the 21 words, dq_out and the codes
    equal the mirror. The spike rules the scale for exactly 16 steps; the index ends at 41."""
    lib = no._load()
    n = 2049
    seed_amax, steps = kr.fp8_script()
    base = kr.fp8_cast_inputs(n, 1, 5).copy() / 16  # |base| < 1
    base[n - 1] = -1.0

    def tensor(a):
        x = (dev(base) * a).to(BF)
        assert x.float().abs().max().item() == a
        return x

    x0 = tensor(seed_amax)
    nb = lib.pdt_amax_blocks(n)
    partial, meta = G(nb, F32), G_meta(None)
    assert lib.pdt_amax_partial(no._p(x0), 1, n, no._p(partial), no._s()) == 0
    assert lib.pdt_fp8_meta_seed(no._p(partial), n, fmt, no._p(meta), no._s()) == 0
    done("seed")
    model = kr.fp8_meta_ref(fmt)
    model.seed(seed_amax)
    kr.assert_same_bits(kr.meta_words(meta), model.words(), "seed")
    fmax = np.float32(kr.FP8_FMAX[fmt])
    q, dq = G(n, U8), G(1, F32)
    for k, a in enumerate(steps):
        what = f"state machine fmt={fmt} step {k}"
        x = tensor(a)
        assert lib.pdt_cast_fp8_delayed(no._p(x), 1, n, no._p(meta), fmt, no._p(q), no._p(dq), no._s()) == 0, what
        torch.cuda.synchronize()
        used, dq_ref = model.roll(a)
        w = kr.meta_words(meta)
        kr.assert_same_bits(w, model.words(), what + " meta")
        kr.assert_same_bits(dq, np.array([dq_ref], dtype=np.float32), what + " dq_out")
        kr.assert_same_bits(q, kr.fp8_cast_ref(x, used, fmt), what + " codes")
        scale = w.view(np.float32)[0]
        if 2 <= k <= 17:
            assert scale == fmax / np.float32(64), what
        elif k == 18:
            assert scale == fmax / np.float32(max(steps[3:19])), what
    done("state machine")
    assert kr.meta_words(meta)[4] == 41


# ------------------------------------------------------------------ pdt_fp8_meta_roll_partial
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nblk", [1, 255, 256, 1024, 1025, 4097])
def test_meta_roll_partial(nblk, fmt):
    """Above 1024 partials the block has 1024 threads, up to there 256 (the 4-way loop from 1024)."""
    lib = no._load()
    g = kr.gen(nblk)
    base = torch.rand(nblk, generator=g, device=DEV) * 2 + 0.125
    for pos in sorted({0, nblk // 2, nblk - 1}):
        for slot in (0.0, 1.5, 9.0):  # nothing recorded, below the largest partial, above it
            what = f"roll_partial nblk={nblk} fmt={fmt} max at {pos} slot={slot}"
            partial = base.clone()
            partial[pos] = 5.0
            model = hand_meta(fmt, 3.0, idx=31, slot_amax=slot)
            meta, dq = G_meta(model.words()), G(1, F32)
            assert lib.pdt_fp8_meta_roll_partial(no._p(meta), no._p(partial), nblk, fmt, no._p(dq), no._s()) == 0, what
            done(what)
            _, dq_ref = model.roll_partial(kr._np32(partial))
            assert model.hist[15] == max(5.0, slot) and model.idx == 32
            kr.assert_same_bits(kr.meta_words(meta), model.words(), what + " meta")
            kr.assert_same_bits(dq, np.array([dq_ref], dtype=np.float32), what + " dq_out")


# -------------------------------------------------------------------------- pdt_cast_fp8_dual
@pytest.mark.parametrize("R,C", [(1, 1), (3, 5), (4, 4), (64, 64), (65, 63), (63, 65), (130, 67), (66, 256)])
def test_cast_dual_transposed(R, C):
    lib = no._load()
    what = f"cast_dual R={R} C={C}"
    x32 = kr.fp8_cast_inputs(R * C, 0, R + C).copy()
    x32[(R * C) // 2] = -kr.FP8_PLANT
    x = dev(x32)
    nb = lib.pdt_amax_blocks(R * C)
    partial, q, qt, dq = G(nb, F32), G((R, C), U8), G((C, R), U8), G(1, F32)
    assert lib.pdt_amax_partial(no._p(x), 0, R * C, no._p(partial), no._s()) == 0, what
    assert lib.pdt_cast_fp8_dual(no._p(x), R, C, no._p(partial), no._p(q), no._p(qt), no._p(dq), no._s()) == 0, what
    done(what)
    s = kr.fp8_scale(kr.FP8_PLANT, 0)
    ref = kr.fp8_cast_ref(x32, s, 0).reshape(R, C)
    kr.assert_same_bits(q, ref, what + " q")
    kr.assert_same_bits(qt, np.ascontiguousarray(ref.T), what + " qt")
    kr.assert_same_bits(dq, np.array([kr.fp8_dq(s)], dtype=np.float32), what + " dq")


# --------------------------------------------------------------------- pdt_gelu_dual_cast_fp8
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [8, 2048, 2056, 1024 * 2048 + 8])
def test_gelu_dual_cast(n, fmt):
    """The kernel re-reads gelu(y) from its own packed bf16 before the cast: the codes equal
    fp8_cast_ref(a_out, s) and the recorded amax equals max |a_out|, exactly, whether aux and a_out
    are written, left out, or a_out is y itself. a_out and aux against float64: one rounding plus
    4 x the error of F.gelu(approximate="tanh") / its autograd in fp32."""
    lib = no._load()
    g = kr.gen(n + fmt)
    z = kr.normal((n,), g, std=3.0)
    z[:7] = torch.tensor([0.0, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0], device=DEV).to(BF)
    ref_g, ref_d = kr.gelu_tanh_ref(z), kr.gelu_tanh_grad_ref(z)
    zz = z.float().requires_grad_()
    g32 = F.gelu(zz, approximate="tanh")
    g32.sum().backward()
    e_g, e_d = (g32.detach().double() - ref_g).abs().max().item(), (zz.grad.double() - ref_d).abs().max().item()
    a_g, a_d = allowance(e_g, ref_g), allowance(e_d, ref_d)
    scale = kr.fp8_scale(3.0, fmt)  # gelu reaches 10: the top saturates
    a_first = ref_codes = amax = None
    for with_aux, a_mode in [(1, "given"), (0, "given"), (1, "none"), (0, "none"), (1, "alias"), (0, "alias")]:
        what = f"gelu_dual_cast n={n} fmt={fmt} aux={with_aux} a_out={a_mode}"
        model = hand_meta(fmt, scale)
        y = G(n, BF, z)
        meta, q, dq = G_meta(model.words()), G(n, U8), G(1, F32)
        aux = G(n, BF) if with_aux else None
        a_out = {"given": G(n, BF), "none": None, "alias": y}[a_mode]
        assert lib.pdt_gelu_dual_cast_fp8(no._p(y), n, no._p(meta), fmt, no._p(q), no._p(aux), no._p(a_out),
                                          no._p(dq), no._s()) == 0, what
        done(what)
        if a_first is None:
            a_first = a_out.clone()
            ref_codes, amax = kr.fp8_cast_ref(a_first, scale, fmt), kr.fp8_amax(a_first)
            k_g = ((kr.f64(a_out) - ref_g).abs() - kr.BF16_HALF * ref_g.abs()).clamp_min(0).max().item()
            k_d = ((kr.f64(aux) - ref_d).abs() - kr.BF16_HALF * ref_d.abs()).clamp_min(0).max().item()
            print(f"MEASURED gelu_dual_cast n={n} fmt={fmt}: gelu reference op max err {e_g:.3e} (allowance "
                  f"{a_g:.3e}), kernel beyond the bf16 half-ulp {k_g:.3e}; gelu' reference op {e_d:.3e} "
                  f"(allowance {a_d:.3e}), kernel {k_d:.3e}")
        if a_out is not None:
            kr.assert_same_bits(a_out, a_first, what + " a_out is the same in every mode")
            kr.assert_bf16_close(a_out, ref_g, ref_g.abs(), what + " a_out", roundings=1, extra=a_g)
        if a_mode != "alias":
            assert torch.equal(y, z), what + " y"
        if aux is not None:
            kr.assert_bf16_close(aux, ref_d, ref_d.abs(), what + " aux", roundings=1, extra=a_d)
        used, dq_ref = model.roll(amax)
        assert used == scale
        kr.assert_same_bits(q, ref_codes, what + " codes")
        kr.assert_same_bits(kr.meta_words(meta), model.words(), what + " meta")
        kr.assert_same_bits(dq, np.array([dq_ref], dtype=np.float32), what + " dq_out")
    model = hand_meta(fmt, scale)
    meta, q = G_meta(model.words()), G(16, U8)
    assert lib.pdt_gelu_dual_cast_fp8(no._p(z), 12, no._p(meta), fmt, no._p(q), None, None, None, no._s()) == -1
    done("n = 12")
    kr.assert_same_bits(kr.meta_words(meta), model.words(), "refused: meta untouched")
    assert bool((q == kr.POISON_BYTE).all())


# ------------------------------------- pdt_cast_fp8_delayed_cs and pdt_cast_fp8_gelu_grad_cs
CS_CASES = [(1, 8), (3, 8), (5, 16), (63, 768), (65, 768), (129, 1032),
            (70, 8200),   # c8n = 1025 > 1024: one row group, two column trips
            (33, 2048),   # 4 row groups, fewer than 4 * RG rows in the band
            (4100, 64)]   # 65 bands


def cs_buffers(lib, rows, cols):
    nb = lib.pdt_cast_cs_bands(rows)
    assert nb == -(-rows // 64)
    return nb, G(nb * cols + lib.pdt_reduce_rows_work(nb, cols), F32), G(cols, F32), G((rows, cols), U8), G(1, F32)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rows,cols", CS_CASES)
def test_cast_delayed_cs(rows, cols, fmt):
    """Integer data in [-8, 8] at the scale FMAX / 5 (the top saturates): codes and state equal the
    mirror, and the column sums are exact in any order."""
    lib = no._load()
    what = f"cast_delayed_cs rows={rows} cols={cols} fmt={fmt}"
    x = kr.ints((rows, cols), kr.gen(rows + cols))
    x[rows // 2, cols - 1] = -8
    model = hand_meta(fmt, kr.fp8_scale(5.0, fmt))
    nb, cpart, bias, q, dq = cs_buffers(lib, rows, cols)
    meta = G_meta(model.words())
    assert lib.pdt_cast_fp8_delayed_cs(no._p(x), rows, cols, no._p(meta), fmt, no._p(q), no._p(dq), no._p(cpart),
                                       no._p(bias), no._s()) == 0, what
    done(what)
    used, dq_ref = model.roll(8.0)
    kr.assert_same_bits(q, kr.fp8_cast_ref(x, used, fmt).reshape(rows, cols), what + " codes")
    kr.assert_same_bits(kr.meta_words(meta), model.words(), what + " meta")
    kr.assert_same_bits(dq, np.array([dq_ref], dtype=np.float32), what + " dq_out")
    kr.assert_exact(bias, kr.colsum_ref(x)[0], what + " bias_out")


@pytest.mark.parametrize("gelu", [0, 1])
def test_cast_cs_refusals(gelu):
    lib = no._load()
    x = torch.ones(8, 16, dtype=BF, device=DEV)
    for rows, cols in ((4, 12), (0, 8)):
        model = hand_meta(1, 2.0)
        meta, q, dq = G_meta(model.words()), G(64, U8), G(1, F32, 1.0)
        cpart, bias = G(256, F32, 1.0), G(16, F32, 1.0)
        if gelu:
            rc = lib.pdt_cast_fp8_gelu_grad_cs(no._p(x), no._p(x), rows, cols, no._p(meta), 1, no._p(q), no._p(dq),
                                               no._p(cpart), no._p(bias), no._s())
        else:
            rc = lib.pdt_cast_fp8_delayed_cs(no._p(x), rows, cols, no._p(meta), 1, no._p(q), no._p(dq), no._p(cpart),
                                             no._p(bias), no._s())
        assert rc == -1, (rows, cols)
        done("refused")
        kr.assert_same_bits(kr.meta_words(meta), model.words(), "refused: meta untouched")
        assert bool((q == kr.POISON_BYTE).all()) and bool((bias == 1).all()) and bool((cpart == 1).all())
        assert dq.item() == 1.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rows,cols", CS_CASES)
def test_cast_gelu_grad_cs(rows, cols, fmt):
    """Codes of x * gelu'(z), z ~ N(0, 2^2) and integer x. The kernel's fp32 gelu' is not observable,
    so (kr.fp8_boundary_check) a code may differ from fp8_cast_ref(float32(x * gelu'_64(z)), s) only
    by one step and only where the float64 product times s lies within allowance * |x| * s of a
    rounding boundary; the allowance is 4 x the error of the autograd of F.gelu(approximate="tanh")
    in fp32. s is kr.fp8_boundary_scale: the largest at which that window stays below half the
    smallest step. The number of differing codes is printed."""
    lib = no._load()
    what = f"cast_gelu_grad_cs rows={rows} cols={cols} fmt={fmt}"
    g = kr.gen(7 * rows + cols + fmt)
    z = kr.normal((rows, cols), g, std=2.0)
    x = kr.ints((rows, cols), g)
    d64 = kr.gelu_tanh_grad_ref(z)
    zz = z.float().requires_grad_()
    F.gelu(zz, approximate="tanh").sum().backward()
    e_ref = (zz.grad.double() - d64).abs().max().item()
    allow = allowance(e_ref, d64)
    s = kr.fp8_boundary_scale(allow, 8, fmt)
    # the history already holds 100 > max |x gelu'|: the next scale is known whatever the fp32 amax
    model = hand_meta(fmt, s)
    model.hist[0] = np.float32(100.0)
    nb, cpart, bias, q, dq = cs_buffers(lib, rows, cols)
    meta = G_meta(model.words())
    assert lib.pdt_cast_fp8_gelu_grad_cs(no._p(x), no._p(z), rows, cols, no._p(meta), fmt, no._p(q), no._p(dq),
                                         no._p(cpart), no._p(bias), no._s()) == 0, what
    done(what)
    p64 = kr.f64(x) * d64
    ndiff = kr.fp8_boundary_check(q, p64.cpu().numpy(), kr.f64(x).abs().cpu().numpy(), s, allow, fmt, what)
    print(f"MEASURED {what}: gelu' reference op max err {e_ref:.3e}, allowance {allow:.3e}, scale {float(s)!r}: "
          f"{ndiff} of {rows * cols} codes differ from the float64 product's, each by one step at a boundary")
    # the state: everything but the recorded amax is exact. The amax is max |fl(x gelu')| over the very
    # values that were cast, and rounding is monotone: amax * s must round to the largest code written
    # (the plain kernel, the same code without the gelu' factor, has its amax checked exactly above)
    _, dq_ref = model.roll(np.float32(p64.abs().max().item()))
    w, wr = kr.meta_words(meta), model.words()
    slot = 5 + 5
    keep = np.arange(kr.FP8_META_WORDS) != slot
    kr.assert_same_bits(w[keep], wr[keep], what + " meta")
    assert kr.fp8_cast_ref(w.view(np.float32)[slot:slot + 1], s, fmt)[0] == int((q & 0x7F).max()), what + " amax"
    kr.assert_same_bits(dq, np.array([dq_ref], dtype=np.float32), what + " dq_out")
    # column sums: the product (1 rounding), at most 2 * 64 rows of a band in a thread, 8 row groups,
    # the bands; gelu' off by the allowance moves a sum by at most allowance * sum |x|
    L = min(rows, 128) + 8 + nb + 1
    kr.assert_f32_close(bias, p64.sum(0), p64.abs().sum(0), what + " bias_out", roundings=L,
                        extra=allow * kr.f64(x).abs().sum(0))
