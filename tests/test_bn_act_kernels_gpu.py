"""csrc/bn_act.hip against float64 references (tests/kernel_ref.py), called directly: finalize
and backward finalize from hand-made partial sums (both rows_reduce geometries, the c < C tails),
the apply passes in every (residual, relu, mask) form, the backward reduction with its four
gates and the backward apply / dual apply -- at the smallest shapes that reach each path.

Every output (workspaces included) is guard-banded and NaN-poisoned; bounds are derived in
kernel_ref's docstring. Exact-family inputs must reproduce the reference exactly."""
import math

import pytest
import torch

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
ULP2 = 2 * 2.0 ** -23  # "within 2 ulp of fp32", relative
EPS = float(torch.tensor(1e-5, dtype=F32))  # the eps the kernel sees (a float argument)


def G(shape, dtype, fill=None):
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def stage1_err(p64, R, C):
    """fp32 error of rows_reduce_kernel's output sums (zero for R <= 256, where the finalize sums
    the rows in fp64): each thread adds ceil(R / 4G) rows, then 3 LDS adds."""
    if R <= 256:
        return torch.zeros(2, C, dtype=kr.F64, device=p64.device)
    Gr = 128 if (R > 2048 and C <= 256) else 64
    return 2 * (math.ceil(R / (4 * Gr)) + 3) * kr.U * p64.abs().sum(1)


def part_buffer(lib, part, R, C):
    """the [2][R][C] partials followed by the (guarded, poisoned) stage-1 workspace"""
    ws = lib.pdt_rows_reduce_workspace(R, C)
    assert ws == (0 if R <= 256 else 2 * (128 if (R > 2048 and C <= 256) else 64) * C)
    buf = G(2 * R * C + ws, F32)
    buf[:2 * R * C].copy_(part.reshape(-1))
    return buf


RS, CS = [1, 3, 256, 257, 2049], [8, 24, 64, 72, 512]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("R", RS)
def test_bn_finalize(R, C):
    lib = no._load()
    g = kr.gen(1000 * R + C)
    for family, affine, running in [("exact", True, True), ("exact", False, False), ("normal", True, True),
                                    ("normal", False, True)]:
        what = f"finalize R={R} C={C} {family} affine={affine} running={running}"
        if family == "exact":
            part = kr.exact_partials(R, C, g)
        else:
            part = torch.stack([kr.normal((R, C), g, F32, 4.0), kr.normal((R, C), g, F32, 4.0).abs() + 8])
        count, mom = 16.0 * R, 0.125
        gamma = (torch.rand(C, generator=g, device=DEV) + 0.5) if affine else None
        beta = kr.normal((C,), g, F32) if affine else None
        rm0, rv0 = kr.normal((C,), g, F32), torch.rand(C, generator=g, device=DEV) + 0.5
        buf = part_buffer(lib, part, R, C)
        mean, invstd, scale, shift = (G(C, F32) for _ in range(4))
        rm, rv = (G(C, F32, rm0), G(C, F32, rv0)) if running else (None, None)
        nbt = G(1, torch.int64, 7) if running else None
        rc = lib.pdt_bn_finalize(no._p(buf), R, C, count, EPS, mom, no._p(gamma), no._p(beta), no._p(mean),
                                 no._p(invstd), no._p(scale), no._p(shift), no._p(rm), no._p(rv), no._p(nbt), no._s())
        assert rc == 0, what
        done(what)
        p64 = kr.f64(part)
        ref = kr.bn_finalize_ref(p64, count, EPS, mom, gamma, beta, rm0 if running else None,
                                 rv0 if running else None, 7 if running else None)
        ds, dq = stage1_err(p64, R, C) / count
        dmean = ds
        dvar = dq + 2 * ref["mean"].abs() * ds
        drel = 0.5 * dvar / (ref["var"] + EPS)  # relative error of invstd from the variance's
        if family == "exact":  # the sums are exact whatever the stage-1 length
            assert torch.equal(mean, ref["mean"].float()), what
            drel = drel * 0
            dmean = dmean * 0
        else:
            kr.assert_close(mean, ref["mean"], dmean + kr.U * ref["mean"].abs(), what + " mean")
        kr.assert_close(invstd, ref["invstd"], ref["invstd"] * (drel + ULP2), what + " invstd")
        kr.assert_close(scale, ref["scale"], ref["scale"].abs() * (drel + ULP2), what + " scale")
        kr.assert_close(shift, ref["shift"], ref["shift_abs"] * (drel + ULP2) + dmean * ref["scale"].abs(),
                        what + " shift")
        if running:
            unb = count / (count - 1)
            kr.assert_close(rm, ref["running_mean"], ref["running_mean_abs"] * ULP2 + mom * dmean, what + " rm")
            kr.assert_close(rv, ref["running_var"], ref["running_var_abs"] * ULP2 + mom * unb * dvar * (family != "exact"),
                            what + " rv")
            assert nbt.item() == ref["nbt"] == 8, what


def test_bn_finalize_count_one():
    """count = 1: the variance is 0 (clamped), invstd = 1/sqrt(eps), and the running variance takes
    the biased value (no division by count - 1 = 0)."""
    lib = no._load()
    C = 24
    g = kr.gen(5)
    s = kr.ints((1, C), g, dtype=F32)
    part = torch.stack([s, s * s])
    buf = part_buffer(lib, part, 1, C)
    mean, invstd, scale, shift = (G(C, F32) for _ in range(4))
    rv0 = torch.rand(C, generator=g, device=DEV) + 0.5
    rm, rv, nbt = G(C, F32, 0.0), G(C, F32, rv0), G(1, torch.int64, 0)
    assert lib.pdt_bn_finalize(no._p(buf), 1, C, 1.0, EPS, 0.5, None, None, no._p(mean), no._p(invstd), no._p(scale),
                               no._p(shift), no._p(rm), no._p(rv), no._p(nbt), no._s()) == 0
    done("count=1")
    ref = kr.bn_finalize_ref(kr.f64(part), 1.0, EPS, 0.5, None, None, torch.zeros(C, device=DEV), rv0, 0)
    assert torch.equal(mean, s[0]) and float(ref["var"].abs().max()) == 0
    kr.assert_close(invstd, ref["invstd"], ref["invstd"] * ULP2, "invstd")
    kr.assert_close(shift, ref["shift"], ref["shift_abs"] * ULP2, "shift")
    kr.assert_close(rm, ref["running_mean"], ref["running_mean_abs"] * ULP2, "rm")
    kr.assert_close(rv, ref["running_var"], ref["running_var_abs"] * ULP2, "rv")
    assert torch.isfinite(rv).all() and nbt.item() == 1


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("R", RS)
def test_bn_bwd_finalize(R, C):
    lib = no._load()
    g = kr.gen(2000 * R + C)
    for family, affine, acc in [("exact", True, 0), ("exact", False, 1), ("normal", True, 1), ("normal", False, 0)]:
        what = f"bwd_finalize R={R} C={C} {family} affine={affine} acc={acc}"
        exact = family == "exact"
        if exact:
            part = torch.stack([kr.ints((R, C), g, dtype=F32), kr.ints((R, C), g, dtype=F32)])
            gamma = kr.pow2((C,), g) if affine else None
            invstd = kr.pow2((C,), g).abs()
            mean = kr.ints((C,), g, -2, 2, dtype=F32)
        else:
            part = torch.stack([kr.normal((R, C), g, F32, 4.0), kr.normal((R, C), g, F32, 4.0)])
            gamma = kr.normal((C,), g, F32) if affine else None
            invstd = torch.rand(C, generator=g, device=DEV) + 0.5
            mean = kr.normal((C,), g, F32)
        count = 16.0 * R
        dg0, db0 = kr.ints((C,), g, dtype=F32), kr.ints((C,), g, dtype=F32)
        buf = part_buffer(lib, part, R, C)
        dgm, dbt = G(C, F32, dg0 if acc else None), G(C, F32, db0 if acc else None)
        k1, k2, k3 = (G(C, F32) for _ in range(3))
        rc = lib.pdt_bn_bwd_finalize(no._p(buf), R, C, count, no._p(gamma), no._p(mean), no._p(invstd), no._p(dgm),
                                     no._p(dbt), no._p(k1), no._p(k2), no._p(k3), acc, no._s())
        assert rc == 0, what
        done(what)
        p64 = kr.f64(part)
        ref = kr.bn_bwd_finalize_ref(p64[0].sum(0), p64[1].sum(0), count, gamma, mean, invstd)
        rdg = ref["dgamma"] + (kr.f64(dg0) if acc else 0)
        rdb = ref["dbeta"] + (kr.f64(db0) if acc else 0)
        if exact:
            kr.assert_exact(dgm, rdg, what + " dgamma")
            kr.assert_exact(dbt, rdb, what + " dbeta")
            kr.assert_exact(k1, ref["k1"], what + " k1")
            ds = dq = torch.zeros(C, dtype=kr.F64, device=DEV)
        else:
            ds, dq = stage1_err(p64, R, C)
        ga = torch.ones(C, dtype=kr.F64, device=DEV) if gamma is None else kr.f64(gamma).abs()
        ist = kr.f64(invstd)
        dk2 = ga * ist ** 3 * dq / count
        kr.assert_close(dgm, rdg, dq * ist + ULP2 * (ref["dgamma"].abs() + rdg.abs()), what + " dgamma")
        kr.assert_close(dbt, rdb, ds + ULP2 * (ref["dbeta"].abs() + rdb.abs()), what + " dbeta")
        kr.assert_close(k1, ref["k1"], ULP2 * ref["k1"].abs(), what + " k1")
        kr.assert_close(k2, ref["k2"], dk2 + ULP2 * ref["k2"].abs(), what + " k2")
        kr.assert_close(k3, ref["k3"], ga * ist * ds / count + dk2 * kr.f64(mean).abs() + ULP2 * ref["k3"].abs()
                        + 2.0 ** -50 * ref["k3_abs"], what + " k3")


# ----------------------------------------------------------------------------------- apply
MC = [(1, 8), (37, 24), (301, 72), (513, 2048), (131075, 64)]  # the last: 4096*256 + 24 chunks


def apply_inputs(M, C, g):
    y, res = kr.normal((M, C), g), kr.normal((M, C), g)
    y.view(-1)[::7] = 0.0  # exact zeros
    sc, sh = torch.rand(C, generator=g, device=DEV) + 0.5, kr.normal((C,), g, F32, 0.5)
    sc[1::3] *= -1
    sc[0], sh[0] = 0.0, -0.0  # channel 0: y*0 + (-0.0) is -0.0 for y <= -0, +0.0 otherwise
    rsc, rsh = torch.rand(C, generator=g, device=DEV) + 0.5, kr.normal((C,), g, F32, 0.5)
    return y, res, sc, sh, rsc, rsh


@pytest.mark.parametrize("M,C", MC)
def test_bn_apply(M, C):
    lib = no._load()
    y, res, sc, sh, rsc, rsh = apply_inputs(M, C, kr.gen(M + C))
    forms = [(r, relu, mask, False) for r, relu, mask in
             [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1)]]
    forms += [(1, 0, 0, True), (1, 1, 0, True), (1, 1, 1, True)]
    for use_res, relu, use_mask, raff in forms:
        what = f"apply M={M} C={C} res={use_res} relu={relu} mask={use_mask} affine_res={raff}"
        out = G((M, C), BF)
        mask = G(M * C // 8, torch.uint8) if use_mask else None
        if raff:
            rc = lib.pdt_bn_apply_res_affine(no._p(y), no._p(res), no._p(out), no._p(sc), no._p(sh), no._p(rsc),
                                             no._p(rsh), M, C, relu, no._p(mask), no._s())
        else:
            rc = lib.pdt_bn_apply(no._p(y), no._p(res) if use_res else None, no._p(out), no._p(sc), no._p(sh), M, C,
                                  relu, no._p(mask), no._s())
        assert rc == 0, what
        done(what)
        ref, terms = kr.bn_apply_ref(y, sc, sh, res if use_res else None, rsc if raff else None,
                                     rsh if raff else None, bool(relu))
        kr.assert_bf16_close(out, ref, terms, what)
        if use_mask:
            kr.assert_exact(mask, kr.relu_mask_ref(out), what + ": mask of the kernel's own output")
            sure = (ref.abs() > kr.bf16_bound(ref, terms)).reshape(-1, 8)
            diff = kr.mask_to_gate(mask ^ kr.relu_mask_ref(ref), (M * C // 8, 8))
            assert not bool((diff & sure).any()), what + ": mask differs from the reference's away from 0"
            if not use_res:  # channel 0 is +-0.0 everywhere: its bit is never set
                assert not bool(kr.mask_to_gate(mask, (M, C))[:, 0].any()), what
        if M * C >= 2 ** 21:
            kr.assert_unbiased_rounding(out, ref, what)


def test_bn_apply_refuses_mask_without_relu():
    lib = no._load()
    y, res, sc, sh, rsc, rsh = apply_inputs(37, 24, kr.gen(3))
    out, mask = G((37, 24), BF, 1.0), G(37 * 3, torch.uint8, 9)
    assert lib.pdt_bn_apply(no._p(y), None, no._p(out), no._p(sc), no._p(sh), 37, 24, 0, no._p(mask), no._s()) == -2
    assert lib.pdt_bn_apply_res_affine(no._p(y), no._p(res), no._p(out), no._p(sc), no._p(sh), no._p(rsc),
                                       no._p(rsh), 37, 24, 0, no._p(mask), no._s()) == -2
    assert lib.pdt_bn_apply(no._p(y), None, no._p(out), no._p(sc), no._p(sh), 37, 20, 1, None, no._s()) == -1
    done("refused")
    assert bool((out == 1).all()) and bool((mask == 9).all())  # nothing was launched


# -------------------------------------------------------------------------- backward reduce
GATES = ["none", "mask", "act", "recompute"]


def gate_inputs(gate, y, g, C):
    """(relu, act, mask, scale, shift, gate64): scale is a power of two and shift a small integer,
    so y*scale + shift is exact in fp32 and its sign is the same in any precision."""
    M = y.shape[0]
    if gate == "none":
        return 0, None, None, None, None, None
    if gate == "recompute":
        sc, sh = kr.pow2((C,), g), kr.ints((C,), g, -2, 2, dtype=F32)
        return 1, None, None, sc, sh, (kr.f64(y) * kr.f64(sc) + kr.f64(sh)) > 0
    act = (kr.normal((M, C), g).float() - 0.25).clamp_min(0).to(BF)
    if gate == "act":
        return 1, act, None, None, None, act > 0
    return 1, None, kr.relu_mask_ref(act), None, None, act > 0


def reduce_case(lib, M, C, blocks, gate, family, g):
    what = f"bwd_reduce M={M} C={C} blocks={blocks} gate={gate} {family}"
    if family == "exact":
        dA, y, mean = kr.exact_bn_bwd_inputs(M, C, g)
    else:
        dA, y, mean = kr.normal((M, C), g), kr.normal((M, C), g), kr.normal((C,), g, F32)
    relu, act, mask, sc, sh, gate64 = gate_inputs(gate, y, g, C)
    part = G((2, blocks, C), F32)
    rc = lib.pdt_bn_bwd_reduce(no._p(dA), no._p(y), no._p(act), no._p(mean), no._p(sc), no._p(sh), no._p(part), M, C,
                               relu, blocks, no._p(mask), no._s())
    assert rc == 0, what
    done(what)
    s, q, sa, qa = kr.bn_bwd_sums_ref(dA, y, gate64, mean)
    got = kr.f64(part).sum(1)
    if family == "exact":
        assert torch.equal(got[0], s) and torch.equal(got[1], q), what
    else:
        rp = 256 // (C // 8)
        L = math.ceil(M / (blocks * rp)) + rp  # a thread's rows, then the block's rp LDS adds
        kr.assert_close(got[0], s, 2 * L * kr.U * sa, what + " sum g")
        kr.assert_close(got[1], q, 2 * (L + 2) * kr.U * qa, what + " sum g (y - mean)")
    idle = part[:, math.ceil(M / (256 // (C // 8))):, :]
    assert bool((idle == 0).all()), what + ": a block without rows must write zeros"


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("rows", ["1", "rp-1", "rp*3+1", "40001"])
@pytest.mark.parametrize("C", [8, 24, 64, 72, 2048])
def test_bn_bwd_reduce(C, rows, gate):
    lib = no._load()
    rp = 256 // (C // 8)
    M = {"1": 1, "rp-1": rp - 1, "rp*3+1": rp * 3 + 1, "40001": 40001}[rows]
    if M < 1:
        M = 2  # (C = 2048: rp = 1)
    g = kr.gen(C + M)
    blocks = lib.pdt_bn_stats_blocks(M, C)
    assert blocks == max(1, min(512, math.ceil(M / rp)))
    # rp*3+1 rows on 3 blocks: block 0 takes a second trip of one row; C = 64: blocks without rows
    plans = [blocks] + ([3] if rows == "rp*3+1" else []) + ([blocks + 5] if C == 64 else [])
    for b in plans:
        for family in ("exact", "normal"):
            reduce_case(lib, M, C, b, gate, family, g)


def test_bn_bwd_reduce_refuses_wide_and_narrow_channels():
    """C / 8 > 256 chunks do not fit a block: the block-count query answers 1 (it used to divide
    by zero on the host) and the reduction refuses with -1, launching nothing."""
    lib = no._load()
    part = G((2, 1, 2056), F32, 3.0)
    x = torch.zeros(4, 2056, dtype=BF, device=DEV)
    mean = torch.zeros(2056, device=DEV)
    for C in (2056, 4096, 4, 0):
        assert lib.pdt_bn_stats_blocks(4, C) == 1
        assert lib.pdt_bn_bwd_reduce(no._p(x), no._p(x), None, no._p(mean), None, None, no._p(part), 4, C, 0, 1, None,
                                     no._s()) == -1
    done("refused")
    assert bool((part == 3).all())


# --------------------------------------------------------------------------- backward apply
@pytest.mark.parametrize("M,C", MC)
def test_bn_bwd_apply(M, C):
    lib = no._load()
    g = kr.gen(7 * M + C)
    dA, y = kr.normal((M, C), g), kr.normal((M, C), g)
    k1, k2, k3 = kr.normal((C,), g, F32), kr.normal((C,), g, F32, 0.3), kr.normal((C,), g, F32, 0.3)
    for gate in GATES:
        relu, act, mask, sc, sh, gate64 = gate_inputs(gate, y, g, C)
        for want_dres in (0, 1):
            what = f"bwd_apply M={M} C={C} gate={gate} dres={want_dres}"
            dy = G((M, C), BF)
            dres = G((M, C), BF) if want_dres else None
            rc = lib.pdt_bn_bwd_apply(no._p(dA), no._p(y), no._p(act), no._p(sc), no._p(sh), no._p(k1), no._p(k2),
                                      no._p(k3), no._p(dy), no._p(dres), M, C, relu, no._p(mask), no._s())
            assert rc == 0, what
            done(what)
            ref, terms, gref = kr.bn_bwd_apply_ref(dA, y, gate64, k1, k2, k3)
            kr.assert_bf16_close(dy, ref, terms, what)
            if want_dres:
                want = dA if gate64 is None else torch.where(gate64, dA, torch.zeros_like(dA))
                assert torch.equal(dres.view(torch.int16), want.view(torch.int16)), what + ": dres bits"
                kr.assert_exact(dres, gref, what + " dres")
    if M * C >= 2 ** 21:
        kr.assert_unbiased_rounding(dy, ref, what)


@pytest.mark.parametrize("M,C", MC)
def test_bn_bwd_apply_dual(M, C):
    lib = no._load()
    g = kr.gen(11 * M + C)
    dA, y1, y2 = kr.normal((M, C), g), kr.normal((M, C), g), kr.normal((M, C), g)
    ka = [kr.normal((C,), g, F32, 0.5) for _ in range(3)]
    kb = [kr.normal((C,), g, F32, 0.5) for _ in range(3)]
    _, _, mask, _, _, gate64 = gate_inputs("mask", y1, g, C)
    dy1, dy2 = G((M, C), BF), G((M, C), BF)
    what = f"bwd_apply_dual M={M} C={C}"
    rc = lib.pdt_bn_bwd_apply_dual(no._p(dA), no._p(mask), no._p(y1), no._p(ka[0]), no._p(ka[1]), no._p(ka[2]),
                                   no._p(dy1), no._p(y2), no._p(kb[0]), no._p(kb[1]), no._p(kb[2]), no._p(dy2), M, C,
                                   no._s())
    assert rc == 0, what
    done(what)
    for dy, yy, kk in ((dy1, y1, ka), (dy2, y2, kb)):
        ref, terms, _ = kr.bn_bwd_apply_ref(dA, yy, gate64, *kk)
        kr.assert_bf16_close(dy, ref, terms, what)
    assert lib.pdt_bn_bwd_apply_dual(no._p(dA), None, no._p(y1), no._p(ka[0]), no._p(ka[1]), no._p(ka[2]), no._p(dy1),
                                     no._p(y2), no._p(kb[0]), no._p(kb[1]), no._p(kb[2]), no._p(dy2), M, C,
                                     no._s()) == -1
