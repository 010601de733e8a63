"""csrc/pool.hip against float64 references (tests/kernel_ref.py): the generic max-pool forward
and gather backward over window geometries with overlap (s = 1), gaps (k < s), padding and
ragged edges, with tie-heavy inputs (first maximum wins), and the global average pool across a
thread-block boundary. Outputs are guard-banded and NaN-poisoned."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF = torch.bfloat16


def G(shape, dtype, fill=None):
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def maxpool_case(lib, k, s, p, N, H, W, C, g, what):
    Ho, Wo = kr.pool_out(H, k, s, p), kr.pool_out(W, k, s, p)
    inputs = {"normal": kr.normal((N, H, W, C), g),
              "constant": torch.full((N, H, W, C), 1.5, dtype=BF, device=DEV),
              "relu": (kr.normal((N, H, W, C), g).float() - 0.25).clamp_min(0).to(BF)}  # ~60 % zeros
    for name, x in inputs.items():
        w = f"{what} {name}"
        y, idx = G((N, Ho, Wo, C), BF), G((N, Ho, Wo, C), torch.uint8)
        assert lib.pdt_maxpool_fwd(no._p(x), no._p(y), no._p(idx), N, H, W, C, Ho, Wo, k, s, p, no._s()) == 0, w
        done(w)
        yr, ir = kr.maxpool_fwd_ref(x, k, s, p)
        kr.assert_exact(y, yr, w + " values")
        y_t = F.max_pool2d(x.permute(0, 3, 1, 2).float(), k, s, p).permute(0, 2, 3, 1).to(BF)
        assert torch.equal(y.view(torch.int16), y_t.contiguous().view(torch.int16)), w + " vs F.max_pool2d"
        kr.assert_exact(idx, ir, w + " argmax")
        for fam in ("exact", "normal"):
            dy = kr.ints((N, Ho, Wo, C), g) if fam == "exact" else kr.normal((N, Ho, Wo, C), g)
            dx = G((N, H, W, C), BF)
            assert lib.pdt_maxpool_bwd(no._p(dy), no._p(idx), no._p(dx), N, H, W, C, Ho, Wo, k, s, p, no._s()) == 0, w
            done(w + " bwd")
            dxr, ab = kr.maxpool_bwd_ref(dy, ir, H, W, k, s, p)
            if fam == "exact":
                # at most ceil(k/s)^2 <= 9 integers of magnitude <= 8: an integer below 256, exact in bf16
                kr.assert_exact(dx, dxr, w + " bwd exact")
            else:
                kr.assert_bf16_close(dx, dxr, ab, w + " bwd", roundings=math.ceil(k / s) ** 2)
            if k < s:  # pixels no window covers
                hole_h = [h for h in range(H) if (h + p) % s >= k or (h + p) // s >= Ho]
                assert hole_h and bool((dx[:, hole_h] == 0).all()), w + " uncovered rows"


GEOM = [(2, 2, 0), (3, 1, 1), (3, 2, 0), (3, 2, 1), (2, 3, 0), (5, 3, 2)]


# (a 1x1 input only where a window fits it: 1 + 2p >= k)
GEOM_HW = [(k, s, p, H, W) for k, s, p in GEOM for H, W in [(1, 1), (5, 7), (8, 9)] if H + 2 * p >= k]


@pytest.mark.parametrize("k,s,p,H,W", GEOM_HW)
def test_maxpool_generic(k, s, p, H, W):
    lib = no._load()
    g = kr.gen(100 * k + 10 * s + p + H)
    for N in (1, 3):
        for C in ((8, 24) if (k, s, p) == (3, 2, 1) else (8,)):
            maxpool_case(lib, k, s, p, N, H, W, C, g, f"maxpool k{k}s{s}p{p} {N}x{H}x{W}x{C}")


@pytest.mark.parametrize("row", ["0", "1"])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 9)])
def test_maxpool_k3s2p1_c64_row_and_generic_backward(monkeypatch, row, H, W):
    """C = 64: PDT_MAXPOOL_BWD_ROW=1 takes the quad-row backward, 0 the generic gather."""
    monkeypatch.setenv("PDT_MAXPOOL_BWD_ROW", row)
    lib = no._load()
    g = kr.gen(64 + H)
    for N in (1, 3):
        maxpool_case(lib, 3, 2, 1, N, H, W, 64, g, f"maxpool k3s2p1 row={row} {N}x{H}x{W}x64")


@pytest.mark.parametrize("C", [8, 72, 2048])
@pytest.mark.parametrize("HW", [1, 16, 49, 50])
def test_avgpool(HW, C):
    lib = no._load()
    g = kr.gen(HW + C)
    for N in (1, 5, 33):  # N * C / 8 = 33 .. 8448 threads: below, across and many 256-thread blocks
        what = f"avgpool N={N} HW={HW} C={C}"
        exact = HW in (1, 16)
        x = kr.ints((N, HW, C), g) if exact else kr.normal((N, HW, C), g, mean=0.5)
        dy = kr.ints((N, C), g) if exact else kr.normal((N, C), g)
        y, dx = G((N, C), BF), G((N, HW, C), BF)
        assert lib.pdt_avgpool_fwd(no._p(x), no._p(y), N, HW, C, no._s()) == 0, what
        done(what)
        assert lib.pdt_avgpool_bwd(no._p(dy), no._p(dx), N, HW, C, no._s()) == 0, what
        done(what + " bwd")
        yr, ya = kr.avgpool_fwd_ref(x)
        dxr, dxa = kr.avgpool_bwd_ref(dy, HW)
        if exact:  # sums of 16 integers <= 8, divided by 16: exact in fp32 and in bf16
            kr.assert_exact(y, yr, what)
            kr.assert_exact(dx, dxr, what + " bwd")
        else:  # HW sequential fp32 adds, the rounded 1/HW and its product
            kr.assert_bf16_close(y, yr, ya, what, roundings=HW + 2)
            kr.assert_bf16_close(dx, dxr, dxa, what + " bwd", roundings=2)
    assert lib.pdt_avgpool_fwd(no._p(x), no._p(y), 1, HW, 12, no._s()) == -1
