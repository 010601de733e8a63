"""Mixup / CutMix inside the packed-image kernel (csrc/image_aug.hip, the MIX instantiation) on an
MI355X: bitwise against the plain kernel wherever the result is one view's pixel, against the
float64 reference (tests/mix_ref.py) where it blends, and PackedImageLoader's resident and staged
modes with mixing on. Outputs are guard-banded and pre-filled with NaN bits; the pad channel must
be +0 bit for bit."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_ref as kr  # noqa: E402
import mix_ref as M  # noqa: E402
import packed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.data import MixedTarget, PackedImageLoader  # noqa: E402
from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

HS, WS = 40, 56
DEV = torch.device("cuda")

# 9 outputs: own and partner views of different sizes and flips (entry 3 at identity scale for S = 32,
# entry 5 for S = 33), gathered through a repeating, non-monotone idx
BOX = [(0, 0, 40, 56, 0), (3, 5, 17, 29, 1), (39, 55, 1, 1, 0), (4, 12, 32, 32, 1), (0, 0, 7, 50, 1),
       (5, 5, 33, 33, 0), (2, 7, 31, 18, 1), (20, 30, 20, 26, 0), (1, 2, 30, 40, 1)]
PBOX = [(10, 3, 20, 41, 1), (0, 0, 40, 56, 0), (4, 12, 32, 32, 0), (17, 20, 9, 30, 1), (5, 5, 33, 33, 1),
        (0, 0, 40, 56, 1), (39, 0, 1, 56, 0), (3, 5, 17, 29, 0), (6, 6, 12, 12, 0)]
IDX = [4, 0, 4, 2, 1, 3, 0, 3, 1]
PIDX = [1, 4, 0, 0, 3, 2, 4, 1, 2]


@pytest.fixture(scope="module")
def src():
    rng = np.random.default_rng(17)
    return torch.from_numpy(rng.integers(0, 256, size=(9, HS, WS, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def plain(src):
    """The plain kernel's own and partner views, computed once: {(S, with_idx): (own, partner)} as
    int16 bit patterns [9, S, S, 4] on the host."""
    src_dev = src.to(DEV)
    views = {}
    for S in (32, 33):
        for with_idx in (True, False):
            views[S, with_idx] = (_plain(src_dev, IDX if with_idx else None, BOX, S), _plain(src_dev, PIDX, PBOX, S))
    return views


def _dev(v, dtype):
    return torch.tensor(v, dtype=dtype, device=DEV)


def _plain(src_dev, idx, boxes, S):
    out = kr.guarded((len(boxes), S, S, 4), torch.bfloat16, DEV)
    no.crop_resize_normalize(src_dev, None if idx is None else _dev(idx, torch.int64), _dev(boxes, torch.int32), out,
                             R.MEAN, R.STD)
    torch.cuda.synchronize()
    kr.check_guards("plain")
    return out.view(torch.int16).cpu()


def _mix(src_dev, idx, boxes, pidx, pboxes, rects, w_own, S, what):
    """Launch the mixing entry point into a guarded, NaN-filled output; returns its int16 bits."""
    out = kr.guarded((len(boxes), S, S, 4), torch.bfloat16, DEV)  # the poison is bf16 0xFFFF, a NaN
    assert torch.isnan(out).all()
    no.crop_resize_normalize_mix(src_dev, None if idx is None else _dev(idx, torch.int64), _dev(boxes, torch.int32),
                                 _dev(pidx, torch.int64), _dev(pboxes, torch.int32), _dev(rects, torch.int32),
                                 torch.as_tensor(np.asarray(w_own, dtype=np.float32)).to(DEV), out, R.MEAN, R.STD)
    torch.cuda.synchronize()
    kr.check_guards(what)
    bits = out.view(torch.int16).cpu()
    assert not bits[..., 3].any(), f"{what}: the pad channel must be +0 bit for bit"
    assert not torch.isnan(out[..., :3]).any(), f"{what}: an output element was not written"
    return bits


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "idx_none"])
@pytest.mark.parametrize("S", [32, 33])
def test_no_mixing_is_the_plain_kernel_bit_for_bit(src, plain, S, with_idx):
    rects = [(0, 0, 0, 0), (3, 5, 3, 20), (4, 7, 20, 7), (S, S, S, S), (0, 0, 0, S), (0, 0, S, 0), (5, 5, 5, 5),
             (S, 0, S, S), (0, S, S, S)]  # every empty form: y0 == y1 with x0 < x1 and the other way round
    idx = IDX if with_idx else None
    got = _mix(src.to(DEV), idx, BOX, PIDX, PBOX, rects, [1.0] * 9, S, "no mixing")
    assert torch.equal(got, plain[S, with_idx][0])


@pytest.mark.parametrize("S", [32, 33])
def test_full_rectangle_is_the_partner_view_bit_for_bit(src, plain, S):
    w_own = [1.0, 1.0, 0.5, 1.0, 0.25, 1.0, 0.0, 1.0, 1.0]  # inside the rectangle the weight does not matter
    got = _mix(src.to(DEV), IDX, BOX, PIDX, PBOX, [(0, 0, S, S)] * 9, w_own, S, "full rectangle")
    assert torch.equal(got, plain[S, True][1])


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "idx_none"])
@pytest.mark.parametrize("S", [32, 33])
def test_cutmix_composite_is_exact(src, plain, S, with_idx):
    """Every pixel is the plain kernel's own-view pixel outside the rectangle and its partner-view
    pixel inside. A workgroup is 256 lanes = 256 pixel pairs: at S = 32 (16 pairs a row) rows 15 | 16,
    at S = 33 (17 pairs a row) inside row 15 -- rows 12..20 cross both."""
    rects = [(2, 3, 10, 12),          # odd x0: splits a lane's pixel pair
             (2, 4, 10, 11),          # odd x1
             (0, 0, 1, 1),            # 1x1 at (0, 0)
             (S - 1, S - 1, S, S),    # 1x1 at (S-1, S-1)
             (5, 0, 6, S),            # one full row
             (0, 7, S, 8),            # one full column
             (4, S - 5, 20, S),       # ends at the last column (S = 33: the 8-byte tail store)
             (12, 3, 20, 29),         # crosses a 256-lane workgroup boundary
             (10, 1, 31, S - 1)]
    own, partner = plain[S, with_idx]
    got = _mix(src.to(DEV), IDX if with_idx else None, BOX, PIDX, PBOX, rects, [1.0] * 9, S, "cutmix")
    want = torch.where(M.inside(rects, S).permute(0, 2, 3, 1), partner, own)
    bad = (got != want).any(dim=3)
    assert not bad.any(), f"first differing (b, y, x): {bad.nonzero()[0].tolist()} of {int(bad.sum())}"


@pytest.mark.parametrize("S", [32, 33])
def test_self_blend_is_exact(src, plain, S):
    """A partner equal to self at w_own = 0.5: fma(0.5, v, 0.5 v) = v."""
    got = _mix(src.to(DEV), IDX, BOX, IDX, BOX, [(0, 0, 0, 0)] * 9, [0.5] * 9, S, "self blend")
    assert torch.equal(got, plain[S, True][0])


@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "idx_none"])
@pytest.mark.parametrize("S", [32, 33])
def test_mixup_against_float64(src, S, with_idx):
    """Bound: packed_ref.assert_pixels_close as it stands. The blend adds two fp32 roundings (the
    product (1 - w) v_partner and the fma) and the rounding of 1 - w on values <= 255: under
    3 * 2^-24 * 255 = 4.6e-5 on the 0..255 scale, 8e-7 after / 255 / std -- inside that function's
    1e-5 absolute term."""
    w_own = [0.0, 0.25, 0.5, float(np.float32(0.3)), 1.0 - 2.0 ** -12, 0.25, float(np.float32(0.3)), 0.5, 0.0]
    rects = [(0, 0, 0, 0)] * 8 + [(3, 3, 9, 20)]  # ... and one rectangle inside a blended image
    idx = IDX if with_idx else None
    got = _mix(src.to(DEV), idx, BOX, PIDX, PBOX, rects, w_own, S, "mixup")
    ref = M.mixed(src, idx, BOX, PIDX, PBOX, rects, w_own, S)
    out = got.view(torch.bfloat16)[..., :3].permute(0, 3, 1, 2)
    for b in range(9):
        R.assert_pixels_close(out[b], ref[b], f"mixup S={S} image {b} w_own={w_own[b]}")


def test_binding_rejects_bad_arguments(src):
    s = src.to(DEV)
    out = torch.empty((2, 8, 8, 4), dtype=torch.bfloat16, device=DEV)
    good = dict(idx=None, box=_dev([[0, 0, 8, 8, 0]] * 2, torch.int32), pidx=_dev([1, 0], torch.int64),
                pbox=_dev([[0, 0, 8, 8, 1]] * 2, torch.int32), rect=_dev([[0, 0, 4, 4]] * 2, torch.int32),
                w_own=_dev([1.0, 0.5], torch.float32))

    def call(**kw):
        a = dict(good, **kw)
        no.crop_resize_normalize_mix(s, a["idx"], a["box"], a["pidx"], a["pbox"], a["rect"], a["w_own"], out, R.MEAN,
                                     R.STD)
    call()
    torch.cuda.synchronize()
    wide = {"pidx": _dev([[1, 0], [0, 1]], torch.int64)[:, 0], "pbox": _dev([[0, 0, 8, 8, 1, 0]] * 2, torch.int32)[:, :5],
            "rect": _dev([[0, 0, 4, 4, 0]] * 2, torch.int32)[:, :4], "w_own": _dev([[1.0, 0], [0.5, 0]], torch.float32)[:, 0]}
    other = {"pidx": torch.int32, "pbox": torch.int64, "rect": torch.int64, "w_own": torch.float64}
    for name in ("pidx", "pbox", "rect", "w_own"):
        assert not wide[name].is_contiguous() and wide[name].shape == good[name].shape
        for bad in (good[name].to(other[name]),   # dtype
                    good[name][:1],               # shape
                    good[name].cpu(),             # device
                    wide[name]):                  # contiguity
            with pytest.raises(AssertionError):
                call(**{name: bad})
    with pytest.raises(AssertionError):
        call(pidx=None)
    lib = no._load()
    m = (no.c_float * 3)(*R.MEAN)
    args = [no._p(s), HS, WS, None, no._p(good["box"]), no._p(good["pidx"]), no._p(good["pbox"]), no._p(good["rect"]),
            no._p(good["w_own"]), no._p(out), 2, 8, 4, no.ctypes.addressof(m), no.ctypes.addressof(m), no._s()]
    for k in (0, 4, 5, 6, 7, 8, 9):  # a null pointer
        assert lib.pdt_crop_resize_norm_mix_u8_bf16(*[None if i == k else a for i, a in enumerate(args)]) == -1
    for k, v in ((10, 0), (11, 0), (12, 8), (1, 0)):  # bad sizes, as the plain entry point
        assert lib.pdt_crop_resize_norm_mix_u8_bf16(*[v if i == k else a for i, a in enumerate(args)]) == -1


# ----------------------------------------------------------------------------- loader
@pytest.fixture(scope="module")
def packed13(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed13")
    images, labels = R.make_set(d, 13, HS, WS, num_classes=5, seed=31)
    return d, images, labels


@pytest.mark.parametrize("batch", [4, 3])
def test_loader_resident_and_staged_mix_identically(packed13, batch):
    """13 images: batch 4 ends with a batch of 1 (it pairs with itself), batch 3 has a self-paired
    middle element. The staged partner is read from the same staging slot."""
    d, images, labels = packed13
    kw = dict(batch_size=batch, image_size=32, seed=6, mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")
    res = PackedImageLoader(d, resident=True, **kw)
    stg = PackedImageLoader(d, resident=False, prefetch=2, **kw)
    assert res.mode == "resident" and stg.mode == "staged" and res.mixing
    for epoch in (0, 1):
        res.set_epoch(epoch)
        stg.set_epoch(epoch)
        br, bs = list(res), list(stg)
        order = list(res.sampler)
        assert len(br) == len(bs) == -(-13 // batch)
        for n, ((xr, tr), (xs, ts)) in enumerate(zip(br, bs)):
            idx = order[batch * n:batch * n + batch]
            assert isinstance(tr, MixedTarget) and isinstance(ts, MixedTarget)
            assert getattr(xr, "pdt_nhwc_pad", None) == 4 and xr.dtype == torch.bfloat16
            assert torch.equal(xr.view(torch.int16), xs.view(torch.int16))
            for a, b in zip(tr, ts):
                assert a.is_cuda and torch.equal(a, b)
            partner, w_own, rect, lam = res.mix(idx, epoch)
            assert tr.label_a.dtype == torch.int64 and tr.lam.dtype == torch.float32
            assert torch.equal(tr.label_a.cpu(), torch.from_numpy(labels[idx]))
            assert torch.equal(tr.label_b.cpu(), torch.from_numpy(labels[idx[::-1]]))
            assert torch.equal(tr.lam.cpu(), lam)
            assert not no.nhwc_padded_view(xs, 4)[:, 3:].any()
            ref = M.mixed_batch(images, idx, res.boxes(idx, epoch), partner, rect, w_own, 32)
            R.assert_pixels_close(xr, ref, f"batch {batch} epoch {epoch} #{n}")
    assert not [t for t in threading.enumerate() if t.name.startswith("PackedImageLoader")]
