"""Float64 reference for Random Erasing in the packed-image pipeline, built on
packed_ref.reference / mix_ref.mixed. Nothing here touches the code under test: the uint32 hashing
is written out again in numpy.

erased(): inside any of a sample's rectangles (y0, x0, y1, x1), half-open, every element is +0
("const") or the draw z below ("pixel"); outside, the view it was given.

The draw of output pixel (oy, ox), channel c in 0..2, for the sample's 32-bit key (the formula in
the header of csrc/image_aug.hip), hash32 being the mixer of csrc/misc.hip:

    kq = hash32(key ^ (oy S + ox) * 0x9E3779B9)
    h1 = hash32(kq ^ (2c + 1) * 0x85EBCA6B),  h2 = hash32(kq ^ (2c + 2) * 0x85EBCA6B)
    u1 = ((h1 >> 8) + 1) / 2^24 in (0, 1],    t = (h2 >> 8) / 2^23 in [0, 2)
    r  = sqrt(-2 ln u1),  z = r cos(pi t)

eps_z -- the fp32 error bound of the kernel's z = sqrtf(-2.f * logf(u1)) * cospif(t). u1 and t are
exact in fp32 (24-bit integers times a power of two) and so is the product by -2. The kernel uses
the accurate library functions logf, sqrtf and cospif of the ROCm device library (OCML), whose
stated accuracy target is the OpenCL C full-profile table "Relative error as ULPs" (OpenCL C 3.0
specification, section 7.4): log <= 3 ulp, sqrt <= 3 ulp, cospi <= 4 ulp. (The HIP math API
reference lists lower measured maxima for the three; the looser, specified figures are used.)
With ulp(x) <= 2^-23 |x|:

  * L = -2 ln u1 carries a relative error <= 3 * 2^-23, which the square root halves: 3 * 2^-24;
  * sqrtf adds <= 3 * 2^-23 relative, so r is within (3 + 6) * 2^-24 r;
  * |cospi| <= 1, so its 4 ulp are <= 4 * 2^-23 absolute: 8 * 2^-24 r in the product;
  * the product rounds once: 2^-24 |z| <= 2^-24 r.

Together |z_kernel - z| <= 18 * 2^-24 * r, times (1 + 2^-10) for the second-order terms:
eps_z = EPS_K * 2^-24 * r * (1 + 2^-10) with EPS_K = 18 -- at most 6.2e-6 (r <= sqrt(48 ln 2) =
5.77), a thousandth of a bf16 ulp of such a value. At u1 = 1, r = 0 and the kernel's z is exactly
(+-)0. The kernel rounds z once to bf16, so an output element must equal the bf16
round-to-nearest-even of some value in [z - eps_z, z + eps_z]: bf16_rne(z - eps_z) <= out <=
bf16_rne(z + eps_z), rounding being monotone. eps_z matters only for a draw within eps_z of a bf16
rounding tie (the two ends then round apart); every other element must be bf16_rne(z) exactly, so a
bf16 output cannot show how much of eps_z the kernel uses. assert_noise_close prints how many
elements were such near-ties.
"""
import numpy as np
import torch

import mix_ref as M
import packed_ref as R

EPS_K = 18
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))
FAULTS = ("shifted", "closed_right_edge", "batch_position_key", "channel_repeated")


def hash32(x):
    """The mixer on uint32 values (any integer array; computed in uint64, wrapped to 32 bits)."""
    x = np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def inside_any(rects, S):
    """bool [B, 1, S, S]: output pixels inside any of the sample's rectangles; rects [B, R, 4]."""
    r = torch.as_tensor(np.asarray(rects), dtype=torch.int64)
    r = r.reshape(r.shape[0], -1, 1, 1, 4)
    yy = torch.arange(S).view(1, 1, S, 1)
    xx = torch.arange(S).view(1, 1, 1, S)
    m = (yy >= r[..., 0]) & (yy < r[..., 2]) & (xx >= r[..., 1]) & (xx < r[..., 3])
    return m.any(dim=1)[:, None]


def noise_parts(keys, S, channel_map=(0, 1, 2)):
    """(r, z): float64 [B, 3, S, S] each, the radius and the draw of every element. keys: the
    samples' uint32 keys (any integers; the low 32 bits count)."""
    keys = np.asarray(keys).astype(np.int64).reshape(-1, 1) & 0xFFFFFFFF
    q = np.arange(S * S, dtype=np.uint64)[None, :]
    kq = hash32(keys.astype(np.uint64) ^ ((q * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)))  # [B, S*S]
    rs, zs = [], []
    for c in channel_map:
        h1 = hash32(kq ^ np.uint64(((2 * c + 1) * 0x85EBCA6B) & 0xFFFFFFFF))
        h2 = hash32(kq ^ np.uint64(((2 * c + 2) * 0x85EBCA6B) & 0xFFFFFFFF))
        u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0
        t = (h2 >> np.uint64(8)).astype(np.float64) / 8388608.0
        r = np.sqrt(-2.0 * np.log(u1))
        rs.append(r)
        zs.append(r * np.cos(np.pi * t))
    shape = (keys.shape[0], 3, S, S)
    return torch.from_numpy(np.stack(rs, 1).reshape(shape)), torch.from_numpy(np.stack(zs, 1).reshape(shape))


def noise(keys, S):
    """float64 [B, 3, S, S]: the draw z of every element."""
    return noise_parts(keys, S)[1]


def eps_z(r):
    """The bound derived above, per element, from the radius r."""
    return EPS_K * 2.0 ** -24 * (1.0 + 2.0 ** -10) * r


def erased(view64, rects, keys, mode, fault=None):
    """float64 [B, 3, S, S]: view64 with the rectangles erased. ``fault`` seeds one of FAULTS, for
    the tests of the tests."""
    assert mode in ("pixel", "const") and fault in (None,) + FAULTS
    B, _, S, _ = view64.shape
    rects = np.asarray(rects).astype(np.int64).reshape(B, -1, 4).copy()
    keys = np.asarray(keys).astype(np.int64).reshape(B)
    if fault == "shifted":
        rects[..., [1, 3]] += (rects[..., 3:4] > rects[..., 1:2])  # non-empty ones, one column right
        rects = np.minimum(rects, S)
    if fault == "closed_right_edge":
        rects[..., 3] += (rects[..., 3] > rects[..., 1]) & (rects[..., 3] < S)
    if fault == "batch_position_key":
        keys = np.arange(B, dtype=np.int64)
    cmap = (0, 0, 2) if fault == "channel_repeated" else (0, 1, 2)
    fill = noise_parts(keys, S, cmap)[1] if mode == "pixel" else torch.zeros_like(view64)
    return torch.where(inside_any(rects, S), fill, view64)


def erased_views(images, idx, box, S, rects, keys, mode, mix=None):
    """erased() over packed_ref.reference (mix None) or mix_ref.mixed (mix = (pidx, pbox, rect,
    w_own)) of the same arguments."""
    if mix is None:
        return erased(R.reference(images, idx, box, S), rects, keys, mode)
    pidx, pbox, rect, w_own = mix
    return erased(M.mixed(images, idx, box, pidx, pbox, rect, w_own, S), rects, keys, mode)


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; one rounding, no detour
    through fp32. Normal range only (the values here are 0 or |x| in [1e-9, 6])."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)  # |m| in [0.5, 1): 8 significand bits = multiples of 2^-8
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def assert_noise_close(out, r, z, what=""):
    """out (bf16 values as float64) against the draw: bf16_rne(z - eps_z) <= out <= bf16_rne(z +
    eps_z). Returns and prints the worst |out - z| / (eps_z + half a bf16 ulp of z)."""
    out, r, z = (np.asarray(v, dtype=np.float64) for v in (out, r, z))
    assert np.isfinite(out).all(), f"{what}: non-finite noise"
    e = EPS_K * 2.0 ** -24 * (1.0 + 2.0 ** -10) * r
    lo, hi = bf16_rne(z - e), bf16_rne(z + e)
    ulp = np.ldexp(1.0, np.frexp(z)[1] - 8)
    ratio = float((np.abs(out - z) / (e + 0.5 * ulp + 1e-300)).max()) if out.size else 0.0
    print(f"{what}: {out.size} noise elements, worst |out - z| / (eps_z + ulp/2) = {ratio:.4f}, "
          f"max |out| = {float(np.abs(out).max()) if out.size else 0:.3f}")
    print(f"{what}: {int((lo != hi).sum())} of {out.size} draws lie within eps_z of a bf16 tie; the others equal bf16_rne(z)")
    bad = (out < lo) | (out > hi)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {out.size} outside the bound, first at {np.argwhere(bad)[0].tolist()}"
    assert float(np.abs(out).max(initial=0.0)) <= bf16_rne(R_MAX + 1e-5)
    return ratio
