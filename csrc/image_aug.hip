// Input pipeline on the device (data/packed.py PackedImageLoader): one launch turns a batch
// of stored uint8 RGB images into the augmented, normalized bf16 batch in the zero-padded
// 4-channel NHWC storage the space-to-depth stem reads in place.
//
// Per output pixel (oy, ox) of image b, with box = (y0, x0, h, w, flip):
//   ox' = flip ? S-1-ox : ox
//   sy = max((oy+0.5) h/S - 0.5, 0), sx = max((ox'+0.5) w/S - 0.5, 0)
//   iy = min(floor(sy), h-1), iy1 = min(iy+1, h-1)   (likewise x: taps clamp to the BOX)
//   v = bilinear blend of the four taps; out = (v/255 - mean[c]) * inv_std[c]; channel 3 = +0
// i.e. F.interpolate(crop, (S, S), mode="bilinear", align_corners=False) + flip + normalize.
//
// The source coordinate is formed in integers: sy = num / 2S with num = (2 oy + 1) h - S, so
// floor(sy) and the blend weight rem / 2S are exact up to one fp32 rounding of the weight, and
// an identity-scale crop (h = S) has weight 0 -- it copies pixels bit for bit.
//
// Streaming kernel, no LDS. A workgroup works inside one image, so the box, the gather index
// and the image base are wave-uniform (scalar loads); a lane produces two adjacent padded
// pixels of one row and writes them with one 16-byte store (8 bytes for the odd-S row tail).
// Every tap is one unaligned dword load covering the pixel's three bytes; edge taps use
// clamped indices, never a branch around a load.
//
// Random Erasing (the ERASE instantiations): output b carries R rectangles (y0, x0, y1, x1),
// half-open, in output coordinates, and a 32-bit noise key. A pixel inside any of them loads no
// taps; its three channels are +0 (mode 0, "const") or N(0, 1) draws (mode 1, "pixel"), and the
// pad channel stays +0. Every other pixel is the one the non-erase kernels produce, bit for bit.
// The draw of pixel (oy, ox), channel c in 0..2, all hashing in uint32 with hash32 the mixer of
// misc.hip:
//   kq = hash32(ekey[b] ^ (oy S + ox) * 0x9E3779B9)
//   h1 = hash32(kq ^ (2c + 1) * 0x85EBCA6B),  h2 = hash32(kq ^ (2c + 2) * 0x85EBCA6B)
//   u1 = ((h1 >> 8) + 1) / 2^24  in (0, 1],   t = (h2 >> 8) / 2^23 = 2 u2  in [0, 2)
//   z  = sqrtf(-2 logf(u1)) * cospif(t)       (Box-Muller; u1, t and -2 logf exact or one rounding)
// so |z| <= sqrt(48 ln 2) = 5.77 and no inf or NaN arises; z is rounded once, to bf16. logf, sqrtf
// and cospif are the accurate library functions (not __logf / __cosf): the argument of cospif is
// exact, so no range-reduction error enters, and the erased pixels are the minority path.
#include "pdt_common.h"

namespace {
constexpr int NT = 256;

// One axis of the bilinear sampler: output coordinate o of n source pixels resized to S.
// S2 = 2S, inv2S = 1 / 2S. (2S+1) n < 2^31 is checked on the host. The blend weights are
// l = rem / 2S and om = 1 - l, the latter as one fma (one rounding), spelled out: every path forms
// it here, so the bits cannot differ between a straight-line path and one behind a per-lane branch.
struct Axis {
  int i0, i1;   // the two taps, clamped to the box
  float l, om;  // the weight of i1 and of i0
};
__device__ __forceinline__ Axis axis_taps(int o, int n, int S, int S2, float inv2S) {
  int num = (2 * o + 1) * n - S;
  num = num < 0 ? 0 : num;
  int i = (int)((float)num * inv2S);  // floor(num / 2S) up to +-1: fixed below
  int r = num - i * S2;
  if (r < 0) { --i; r += S2; }
  if (r >= S2) { ++i; r -= S2; }
  const int i0 = i < n - 1 ? i : n - 1;
  return Axis{i0, i0 + 1 < n - 1 ? i0 + 1 : n - 1, (float)r * inv2S, fmaf(-inv2S, (float)r, 1.f)};
}

// The three bytes of the pixel at byte offset off of an image: w >> sh has them in bits 0..23 (R,
// G, B from the low byte). One unaligned dword load that never leaves the image: bytes
// [off-1, off+3) for off > 0, bytes [0, 4) for the first pixel (an image has >= 4 bytes, host
// check). DEFER leaves the shift (0 or 8) to the caller; otherwise it is applied here and sh is 0.
template <bool DEFER>
__device__ __forceinline__ uint32_t load_rgb(const uint8_t* __restrict__ img, uint32_t off, uint32_t& sh) {
  const uint32_t back = off > 0 ? 1u : 0u;
  uint32_t w;
  __builtin_memcpy(&w, img + (off - back), 4);
  sh = DEFER ? back * 8 : 0u;
  return DEFER ? w : w >> (back * 8);
}

struct PixelOut {
  uint32_t lo, hi;  // bf16 (c0, c1), (c2, 0)
};

struct Rgb {
  float v[3];  // the bilinear sample, fp32 on the 0..255 scale
};

struct Taps {
  uint32_t p00, p01, p10, p11;  // load_rgb of the four taps
  uint32_t sh;                  // their four shifts, one per byte
  float ly, lx, omy, omx;       // the weights l and 1 - l of the two axes
};

template <bool DEFER>
__device__ __forceinline__ Taps load_taps(const uint8_t* __restrict__ img, uint32_t row0, uint32_t row1, const Axis& y,
                                          const Axis& x) {
  uint32_t s00, s01, s10, s11;
  Taps t;
  t.p00 = load_rgb<DEFER>(img, (row0 + (uint32_t)x.i0) * 3u, s00);
  t.p01 = load_rgb<DEFER>(img, (row0 + (uint32_t)x.i1) * 3u, s01);
  t.p10 = load_rgb<DEFER>(img, (row1 + (uint32_t)x.i0) * 3u, s10);
  t.p11 = load_rgb<DEFER>(img, (row1 + (uint32_t)x.i1) * 3u, s11);
  t.sh = s00 | (s01 << 8) | (s10 << 16) | (s11 << 24);
  t.ly = y.l, t.lx = x.l, t.omy = y.om, t.omx = x.om;
  return t;
}

// the bilinear blend, without the normalization
__device__ __forceinline__ Rgb blend_taps(const Taps& t) {
  const uint32_t p00 = t.p00 >> (t.sh & 0xffu), p01 = t.p01 >> ((t.sh >> 8) & 0xffu);
  const uint32_t p10 = t.p10 >> ((t.sh >> 16) & 0xffu), p11 = t.p11 >> (t.sh >> 24);
  const float w00 = t.omy * t.omx, w01 = t.omy * t.lx, w10 = t.ly * t.omx, w11 = t.ly * t.lx;
  Rgb r;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = (float)((p00 >> (8 * c)) & 0xffu), b = (float)((p01 >> (8 * c)) & 0xffu);
    const float d = (float)((p10 >> (8 * c)) & 0xffu), e = (float)((p11 >> (8 * c)) & 0xffu);
    r.v[c] = fmaf(w11, e, fmaf(w10, d, fmaf(w01, b, w00 * a)));
  }
  return r;
}

// normalize and round once, to bf16
__device__ __forceinline__ PixelOut finish(const Rgb& r, float m0, float m1, float m2, float s0, float s1, float s2) {
  constexpr float K = 1.f / 255.f;
  PixelOut o;
  o.lo = pack2bf((fmaf(r.v[0], K, -m0)) * s0, (fmaf(r.v[1], K, -m1)) * s1);
  o.hi = pack2bf((fmaf(r.v[2], K, -m2)) * s2, 0.f);
  return o;
}

// One augmented view: an image and its crop box. Wave-uniform as loaded; a CutMix lane holds its
// own choice of two.
struct View {
  const uint8_t* img;
  int y0, x0, h, w, flip;
};

__device__ __forceinline__ View select_view(bool in, const View& par, const View& own) {
  return View{in ? par.img : own.img, in ? par.y0 : own.y0, in ? par.x0 : own.x0,
              in ? par.h : own.h,     in ? par.w : own.w,   in ? par.flip : own.flip};
}

// The loaded taps of output pixel (oy, ox) of view v, formed from scratch (CutMix: the lane's
// two pixels may read different views). PREDICATED (the ERASE paths): only a lane that samples
// (on) issues loads, and their shifts are left to blend_taps, behind the caller's pin -- inside the
// per-lane branch a shift would wait for its load there, and the other pixel's loads would issue
// behind that wait. Otherwise on is ignored and the loads are shifted at once.
template <bool PREDICATED>
__device__ __forceinline__ Taps view_taps(bool on, const View& v, int oy, int ox, int Ws, int S, int S2, float inv2S) {
  Taps t{};
  if (!PREDICATED || on) {
    const Axis y = axis_taps(oy, v.h, S, S2, inv2S), x = axis_taps(v.flip ? S - 1 - ox : ox, v.w, S, S2, inv2S);
    t = load_taps<PREDICATED>(v.img, (uint32_t)((v.y0 + y.i0) * Ws + v.x0), (uint32_t)((v.y0 + y.i1) * Ws + v.x0),
                              y, x);
  }
  return t;
}

// Mixup / CutMix operands of output b (MIX kernels): the partner's augmented view -- its gather
// index and its own box and flip --, the cut rectangle (y0, x0, y1, x1), half-open, in output
// coordinates, and the weight of the own pixels outside it.
struct MixArgs {
  const int64_t* pidx;
  const int* pbox;
  const int* rect;
  const float* w_own;
};
struct NoMix {};

// The kernel's store of the pair at (b, oy, ox0): 4 bf16 (8 bytes) per padded pixel, 64-bit pixel index
__device__ __forceinline__ void store_pair(u16* __restrict__ out, long b, int S, int oy, int ox0, bool pair, PixelOut a,
                                           PixelOut c) {
  uint2* o = reinterpret_cast<uint2*>(out) + ((b * S + oy) * S + ox0);
  if (pair) {
    // 8-byte aligned always, 16-byte aligned for even S
    typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
    *reinterpret_cast<u32x4_a8*>(o) = u32x4_a8{a.lo, a.hi, c.lo, c.hi};
  } else {
    *o = uint2{a.lo, a.hi};
  }
}

// Random Erasing operands of output b (ERASE kernels): erect int32 [B][R][4], ekey uint32 [B],
// mode 0 = const / 1 = pixel.
struct EraseArgs {
  const int* erect;
  const uint32_t* ekey;
  int R, mode;
};
struct MixEraseArgs : MixArgs {
  EraseArgs er;
};

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// The fill of erased pixel q = oy S + ox (the formula in the file header); mode is wave-uniform.
__device__ __forceinline__ PixelOut erase_fill(uint32_t key, uint32_t q, int mode) {
  if (!mode) return PixelOut{0u, 0u};
  const uint32_t kq = hash32(key ^ q * 0x9E3779B9u);
  float z[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t h1 = hash32(kq ^ (uint32_t)(2 * c + 1) * 0x85EBCA6Bu);
    const uint32_t h2 = hash32(kq ^ (uint32_t)(2 * c + 2) * 0x85EBCA6Bu);
    const float u1 = (float)((h1 >> 8) + 1u) * (1.f / 16777216.f);
    const float t = (float)(h2 >> 8) * (1.f / 8388608.f);
    z[c] = sqrtf(-2.f * logf(u1)) * cospif(t);
  }
  return PixelOut{pack2bf(z[0], z[1]), pack2bf(z[2], 0.f)};
}

// Mixup of one pixel on the fp32 0..255 values: the partner's inside the rectangle
__device__ __forceinline__ Rgb mixup_rgb(const Rgb& own, const Rgb& par, bool in, float wo, float wp) {
  Rgb r;
#pragma unroll
  for (int c = 0; c < 3; ++c) r.v[c] = in ? par.v[c] : fmaf(wo, own.v[c], wp * par.v[c]);
  return r;
}

// The mix operands of image b as a lane uses them: its own view and the partner's, whether its
// two pixels lie inside the cut rectangle, the weight of the own pixels outside it, and whether
// anything mixes at all (wave-uniform).
struct MixOps {
  View own, par;
  bool ina, inc;
  float wo;
  bool any;
};
__device__ __forceinline__ MixOps load_mix(const MixArgs& mix, const uint8_t* __restrict__ src, long img_bytes,
                                           uint32_t b, const View& own, int oy, int ox0, int ox1) {
  const int* rc = mix.rect + (long)b * 4;
  const int ry0 = rc[0], rx0 = rc[1], ry1 = rc[2], rx1 = rc[3];
  const float wo = mix.w_own[b];
  const int* pb = mix.pbox + (long)b * 5;
  const View par{src + (long)mix.pidx[b] * img_bytes, pb[0], pb[1], pb[2], pb[3], pb[4]};
  const bool iny = oy >= ry0 && oy < ry1;
  return MixOps{own, par, iny && ox0 >= rx0 && ox0 < rx1, iny && ox1 >= rx0 && ox1 < rx1, wo,
                wo != 1.f || (ry0 < ry1 && rx0 < rx1)};
}

// grid.x = B * nblk: workgroup (b, k) covers pixel pairs [k NT, (k+1) NT) of image b's S * P
// pairs (P = ceil(S / 2) pairs per output row).
//
// MIX: per output pixel, inside the rectangle the partner's sample; else, at w_own == 1, the own
// sample; else fma(w_own, own, (1 - w_own) partner) on the fp32 0..255 values (one rounding, to
// bf16, as without mixing). w_own, the rectangle and the partner's box and base are
// wave-uniform, so the three cases are scalar branches; the rectangle test is per lane and per
// pixel (a lane's two pixels can lie on either side of an edge):
//   * nothing to mix (w_own == 1, empty rectangle): the plain path, instruction for instruction;
//   * CutMix (w_own == 1): each pixel selects its view -- image base and box -- and samples once;
//   * Mixup: both pixels' taps of both views are in flight together, then the blend.
//
// ERASE: the R rectangles of image b are wave-uniform (scalar loads). All empty: fall through to
// the code above and below, as the non-erase instantiation runs it. Otherwise the rectangle test
// is per lane and per pixel; an erased pixel (and the dropped second pixel of the odd-S tail)
// issues no load, every other pixel samples as its mixing case says, one view_taps per pixel.
template <bool MIX, bool ERASE, class Mix>
__global__ void __launch_bounds__(NT)
crop_resize_norm_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx, const int* __restrict__ box,
                        u16* __restrict__ out, long img_bytes, int Ws, int S, int P, uint32_t nblk, FastDiv dP,
                        float inv2S, float m0, float m1, float m2, float s0, float s1, float s2, Mix mix) {
  const uint32_t b = blockIdx.x / nblk;
  const uint32_t p = (blockIdx.x - b * nblk) * NT + threadIdx.x;
  if (p >= (uint32_t)(S * P)) return;
  const int* bx = box + (long)b * 5;
  const long im = idx ? (long)idx[b] : (long)b;
  // 64-bit image base; offsets inside an image are 32-bit
  const View own{src + im * img_bytes, bx[0], bx[1], bx[2], bx[3], bx[4]};

  const int oy = (int)fdiv(p, dP);
  const int ox0 = 2 * ((int)p - oy * P);
  const bool pair = ox0 + 1 < S;
  const int ox1 = pair ? ox0 + 1 : ox0;  // odd-S tail: the second pixel is computed and dropped
  const int S2 = 2 * S;

  if constexpr (ERASE) {
    const EraseArgs* era;
    if constexpr (MIX) era = &mix.er; else era = &mix;
    const int R = era->R;
    const int* er = era->erect + (long)b * R * 4;
    // all eight slots at once, the ones past R reading rectangle R - 1 again: no loop, so these
    // scalar loads issue beside the box's and the decision costs one round trip, not one per slot
    bool any = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int* e = er + 4 * min(r, R - 1);
      const int ey0 = e[0], ex0 = e[1], ey1 = e[2], ex1 = e[3];
      any |= (ey0 < ey1) & (ex0 < ex1);
    }
    if (any) {
      bool ea = false, ec = false;
      for (int r = 0; r < R; ++r) {
        const int ey0 = er[4 * r], ex0 = er[4 * r + 1], ey1 = er[4 * r + 2], ex1 = er[4 * r + 3];
        const bool iny = oy >= ey0 && oy < ey1;
        ea |= iny && ox0 >= ex0 && ox0 < ex1;
        ec |= iny && ox1 >= ex0 && ox1 < ex1;
      }
      const uint32_t key = era->ekey[b];
      const int mode = era->mode;
      const uint32_t q = (uint32_t)(oy * S + ox0);
      const bool sa = !ea, sc = pair && !ec;  // the pixels that sample
      PixelOut a{0u, 0u}, c{0u, 0u};
      MixOps m{own, own, false, false, 1.f, false};
      if constexpr (MIX) m = load_mix(mix, src, img_bytes, b, own, oy, ox0, ox1);
      if (m.wo != 1.f) {
        Taps oa = view_taps<true>(sa, own, oy, ox0, Ws, S, S2, inv2S), oc = view_taps<true>(sc, own, oy, ox1, Ws, S, S2, inv2S);
        Taps qa = view_taps<true>(sa, m.par, oy, ox0, Ws, S, S2, inv2S), qc = view_taps<true>(sc, m.par, oy, ox1, Ws, S, S2, inv2S);
        asm volatile("" : "+v"(oa.p00), "+v"(oa.p01), "+v"(oa.p10), "+v"(oa.p11), "+v"(oc.p00), "+v"(oc.p01),
                          "+v"(oc.p10), "+v"(oc.p11), "+v"(qa.p00), "+v"(qa.p01), "+v"(qa.p10), "+v"(qa.p11),
                          "+v"(qc.p00), "+v"(qc.p01), "+v"(qc.p10), "+v"(qc.p11));
        const float wp = 1.f - m.wo;
        if (sa) a = finish(mixup_rgb(blend_taps(oa), blend_taps(qa), m.ina, m.wo, wp), m0, m1, m2, s0, s1, s2);
        if (sc) c = finish(mixup_rgb(blend_taps(oc), blend_taps(qc), m.inc, m.wo, wp), m0, m1, m2, s0, s1, s2);
      } else {
        Taps ta = view_taps<true>(sa, select_view(m.ina, m.par, own), oy, ox0, Ws, S, S2, inv2S);
        Taps tc = view_taps<true>(sc, select_view(m.inc, m.par, own), oy, ox1, Ws, S, S2, inv2S);
        // every load issued before the first use (the pins below, for the same reason)
        asm volatile("" : "+v"(ta.p00), "+v"(ta.p01), "+v"(ta.p10), "+v"(ta.p11), "+v"(tc.p00), "+v"(tc.p01),
                          "+v"(tc.p10), "+v"(tc.p11));
        if (sa) a = finish(blend_taps(ta), m0, m1, m2, s0, s1, s2);
        if (sc) c = finish(blend_taps(tc), m0, m1, m2, s0, s1, s2);
      }
      if (ea) a = erase_fill(key, q, mode);
      if (pair && ec) c = erase_fill(key, q + 1u, mode);
      store_pair(out, b, S, oy, ox0, pair, a, c);
      return;
    }
  }

  if constexpr (MIX) {
    const MixOps m = load_mix(mix, src, img_bytes, b, own, oy, ox0, ox1);
    if (m.any) {
      if (m.wo == 1.f) {
        Taps ta = view_taps<false>(true, select_view(m.ina, m.par, own), oy, ox0, Ws, S, S2, inv2S);
        Taps tc = view_taps<false>(true, select_view(m.inc, m.par, own), oy, ox1, Ws, S, S2, inv2S);
        // every load issued before the first use (the pin below, for the same reason)
        asm volatile("" : "+v"(ta.p00), "+v"(ta.p01), "+v"(ta.p10), "+v"(ta.p11), "+v"(tc.p00), "+v"(tc.p01),
                          "+v"(tc.p10), "+v"(tc.p11));
        store_pair(out, b, S, oy, ox0, pair, finish(blend_taps(ta), m0, m1, m2, s0, s1, s2),
                   finish(blend_taps(tc), m0, m1, m2, s0, s1, s2));
        return;
      }
      // Mixup: both pixels' taps of both views, 16 loads in flight
      Taps oa = view_taps<false>(true, own, oy, ox0, Ws, S, S2, inv2S), oc = view_taps<false>(true, own, oy, ox1, Ws, S, S2, inv2S);
      Taps qa = view_taps<false>(true, m.par, oy, ox0, Ws, S, S2, inv2S), qc = view_taps<false>(true, m.par, oy, ox1, Ws, S, S2, inv2S);
      asm volatile("" : "+v"(oa.p00), "+v"(oa.p01), "+v"(oa.p10), "+v"(oa.p11), "+v"(oc.p00), "+v"(oc.p01),
                        "+v"(oc.p10), "+v"(oc.p11), "+v"(qa.p00), "+v"(qa.p01), "+v"(qa.p10), "+v"(qa.p11),
                        "+v"(qc.p00), "+v"(qc.p01), "+v"(qc.p10), "+v"(qc.p11));
      const Rgb ova = blend_taps(oa), ovc = blend_taps(oc), pva = blend_taps(qa), pvc = blend_taps(qc);
      const float wp = 1.f - m.wo;
      store_pair(out, b, S, oy, ox0, pair, finish(mixup_rgb(ova, pva, m.ina, m.wo, wp), m0, m1, m2, s0, s1, s2),
                 finish(mixup_rgb(ovc, pvc, m.inc, m.wo, wp), m0, m1, m2, s0, s1, s2));
      return;
    }
  }

  // the plain path: one row computation shared by the lane's two pixels
  const Axis y = axis_taps(oy, own.h, S, S2, inv2S);
  const uint32_t row0 = (uint32_t)((own.y0 + y.i0) * Ws + own.x0), row1 = (uint32_t)((own.y0 + y.i1) * Ws + own.x0);
  const Axis xa = axis_taps(own.flip ? S - 1 - ox0 : ox0, own.w, S, S2, inv2S);
  const Axis xc = axis_taps(own.flip ? S - 1 - ox1 : ox1, own.w, S, S2, inv2S);
  const PixelOut a = finish(blend_taps(load_taps<false>(own.img, row0, row1, y, xa)), m0, m1, m2, s0, s1, s2);
  PixelOut c = finish(blend_taps(load_taps<false>(own.img, row0, row1, y, xc)), m0, m1, m2, s0, s1, s2);
  // pin the second pixel here: left alone, the compiler sinks its four loads into the `pair`
  // branch of the store, behind the first pixel's waits (half the loads in flight per lane)
  asm volatile("" : "+v"(c.lo), "+v"(c.hi));
  store_pair(out, b, S, oy, ox0, pair, a, c);
}

template <bool MIX, bool ERASE, class Mix>
int launch(const void* src, int Hs, int Ws, const int64_t* idx, const int* box, Mix mix, void* out, long B, int S,
           int Cp, const float* mean, const float* inv_std, hipStream_t st) {
  if (!src || !box || !out || !mean || !inv_std) return -1;
  if (B <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || Cp != 4) return -1;
  if (Hs > 32768 || Ws > 32768 || S > 16384) return -1;  // (2S+1) h fits an int
  const long img_bytes = (long)Hs * Ws * 3;
  if (img_bytes < 4 || img_bytes >= (1L << 31)) return -1;  // dword taps; 32-bit offsets in an image
  const int P = (S + 1) / 2;
  const long nblk = ((long)S * P + NT - 1) / NT;
  if (B * nblk > 0x7fffffffL) return -1;
  hipLaunchKernelGGL((crop_resize_norm_kernel<MIX, ERASE, Mix>), dim3((unsigned)(B * nblk)), dim3(NT), 0, st,
                     (const uint8_t*)src, idx, box, (u16*)out, img_bytes, Ws, S, P, (uint32_t)nblk,
                     make_fastdiv((uint32_t)P), 1.f / (float)(2 * S), mean[0], mean[1], mean[2], inv_std[0],
                     inv_std[1], inv_std[2], mix);
  PDT_RETURN_LAUNCH();
}
}  // namespace

// src: uint8 [n][Hs][Ws][3] (device); idx: int64 [B] source image of each output (device; null:
// output b reads image b); box: int32 [B][5] = y0, x0, h, w, flip (device); out: bf16
// [B][S][S][Cp], Cp = 4; mean / inv_std: 3 host floats. The boxes and indices are trusted (the
// loader validates them on the host before the upload).
PDT_API int pdt_crop_resize_norm_u8_bf16(const void* src, int Hs, int Ws, const int64_t* idx, const int* box, void* out,
                                         long B, int S, int Cp, const float* mean, const float* inv_std,
                                         hipStream_t st) {
  return launch<false, false>(src, Hs, Ws, idx, box, NoMix{}, out, B, S, Cp, mean, inv_std, st);
}

// The same with Mixup / CutMix (see the kernel): pidx int64 [B] the partner's source image, pbox
// int32 [B][5] the partner's own box and flip, rect int32 [B][4] = y0, x0, y1, x1 (half-open,
// inside [0, S]^2), w_own fp32 [B] in [0, 1]; all on the device and trusted like the boxes.
PDT_API int pdt_crop_resize_norm_mix_u8_bf16(const void* src, int Hs, int Ws, const int64_t* idx, const int* box,
                                             const int64_t* pidx, const int* pbox, const int* rect,
                                             const float* w_own, void* out, long B, int S, int Cp, const float* mean,
                                             const float* inv_std, hipStream_t st) {
  if (!pidx || !pbox || !rect || !w_own) return -1;
  return launch<true, false>(src, Hs, Ws, idx, box, MixArgs{pidx, pbox, rect, w_own}, out, B, S, Cp, mean, inv_std, st);
}

// Either of the two with Random Erasing (see the kernel). pidx, pbox, rect, w_own: all four null
// (no mixing) or all four set (mixing, as above). erect int32 [B][R][4] = y0, x0, y1, x1 (half-open,
// inside [0, S]^2; empty when y0 == y1 or x0 == x1), R in 1..8; ekey uint32 [B], the noise key of
// each output; emode 0 = const (+0), 1 = pixel (N(0, 1) per element). On the device and trusted
// like the boxes (data/packed.py: validate_erase).
PDT_API int pdt_crop_resize_norm_erase_u8_bf16(const void* src, int Hs, int Ws, const int64_t* idx, const int* box,
                                               const int64_t* pidx, const int* pbox, const int* rect,
                                               const float* w_own, const int* erect, int R, const void* ekey,
                                               int emode, void* out, long B, int S, int Cp, const float* mean,
                                               const float* inv_std, hipStream_t st) {
  const int nmix = (pidx != nullptr) + (pbox != nullptr) + (rect != nullptr) + (w_own != nullptr);
  if (nmix != 0 && nmix != 4) return -1;
  if (!erect || !ekey || R < 1 || R > 8 || (emode != 0 && emode != 1)) return -1;
  const EraseArgs er{erect, (const uint32_t*)ekey, R, emode};
  if (nmix == 0) return launch<false, true>(src, Hs, Ws, idx, box, er, out, B, S, Cp, mean, inv_std, st);
  MixEraseArgs me;
  me.pidx = pidx, me.pbox = pbox, me.rect = rect, me.w_own = w_own, me.er = er;
  return launch<true, true>(src, Hs, Ws, idx, box, me, out, B, S, Cp, mean, inv_std, st);
}
