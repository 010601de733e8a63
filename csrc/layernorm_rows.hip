// LayerNorm (bf16 in/out, fp32 statistics) for the row widths csrc/layernorm.hip does not
// cover: D % 8 == 0, 8 <= D <= 1016, D % 256 != 0 (ViT-Ti/S: 192 / 384; channels-last widths
// 96 / 192 / 384). Multiples of 256 stay with layernorm.hip.
//
// A row is D / 8 chunks of eight bf16 (16 bytes) and one lane owns one chunk per stream: one
// 16-byte load or store per chunk. A row is served by a group of G lanes and a wave serves 64 / G
// rows at once:
//     D   8 .. 128   G = 16, 1 chunk per lane, 4 rows per wave
//       136 .. 248   G = 32, 1 chunk per lane, 2 rows per wave
//       264 .. 504   G = 64, 1 chunk per lane, 1 row per wave
//       520 .. 1016  G = 64, 2 chunks per lane, 1 row per wave
// D is a run-time argument: a lane whose chunk index is >= D / 8, and every lane of a group whose
// row is past `rows`, loads nothing, contributes 0 to every sum and stores nothing. Group sums
// are row16_sum inside a DPP row, then xor16_reduce (G >= 32) and xor32_reduce (G = 64): no LDS
// and no ds_bpermute on the row path, and every lane of the wave reaches them (loads and stores
// are predicated, nothing returns early inside a wave that has a row).
// Backward: the same mapping, each workgroup walking row trips grid-stride; the column sums of
// (dy * xhat, dy) stay in registers over the trips, the groups of a wave are combined with the
// permlane swaps, the waves through LDS in wave order, and each workgroup writes one row of a
// [2][blocks][D] buffer that a fixed-order column-sum pass finishes (no atomics).
#include "pdt_common.h"

// every instantiation and flavour rounds as written (the drop-path flavours must reproduce the
// plain ones bit for bit): an fma is an explicit fmaf, nothing else is contracted
#pragma clang fp contract(off)

namespace {

constexpr int WPB = 4;  // waves per block

__device__ __forceinline__ void unpack8(const u32x4& w, float* f) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = lo_bf(w[k]);
    f[2 * k + 1] = hi_bf(w[k]);
  }
}
__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 w;
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = pack2bf(f[2 * k], f[2 * k + 1]);
  return w;
}
__device__ __forceinline__ void ldf8(const float* p, float* f) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = a[e];
    f[4 + e] = b[e];
  }
}

// sum over the G lanes of a group (G = 16, 32, 64; groups are aligned); every lane gets it
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  v = row16_sum(v);
  if constexpr (G >= 32) v = xor16_reduce(v, AddOp{});
  if constexpr (G == 64) v = xor32_reduce(v, AddOp{});
  return v;
}

// MODE 0: y = LN(x). MODE 1: xsum = bf16(x + r), y = LN(xsum). MODE 2 (stochastic depth): xsum =
// bf16(r + dscale[row / rps] * x). With several rows per wave the scale is a per-group value and
// a per-lane predicate on the branch loads: a dropped sample's branch is never loaded and its
// xsum is r's 16 bytes themselves, whatever the branch holds.
template <int G, int CPL, int MODE>
__global__ void __launch_bounds__(64 * WPB) lnr_fwd_kernel(const u16* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ b, u16* __restrict__ y,
                                                           float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                           int rows, int D, float invD, float eps,
                                                           const u16* __restrict__ radd, u16* __restrict__ xsum,
                                                           const float* __restrict__ dscale, int rps) {
  constexpr int RPW = 64 / G;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1);
  const int row0 = (blockIdx.x * WPB + (threadIdx.x >> 6)) * RPW;
  if (row0 >= rows) return;  // the whole wave: no lane of it has a row
  const int row = row0 + lane / G;
  const bool rok = row < rows;
  const int nch = D >> 3;
  bool act[CPL];
  long off[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int chunk = c * G + gl;
    act[c] = rok && chunk < nch;
    off[c] = (long)row * D + chunk * 8;
  }
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 xw[CPL], rw[CPL];
  float v[CPL][8];
  if constexpr (MODE == 2) {
    const float sc = rok ? dscale[row / rps] : 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) rw[c] = act[c] ? *reinterpret_cast<const u32x4*>(radd + off[c]) : zero;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      xw[c] = (act[c] && sc != 0.f) ? *reinterpret_cast<const u32x4*>(x + off[c]) : zero;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      float xv[8], r[8], o[8];
      unpack8(xw[c], xv);
      unpack8(rw[c], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf(sc, xv[e], r[e]);
      const u32x4 kept = pack8(o);
      u32x4 w;
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = sc != 0.f ? kept[k] : rw[c][k];  // dropped: r, bit for bit
      unpack8(w, v[c]);
      if (act[c]) *reinterpret_cast<u32x4*>(xsum + off[c]) = w;
    }
  } else if constexpr (MODE == 1) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      xw[c] = act[c] ? *reinterpret_cast<const u32x4*>(x + off[c]) : zero;
      rw[c] = act[c] ? *reinterpret_cast<const u32x4*>(radd + off[c]) : zero;
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      float xv[8], r[8], o[8];
      unpack8(xw[c], xv);
      unpack8(rw[c], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = xv[e] + r[e];
      const u32x4 w = pack8(o);
      unpack8(w, v[c]);
      if (act[c]) *reinterpret_cast<u32x4*>(xsum + off[c]) = w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < CPL; ++c) xw[c] = act[c] ? *reinterpret_cast<const u32x4*>(x + off[c]) : zero;
#pragma unroll
    for (int c = 0; c < CPL; ++c) unpack8(xw[c], v[c]);
  }
  // two-pass statistics in registers; a lane without a chunk holds zeros and subtracts a zero mean
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[c][e];
  const float mean = group_sum<G>(s) * invD;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const float mc = act[c] ? mean : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = v[c][e] - mc;
      q = fmaf(d, d, q);
    }
  }
  const float rstd = rsqrtf(fmaf(group_sum<G>(q), invD, eps));
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    if (act[c]) {
      const int col = (c * G + gl) * 8;
      float gg[8], bb[8], o[8];
      ldf8(g + col, gg);
      ldf8(b + col, bb);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = fmaf((v[c][e] - mean) * rstd, gg[e], bb[e]);
      *reinterpret_cast<u32x4*>(y + off[c]) = pack8(o);
    }
  }
  if (gl == 0 && rok) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
}

// dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat)) (+ addend), dxhat = dy * g.
// DP: also dyb = bf16(dscale[row / rps] * dx as stored), +0 selected on a dropped sample's rows.
// A trip is the WPB * 64 / G rows the workgroup serves at once; trips are walked grid-stride.
template <int G, int CPL, bool DP>
__global__ void __launch_bounds__(64 * WPB) lnr_bwd_kernel(const u16* __restrict__ dy, const u16* __restrict__ x,
                                                           const float* __restrict__ g,
                                                           const float* __restrict__ mean_in,
                                                           const float* __restrict__ rstd_in, u16* __restrict__ dx,
                                                           float* __restrict__ part, int rows, int D, float invD,
                                                           int trips, const u16* __restrict__ addend,
                                                           const float* __restrict__ dscale, int rps,
                                                           u16* __restrict__ dyb) {
  constexpr int RPW = 64 / G;
  constexpr int W = G * CPL * 8;  // columns the instantiation spans (>= D)
  __shared__ float red[2][WPB][W];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane & (G - 1);
  const int nch = D >> 3;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  float gv[CPL][8], dg[CPL][8], db[CPL][8];
  bool cok[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    cok[c] = c * G + gl < nch;
#pragma unroll
    for (int e = 0; e < 8; ++e) gv[c][e] = dg[c][e] = db[c][e] = 0.f;
    if (cok[c]) ldf8(g + (c * G + gl) * 8, gv[c]);  // gamma is per column: loaded once
  }
  for (int trip = blockIdx.x; trip < trips; trip += gridDim.x) {
    const int row = (trip * WPB + w) * RPW + lane / G;
    const bool rok = row < rows;
    u32x4 xw[CPL], dw[CPL], aw[CPL];
    long off[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool act = rok && cok[c];
      off[c] = (long)row * D + (c * G + gl) * 8;
      xw[c] = act ? *reinterpret_cast<const u32x4*>(x + off[c]) : zero;
      dw[c] = act ? *reinterpret_cast<const u32x4*>(dy + off[c]) : zero;
      aw[c] = (act && addend != nullptr) ? *reinterpret_cast<const u32x4*>(addend + off[c]) : zero;
    }
    const float mean = rok ? mean_in[row] : 0.f, rstd = rok ? rstd_in[row] : 0.f;
    float sc = 0.f;
    if constexpr (DP) sc = rok ? dscale[row / rps] : 0.f;
    float xh[CPL][8], gy[CPL][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      float xv[8], dv[8];
      unpack8(xw[c], xv);
      unpack8(dw[c], dv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // a lane without a chunk: dv = 0 and gamma = 0, so every term is 0
        xh[c][e] = (xv[e] - mean) * rstd;
        gy[c][e] = dv[e] * gv[c][e];
        s1 += gy[c][e];
        s2 += gy[c][e] * xh[c][e];
        dg[c][e] += dv[e] * xh[c][e];
        db[c][e] += dv[e];
      }
    }
    const float m1 = group_sum<G>(s1) * invD, m2 = group_sum<G>(s2) * invD;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      float ad[8], o[8];
      unpack8(aw[c], ad);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = rstd * (gy[c][e] - m1 - xh[c][e] * m2);
      if (addend != nullptr) {  // residual-branch gradient of the same tensor: dx += addend
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += ad[e];
      }
      const u32x4 ow = pack8(o);
      if (rok && cok[c]) *reinterpret_cast<u32x4*>(dx + off[c]) = ow;
      if constexpr (DP) {
        float st[8];
        unpack8(ow, st);
#pragma unroll
        for (int e = 0; e < 8; ++e) st[e] = sc != 0.f ? sc * st[e] : 0.f;
        if (rok && cok[c]) *reinterpret_cast<u32x4*>(dyb + off[c]) = pack8(st);
      }
    }
  }
  // the groups of a wave hold the same columns: combine them, then the waves through LDS
#pragma unroll
  for (int c = 0; c < CPL; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (G == 16) {
        dg[c][e] = xor16_reduce(dg[c][e], AddOp{});
        db[c][e] = xor16_reduce(db[c][e], AddOp{});
      }
      if constexpr (G <= 32) {
        dg[c][e] = xor32_reduce(dg[c][e], AddOp{});
        db[c][e] = xor32_reduce(db[c][e], AddOp{});
      }
    }
  if (lane < G) {
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[0][w][(c * G + gl) * 8 + e] = dg[c][e];
        red[1][w][(c * G + gl) * 8 + e] = db[c][e];
      }
  }
  __syncthreads();
  for (int col = threadIdx.x; col < D; col += 64 * WPB) {
    float a = 0.f, bsum = 0.f;
#pragma unroll
    for (int k = 0; k < WPB; ++k) {
      a += red[0][k][col];
      bsum += red[1][k][col];
    }
    part[(long)blockIdx.x * D + col] = a;
    part[(long)(gridDim.x + blockIdx.x) * D + col] = bsum;
  }
}

// out[c] (+)= sum_r part[r][c] for the two halves (dgamma, dbeta): the equal of layernorm.hip's
// column-sum pass (64 columns x 16 row groups, 8 rows per trip, combined through LDS in a fixed
// order), kept here so that file's code objects stay as they are.
constexpr int CS_RG = 16;
__global__ void __launch_bounds__(64 * CS_RG) lnr_colsum_kernel(const float* __restrict__ part, float* __restrict__ dg,
                                                                float* __restrict__ db, int R, int D, int accumulate) {
  __shared__ float sa[CS_RG][64], sb[CS_RG][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float a = 0.f, b = 0.f;
  if (c < D) {
    int r = rg;
    for (; r + 7 * CS_RG < R; r += 8 * CS_RG) {
      float x[8], y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        x[u] = part[(long)(r + u * CS_RG) * D + c];
        y[u] = part[(long)(R + r + u * CS_RG) * D + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        a += x[u];
        b += y[u];
      }
    }
    for (; r < R; r += CS_RG) {
      a += part[(long)r * D + c];
      b += part[(long)(R + r) * D + c];
    }
  }
  sa[rg][cl] = a;
  sb[rg][cl] = b;
  __syncthreads();
  if (rg == 0 && c < D) {
    a = 0.f;
    b = 0.f;
#pragma unroll
    for (int k = 0; k < CS_RG; ++k) {
      a += sa[k][cl];
      b += sb[k][cl];
    }
    dg[c] = accumulate ? dg[c] + a : a;
    db[c] = accumulate ? db[c] + b : b;
  }
}

}  // namespace

// instantiation for width D: 1 G=16, 2 G=32, 3 G=64, 4 G=64 with two chunks per lane; 0: not
// covered (multiples of 256 belong to layernorm.hip)
static int lnr_inst(int D) {
  if (D < 8 || D > 1016 || D % 8 != 0 || D % 256 == 0) return 0;
  return D <= 128 ? 1 : D <= 248 ? 2 : D <= 504 ? 3 : 4;
}

template <int I>
struct LnrGeom {
  static constexpr int G = I == 1 ? 16 : I == 2 ? 32 : 64;
  static constexpr int CPL = I == 4 ? 2 : 1;
};

static int lnr_rows_per_trip(int inst) { return WPB * (inst == 1 ? 4 : inst == 2 ? 2 : 1); }

static int lnr_fwd_launch(const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, int rows,
                          int D, float eps, const void* r, void* xsum, const float* scale, int rps, hipStream_t st) {
  const int inst = lnr_inst(D);
  if (!inst || rows < 1) return -1;
  const int rpt = lnr_rows_per_trip(inst);
  dim3 grid((rows + rpt - 1) / rpt), blk(64 * WPB);
  pdt_dispatch<1, 4>(inst, [&](auto n) {
    using Geo = LnrGeom<decltype(n)::value>;
    auto kern = scale ? lnr_fwd_kernel<Geo::G, Geo::CPL, 2>
                      : (r ? lnr_fwd_kernel<Geo::G, Geo::CPL, 1> : lnr_fwd_kernel<Geo::G, Geo::CPL, 0>);
    hipLaunchKernelGGL(kern, grid, blk, 0, st, (const u16*)x, g, b, (u16*)y, mean, rstd, rows, D, 1.f / D, eps,
                       (const u16*)r, (u16*)xsum, scale, rps);
  });
  PDT_RETURN_LAUNCH();
}

// y = LayerNorm(x) over rows of width D (bf16), mean / rstd per row (fp32); -1 with nothing
// launched for a width outside this file's set.
PDT_API int pdt_lnr_fwd(const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, int rows,
                        int D, float eps, hipStream_t st) {
  return lnr_fwd_launch(x, g, b, y, mean, rstd, rows, D, eps, nullptr, nullptr, nullptr, 1, st);
}

// LayerNorm of xsum = bf16(x + r) (written to xsum); with scale (rows / rows_per_sample floats,
// each 0 or 1/keep): xsum = bf16(r + scale[row / rows_per_sample] * x), and where the scale is 0
// x is not read and xsum holds r's bits.
PDT_API int pdt_lnr_add_fwd(const void* x, const void* r, void* xsum, const float* g, const float* b, void* y,
                            float* mean, float* rstd, int rows, int D, float eps, const float* scale,
                            int rows_per_sample, hipStream_t st) {
  if (!r || !xsum || (scale && rows_per_sample < 1)) return -1;
  return lnr_fwd_launch(x, g, b, y, mean, rstd, rows, D, eps, r, xsum, scale, rows_per_sample, st);
}

// workgroups of pdt_lnr_bwd (rows of its [2][blocks][D] partial buffer): one per row trip, at
// most 1024; 0 for a width outside this file's set
PDT_API int pdt_lnr_bwd_blocks(int rows, int D) {
  const int inst = lnr_inst(D);
  if (!inst || rows < 1) return 0;
  const int rpt = lnr_rows_per_trip(inst);
  const int trips = (rows + rpt - 1) / rpt;
  return trips < 1024 ? trips : 1024;
}

// LayerNorm backward from the saved row statistics: dx (+ addend, optional), dg / db (= or += with
// accumulate). scale with dyb (both or neither): the backward of pdt_lnr_add_fwd's scaled sum --
// dx is the gradient of r, dyb = bf16(scale * dx as stored) that of x, +0 on dropped samples.
// part: 2 * pdt_lnr_bwd_blocks(rows, D) * D floats.
PDT_API int pdt_lnr_bwd(const void* dy, const void* x, const float* g, const float* mean, const float* rstd, void* dx,
                        void* dyb, float* dg, float* db, float* part, int rows, int D, int accumulate,
                        const void* addend, const float* scale, int rows_per_sample, hipStream_t st) {
  const int inst = lnr_inst(D);
  if (!inst || rows < 1 || (scale != nullptr) != (dyb != nullptr) || (scale && rows_per_sample < 1)) return -1;
  const int rpt = lnr_rows_per_trip(inst);
  const int trips = (rows + rpt - 1) / rpt;
  const int blocks = pdt_lnr_bwd_blocks(rows, D);
  pdt_dispatch<1, 4>(inst, [&](auto n) {
    using Geo = LnrGeom<decltype(n)::value>;
    auto kern = scale ? lnr_bwd_kernel<Geo::G, Geo::CPL, true> : lnr_bwd_kernel<Geo::G, Geo::CPL, false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * WPB), 0, st, (const u16*)dy, (const u16*)x, g, mean, rstd,
                       (u16*)dx, part, rows, D, 1.f / D, trips, (const u16*)addend, scale, rows_per_sample,
                       (u16*)dyb);
  });
  const int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(lnr_colsum_kernel, dim3((D + 63) / 64), dim3(64 * CS_RG), 0, st, part, dg, db, blocks, D,
                     accumulate);
  PDT_RETURN_LAUNCH();
}
