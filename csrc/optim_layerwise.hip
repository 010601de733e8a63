// Layer-wise adaptive optimizers (LARS, LAMB) with on-device gradient-norm clipping, and the
// deterministic multi-tensor L2 norm they are built on.
//
// Same work list as csrc/optim.hip (csrc/optim_common.h): a 24-byte Chunk {tensor, pad, offset,
// len} table, one pointer table per role, workgroups of 256 threads walking chunks grid-stride.
// Two more device tables, built by the host once per parameter set:
//   chunk_begin[n_tensors + 1]  a tensor's chunks are consecutive: [chunk_begin[t], chunk_begin[t + 1])
//   flags[n_tensors]            bit 0: layer-wise adaptation and weight decay apply
//
// Norms: a sum-of-squares pass writes one fp32 partial per (chunk, role) -- lanes reduced with
// warp_sum, the four waves through LDS in a fixed order, no atomics -- and a one-workgroup
// finalize sums each tensor's partials in chunk order (fp64) and the tensors in tensor order
// into the global sum. Everything stays in device memory, so a HIP graph replays it, and the
// result depends only on the data and its alignment: two runs are bitwise equal.
//
//   norms[role * n_tensors + t]   per-tensor L2 norms (fp32)
//   glob                          4 floats: [0..1] the running global sum of squares (one
//                                 double), [2] the global gradient norm, [3] the clip
//                                 coefficient min(1, max_grad_norm / (gnorm + 1e-6))
//
// All arithmetic is fp32 on fp32 masters; the bf16 shadow of each parameter is written in the
// pass that updates it, as sgd_kernel does.
#include "optim_common.h"

namespace {

constexpr int NW = NT / 64;

// workgroup sums of two per-lane values in a fixed order: lanes by warp_sum, then the four
// waves left to right; thread 0 stores them to out[0] (and out[1] when `two`). Every thread of
// the workgroup must call it (barriers); `red` may be reused right after it returns.
__device__ __forceinline__ void block_sum2(float a, float b, bool two, float (*red)[NW], float* out) {
  a = warp_sum(a);
  b = warp_sum(b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    if (two) out[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
  __syncthreads();
}

__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// partials[c][0] = sum a^2 over chunk c, partials[c][1] = sum b^2 (b optional)
__global__ void sumsq_kernel(const Chunk* __restrict__ chunks, int nchunks, const float* const* __restrict__ a,
                             const float* const* __restrict__ b, float* __restrict__ partials) {
  __shared__ float red[2][NW];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    const float* pa = a[ch.tensor] + ch.offset;
    const float* pb = b ? b[ch.tensor] + ch.offset : nullptr;
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
    // (gradients can be unaligned views into DDP's buckets)
    const bool aligned = (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
    walk_chunk(
        ch.len, aligned,
        [&](long j) {
          const f32x4 va = reinterpret_cast<const f32x4*>(pa)[j];
          sa += va * va;
          if (pb) {
            const f32x4 vb = reinterpret_cast<const f32x4*>(pb)[j];
            sb += vb * vb;
          }
        },
        [&](long i) {
          const float x = pa[i];
          sa[0] += x * x;
          if (pb) {
            const float y = pb[i];
            sb[0] += y * y;
          }
        });
    block_sum2(sum4(sa), sum4(sb), pb != nullptr, red, partials + 2 * (long)c);
  }
}

// One workgroup. Per tensor: norms[r][t] = sqrt(sum of its partials, in chunk order). With
// glob and grole >= 0, role grole's per-tensor sums are added in tensor order to the running
// global sum (restarted from 0 when start_zero) and the norm / clip coefficient rewritten:
// the launches of several param groups chain through glob in stream order.
__global__ void norm_finalize_kernel(const float* __restrict__ partials, const int* __restrict__ chunk_begin, int nt,
                                     int nroles, int grole, float* __restrict__ norms, float* glob, int start_zero,
                                     float max_grad_norm) {
  __shared__ double tile[NT];
  const bool global = glob != nullptr && grole >= 0;
  double acc = 0.0;
  if (global && !start_zero) acc = *reinterpret_cast<const double*>(glob);
  for (int t0 = 0; t0 < nt; t0 += NT) {
    const int t = t0 + threadIdx.x;
    double gs = 0.0;
    if (t < nt) {
      const int c0 = chunk_begin[t], c1 = chunk_begin[t + 1];
      for (int r = 0; r < nroles; ++r) {
        double s = 0.0;
        for (int c = c0; c < c1; ++c) s += (double)partials[2 * (long)c + r];
        norms[(long)r * nt + t] = (float)sqrt(s);
        if (r == grole) gs = s;
      }
    }
    if (global) {
      tile[threadIdx.x] = gs;
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = nt - t0 < NT ? nt - t0 : NT;
        for (int i = 0; i < n; ++i) acc += tile[i];
      }
      __syncthreads();
    }
  }
  if (global && threadIdx.x == 0) {
    *reinterpret_cast<double*>(glob) = acc;
    const float gn = (float)sqrt(acc);
    glob[2] = gn;
    glob[3] = max_grad_norm > 0.f ? fminf(1.f, max_grad_norm / (gn + 1e-6f)) : 1.f;
  }
}

// LARS: SGD-momentum with a per-tensor trust ratio. g' = clip g, wn = |w|, gn = clip |g|:
//   adapted:  q = (wn > 0 && gn > 0) ? trust wn / (gn + wd wn + eps) : 1;  d = q (g' + wd w)
//   excluded: d = g'
//   buf = momentum buf + d;  d = nesterov ? d + momentum buf : buf;  w -= lr d
// The host creates momentum buffers zeroed, so a tensor's first step gives buf = d with no
// first-step argument (which a replayed graph could not change).
__global__ void lars_kernel(const Chunk* __restrict__ chunks, int nchunks, float* const* __restrict__ params,
                            const float* const* __restrict__ grads, float* const* __restrict__ bufs,
                            u16* const* __restrict__ shadows, const int* __restrict__ flags,
                            const float* __restrict__ norms, int nt, const float* __restrict__ glob, float lr,
                            float momentum, float wd, int nesterov, float trust, float eps,
                            const float* __restrict__ dev) {
  if (dev != nullptr) lr = dev[0];  // capturable: the lr a replayed graph must not freeze
  const float clip = glob ? glob[3] : 1.f;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    const int t = ch.tensor;
    float* p = params[t] + ch.offset;
    const float* g = grads[t] + ch.offset;
    float* b = role_ptr(bufs, t, ch.offset);
    u16* sh = role_ptr(shadows, t, ch.offset);
    const bool hb = b != nullptr;
    float q = 1.f, wdt = 0.f;
    if (flags[t] & 1) {
      const float wn = norms[t], gn = clip * norms[(long)nt + t];
      wdt = wd;
      if (wn > 0.f && gn > 0.f) q = trust * wn / (gn + wd * wn + eps);
    }
    // one element: returns the new parameter, updates the momentum buffer value in place
    auto upd = [&](float gi, float pi, float& bi) {
      float d = q * (clip * gi + wdt * pi);
      if (hb) {
        bi = momentum * bi + d;
        d = nesterov ? d + momentum * bi : bi;
      }
      return pi - lr * d;
    };
    const uintptr_t al = (uintptr_t)p | (uintptr_t)g | (uintptr_t)b;
    walk_chunk(
        ch.len, (al & 15) == 0 && ((uintptr_t)sh & 7) == 0,
        [&](long j) {
          const f32x4 gv = reinterpret_cast<const f32x4*>(g)[j];
          f32x4 pv = reinterpret_cast<const f32x4*>(p)[j];
          f32x4 bv = hb ? reinterpret_cast<const f32x4*>(b)[j] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float be = bv[e];
            pv[e] = upd(gv[e], pv[e], be);
            bv[e] = be;
          }
          reinterpret_cast<f32x4*>(p)[j] = pv;
          if (hb) reinterpret_cast<f32x4*>(b)[j] = bv;
          if (sh) store_shadow4(sh, j, pv);
        },
        [&](long i) {
          float bi = hb ? b[i] : 0.f;
          const float pi = upd(g[i], p[i], bi);
          if (hb) b[i] = bi;
          p[i] = pi;
          if (sh) sh[i] = f2bf(pi);
        });
  }
}

// LAMB's update direction from the stored moments: both stages evaluate exactly this
__device__ __forceinline__ float lamb_u(float m, float v, float w, float bc1, float bc2, float eps, float wdt) {
  return (m / bc1) / (sqrtf(v / bc2) + eps) + wdt * w;
}

// capturable LAMB: t += 1 and the bias corrections of the new t (fp64 pow, once), ahead of
// stage 1 in the same stream. dev = [lr, t, bc1, bc2]
__global__ void lamb_tick_kernel(float* dev, double b1, double b2) {
  if (threadIdx.x == 0) {
    const float t = dev[1] + 1.f;
    dev[1] = t;
    dev[2] = (float)(1.0 - pow(b1, (double)t));
    dev[3] = (float)(1.0 - pow(b2, (double)t));
  }
}

// LAMB stage 1: m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g'^2 (g' = clip g; omb1 / omb2 are
// 1 - b1 / 1 - b2 rounded from the host's doubles: 1.f - 0.999f is off by 1.3e-5), and the
// per-chunk partials of |u|^2 (role 0) and |w|^2 (role 1), u = lamb_u(m, v, w) with the
// weight decay only on adapted tensors. u is not stored: stage 2 recomputes it.
__global__ void lamb_stage1_kernel(const Chunk* __restrict__ chunks, int nchunks,
                                   const float* const* __restrict__ params, const float* const* __restrict__ grads,
                                   float* const* __restrict__ exp_avg, float* const* __restrict__ exp_avg_sq,
                                   const int* __restrict__ flags, float* __restrict__ partials,
                                   const float* __restrict__ glob, float b1, float b2, float omb1, float omb2,
                                   float eps, float wd, float bc1, float bc2, const float* __restrict__ dev) {
  __shared__ float red[2][NW];
  if (dev != nullptr) {
    bc1 = dev[2];
    bc2 = dev[3];
  }
  const float clip = glob ? glob[3] : 1.f;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    const int t = ch.tensor;
    const float* p = params[t] + ch.offset;
    const float* g = grads[t] + ch.offset;
    float* m = exp_avg[t] + ch.offset;
    float* v = exp_avg_sq[t] + ch.offset;
    const float wdt = (flags[t] & 1) ? wd : 0.f;
    f32x4 su = {0.f, 0.f, 0.f, 0.f}, sw = {0.f, 0.f, 0.f, 0.f};
    // one element: updates the moments in place, returns u
    auto upd = [&](float gi, float pi, float& mi, float& vi) {
      gi *= clip;
      mi = b1 * mi + omb1 * gi;
      vi = b2 * vi + omb2 * gi * gi;
      return lamb_u(mi, vi, pi, bc1, bc2, eps, wdt);
    };
    const uintptr_t al = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
    walk_chunk(
        ch.len, (al & 15) == 0,
        [&](long j) {
          const f32x4 gv = reinterpret_cast<const f32x4*>(g)[j];
          const f32x4 pv = reinterpret_cast<const f32x4*>(p)[j];
          f32x4 mv = reinterpret_cast<const f32x4*>(m)[j];
          f32x4 vv = reinterpret_cast<const f32x4*>(v)[j];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float me = mv[e], ve = vv[e];
            const float u = upd(gv[e], pv[e], me, ve);
            mv[e] = me;
            vv[e] = ve;
            su[e] += u * u;
          }
          sw += pv * pv;
          reinterpret_cast<f32x4*>(m)[j] = mv;
          reinterpret_cast<f32x4*>(v)[j] = vv;
        },
        [&](long i) {
          float mi = m[i], vi = v[i];
          const float pi = p[i];
          const float u = upd(g[i], pi, mi, vi);
          m[i] = mi;
          v[i] = vi;
          su[0] += u * u;
          sw[0] += pi * pi;
        });
    block_sum2(sum4(su), sum4(sw), true, red, partials + 2 * (long)c);
  }
}

// LAMB stage 2: r = (adapted && wn > 0 && un > 0) ? wn / un : 1;  w -= lr r u
// (norms role 0 = |u|, role 1 = |w|, from stage 1's partials)
__global__ void lamb_stage2_kernel(const Chunk* __restrict__ chunks, int nchunks, float* const* __restrict__ params,
                                   const float* const* __restrict__ exp_avg,
                                   const float* const* __restrict__ exp_avg_sq, u16* const* __restrict__ shadows,
                                   const int* __restrict__ flags, const float* __restrict__ norms, int nt, float lr,
                                   float eps, float wd, float bc1, float bc2, const float* __restrict__ dev) {
  if (dev != nullptr) {
    lr = dev[0];
    bc1 = dev[2];
    bc2 = dev[3];
  }
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    const int t = ch.tensor;
    float* p = params[t] + ch.offset;
    const float* m = exp_avg[t] + ch.offset;
    const float* v = exp_avg_sq[t] + ch.offset;
    u16* sh = role_ptr(shadows, t, ch.offset);
    float r = 1.f, wdt = 0.f;
    if (flags[t] & 1) {
      const float un = norms[t], wn = norms[(long)nt + t];
      wdt = wd;
      if (wn > 0.f && un > 0.f) r = wn / un;
    }
    const float step = lr * r;
    const uintptr_t al = (uintptr_t)p | (uintptr_t)m | (uintptr_t)v;
    walk_chunk(
        ch.len, (al & 15) == 0 && ((uintptr_t)sh & 7) == 0,
        [&](long j) {
          f32x4 pv = reinterpret_cast<const f32x4*>(p)[j];
          const f32x4 mv = reinterpret_cast<const f32x4*>(m)[j];
          const f32x4 vv = reinterpret_cast<const f32x4*>(v)[j];
#pragma unroll
          for (int e = 0; e < 4; ++e) pv[e] -= step * lamb_u(mv[e], vv[e], pv[e], bc1, bc2, eps, wdt);
          reinterpret_cast<f32x4*>(p)[j] = pv;
          if (sh) store_shadow4(sh, j, pv);
        },
        [&](long i) {
          const float pi = p[i] - step * lamb_u(m[i], v[i], p[i], bc1, bc2, eps, wdt);
          p[i] = pi;
          if (sh) sh[i] = f2bf(pi);
        });
  }
}

}  // namespace

// Per-chunk sums of squares of one or two roles (b may be null): partials[2 c + role].
PDT_API int pdt_sumsq_chunks(const void* chunks, int nchunks, const void* a, const void* b, float* partials,
                             hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (const float* const*)a, (const float* const*)b, partials);
  PDT_RETURN_LAUNCH();
}

// Per-tensor norms from the partials; with glob and grole in [0, nroles), role grole also goes
// into the global gradient norm / clip coefficient (see the header comment for glob's layout).
PDT_API int pdt_norm_finalize(const float* partials, const int* chunk_begin, int n_tensors, int nroles, int grole,
                              float* norms, float* glob, int start_zero, float max_grad_norm, hipStream_t st) {
  if (nroles < 1 || nroles > 2 || grole >= nroles || n_tensors < 0) return -1;
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(NT), 0, st, partials, chunk_begin, n_tensors, nroles, grole,
                     norms, glob, start_zero, max_grad_norm);
  PDT_RETURN_LAUNCH();
}

// norms: role 0 = |w|, role 1 = |g| (unclipped); glob (optional) supplies the clip coefficient;
// dev (optional, capturable) = [lr].
PDT_API int pdt_lars_step(const void* chunks, int nchunks, void* params, const void* grads, void* bufs, void* shadows,
                          const int* flags, const float* norms, int n_tensors, const float* glob, float lr,
                          float momentum, float wd, int nesterov, float trust, float eps, const float* dev,
                          hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(lars_kernel, dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (float* const*)params, (const float* const*)grads, (float* const*)bufs, (u16* const*)shadows,
                     flags, norms, n_tensors, glob, lr, momentum, wd, nesterov, trust, eps, dev);
  PDT_RETURN_LAUNCH();
}

// dev = [lr, t, bc1, bc2]: t += 1 and the bias corrections for it, on the device
PDT_API int pdt_lamb_tick(float* dev, double b1, double b2, hipStream_t st) {
  if (dev == nullptr) return -1;
  hipLaunchKernelGGL(lamb_tick_kernel, dim3(1), dim3(64), 0, st, dev, b1, b2);
  PDT_RETURN_LAUNCH();
}

PDT_API int pdt_lamb_stage1(const void* chunks, int nchunks, const void* params, const void* grads, void* exp_avg,
                            void* exp_avg_sq, const int* flags, float* partials, const float* glob, float b1, float b2,
                            float omb1, float omb2, float eps, float wd, float bc1, float bc2, const float* dev,
                            hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(lamb_stage1_kernel, dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (const float* const*)params, (const float* const*)grads, (float* const*)exp_avg,
                     (float* const*)exp_avg_sq, flags, partials, glob, b1, b2, omb1, omb2, eps, wd, bc1, bc2,
                     dev);
  PDT_RETURN_LAUNCH();
}

PDT_API int pdt_lamb_stage2(const void* chunks, int nchunks, void* params, const void* exp_avg,
                            const void* exp_avg_sq, void* shadows, const int* flags, const float* norms,
                            int n_tensors, float lr, float eps, float wd, float bc1, float bc2, const float* dev,
                            hipStream_t st) {
  if (nchunks <= 0) return 0;
  hipLaunchKernelGGL(lamb_stage2_kernel, dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (float* const*)params, (const float* const*)exp_avg, (const float* const*)exp_avg_sq,
                     (u16* const*)shadows, flags, norms, n_tensors, lr, eps, wd, bc1, bc2, dev);
  PDT_RETURN_LAUNCH();
}
