// Multi-tensor fused optimizer steps (one launch for every parameter tensor).
// Reference: the torch.optim.Adam(amsgrad) step of the reference project (config/config.json,
// "optimizer"; stepped once per batch in trainer/trainer.py); SGD-momentum is the ResNet recipe.
//
// Work list (csrc/optim_common.h): each workgroup walks chunks {tensor id, element offset,
// length} with a grid-stride loop and reads the tensor's pointers from a pointer table.
// fp32 master params / grads / states; optionally a bf16 shadow copy of each
// param is written in the same pass (the copy the bf16 conv/GEMM kernels read),
// so no separate cast kernel runs per step.
#include <cfloat>

#include "optim_common.h"

namespace {

// The GUARD instantiations (the ..._step3 entry points) take two more kernel arguments, the
// pack G = (const float* glob, int skip_nonfinite): glob[2] is the global gradient norm before
// clipping and glob[3] the clip coefficient (csrc/optim_layerwise.hip: norm_finalize_kernel),
// both read once per workgroup into scalar registers. Each gradient is multiplied by
// clip * grad_scale, and with skip_nonfinite a norm that is inf or NaN ends the workgroup
// before its first load of a tensor, so that launch stores nothing. Without GUARD the pack is
// empty and the kernels are what they were before the flag existed, instruction for
// instruction (profiles/optim_clip.txt).
//
// Folds the clip coefficient into grad_scale; false: decline the step.
__device__ __forceinline__ bool guard_scale(float& grad_scale, const float* __restrict__ glob, int skip_nonfinite) {
  if (skip_nonfinite && !(glob[2] <= FLT_MAX)) return false;
  grad_scale *= glob[3];
  return true;
}

// SGD (torch semantics): g += wd*p; buf = mom*buf + (1-damp)*g (buf = g on
// first step); g = nesterov ? g + mom*buf : buf; p -= lr*g
template <bool GUARD, typename... G>
__global__ void sgd_kernel(const Chunk* __restrict__ chunks, int nchunks, float* const* __restrict__ params,
                           const float* const* __restrict__ grads, float* const* __restrict__ bufs,
                           u16* const* __restrict__ shadows, float lr, float momentum, float dampening, float wd,
                           int nesterov, int first, float grad_scale, const float* __restrict__ dev, G... guard) {
  if constexpr (GUARD) {
    if (!guard_scale(grad_scale, guard...)) return;
  }
  if (dev != nullptr) lr = dev[0];  // capturable: the lr a replayed graph must not freeze
  // one element: returns the new parameter, updates the momentum buffer value in place
  auto upd = [&](float gi, float pi, float& bi, bool has_b) {
    gi *= grad_scale;
    if (wd != 0.f) gi += wd * pi;
    if (momentum != 0.f && has_b) {
      bi = first ? gi : momentum * bi + (1.f - dampening) * gi;
      gi = nesterov ? gi + momentum * bi : bi;
    }
    return pi - lr * gi;
  };
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    float* p = params[ch.tensor] + ch.offset;
    const float* g = grads[ch.tensor] + ch.offset;
    float* b = role_ptr(bufs, ch.tensor, ch.offset);
    u16* sh = role_ptr(shadows, ch.tensor, ch.offset);
    const bool hb = b != nullptr;
    // 16-B vector path when every stream is aligned (gradients can be unaligned views
    // into DDP's buckets): 4 elements per lane, all loads issued before the math
    const uintptr_t al = (uintptr_t)p | (uintptr_t)g | (hb ? (uintptr_t)b : 0);
    walk_chunk(
        ch.len, (al & 15) == 0 && (!sh || ((uintptr_t)sh & 7) == 0),
        [&](long j) {
          const f32x4 gv = reinterpret_cast<const f32x4*>(g)[j];
          f32x4 pv = reinterpret_cast<const f32x4*>(p)[j];
          f32x4 bv = hb ? reinterpret_cast<const f32x4*>(b)[j] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float be = bv[e];
            pv[e] = upd(gv[e], pv[e], be, hb);
            bv[e] = be;
          }
          reinterpret_cast<f32x4*>(p)[j] = pv;
          if (hb && momentum != 0.f) reinterpret_cast<f32x4*>(b)[j] = bv;
          if (sh) store_shadow4(sh, j, pv);
        },
        [&](long i) {
          float bi = hb ? b[i] : 0.f;
          const float pi = upd(g[i], p[i], bi, hb);
          if (hb && momentum != 0.f) b[i] = bi;
          p[i] = pi;
          if (sh) sh[i] = f2bf(pi);
        });
  }
}

// Adam / AdamW (decoupled=1), optional AMSGrad. bc1 = 1-b1^t, bc2 = 1-b2^t.
template <bool GUARD, typename... G>
__global__ void adam_kernel(const Chunk* __restrict__ chunks, int nchunks, float* const* __restrict__ params,
                            const float* const* __restrict__ grads, float* const* __restrict__ exp_avg,
                            float* const* __restrict__ exp_avg_sq, float* const* __restrict__ max_sq,
                            u16* const* __restrict__ shadows, float lr, float b1, float b2, float eps, float wd,
                            int decoupled, float bc1, float bc2, float grad_scale, const float* __restrict__ dev,
                            G... guard) {
  if constexpr (GUARD) {
    if (!guard_scale(grad_scale, guard...)) return;
  }
  if (dev != nullptr) {  // capturable: lr and the step count t live in device memory
    lr = dev[0];
    bc1 = 1.f - powf(b1, dev[1]);
    bc2 = 1.f - powf(b2, dev[1]);
  }
  const float step_size = lr / bc1;
  const float inv_sqrt_bc2 = 1.f / sqrtf(bc2);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    float* p = params[ch.tensor] + ch.offset;
    const float* g = grads[ch.tensor] + ch.offset;
    float* m = exp_avg[ch.tensor] + ch.offset;
    float* v = exp_avg_sq[ch.tensor] + ch.offset;
    float* vm = max_sq ? max_sq[ch.tensor] + ch.offset : nullptr;
    u16* sh = role_ptr(shadows, ch.tensor, ch.offset);
    for (long i = threadIdx.x; i < ch.len; i += NT) {
      float gi = g[i] * grad_scale;
      float pi = p[i];
      if (wd != 0.f) {
        if (decoupled) pi *= (1.f - lr * wd);
        else gi += wd * pi;
      }
      float mi = b1 * m[i] + (1.f - b1) * gi;
      float vi = b2 * v[i] + (1.f - b2) * gi * gi;
      m[i] = mi;
      v[i] = vi;
      float vv = vi;
      if (vm) {
        vv = fmaxf(vm[i], vi);
        vm[i] = vv;
      }
      float denom = sqrtf(vv) * inv_sqrt_bc2 + eps;
      pi -= step_size * mi / denom;
      p[i] = pi;
      if (sh) sh[i] = f2bf(pi);
    }
  }
}

// capturable Adam: t += 1 on the device, ahead of the step kernel in the same stream
__global__ void opt_tick_kernel(float* dev) {
  if (threadIdx.x == 0) dev[1] += 1.f;
}

// The tick under skip_nonfinite, making the step kernels' test: on a finite norm t += 1 (dev
// may be null: nothing counts steps on the device), otherwise *skipped += 1 (skipped may be
// null: another launch of this step counts it). One thread.
__global__ void opt_tick_guard_kernel(float* dev, const float* __restrict__ glob, int* skipped) {
  if (threadIdx.x != 0) return;
  if (glob[2] <= FLT_MAX) {
    if (dev != nullptr) dev[1] += 1.f;
  } else if (skipped != nullptr) {
    *skipped += 1;
  }
}

}  // namespace

PDT_API int pdt_chunk_struct_size() { return (int)sizeof(Chunk); }

// dev (optional, "capturable"): [lr] for SGD, [lr, t] for Adam in device memory, read by the
// kernels instead of the lr / bias-correction arguments, so a HIP graph that captured the step
// replays it with the current learning rate and step count (the host rewrites dev[0] when the
// lr changes; Adam's t is incremented on the device by opt_tick_kernel when tick != 0).
PDT_API int pdt_sgd_step2(const void* chunks, int nchunks, void* params, const void* grads, void* bufs, void* shadows,
                          float lr, float momentum, float dampening, float wd, int nesterov, int first,
                          float grad_scale, const float* dev, hipStream_t st) {
  hipLaunchKernelGGL((sgd_kernel<false>), dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (float* const*)params, (const float* const*)grads, (float* const*)bufs,
                     (u16* const*)shadows, lr, momentum, dampening, wd, nesterov, first, grad_scale, dev);
  PDT_RETURN_LAUNCH();
}

// pdt_sgd_step2 with the global gradient norm and clip coefficient read from glob (guard_scale).
// skipped (optional, with skip_nonfinite): a one-thread launch adds 1 to it when the step is
// declined; the caller passes it with one launch per optimizer step.
PDT_API int pdt_sgd_step3(const void* chunks, int nchunks, void* params, const void* grads, void* bufs, void* shadows,
                          float lr, float momentum, float dampening, float wd, int nesterov, int first,
                          float grad_scale, const float* dev, const float* glob, int skip_nonfinite, int* skipped,
                          hipStream_t st) {
  if (glob == nullptr) return -1;
  if (skip_nonfinite && skipped != nullptr) {
    hipLaunchKernelGGL(opt_tick_guard_kernel, dim3(1), dim3(64), 0, st, (float*)nullptr, glob, skipped);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((sgd_kernel<true, const float*, int>), dim3(grid_for(nchunks)), dim3(NT), 0, st,
                     (const Chunk*)chunks, nchunks, (float* const*)params, (const float* const*)grads,
                     (float* const*)bufs, (u16* const*)shadows, lr, momentum, dampening, wd, nesterov, first,
                     grad_scale, dev, glob, skip_nonfinite);
  PDT_RETURN_LAUNCH();
}

PDT_API int pdt_adam_step2(const void* chunks, int nchunks, void* params, const void* grads, void* exp_avg,
                           void* exp_avg_sq, void* max_sq, void* shadows, float lr, float b1, float b2, float eps,
                           float wd, int decoupled, float bc1, float bc2, float grad_scale, float* dev, int tick,
                           hipStream_t st) {
  if (tick && dev == nullptr) return -1;
  if (tick) {
    hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, st, dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((adam_kernel<false>), dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (float* const*)params, (const float* const*)grads, (float* const*)exp_avg,
                     (float* const*)exp_avg_sq, (float* const*)max_sq, (u16* const*)shadows, lr, b1, b2, eps, wd,
                     decoupled, bc1, bc2, grad_scale, (const float*)dev);
  PDT_RETURN_LAUNCH();
}

// pdt_adam_step2 with the global gradient norm and clip coefficient read from glob (see
// guard_scale). With skip_nonfinite the tick is the guarded one: t does not advance on a declined
// step, and skipped (optional, passed with one launch per optimizer step) counts it.
PDT_API int pdt_adam_step3(const void* chunks, int nchunks, void* params, const void* grads, void* exp_avg,
                           void* exp_avg_sq, void* max_sq, void* shadows, float lr, float b1, float b2, float eps,
                           float wd, int decoupled, float bc1, float bc2, float grad_scale, float* dev, int tick,
                           const float* glob, int skip_nonfinite, int* skipped, hipStream_t st) {
  if (glob == nullptr || (tick && dev == nullptr)) return -1;
  if (skip_nonfinite && (tick || skipped != nullptr)) {
    hipLaunchKernelGGL(opt_tick_guard_kernel, dim3(1), dim3(64), 0, st, tick ? dev : (float*)nullptr, glob,
                       skipped);
  } else if (tick) {
    hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, st, dev);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((adam_kernel<true, const float*, int>), dim3(grid_for(nchunks)), dim3(NT), 0, st,
                     (const Chunk*)chunks, nchunks, (float* const*)params, (const float* const*)grads,
                     (float* const*)exp_avg, (float* const*)exp_avg_sq, (float* const*)max_sq, (u16* const*)shadows, lr, b1, b2, eps, wd,
                     decoupled, bc1, bc2, grad_scale, (const float*)dev, glob, skip_nonfinite);
  PDT_RETURN_LAUNCH();
}
