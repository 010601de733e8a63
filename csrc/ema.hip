// Multi-tensor exponential moving average of the weights (one launch for every averaged tensor):
//
//   e <- e + w (p - e),  w = 1 - d, in fp32
//
// the form of torch.lerp(e, p, w) for w < 0.5: where p == e the result is e bit for bit, whatever
// w is (but for the sign of zero: e == p == -0 gives -0 + w (+0) = +0, as torch.lerp does).
// Optionally the bf16 shadow of each averaged tensor is written in the same pass (the copy
// the bf16 conv / GEMM kernels read), so a forward on the averaged weights casts nothing.
//
// Work list (csrc/optim_common.h): each workgroup walks chunks {tensor id, element offset,
// length} with a grid-stride loop and reads the tensor's pointers from a pointer table. A
// streaming pass: 12 bytes per element, 14 with the shadow.
//
// State: dev = [t, d, w] (fp32) in device memory. t is the number of updates done so far; a
// one-thread tick kernel ahead of the update in the same stream forms this update's decay d and
// weight w from t and then increments t, so eager and captured updates take the same path and a
// replayed HIP graph advances the warm-up on the device. t as fp32 is exact up to 2^24 updates
// (16.7 M; after that t + 1 == t, and the warm-up ramp is long past its cap).
#include "optim_common.h"

namespace {

// d = warmup ? min(decay, (1 + t) / (10 + t)) : decay;  w = 1 - d;  t += 1
__global__ void ema_tick_kernel(float* dev, float decay, int warmup) {
  if (threadIdx.x == 0) {
    const float t = dev[0];
    const float d = warmup ? fminf(decay, (1.f + t) / (10.f + t)) : decay;
    dev[1] = d;
    dev[2] = 1.f - d;
    dev[0] = t + 1.f;
  }
}

__global__ void ema_kernel(const Chunk* __restrict__ chunks, int nchunks, float* const* __restrict__ ema,
                           const float* const* __restrict__ src, u16* const* __restrict__ shadows,
                           const float* __restrict__ dev) {
  const float w = dev[2];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = chunks[c];
    float* e = ema[ch.tensor] + ch.offset;
    const float* p = src[ch.tensor] + ch.offset;
    u16* sh = role_ptr(shadows, ch.tensor, ch.offset);
    // 16-B vector path when both streams (and the shadow, 8-B) are aligned: 4 elements per
    // lane, both loads issued before the math
    const uintptr_t al = (uintptr_t)e | (uintptr_t)p;
    walk_chunk(
        ch.len, (al & 15) == 0 && (!sh || ((uintptr_t)sh & 7) == 0),
        [&](long j) {
          const f32x4 pv = reinterpret_cast<const f32x4*>(p)[j];
          f32x4 ev = reinterpret_cast<const f32x4*>(e)[j];
#pragma unroll
          for (int k = 0; k < 4; ++k) ev[k] = ev[k] + w * (pv[k] - ev[k]);
          reinterpret_cast<f32x4*>(e)[j] = ev;
          if (sh) store_shadow4(sh, j, ev);
        },
        [&](long i) {
          const float pi = p[i];
          float ei = e[i];
          ei = ei + w * (pi - ei);
          e[i] = ei;
          if (sh) sh[i] = f2bf(ei);
        });
  }
}

}  // namespace

// ema / src / shadows: device pointer tables (float*, const float*, bf16*) indexed by a chunk's
// tensor id; shadows, or any entry of it, may be null. dev = [t, d, w] (see above; required).
// Launches the tick, then the update that reads w from dev.
PDT_API int pdt_ema_update(const void* chunks, int nchunks, void* ema, const void* src, void* shadows, float* dev,
                           float decay, int warmup, hipStream_t st) {
  if (dev == nullptr) return -1;
  hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(64), 0, st, dev, decay, warmup);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for(nchunks)), dim3(NT), 0, st, (const Chunk*)chunks, nchunks,
                     (float* const*)ema, (const float* const*)src, (u16* const*)shadows, (const float*)dev);
  PDT_RETURN_LAUNCH();
}
