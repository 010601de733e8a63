// Stochastic depth (drop-path): the per-sample branch scales of one training forward.
//
//   scale[j][b] = u(seed, step, j, sample0 + b) >= p[j] ? inv_keep[j] : 0
//
// for branch j (2i: block i's attention branch, 2i + 1: its MLP branch) and sample b of this
// rank's batch; sample0 = rank * B, so a sample's draw depends on its global index alone and not
// on how the batch is split over ranks. The LayerNorm-add kernels (csrc/layernorm.hip, DP) read
// one row of the table.
//
// The draw -- defined here, mirrored in torch by ops/drop_path.py (drop_path_hash) -- is
// counter-based, in the style of hash32 in csrc/misc.hip (the same mixer), all in uint32:
//
//   k0 = hash32(seed ^ step * 0x9E3779B9)
//   k1 = hash32(k0 ^ j * 0x85EBCA6B)
//   h  = hash32(k1 ^ sample * 0xC2B2AE35)
//   u  = (h >> 8) / 2^24        (exact in fp32, in [0, 1))
//
// and the sample is kept iff u >= p[j], compared in fp32. p and inv_keep = 1 / (1 - p) come from
// the host as fp32, so nothing is divided here.
//
// State: state = [seed, step] (two 32-bit words) in device memory. A one-thread tick launch behind
// the fill in the same stream increments step, so an eager forward and a replayed HIP graph
// advance the counter alike, with no host sync and no atomics (stream order puts the increment
// after the fill's reads).
#include "pdt_common.h"

namespace {
constexpr int NT = 256;

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

__global__ void __launch_bounds__(NT) drop_path_scales_kernel(float* __restrict__ scale,
                                                              const uint32_t* __restrict__ state,
                                                              const float* __restrict__ p,
                                                              const float* __restrict__ inv_keep, int n_branches,
                                                              int B, uint32_t sample0) {
  const uint32_t k0 = hash32(state[0] ^ state[1] * 0x9E3779B9u);
  const long total = (long)n_branches * B;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int j = (int)(i / B);
    const int b = (int)(i - (long)j * B);
    const uint32_t k1 = hash32(k0 ^ (uint32_t)j * 0x85EBCA6Bu);
    const uint32_t h = hash32(k1 ^ (sample0 + (uint32_t)b) * 0xC2B2AE35u);
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
    scale[i] = u >= p[j] ? inv_keep[j] : 0.f;
  }
}

__global__ void drop_path_tick_kernel(uint32_t* state) {
  if (threadIdx.x == 0) state[1] = state[1] + 1u;
}

}  // namespace

// scale: [n_branches][B] floats (written); state: [seed, step] (step incremented after the fill);
// p / inv_keep: n_branches floats each; sample0: the global index of this rank's first sample.
PDT_API int pdt_drop_path_scales(float* scale, int* state, const float* p, const float* inv_keep, int n_branches,
                                 int B, long sample0, hipStream_t st) {
  if (!scale || !state || !p || !inv_keep || n_branches < 1 || B < 1) return -1;
  const long total = (long)n_branches * B;
  long blocks = (total + NT - 1) / NT;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(drop_path_scales_kernel, dim3((int)blocks), dim3(NT), 0, st, scale, (const uint32_t*)state, p,
                     inv_keep, n_branches, B, (uint32_t)sample0);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(drop_path_tick_kernel, dim3(1), dim3(64), 0, st, (uint32_t*)state);
  PDT_RETURN_LAUNCH();
}
