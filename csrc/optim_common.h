// Shared by the multi-tensor optimizer kernels (csrc/optim.hip, csrc/optim_layerwise.hip): the
// work list and how a workgroup walks one chunk of it.
//
// Work list: the host builds, once per parameter set, a device table of chunks {tensor id,
// element offset, length} and one pointer table per role (parameters, gradients, states, bf16
// shadows); workgroups of NT threads walk the chunks with a grid-stride loop.
#pragma once
#include "pdt_common.h"

namespace {

struct Chunk {
  int tensor;
  int pad;
  long offset;
  long len;
};

constexpr int NT = 256;

int grid_for(int n) { return n < 2048 ? (n < 1 ? 1 : n) : 2048; }

// a chunk's pointer for one role; the whole table and single entries of it may be null
template <typename T>
__device__ __forceinline__ T* role_ptr(T* const* table, int tensor, long offset) {
  return table ? (table[tensor] ? table[tensor] + offset : nullptr) : nullptr;
}

// walk one chunk: 4 elements per lane (16-B loads / stores) while `aligned`, scalar otherwise
// and for the tail
template <typename F4, typename F1>
__device__ __forceinline__ void walk_chunk(long len, bool aligned, F4 f4, F1 f1) {
  long i0 = 0;
  if (aligned) {
    const long n4 = len >> 2;
    for (long j = threadIdx.x; j < n4; j += NT) f4(j);
    i0 = n4 << 2;
  }
  for (long i = i0 + threadIdx.x; i < len; i += NT) f1(i);
}

// the bf16 shadow of parameters 4 j .. 4 j + 3 (sh 8-byte aligned)
__device__ __forceinline__ void store_shadow4(u16* sh, long j, f32x4 pv) {
  uint2 w;
  w.x = pack2bf(pv[0], pv[1]);
  w.y = pack2bf(pv[2], pv[3]);
  reinterpret_cast<uint2*>(sh)[j] = w;
}

}  // namespace
