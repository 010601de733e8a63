// Streaming evaluation statistics: one pass over a batch of logits that scores every row (its
// loss and the rank of its target) and adds the batch into a few device scalars, so a validation
// pass keeps no logits and gathers nothing.
//
// rows   : one wave per row, 4 rows per 256-thread workgroup. x[t] is read once (the row index is
//          wave-uniform, so the target and x[t] come through scalar loads); one pass then forms
//          the online-softmax (m, s), the row sum (label smoothing) and the two counts
//            gt = #{j : x[j] > x[t]},  eqb = #{j < t : x[j] == x[t]}
//          with 16-byte loads where the row's first element is 16-byte aligned (decided per row:
//          a row stride that is no multiple of 16 bytes alternates) and scalar loads otherwise
//          and for the tail. rank = gt + eqb is the target's position in a stable descending sort
//          (0 iff torch.argmax returns t; -0 == +0). A row with a NaN logit, or a target outside
//          [0, V), gets rank = V; the latter also loss = 0, like xent_fwd_kernel.
//          loss: cross-entropy  lse - (1-eps) x[t] - eps mean(x)  (xent_fwd_kernel's formula), or
//          NLL on log-probabilities, -x[t].
// reduce : one workgroup: loss_rows summed in a fixed order in fp64, rows with rank < min(k, V)
//          counted for every k (a row of rank V is never correct, so k >= V counts exactly the
//          valid rows), out-of-range targets counted; thread 0 ADDS them into the accumulators
//          with a plain read-modify-write -- launches on one stream serialise, no atomics, the
//          result is deterministic.
#include "pdt_common.h"

namespace {

constexpr int EVAL_MAX_K = 8;
struct EvalKs {
  int nk;
  int k[EVAL_MAX_K];
};

struct RowAcc {
  float m = -INFINITY, s = 0.f, sx = 0.f;
  int gt = 0, eqb = 0, nan = 0;
};

// One column into a lane's state. The online softmax is xent_fwd_kernel's, edge cases included: a
// -inf logit is absorbed (exp(-inf - m) = 0) once the lane has seen a finite value, but as a
// lane's FIRST column it gives exp(-inf - -inf) = NaN, so a row with masked (-inf) classes can
// score a NaN loss here exactly where the training loss does; the rank counts are not affected.
template <bool NLL>
__device__ __forceinline__ void eval_add(RowAcc& a, float v, long j, float xt, long t) {
  a.gt += v > xt;
  a.eqb += (v == xt) & (j < t);
  a.nan |= v != v;
  if (!NLL) {
    a.sx += v;
    if (v > a.m) {
      a.s = a.s * __expf(a.m - v) + 1.f;
      a.m = v;
    } else {
      a.s += __expf(v - a.m);
    }
  }
}

template <bool BF16, bool NLL>
__global__ void __launch_bounds__(256) eval_rows_kernel(const void* __restrict__ logits, long ld,
                                                        const long* __restrict__ target,
                                                        float* __restrict__ loss_rows, int* __restrict__ rank, int B,
                                                        int V, float eps) {
  typedef typename std::conditional<BF16, u16, float>::type T;
  constexpr int VEC = BF16 ? 8 : 4;  // elements of a 16-byte load
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (row >= B) return;
  const T* __restrict__ x = reinterpret_cast<const T*>(logits) + (long)row * ld;
  const long t = target[row];
  const bool valid = t >= 0 && t < V;
  float xt = 0.f;
  if (valid) {
    if constexpr (BF16) xt = bf2f(x[t]);
    else xt = x[t];
  }
  RowAcc a;
  long body = 0;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    body = (long)(V / VEC) * VEC;
    for (long c = (long)lane * VEC; c < body; c += 64 * VEC) {
      if constexpr (BF16) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(x + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          eval_add<NLL>(a, lo_bf(w[e]), c + 2 * e, xt, t);
          eval_add<NLL>(a, hi_bf(w[e]), c + 2 * e + 1, xt, t);
        }
      } else {
        const f32x4 w = *reinterpret_cast<const f32x4*>(x + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) eval_add<NLL>(a, w[e], c + e, xt, t);
      }
    }
  }
  for (long j = body + lane; j < V; j += 64) {
    float v;
    if constexpr (BF16) v = bf2f(x[j]);
    else v = x[j];
    eval_add<NLL>(a, v, j, xt, t);
  }
  const int above = warp_sum_i(a.gt + a.eqb);
  const bool any_nan = __ballot(a.nan != 0) != 0;
  float loss;
  if constexpr (NLL) {
    loss = -xt;
  } else {
    const float M = warp_max(a.m);  // (a lane without a column holds -inf, s = 0)
    const float S = warp_sum(a.m == -INFINITY ? 0.f : a.s * __expf(a.m - M));
    const float sx = warp_sum(a.sx);
    loss = M + __logf(S) - (1.f - eps) * xt - eps * (sx / V);
  }
  if (lane == 0) {
    loss_rows[row] = valid ? loss : 0.f;
    rank[row] = (valid && !any_nan) ? above : V;
  }
}

__global__ void __launch_bounds__(256) eval_reduce_kernel(const float* __restrict__ loss_rows,
                                                          const int* __restrict__ rank,
                                                          const long* __restrict__ target, int B, int V,
                                                          const EvalKs ks, double* __restrict__ loss_sum,
                                                          long* __restrict__ counts) {
  __shared__ double dred[256];
  __shared__ int ired[1 + EVAL_MAX_K][256];
  const int tid = threadIdx.x;
  double a = 0.0;
  int c[1 + EVAL_MAX_K] = {};
  for (long i = tid; i < B; i += 256) {
    a += (double)loss_rows[i];
    const int r = rank[i];
    const long t = target[i];
    c[0] += (t < 0) | (t >= V);
#pragma unroll
    for (int e = 0; e < EVAL_MAX_K; ++e) c[1 + e] += (e < ks.nk) & (r < min(ks.k[e], V));
  }
  dred[tid] = a;
#pragma unroll
  for (int e = 0; e <= EVAL_MAX_K; ++e) ired[e][tid] = c[e];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      dred[tid] += dred[tid + o];
#pragma unroll
      for (int e = 0; e <= EVAL_MAX_K; ++e) ired[e][tid] += ired[e][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    loss_sum[0] += dred[0];
    counts[0] += B;
    counts[1] += ired[0][0];
    for (int e = 0; e < ks.nk; ++e) counts[2 + e] += ired[1 + e][0];
  }
}

}  // namespace

// kind: 0 = cross-entropy with label smoothing eps, 1 = NLL on log-probabilities (eps unused).
// ks: nk <= 8 values k >= 1 in HOST memory (they travel to the kernel by value). loss_sum: one
// double, counts: 2 + nk int64 (rows, out-of-range targets, correct at each k) -- both added to.
PDT_API int pdt_eval_stats(const void* logits, int bf16, long ld, const long* target, int kind, float eps,
                           const int* ks, int nk, float* loss_rows, int* rank, double* loss_sum, long* counts, int B,
                           int V, hipStream_t st) {
  if (!logits || !target || !loss_rows || !rank || !loss_sum || !counts || B <= 0 || V <= 0 || ld < V) return -1;
  if (nk < 0 || nk > EVAL_MAX_K || (nk > 0 && !ks) || (kind != 0 && kind != 1)) return -1;
  EvalKs k{};
  k.nk = nk;
  for (int e = 0; e < nk; ++e) {
    if (ks[e] < 1) return -1;
    k.k[e] = ks[e];
  }
  const dim3 blk(256), grd((unsigned)((B + 3L) / 4));
  const bool nll = kind == 1;
#define PDT_EVAL_ROWS(BF, NL) \
  hipLaunchKernelGGL((eval_rows_kernel<BF, NL>), grd, blk, 0, st, logits, ld, target, loss_rows, rank, B, V, eps)
  if (bf16) {
    if (nll) PDT_EVAL_ROWS(true, true);
    else PDT_EVAL_ROWS(true, false);
  } else {
    if (nll) PDT_EVAL_ROWS(false, true);
    else PDT_EVAL_ROWS(false, false);
  }
#undef PDT_EVAL_ROWS
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(256), 0, st, loss_rows, rank, target, B, V, k, loss_sum,
                     counts);
  PDT_RETURN_LAUNCH();
}
