// fa_sink_kernels.hip -- the sinks' gradient of fa_bwd_varlen_sink (include/fa_mi355.h, "Attention sinks").
//
// The sink is one more term in every row's softmax that carries no value, so with p_i = exp(sinks[h] - lse[h, i]) its weight in row i
//     d loss / d sinks[h] = sum_i p_i (0 - delta[h, i]) = -sum_i exp(sinks[h] - lse[h, i]) delta[h, i],   delta = rowsum(dO o O),
// over the query tokens i a sequence OWNS. lse is the forward's (it contains the sink) and delta is what the dQ kernel has just left in
// the workspace: this kernel is launched behind the dQ / dK/dV pair on the same stream and reads both, nothing else.
//
//   dsink_kernel   one workgroup of DSINK_THREADS threads per query head. It walks cu_seqlens_q with the clamps of the dQ kernel (entries
//                  to [0, total_q], a non-increasing pair is length 0, a length stops at max_seqlen_q): tokens owned by nobody and rows
//                  past the clamp hold whatever the workspace held before the call and are never read. Thread t adds rows t, t + T, ...
//                  of every sequence in order, then the T partial sums meet in a fixed binary tree in LDS: no atomics, the same bits on
//                  every run. A dead row (no visible key: lse = sink, O = 0) adds exp(0) . 0 = 0.
// The grid is the head count: host scalars only, so the call stays graph-capturable. A translation unit of its own: the backward files
// keep exactly their kernels.
#include "fa_common.h"

namespace fa {

constexpr int DSINK_THREADS = 1024;
constexpr int DSINK_UNROLL = 4;  // rows per thread and trip

__global__ __launch_bounds__(DSINK_THREADS) void dsink_kernel(const float *__restrict__ sinks, const float *__restrict__ lse,
                                                              const float *__restrict__ delta, float *__restrict__ dsinks,
                                                              const int *__restrict__ cu_q, int B, int total_q, int max_q) {
  __shared__ float part[DSINK_THREADS];
  const int h = blockIdx.x, t = threadIdx.x;
  const float sink = sinks[h];
  const float *lh = lse + (long long)h * total_q, *dh = delta + (long long)h * total_q;
  float acc = 0.0f;
  for (int b = 0; b < B; ++b) {
    const int sq = min(max(cu_q[b], 0), total_q), eq = min(max(cu_q[b + 1], 0), total_q);
    const int LQ = min(max(eq - sq, 0), max_q);
    // four rows per trip, their eight loads in flight together; the additions keep their order: rows t, t + 1024, t + 2048, ...
    // (64-bit row index: the last trip looks up to 4096 rows past a length that may sit just under 2^31)
    for (long long i = t; i < LQ; i += DSINK_UNROLL * DSINK_THREADS) {
      float x[DSINK_UNROLL], d[DSINK_UNROLL];
#pragma unroll
      for (int u = 0; u < DSINK_UNROLL; ++u) {
        const long long r = i + u * DSINK_THREADS;
        x[u] = r < LQ ? lh[sq + r] : 0.0f;
        d[u] = r < LQ ? dh[sq + r] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < DSINK_UNROLL; ++u)
        if (i + u * DSINK_THREADS < LQ) acc += expf(sink - x[u]) * d[u];
    }
  }
  part[t] = acc;
  __syncthreads();
  for (int w = DSINK_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) dsinks[h] = -part[0];
}

hipError_t launch_dsink(const float *sinks, const float *lse, const float *delta, float *dsinks, const int *cu_q, int B, int H, int total_q,
                        int max_q, hipStream_t s) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(dsink_kernel, dim3(H), dim3(DSINK_THREADS), 0, s, sinks, lse, delta, dsinks, cu_q, B, total_q, max_q);
  return hipGetLastError();
}

}  // namespace fa
