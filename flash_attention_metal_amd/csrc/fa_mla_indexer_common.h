// fa_mla_indexer_common.h -- what the indexer's kernels (fa_mla_indexer_kernel.hip, fa_mla_indexer_kv8_kernel.hip,
// fa_mla_indexer_select_split_kernel.hip) share on the device: a sequence's tokens and keys under fa_fwd_varlen_paged's clamps, the
// bottom-right causal rule, and the select kernels' workgroup scan and logit image.
#pragma once

#include "fa_mfma_common.h"

namespace fa {

// sequence b's tokens and keys, under fa_fwd_varlen_paged's clamps
struct IdxSeq {
  int sq, Lq, L;
};
__device__ __forceinline__ IdxSeq idx_seq(const int *cu_q, const int *seqlens, int b, int total_q, int max_q, int cap) {
  const int s = min(max(__builtin_amdgcn_readfirstlane(cu_q[b]), 0), total_q), e = min(max(__builtin_amdgcn_readfirstlane(cu_q[b + 1]), 0), total_q);
  return {s, min(max(e - s, 0), max_q), min(max(__builtin_amdgcn_readfirstlane(seqlens[b]), 0), cap)};
}
// keys token i of the sequence sees: the bottom-right causal rule
__device__ __forceinline__ int idx_visible(const IdxSeq &q, int i) { return min(max(q.L - q.Lq + i + 1, 0), q.L); }

// ---- what the select kernels (fa_mla_indexer_kernel.hip, fa_mla_indexer_select_split_kernel.hip) share: workgroups of 256 threads
constexpr int IDX_SEL_THREADS = 256;
// exclusive scan of x over the 256 threads of the workgroup, and the total; ws: four ints of LDS
__device__ __forceinline__ int idx_block_scan(int x, int &total, int *ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(incl, d, 64);
    if (lane >= d) incl += y;
  }
  if (lane == 63) ws[w] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < IDX_SEL_THREADS / 64; ++i) {
    const int s = ws[i];
    base += i < w ? s : 0;
    total += s;
  }
  __syncthreads();  // (ws is rewritten by the next scan)
  return base + incl - x;
}
// the order-preserving image of a logit: a > b as floats iff image(a) > image(b) as unsigned ints, -0 counted as +0
__device__ __forceinline__ unsigned idx_image(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace fa
