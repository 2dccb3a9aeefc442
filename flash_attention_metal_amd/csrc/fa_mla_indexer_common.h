// fa_mla_indexer_common.h -- what the indexer's kernels (fa_mla_indexer_kernel.hip, fa_mla_indexer_kv8_kernel.hip) share on the device:
// a sequence's tokens and keys under fa_fwd_varlen_paged's clamps, and the bottom-right causal rule.
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

}  // namespace fa
