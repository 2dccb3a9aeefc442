// fa_bwd_varlen_kernels.hip -- the backward over packed variable-length sequences (fa_bwd_varlen): the two bodies of fa_bwd_body.h in
// their varlen mode, for {f16, bf16} x head_dim {64, 128} x {causal, full}.
//
//   bwd_dq_varlen_kernel     one workgroup per (sequence, query head, 128 query rows up to max_seqlen_q)
//   bwd_dkdv_varlen_kernel   one workgroup per (sequence, key/value head, 128 keys up to max_seqlen_k); it visits the head's group of
//                            query heads in the dense order
//
// The host does not know the lengths: the grids are sized by max_seqlen, every block reads its sequence's two cu_seqlens pairs with
// scalar loads, clamps them as the forward does, and leaves in front of every barrier if it owns nothing. From LDS onwards the code is
// the dense kernels' (fa_bwd_kernels.hip), so the gradients of a sequence are bit for bit those fa_bwd_ex computes for it alone.
// A translation unit of its own: the dense file keeps exactly its kernels, and these are built with the same flags.
#include "fa_bwd_body.h"

namespace fa {

// Workgroups per CU the varlen kernels are compiled for: the dense kernels' (three at head_dim 64, two at 128). The run-time pitches and
// sequence bases live in scalar registers, and what the varlen arms do to stay inside the dense register caps without scratch (none at
// all, where the dense head_dim-128 dK/dV kernel parks 32 bytes) is noted where they do it (tests/test_varlen_bwd_isa.py).
constexpr int bwd_varlen_occ(int D) { return bwd_occ(D); }

#define FA_BWD_VARLEN 1
template <typename Tag, int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, bwd_varlen_occ(D)) void bwd_dq_varlen_kernel(BwdVarlenParams p) {
  constexpr bool PAD = false;  // head_dim 64 / 128 only
#include "fa_bwd_dq_body.inc"
}

template <typename Tag, int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, bwd_varlen_occ(D)) void bwd_dkdv_varlen_kernel(BwdVarlenParams p) {
  constexpr bool PAD = false;
#include "fa_bwd_dkdv_body.inc"
}
#undef FA_BWD_VARLEN

bool bwd_varlen_supported(int dtype, int D) { return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && (D == 64 || D == 128); }

hipError_t launch_bwd_varlen(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                             float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                             int total_k, int max_q, int max_k, int D, float scale, long long q_rs, long long q_hs, long long kv_rs,
                             long long kv_hs, int causal, int dtype, hipStream_t s) {
  BwdVarlenParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.d_o = d_o; p.lse = lse;
  p.dq = dq; p.dk = dk; p.dv = dv; p.delta = ws;
  p.B = B; p.H = H; p.N = max_q; p.D = D; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_hs; p.is_causal = causal;
  p.Hkv = Hkv; p.Nk = max_k; p.kv_batch_stride = 0; p.kv_head_stride = kv_hs;
  p.cu_q = cu_q; p.cu_k = cu_k; p.total_q = total_q; p.total_k = total_k; p.q_rs = q_rs; p.kv_rs = kv_rs;
  return with_tag(dtype, [&](auto tag) {
    return with_dim_causal<64, 128>(D, causal, [&](auto d, auto c) {
      return launch_bwd_pair(bwd_dq_varlen_kernel<decltype(tag), d(), c()>, bwd_dkdv_varlen_kernel<decltype(tag), d(), c()>, p, d(), s);
    });
  });
}

}  // namespace fa
