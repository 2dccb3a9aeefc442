// fa_bwd_window_kernels.hip -- the backward over packed variable-length sequences under a sliding window (fa_bwd_varlen_window): the two
// bodies of fa_bwd_body.h in their window mode (FA_BWD_WINDOW = 1 on top of the varlen mode), for {f16, bf16} x head_dim {64, 128}.
//
//   bwd_dq_window_kernel     one workgroup per (sequence, query head, 128 query rows): it walks the key tiles of window_key_range of its
//                            rows only, each wave skips tiles outside its own 32 rows' bounds, the mask has two sides
//   bwd_dkdv_window_kernel   one workgroup per (sequence, key/value head, 128 keys): per query head of the group it walks the query tiles
//                            of window_query_range of its keys only; keys no query sees store their zero accumulators
//
// Both bounds are run-time scalars the host has made non-negative (BwdWindowParams). From LDS onwards the code is the dense kernels'
// (fa_bwd_kernels.hip): under bounds that never bind a sequence's gradients are bit for bit those of fa_bwd_varlen.
// A translation unit of its own: the dense and the varlen file keep exactly their kernels, and these are built with the same flags.
#include "fa_bwd_body.h"

namespace fa {

// the varlen kernels' occupancy: three workgroups per CU at head_dim 64, two at 128 (tests/test_window_bwd_isa.py)
constexpr int bwd_window_occ(int D) { return bwd_occ(D); }

#define FA_BWD_VARLEN 1
#undef FA_BWD_WINDOW
#define FA_BWD_WINDOW 1
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, bwd_window_occ(D)) void bwd_dq_window_kernel(BwdWindowParams p) {
  constexpr bool PAD = false;    // head_dim 64 / 128 only
  constexpr bool CAUSAL = true;  // the block order of the masked kernels; every mask expression has a window arm of its own
#include "fa_bwd_dq_body.inc"
}

template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, bwd_window_occ(D)) void bwd_dkdv_window_kernel(BwdWindowParams p) {
  constexpr bool PAD = false;
  constexpr bool CAUSAL = true;
#include "fa_bwd_dkdv_body.inc"
}
#undef FA_BWD_WINDOW
#define FA_BWD_WINDOW 0
#undef FA_BWD_VARLEN

hipError_t launch_bwd_varlen_window(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                                    float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                                    int total_k, int max_q, int max_k, int D, float scale, long long q_rs, long long q_hs, long long kv_rs,
                                    long long kv_hs, int wl, int wr, int dtype, hipStream_t s) {
  BwdWindowParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.d_o = d_o; p.lse = lse;
  p.dq = dq; p.dk = dk; p.dv = dv; p.delta = ws;
  p.B = B; p.H = H; p.N = max_q; p.D = D; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_hs; p.is_causal = 1;
  p.Hkv = Hkv; p.Nk = max_k; p.kv_batch_stride = 0; p.kv_head_stride = kv_hs;
  p.cu_q = cu_q; p.cu_k = cu_k; p.total_q = total_q; p.total_k = total_k; p.q_rs = q_rs; p.kv_rs = kv_rs;
  p.wl = wl; p.wr = wr;
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(D, [&](auto d) {
      return launch_bwd_pair(bwd_dq_window_kernel<decltype(tag), d()>, bwd_dkdv_window_kernel<decltype(tag), d()>, p, d(), s);
    });
  });
}

}  // namespace fa
