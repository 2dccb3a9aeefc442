// fa_bwd_softcap_kernels.hip -- the backward over packed variable-length sequences under a sliding window and a logit cap
// (fa_bwd_varlen_softcap): the two bodies of fa_bwd_body.h in their softcap mode (FA_BWD_SOFTCAP = 1 on top of the window mode), for
// {f16, bf16} x head_dim {64, 128}.
//
//   bwd_dq_softcap_kernel     the windowed dQ kernel over capped scores softcap . tanh(scale . s / softcap)
//   bwd_dkdv_softcap_kernel   the windowed dK/dV kernel likewise
//
// The pre-scaled operand (Q~ / K~) carries 2 log2(e) scale / softcap: the matrix core delivers the argument of the one exponential tanh
// needs, t = 1 - 2 / (1 + 2^y). The score chain starts from zero; the row's -lse.log2e is applied behind tanh, P = exp2(fma(t, C, -lse2))
// with C = softcap . log2(e), and dS = P (dP - delta) (1 - t^2). The final multiplies by scale, delta and every write rule are the
// windowed kernels'. A translation unit of its own: the other backward files keep exactly their kernels; built with their flags.
#include "fa_bwd_body.h"

namespace fa {

// the windowed kernels' occupancy: three workgroups per CU at head_dim 64, two at 128 (tests/test_softcap_isa.py)
constexpr int bwd_softcap_occ(int D) { return bwd_occ(D); }

#define FA_BWD_VARLEN 1
#undef FA_BWD_WINDOW
#define FA_BWD_WINDOW 1
#undef FA_BWD_SOFTCAP
#define FA_BWD_SOFTCAP 1
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, bwd_softcap_occ(D)) void bwd_dq_softcap_kernel(BwdSoftcapParams p) {
  constexpr bool PAD = false;    // head_dim 64 / 128 only
  constexpr bool CAUSAL = true;  // the block order of the masked kernels; every mask expression has a window arm of its own
#include "fa_bwd_dq_body.inc"
}

template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, bwd_softcap_occ(D)) void bwd_dkdv_softcap_kernel(BwdSoftcapParams p) {
  constexpr bool PAD = false;
  constexpr bool CAUSAL = true;
#include "fa_bwd_dkdv_body.inc"
}
#undef FA_BWD_SOFTCAP
#define FA_BWD_SOFTCAP 0
#undef FA_BWD_WINDOW
#define FA_BWD_WINDOW 0
#undef FA_BWD_VARLEN

hipError_t launch_bwd_varlen_softcap(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                                     float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                                     int total_k, int max_q, int max_k, int D, float scale, long long q_rs, long long q_hs, long long kv_rs,
                                     long long kv_hs, int wl, int wr, float softcap, int dtype, hipStream_t s) {
  BwdSoftcapParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.d_o = d_o; p.lse = lse;
  p.dq = dq; p.dk = dk; p.dv = dv; p.delta = ws;
  p.B = B; p.H = H; p.N = max_q; p.D = D; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_hs; p.is_causal = 1;
  p.Hkv = Hkv; p.Nk = max_k; p.kv_batch_stride = 0; p.kv_head_stride = kv_hs;
  p.cu_q = cu_q; p.cu_k = cu_k; p.total_q = total_q; p.total_k = total_k; p.q_rs = q_rs; p.kv_rs = kv_rs;
  p.wl = wl; p.wr = wr; p.softcap = softcap; p.cap_log2 = softcap * LOG2E;
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(D, [&](auto d) {
      return launch_bwd_pair(bwd_dq_softcap_kernel<decltype(tag), d()>, bwd_dkdv_softcap_kernel<decltype(tag), d()>, p, d(), s);
    });
  });
}

}  // namespace fa
