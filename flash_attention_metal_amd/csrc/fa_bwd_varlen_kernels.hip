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

// dQ first: it leaves delta in the workspace for the dK/dV kernel (same stream). p.N / p.Nk hold max_seqlen_q / max_seqlen_k: blocks
// past the end of their sequence return at once.
template <typename Tag, int D, bool CAUSAL>
static hipError_t launch_bwd_varlen_one(const BwdVarlenParams &p, hipStream_t s) {
  constexpr int BTILE = BN * D * 2;
  const int nBq = (p.N + BM - 1) / BM, nBk = (p.Nk + BM - 1) / BM;
  const size_t smem_dq = 4 * bwd_sub_dq(D) * BTILE, smem_kv = 4 * bwd_sub_kv(D) * BTILE + 2 * 2 * bwd_sub_kv(D) * BN * 4;  // as launch_bwd_one
  auto kq = bwd_dq_varlen_kernel<Tag, D, CAUSAL>;
  auto kk = bwd_dkdv_varlen_kernel<Tag, D, CAUSAL>;
  hipError_t e = hipSuccess;
  if (smem_kv > 48 * 1024) e = set_dyn_lds_once((const void *)kk, (int)smem_kv);
  if (e != hipSuccess) return e;
  if (smem_dq > 48 * 1024) {
    e = set_dyn_lds_once((const void *)kq, (int)smem_dq);
    if (e != hipSuccess) return e;
  }
  (void)hipGetLastError();  // do not report an older sticky error as this launch's
  hipLaunchKernelGGL(kq, dim3(nBq * p.B * p.H), dim3(NTHREADS), smem_dq, s, p);
  hipLaunchKernelGGL(kk, dim3(nBk * p.B * p.Hkv), dim3(NTHREADS), smem_kv, s, p);
  return hipGetLastError();
}

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
  auto go = [&](auto tag) -> hipError_t {
    using Tag = decltype(tag);
    if (D == 64) return causal ? launch_bwd_varlen_one<Tag, 64, true>(p, s) : launch_bwd_varlen_one<Tag, 64, false>(p, s);
    if (D == 128) return causal ? launch_bwd_varlen_one<Tag, 128, true>(p, s) : launch_bwd_varlen_one<Tag, 128, false>(p, s);
    return hipErrorInvalidValue;
  };
  return dtype == FA_DTYPE_F16 ? go(F16{}) : go(BF16{});
}

}  // namespace fa
