// fa_bwd_body.h -- what the translation units of the backward share: fa_bwd_kernels.hip (dense: fa_bwd / fa_bwd_ex),
// fa_bwd_varlen_kernels.hip (packed variable-length sequences: fa_bwd_varlen) and fa_bwd_window_kernels.hip (the same under a sliding
// window: fa_bwd_varlen_window, FA_BWD_WINDOW = 1 on top of FA_BWD_VARLEN = 1; fa_bwd_softcap_kernels.hip adds FA_BWD_SOFTCAP = 1 on top of
// that: fa_bwd_varlen_softcap). The algorithm and its history are described at the top of
// fa_bwd_kernels.hip. Here: the parameter blocks and the per-head-dim constants; the two kernel bodies themselves are the texts
// fa_bwd_dq_body.inc and fa_bwd_dkdv_body.inc, which each __global__ function of either file includes as its body with FA_BWD_VARLEN
// set to 0 or 1. Text, not a function: behind a forced-inline function the compiler copies the parameter block before it inlines, which
// moves the dense kernels' instruction schedule; as text they compile to exactly the code they had (tools/isa_kernel_diff.py).
#pragma once
#include "fa_mfma_common.h"

namespace fa {

struct BwdParams {
  const void *q, *k, *v, *o, *d_o;
  const float *lse;
  float *dq, *dk, *dv;
  float *delta;  // workspace [B,H,N]
  int B, H, N, D;  // H = query heads, N = query rows per head
  int Nk;          // keys per head (causal: bottom-right aligned, key j visible to query i iff j <= i + Nk - N; Nk >= N then)
  float scale;
  long long batch_stride, head_stride;  // of Q, O, dO, dQ (elements)
  int is_causal;
  int Hkv;                                    // key/value heads: query head h reads (and dK/dV sum over) key head h / (H / Hkv)
  long long kv_batch_stride, kv_head_stride;  // of K, V, dK, dV
};

// one fa_bwd_varlen call (the varlen mode of the bodies below, as VarlenParams is the forward's): q / o / d_o / dq are [total_q, H, D]
// and k / v / dk / dv [total_k, Hkv, D] under a row (token) stride and the head strides of BwdParams; lse and delta are [H, total_q];
// B counts sequences, N / Nk hold max_seqlen_q / max_seqlen_k (the grids depend on nothing else), batch strides are unused. Sequence b
// owns tokens cu_q[b] .. cu_q[b+1) and keys cu_k[b] .. cu_k[b+1): both tables are device memory read by the kernels only.
struct BwdVarlenParams : BwdParams {
  const int *cu_q, *cu_k;  // int32 [B + 1]
  int total_q, total_k;    // tokens in q and in k: every table entry is clamped to [0, total]
  long long q_rs, kv_rs;   // row strides, elements
};

// one fa_bwd_varlen_window call (the window mode of the bodies, FA_BWD_WINDOW = 1 on top of the varlen mode; fa_bwd_window_kernels.hip):
// the varlen call's parameters plus both bounds, which the host has made non-negative (an unbounded or oversized side is the smallest
// value that can never bind: wl <= max_seqlen_k, wr <= max_seqlen_q -- so that coff - wl and row + coff + wr stay inside an int)
struct BwdWindowParams : BwdVarlenParams {
  int wl, wr;
};

// one fa_bwd_varlen_softcap call (the softcap mode of the bodies, FA_BWD_SOFTCAP = 1 on top of the window mode;
// fa_bwd_softcap_kernels.hip): the windowed call's parameters plus the cap, a finite positive host scalar
struct BwdSoftcapParams : BwdWindowParams {
  float softcap;
  float cap_log2;  // softcap * log2(e), the capped scores' factor to log2 units
};

constexpr float LOG2E = 1.4426950408889634f;

#ifndef FA_BWD_WINDOW
#define FA_BWD_WINDOW 0  // the bodies' window mode: 1 only around the kernels of fa_bwd_window_kernels.hip
#endif

#ifndef FA_BWD_SOFTCAP
#define FA_BWD_SOFTCAP 0  // the bodies' softcap mode (on top of the window mode): 1 only around the kernels of fa_bwd_softcap_kernels.hip
#endif

#ifndef FA_BWD_DMA
#define FA_BWD_DMA 1  // 1: the streamed tiles go global -> LDS by LDS-DMA (buffer_load ... lds; the chunk swizzle sits on the source address):
#endif                // no staging registers, no ds_write_b128 (as in the forward kernels, profiles/r03/ab_mfma_lds_dma.log); 0 = register staging
#ifndef FA_BWD_LA
#define FA_BWD_LA 3  // row fragments are read this many MFMAs ahead of their use
#endif
#ifndef FA_BWD_LA2
#define FA_BWD_LA2 2  // the same for the transposed fragments
#endif
#ifndef FA_BWD_KV128_LA
#define FA_BWD_KV128_LA 1  // the head_dim-128 dK/dV kernel (256 registers at two workgroups per CU) affords one step of each
#define FA_BWD_KV128_LA2 1
#endif
// Workgroups per CU the kernels are compiled for: three at head_dim 64 (register cap 168, 32-34 KiB of LDS), two at 128
// (cap 256, 64-66 KiB). Round 3 first ran two / one (205-214 registers): see bwd_dq_kernel for what brought them down.
constexpr int bwd_occ(int D) { return D == 64 ? 3 : D == 128 ? 2 : 1; }  // (head_dim 256: one workgroup per CU, 512 registers, 128 KiB of LDS)
// 64-row sub-tiles per staged tile: one barrier and one staging pass per SUB * 64 keys (dQ) / queries (dK, dV). 2 paid while
// one workgroup per CU exposed every barrier (+16 % at head_dim 128 then); at the occupancy above 1 is faster and is what
// fits the LDS (profiles/r03/ab_bwd_dq_per_half.log).
#ifndef FA_BWD_SUB
#define FA_BWD_SUB 1
#endif
constexpr int bwd_sub_dq(int D) { return FA_BWD_SUB; }
constexpr int bwd_sub_kv(int D) { return FA_BWD_SUB; }

// Dynamic LDS of the two bodies: K and V (dQ) / Q and dO (dK, dV) double buffers of staged tiles; the dK/dV body keeps the -lse.log2e
// and -delta rows of both buffers behind them
constexpr size_t bwd_dq_lds_bytes(int D) { return (size_t)4 * bwd_sub_dq(D) * BN * D * 2; }
constexpr size_t bwd_dkdv_lds_bytes(int D) { return (size_t)4 * bwd_sub_kv(D) * BN * D * 2 + 2 * 2 * bwd_sub_kv(D) * BN * 4; }

// One backward call: dQ first -- it leaves delta in the workspace for the dK/dV kernel -- then dK/dV on the same stream, one error
// check at the end. p.N / p.Nk size the grids (varlen: max_seqlen_q / max_seqlen_k, blocks past the end of their sequence return at once).
template <typename KQ, typename KK, typename PT>
inline hipError_t launch_bwd_pair(KQ kq, KK kk, const PT &p, int D, hipStream_t s) {
  const int nBq = (p.N + BM - 1) / BM, nBk = (p.Nk + BM - 1) / BM;
  const size_t smem_dq = bwd_dq_lds_bytes(D), smem_kv = bwd_dkdv_lds_bytes(D);
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

// per-head-dim constants of the kernels below (the reference kernel is head_dim 64 only, kernels.metal:905-1265;
// 128 is the same algorithm with twice the k-steps / output blocks and two workgroups per CU)
#define FA_BWD_CONSTS(D, SUBS)                                                                   \
  constexpr int BSUB = (SUBS);     /* sub-tiles per staged tile */                               \
  constexpr int BT = BSUB * BN;    /* rows of a staged tile */                                   \
  constexpr int BD = (D);          /* head dim */                                                \
  constexpr int BRB = BD * 2;      /* row bytes */                                               \
  constexpr int BCPR = BD / 8;     /* 16-byte chunks per row */                                  \
  constexpr int BKS = BD / 16;     /* k-steps over the head dim */                               \
  constexpr int BDB = BD / 32;     /* 32-wide output blocks over the head dim */                 \
  constexpr int BTILE = BN * BRB;  /* one 64-row sub-tile image */                               \
  constexpr int STILE = BSUB * BTILE; /* one staged tile (BT rows) */                             \
  /* XOR on the 16-byte chunk index of a row: conflict-free for ds_read_b128 row reads, ds_read_b64_tr_b16 and ds_write_b128 */ \
  auto u_swz = [](int row) { return BD == 64 ? ((((row >> 1) & 1) << 2) | ((row >> 3) & 3)) : (((row & 3) << 2) | ((row >> 2) & 3)); }; \
  /* transposed read of the 4-row x 32-column block (R0 + 4h + vq, columns 32db ..), R0 a multiple of 8: the swizzle's low   */ \
  /* bits depend on R0 only through `variant` = (R0 >> 3) & 3 (head_dim 64) or (R0 >> 3) & 1 (head_dim 128): NTV base addresses */ \
  constexpr int NTV = BD == 64 ? 4 : 2;                                                       \
  auto tr_off = [&](int variant, int db, int h_, int g1_, int vq_, int vp_) {                 \
    const int row = 8 * variant + 4 * h_ + vq_; /* a representative R0 = 8 * variant */        \
    return (4 * h_ + vq_) * BRB + ((((4 * db) + 2 * g1_ + (vp_ >> 1)) ^ u_swz(row)) << 4) + 8 * (vp_ & 1); \
  };                                                                                          \
  /* LDS-DMA: wave w moves the 1-KiB pieces w, w+4, ... of a staged tile; lane L fills LDS bytes [16 L, 16 L + 16) of its    */ \
  /* piece = row RPP w + L / BCPR, physical chunk L % BCPR, which holds logical chunk (L % BCPR) ^ u_swz(row); the swizzle */ \
  /* does not depend on the piece index (4 RPP rows per step of the piece index: a multiple of its period)                */ \
  constexpr int RPP = 1024 / BRB, NPW = (BT / RPP) / 4;                                       \
  auto dma_off = [&](int wave_, int lane_) {                                                  \
    const int row = wave_ * RPP + lane_ / BCPR, pc = lane_ % BCPR;                            \
    return (unsigned)(row * BRB + ((pc ^ u_swz(row)) << 4));                                  \
  };                                                                                          \
  (void)BT; (void)BCPR; (void)BKS; (void)BDB; (void)BTILE; (void)STILE; (void)u_swz; (void)tr_off; (void)NTV; (void)RPP; (void)NPW; (void)dma_off

// Head dims other than 64 / 128 (any multiple of 8 up to 128: 32, 96, ...) run the next larger instantiation on ZERO-PADDED rows
// (PAD): rows keep their packed pitch of p.D elements in global memory; the LDS images and the register fragments have the
// kernel's pitch, and every 16-byte chunk at or past column p.D is fetched from an offset outside the buffer descriptor's range,
// which reads as zeros (register fragments and LDS-DMA alike). The padding columns then add 0 to every score and receive
// gradients that are never stored. Same arithmetic per real column, (BD - D) / BD of the matrix work wasted (D = 96: a quarter).
#define FA_BWD_PAD(PAD_)                                                                                      \
  const int GRB = (PAD_) ? p.D * 2 : BRB; /* row bytes in global memory */                                    \
  constexpr unsigned OOB = 0x80000000u;   /* past any head (bwd_impl keeps padded heads below 2 GiB) */       \
  auto gcol = [&](int chunk) -> unsigned { return (!(PAD_) || chunk * 8 < p.D) ? (unsigned)chunk * 16 : OOB; }; \
  auto dma_off_pad = [&](int wave_, int lane_) {                                                              \
    const int row = wave_ * RPP + lane_ / BCPR, lc = (lane_ % BCPR) ^ u_swz(row);                             \
    return (unsigned)(row * GRB) + gcol(lc);                                                                  \
  };                                                                                                          \
  (void)gcol; (void)dma_off_pad; (void)OOB

// Varlen mode of the two bodies (FA_BWD_VARLEN = 1; as the forward's, fa_mfma_kernel.hip): the "batch" index of the block map selects a
// sequence of a packed batch; its lengths come from the cu_seqlens tables in device memory and take the place of N / Nk, its rows are
// addressed with a run-time pitch (as the PAD arm does: row * pitch plus per-piece offsets). Each varlen expression is one arm of a
// compile-time choice whose other arm is the dense expression; everything from LDS onwards -- images, swizzles, MFMA order, roundings
// -- is shared, so a sequence's gradients come out bit for bit as the dense kernels compute them for it alone.
// FA_VP names the varlen fields of the parameter block: the kernel's own parameter in a varlen kernel, and in a dense kernel -- where
// it stands in discarded statements only -- this function, which is declared and never defined.
__device__ const BwdVarlenParams &bwd_no_varlen_params();

}  // namespace fa
