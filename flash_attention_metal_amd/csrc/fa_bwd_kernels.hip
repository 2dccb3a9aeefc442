// fa_bwd_kernels.hip -- backward of the operator on the CDNA4 matrix cores (head_dim 64 and 128).
//
// Replaces /root/reference/kernels.metal:905-1265 (flash_attention_backward_kernel): same
// math -- D_i = rowsum(dO o O) (:983-990), P = exp(S*scale - L_i) recomputed from the forward's
// LSE (:1082-1089), dV += P^T dO, dP = dO V^T, dS = P o (dP - D_i) * scale (:1160-1169),
// dQ += dS K, dK += dS^T Q -- nothing else. The reference flushes dK/dV with global float
// atomics from every Q block (:1221-1246); here no gradient is accumulated across workgroups:
//
//   bwd_dq_kernel      one workgroup per 128 query rows, loops over KV tiles (like the forward):
//                        delta[b,h,i] = sum_d dO*O of its rows, formed in the prologue from the dO fragments it holds
//                        anyway and left in the workspace (B*H*N floats) for the dK/dV kernel (round 2: a kernel of its own),
//                        S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T o (dP^T - delta) * scale,
//                        dQ^T += K^T.dS^T
//   bwd_dkdv_kernel    one workgroup per 128 keys, loops over Q tiles:
//                        S = Q.K^T, dP = dO.V^T, P, dS (as above),
//                        dV^T += dO^T.P,  dK^T += Q^T.dS
//
// S and dP are computed twice (7 matrix products instead of 5) in exchange for deterministic,
// atomic-free, bitwise reproducible gradients. (The single-pass 5-product form sums dQ across key blocks with float
// atomics: at head_dim 64 that is 570 MB of adds for BASELINE config 3's shape with 256 keys per workgroup, 436 us MEASURED
// (tools/probes/probe_dq_atomic_floor.hip: 1.31-1.34 TB/s, MI355X_MICROARCH.md, Global float atomics) -- as long as both kernels here
// together; 861 us vs ~850 at head_dim 128: the bytes per FLOP do not depend on the head dim. DESIGN 4.6b.)
// Round 3: the row constants ride in the accumulators (cdna guide, attention backward): the operand held in registers is
// pre-scaled by scale*log2(e) (Q~ in the dQ kernel -- bit for bit the forward's operand --, K~ in the dK/dV kernel) and the
// score chains start from -LSE*log2(e), the dP chains from -delta, so P = exp2(S') and dS = P * dP' are one
// transcendental and one multiply per score; the softmax scale is applied once to the finished dQ / dK. Both kernels reuse the forward's machinery
// (fa_mfma_kernel.hip): one operand's fragments live in registers, the other side streams
// through double-buffered LDS tiles; the score tile comes out of v_mfma_f32_32x32x16 with the
// reduction index of the NEXT product in its registers, so P / dS feed that product as the B
// operand without leaving the register file, and the transposed A operands (K^T, dO^T, Q^T) are
// ds_read_b64_tr_b16 reads of row-major tiles. A tile that is read both by rows and transposed sits in LDS ONCE, under a
// chunk swizzle that keeps both kinds of read (and the staging stores) free of bank conflicts (cdna guide T10, "one image
// for row reads and transposed reads"; round 2 kept two images and paid the LDS store bandwidth twice -- these kernels
// are LDS-bound: every MFMA takes a 1 KiB fragment from LDS, half the LDS bandwidth at full matrix rate, before any store).
// Second half of round 3: each 64-row sub-tile is worked one 32-row half at a time (scores, P / dS, then that half's share
// of the second products), so one score and one dP tuple are live; the per-lane LDS addresses are ABSOLUTE addresses in the
// current buffer, moved to the other buffer in place once per tile. Together: 160-166 registers, three workgroups per CU at
// head_dim 64 (config-3 shape 692 -> 811 TFLOP/s with the SLP vectorizer off, profiles/r03/ab_bwd_*.log).
// Grouped-query heads (fa_bwd_ex): the dK/dV workgroup of a key/value head visits its H / Hkv query heads in turn.
#include "fa_bwd_body.h"

namespace fa {

// the two bodies in their dense mode (fa_bwd_body.h)
#define FA_BWD_VARLEN 0
template <typename Tag, int D, bool CAUSAL, bool PAD>
__global__ __launch_bounds__(NTHREADS, bwd_occ(D)) void bwd_dq_kernel(BwdParams p) {
#include "fa_bwd_dq_body.inc"
}

template <typename Tag, int D, bool CAUSAL, bool PAD>
__global__ __launch_bounds__(NTHREADS, bwd_occ(D)) void bwd_dkdv_kernel(BwdParams p) {
#include "fa_bwd_dkdv_body.inc"
}
#undef FA_BWD_VARLEN

// ---------------------------------------------------------------------------
bool bwd_supported(int dtype, int D) {
  if (dtype == FA_DTYPE_FP8_E4M3) return D >= 16 && D <= 128 && D % 16 == 0;  // (rows of whole 16-byte chunks: the widening pass)
  return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && ((D >= 8 && D <= 128 && D % 8 == 0) || D == 256);
}

// e4m3 inputs (the forward's config-5 family): Q, K, V are widened to bf16 -- exactly: every e4m3 value is a bf16 value -- into the
// caller's workspace by one streaming pass, under their own element strides, and the bf16 kernels run on the copies (O and dO of that
// family are bf16 already). 3 bytes of traffic per element against the backward's hundreds of FLOPs per element.
__global__ __launch_bounds__(256) void widen_e4m3_kernel(const unsigned *in, unsigned *out, long long n16) {
  // one thread = 16 elements: 16 bytes in, 32 bytes out
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) {
    const u32x4 w = *reinterpret_cast<const u32x4 *>(in + 4 * i);
    u32x4 lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      typedef float f32x2 __attribute__((ext_vector_type(2)));
      const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
      // bf16 = the upper half of the fp32 pattern (exact here: an e4m3 value has 3 mantissa bits)
      // (scalar temporaries on purpose: __builtin_bit_cast applied directly to a vector element expression reads element 0, see below)
      const float a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
      const unsigned p0 = (__builtin_bit_cast(unsigned, a0) >> 16) | (__builtin_bit_cast(unsigned, a1) & 0xffff0000u);
      const unsigned p1 = (__builtin_bit_cast(unsigned, b0) >> 16) | (__builtin_bit_cast(unsigned, b1) & 0xffff0000u);
      if (j < 2) { lo[2 * j] = p0; lo[2 * j + 1] = p1; } else { hi[2 * (j - 2)] = p0; hi[2 * (j - 2) + 1] = p1; }
    }
    *reinterpret_cast<u32x4 *>(out + 8 * i) = lo;
    *reinterpret_cast<u32x4 *>(out + 8 * i + 4) = hi;
  }
}

// n elements (a multiple of 16, 16-byte aligned source) of e4m3 -> bf16
hipError_t launch_widen_e4m3(const void *in, void *out, long long n, hipStream_t s) {
  const long long n16 = n / 16;
  long long blocks = (n16 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (blocks < 1) blocks = 1;
  (void)hipGetLastError();
  hipLaunchKernelGGL(widen_e4m3_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const unsigned *)in, (unsigned *)out, n16);
  return hipGetLastError();
}

template <typename Tag, int D, bool CAUSAL, bool PAD>
static hipError_t launch_bwd_one(const BwdParams &p, hipStream_t s) {
  return launch_bwd_pair(bwd_dq_kernel<Tag, D, CAUSAL, PAD>, bwd_dkdv_kernel<Tag, D, CAUSAL, PAD>, p, D, s);
}

// head dims without a kernel of their own: the next larger instantiation on zero-padded rows (PAD)
template <typename Tag>
static hipError_t launch_bwd_dt(const BwdParams &p, hipStream_t s) {
  if (p.D == 64 || p.D == 128 || p.D == 256)
    return with_dim_causal<64, 128, 256>(p.D, p.is_causal, [&](auto d, auto c) { return launch_bwd_one<Tag, d(), c(), false>(p, s); });
  return with_dim_causal<64, 128>(p.D < 64 ? 64 : 128, p.is_causal, [&](auto d, auto c) { return launch_bwd_one<Tag, d(), c(), true>(p, s); });
}

hipError_t launch_bwd(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                      float *dq, float *dk, float *dv, float *ws, int B, int H, int Hkv, int N, int Nk, int D, float scale,
                      long long bs, long long hs, long long kv_bs, long long kv_hs, int causal, int dtype, hipStream_t s) {
  BwdParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.d_o = d_o; p.lse = lse;
  p.dq = dq; p.dk = dk; p.dv = dv; p.delta = ws;
  p.B = B; p.H = H; p.N = N; p.D = D; p.scale = scale;
  p.batch_stride = bs; p.head_stride = hs; p.is_causal = causal;
  p.Hkv = Hkv; p.Nk = Nk; p.kv_batch_stride = kv_bs; p.kv_head_stride = kv_hs;
  return dtype == FA_DTYPE_F16 ? launch_bwd_dt<F16>(p, s) : launch_bwd_dt<BF16>(p, s);
}

}  // namespace fa
