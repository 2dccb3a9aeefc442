// fa_mla_sparse_bwd_kernel.hip -- the backward of the absorbed latent-attention step over a per-token list of keys: entry point
// fa_bwd_mla_sparse (the backward of fa_fwd_mla_decode_sparse; include/fa_mi355.h).
//
// One launch, one workgroup of FOUR WAVES per (token, block of 32 heads). Heads are the rows of the matrix instructions, as in the forward;
// a tile is the 64 rows of 64 list entries, staged by fa_mla_sparse_kernel.hip's scheme into fa_mla_body.h's image (wave w stages rows
// 16 w .. 16 w + 15: one descriptor per latent row on the row's 64-bit address, num_records = 0 for an entry behind n_t or outside the
// pool; the rotary 128 bytes through registers), double buffered. No key split: T is in the thousands in training.
//   * THE BUDGET. Q and dO of 64 heads next to one tile do not fit LDS, so they live in registers as MFMA operands -- in the TWO forms the
//     five products ask for: by head rows (16 heads x 576 / 512 columns: 72 + 64 registers, the forward's fragments) for the products
//     that contract over the row width, and by columns (32 heads x a slice of 144 / 128 columns: 36 + 32 registers) for the products that
//     contract over heads. A block of 64 heads would double the second form and the dQ accumulator (to 416 registers under the tile's
//     temporaries): the head block is 32, and everything a wave keeps is 276 registers.
//   * PHASE 1, by (head tile, key half): wave w = (hw = w & 1, kw = w >> 1) forms S^T and dP^T of heads 16 hw .. + 15 against keys
//     32 kw .. + 31 of the tile -- one K fragment read feeds both products over the latent columns, the rotary columns feed S alone --,
//     then P = exp2(S~ - lse . log2 e) (0 behind n_t and in padding heads), dS = P (dP - delta), both ROUNDED TO THE TYPE, into the
//     exchange area of LDS: dS by [head][key] for phase 2, dS and P by [key][head] for phase 3. One barrier.
//   * PHASE 2, by columns: wave w owns latent columns 128 w .. + 127 and rotary columns 16 w .. + 15. dQ^T[column][head] += K^T . dS^T over
//     the tile's 64 keys and the block's 32 heads: the forward's transposed reads of the image as A (its PV product; the rotary part is
//     read the same way under its own swizzle), dS^T from the exchange area as B in the key order those reads imply.
//   * PHASE 3, the same columns: dKV[key][column] = scale . dS^T . Q + P^T . dO contracts over the block's 32 heads in ONE k-step per
//     product; the two accumulators are combined in fp32 and leave by one vector fp32 atomic add per (listed row, column) -- the sum over
//     the workgroup's heads is complete before it. A lane's four rows are keys 16 kt + 4 g + i: their slots stand in LDS since staging
//     (-1: behind n_t or outside the pool -- no address is formed, nothing is added).
//   * delta = sum_d dO . O (fp32, from O as given) is formed in the prologue from the head-row fragments and written to the workspace
//     [T, Hq]; the kernel uses its registers, so nothing depends on the workspace's prior contents.
//   * ROUNDING POINTS: the existing backward's (tests/backward_bound.py head_model): Q~ = round(scale . log2 e . Q) for S, LSE in fp32
//     times log2 e, P and dS rounded to the type before the second products; dKV's key side uses Q itself.
//   * dq is written (scale . accumulator; zeros for n_t = 0, recognised by the integer) and is bitwise reproducible; dkv is accumulated
//     into by atomics in an order that varies from run to run: not bitwise reproducible.
//   * BARRIERS: two per tile, both met by every wave in every iteration (token and n_t are workgroup-uniform); padding heads compute on
//     zero fragments and store nothing.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types

constexpr int SB_NW = 4;                        // waves of a workgroup
constexpr int SB_HT = 2, SB_HB = 16 * SB_HT;    // 16-head tiles / heads of a workgroup's block
constexpr int SB_DL = MLA_DV / 16 / SB_NW;      // 16-column latent tiles of a wave's slice: 8; one rotary tile behind them
static_assert(SB_DL == 8 && MLA_DR == 16 * SB_NW && SB_HB == 32, "a wave's slice is 128 latent + 16 rotary columns; 32 heads are one k-step");
// the exchange area behind the double buffer (rows padded against bank conflicts), then the slots of the two buffers' rows
constexpr int SB_TRB = BN * 2 + 8;              // row bytes of dS by [head][key]
constexpr int SB_KRB = SB_HB * 2 + 16;          // row bytes of dS / P by [key][head]
constexpr int SB_DST = 2 * MLA_IMG;
constexpr int SB_DSK = SB_DST + SB_HB * SB_TRB;
constexpr int SB_PK = SB_DSK + BN * SB_KRB;
constexpr int SB_SLOT = SB_PK + BN * SB_KRB;
constexpr int SB_LDS = SB_SLOT + 2 * BN * 4;
static_assert(SB_LDS <= 160 * 1024 && SB_DSK % 16 == 0 && SB_PK % 16 == 0, "LDS of gfx950; 16-byte reads of the exchange area");

__device__ __forceinline__ u32x2 lds_read_b64(const lds_char *p) { return *reinterpret_cast<const __attribute__((address_space(3))) u32x2 *>(p); }

template <typename Tag>
__global__ __launch_bounds__(64 * SB_NW) void mla_sparse_bwd_kernel(MlaSparseBwdParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  typedef elem elem4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) elem lds_elem;
  constexpr bool CAUSAL = false;  // visibility is the list
  constexpr int NW = SB_NW;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // rows (= list entries) of a tile this wave stages
  static_assert(RW == 16, "sixteen entries per wave: one per lane of the first sixteen, two rotary pieces of eight rows");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int hw = w & 1, kw = w >> 1;
  const int b = blockIdx.x;                // the token
  const int rb = blockIdx.y * SB_HT + hw;  // phase 1: the wave's 16-head tile
  const int R = p.Hq * p.Nq;
  const int Nk = p.counts ? min(max(__builtin_amdgcn_readfirstlane(p.counts[b]), 0), p.topk) : p.topk;  // n_t
  const int coff = Nk - p.Nq;
  const int nT = (Nk + BN - 1) / BN;

#define FA_MLA_BODY_PART 1  // the Q fragments qf[] (pre-scaled; zeros in padding rows), the LDS read offsets kl[], kr[], vl[]
#include "fa_mla_body.h"
  (void)rlim;

  // ---- dO by head rows, delta and the LSE of the lane's head (16 rb + c)
  const int hrow = 16 * rb + c;
  const bool hvalid = hrow < p.Hq;
  vec8 dof[KSL];
  float delta = 0.0f, lse2 = 0.0f;
  {
    const elem *dop = (const elem *)p.d_o + (long long)b * p.o_bs + (long long)hrow * p.o_hs;
    const elem *op = (const elem *)p.o + (long long)b * p.o_bs + (long long)hrow * p.o_hs;
#pragma unroll
    for (int ks = 0; ks < KSL; ++ks) {
      u32x4 t = {0u, 0u, 0u, 0u}, u = {0u, 0u, 0u, 0u};
      if (hvalid) {
        t = *reinterpret_cast<const u32x4 *>(dop + 32 * ks + 8 * g);
        u = *reinterpret_cast<const u32x4 *>(op + 32 * ks + 8 * g);
      }
      dof[ks] = __builtin_bit_cast(vec8, t);
      const vec8 of = __builtin_bit_cast(vec8, u);
#pragma unroll
      for (int j = 0; j < 8; ++j) delta += (float)dof[ks][j] * (float)of[j];
    }
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
    if (hvalid) {
      lse2 = p.lse[(long long)b * p.Hq + hrow] * 1.4426950408889634f;
      if (kw == 0 && g == 0) p.delta[(long long)b * p.Hq + hrow] = delta;
    }
  }

  // ---- Q and dO by columns: lane (c, g) holds heads 8 g .. 8 g + 7 of the block at column c of tile dl of the wave's slice
  auto slice_col = [&](int dl) __attribute__((always_inline)) { return dl < SB_DL ? 16 * (SB_DL * w + dl) : MLA_DV + 16 * w; };
  vec8 qT[SB_DL + 1], doT[SB_DL];
  {
    const int h0 = SB_HB * blockIdx.y + 8 * g;
    const elem *qb = (const elem *)p.q + (long long)b * p.q_bs + c;
    const elem *db = (const elem *)p.d_o + (long long)b * p.o_bs + c;
#pragma unroll
    for (int dl = 0; dl <= SB_DL; ++dl)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = h0 + j < p.Hq;
        qT[dl][j] = ok ? qb[(long long)(h0 + j) * p.q_hs + slice_col(dl)] : (elem)0.0f;
        if (dl < SB_DL) doT[dl][j] = ok ? db[(long long)(h0 + j) * p.o_hs + slice_col(dl)] : (elem)0.0f;
      }
  }

  // ---- staging (fa_mla_sparse_kernel.hip's): this wave moves rows jr0 .. jr0 + 15 of a tile and leaves their slots in LDS
  const int jr0 = RW * w;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const unsigned dma_l0 = (unsigned)lane << 4;
  const int drow = lane >> 3, dpc = lane & 7;
  const int *list = p.indices + (long long)b * p.idx_stride;
  auto slot_off = [&](int x) __attribute__((always_inline)) { return ((long long)(x >> lp) * p.page_stride + (long long)(x & PM) * p.row_stride) * 2; };
  int ev = -1;
  auto fetch_entries = [&](int t) __attribute__((always_inline)) {
    const int j = t * BN + jr0 + lane;
    ev = -1;
    if (lane < RW && j < Nk) ev = list[j];
  };
  u32x4 rot[RW / 8];
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const unsigned lbase = (unsigned)(__UINTPTR_TYPE__)smem + buf * MLA_IMG;
    const unsigned ll = lbase + jr0 * MLA_LRB;
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const int x = __builtin_amdgcn_readlane(ev, j);
      const bool ok = (unsigned)x < (unsigned)p.num_slots;  // behind the count (-1) or outside the pool: zeros
      const long long off = ok ? slot_off(x) : 0;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.kv + off), 0, ok ? MLA_DQK * 2 : 0, 0x00020000);
      const unsigned vo = dma_l0 ^ (unsigned)(mla_swz(j & 15) << 4);
      const unsigned ld = ll + j * MLA_LRB;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs) : "memory");
    }
#pragma unroll
    for (int k = 0; k < RW / 8; ++k) {
      const int x = __shfl(ev, 8 * k + drow, 64);
      rot[k] = u32x4{0u, 0u, 0u, 0u};
      if ((unsigned)x < (unsigned)p.num_slots) rot[k] = *reinterpret_cast<const u32x4 *>((const char *)p.kv + slot_off(x) + MLA_LRB + dpc * 16);
    }
    // the slot of row jr0 + lane, -1 where no gradient leaves for it
    if (lane < RW) lds_write_b32(smem + SB_SLOT + (buf * BN + jr0 + lane) * 4, (unsigned)ev < (unsigned)p.num_slots ? (unsigned)ev : ~0u);
    fetch_entries(t + 1);
  };
  auto write_rot = [&](int buf) __attribute__((always_inline)) {
    lds_char *img = smem + buf * MLA_IMG;
#pragma unroll
    for (int k = 0; k < RW / 8; ++k) {
      const int row = jr0 + 8 * k + drow;
      lds_write_b128(img + (unsigned)(MLA_LAT + row * MLA_RRB + ((dpc ^ ((row >> 1) & 7)) << 4)), rot[k]);
    }
  };

  // dQ^T of the wave's slice: dqacc[dl][ht][i] = dQ[head 16 ht + c][column slice_col(dl) + 4 g + i]
  f32x4 dqacc[SB_DL + 1][SB_HT];
#pragma unroll
  for (int dl = 0; dl <= SB_DL; ++dl)
#pragma unroll
    for (int ht = 0; ht < SB_HT; ++ht)
#pragma unroll
      for (int i = 0; i < 4; ++i) dqacc[dl][ht][i] = 0.0f;

  // per-lane offsets of the three phases
  const unsigned kwl = kw * 32 * MLA_LRB, kwr = kw * 32 * MLA_RRB;  // phase 1: the wave's key half
  const unsigned rtr = (unsigned)(MLA_LAT + vrow * MLA_RRB + (((2 * w + (vp >> 1)) ^ ((vrow >> 1) & 7)) << 4) + 8 * (vp & 1));  // phase 2: rotary tile w
  const unsigned xt_w = (unsigned)(SB_DST + (16 * hw + c) * SB_TRB + 2 * (32 * kw + 4 * g));  // dS by [head][key]: the lane's four keys of kt = 2 kw
  const unsigned xk_w = (unsigned)((32 * kw + 4 * g) * SB_KRB + 2 * (16 * hw + c));            // dS / P by [key][head]: key 32 kw + 4 g, the lane's head
  const unsigned xt_r = (unsigned)(SB_DST + c * SB_TRB + 8 * g);                                // phase 2: head c, keys 4 g ..
  const unsigned xk_r = (unsigned)(c * SB_KRB + 16 * g);                                        // phase 3: key c, heads 8 g ..
  const float scale = p.scale;

  if (nT > 0) fetch_entries(0);
  // iteration t: wait for tile t, send for tile t + 1, run tile t, write tile t + 1's rotary chunks; iteration -1 only stages tile 0
  for (int t = -1; t < nT; ++t) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces, slots and rotary writes of tile t have landed
    __builtin_amdgcn_s_barrier();                                // everyone's have, and everyone has left iteration t - 1
    const int nb = (t + 1) & 1;
    if (t + 1 < nT) stage(t + 1, nb);
    if (t >= 0) {
      const lds_char *img = smem + (t & 1) * MLA_IMG;
      // ---- phase 1: S^T = K.Q~^T (log2 units) and dP^T = V.dO^T of (16 heads, 32 keys): x[k][i] = X[head c][key 32 kw + 16 k + 4 g + i]
      f32x4 sc[2], dp[2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[k][i] = dp[k][i] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < KSL + KSR; ++ks)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const lds_char *kp = ks < KSL ? img + kl[ks & 3] + ((ks >> 2) << 8) + kwl + k * 16 * MLA_LRB : img + kr[ks < KSL ? 0 : ks - KSL] + kwr + k * 16 * MLA_RRB;
          const vec8 kf = __builtin_bit_cast(vec8, lds_read_b128(kp));
          sc[k] = M::mfma(kf, qf[ks], sc[k]);
          if (ks < KSL) dp[k] = M::mfma(kf, dof[ks < KSL ? ks : 0], dp[k]);
        }
      // P and dS, rounded to the type, into the exchange area
      {
        const int key0 = t * BN + 32 * kw + 4 * g;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          elem4 d4;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool vis = hvalid && key0 + 16 * k + i < Nk;
            const float pv = vis ? __builtin_amdgcn_exp2f(sc[k][i] - lse2) : 0.0f;
            const elem pe = (elem)pv, de = (elem)(pv * (dp[k][i] - delta));
            d4[i] = de;
            *reinterpret_cast<lds_elem *>(smem + SB_DSK + xk_w + (16 * k + i) * SB_KRB) = de;
            *reinterpret_cast<lds_elem *>(smem + SB_PK + xk_w + (16 * k + i) * SB_KRB) = pe;
          }
          lds_write_b64(smem + xt_w + 32 * k, __builtin_bit_cast(u32x2, d4));
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // ---- phase 2: dQ^T += K^T.dS^T over the wave's columns. B: lane (c, g) holds dS[head 16 ht + c] at keys 32 kp + 16 (j >> 2) + 4 g
      // + (j & 3), the order in which the transposed reads deliver K
      {
        vec8 dsb[2][SB_HT];
#pragma unroll
        for (int kp = 0; kp < 2; ++kp)
#pragma unroll
          for (int ht = 0; ht < SB_HT; ++ht) {
            const lds_char *x = smem + xt_r + ht * 16 * SB_TRB + 64 * kp;
            const u32x2 lo = lds_read_b64(x), hi = lds_read_b64(x + 32);
            dsb[kp][ht] = __builtin_bit_cast(vec8, u32x4{lo[0], lo[1], hi[0], hi[1]});
          }
#pragma unroll
        for (int dl = 0; dl <= SB_DL; ++dl)
#pragma unroll
          for (int kp = 0; kp < 2; ++kp) {
            const lds_char *vb = dl < SB_DL ? img + vl[dl < SB_DL ? dl : 0] + (w << 8) + (32 * kp) * MLA_LRB : img + rtr + (32 * kp) * MLA_RRB;
            const s16x4 lo = lds_read_tr16(vb), hi = lds_read_tr16(vb + 16 * (dl < SB_DL ? MLA_LRB : MLA_RRB));
            const vec8 kt8 = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
            for (int ht = 0; ht < SB_HT; ++ht) dqacc[dl][ht] = M::mfma(kt8, dsb[kp][ht], dqacc[dl][ht]);
          }
      }
      // ---- phase 3: dKV[key][column] = scale . dS^T.Q + P^T.dO over the block's heads, one atomic add per (listed row, column)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const vec8 ads = __builtin_bit_cast(vec8, lds_read_b128(smem + SB_DSK + xk_r + kt * 16 * SB_KRB));
        const vec8 ap = __builtin_bit_cast(vec8, lds_read_b128(smem + SB_PK + xk_r + kt * 16 * SB_KRB));
        const u32x4 xs = lds_read_b128(smem + SB_SLOT + ((t & 1) * BN + 16 * kt + 4 * g) * 4);  // the slots of keys 16 kt + 4 g + i
        float *rowp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int x = (int)xs[i];
          rowp[i] = x < 0 ? nullptr : p.dkv + ((long long)(x >> lp) * p.dkv_page_stride + (long long)(x & PM) * p.dkv_row_stride) + c;
        }
#pragma unroll
        for (int dl = 0; dl <= SB_DL; ++dl) {
          const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
          const f32x4 ka = M::mfma(ads, qT[dl], zero);
          f32x4 out;
          if (dl < SB_DL) {
            const f32x4 va = M::mfma(ap, doT[dl < SB_DL ? dl : 0], zero);
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = scale * ka[i] + va[i];
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = scale * ka[i];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (rowp[i]) unsafeAtomicAdd(rowp[i] + slice_col(dl), out[i]);
        }
      }
    }
    if (t + 1 < nT) write_rot(nb);
  }

  // ---- dq = scale . dQ, fp32, under q's element strides: lane (c, g) writes columns slice_col(dl) + 4 g .. + 3 of head 16 ht + c
#pragma unroll
  for (int ht = 0; ht < SB_HT; ++ht) {
    const int h = SB_HB * blockIdx.y + 16 * ht + c;
    if (h < p.Hq) {
      float *dqp = p.dq + (long long)b * p.q_bs + (long long)h * p.q_hs + 4 * g;
#pragma unroll
      for (int dl = 0; dl <= SB_DL; ++dl) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = scale * dqacc[dl][ht][i];
        *reinterpret_cast<f32x4 *>(dqp + slice_col(dl)) = v;
      }
    }
  }
}

// delta [T, Hq] fp32, rounded up to 16 bytes
long long mla_sparse_bwd_workspace_bytes(int T, int Hq) { return ((long long)T * Hq * 4 + 15) / 16 * 16; }

// One launch: T x ceil(Hq / 32) workgroups of four waves under the double buffer and the exchange area
hipError_t launch_bwd_mla_sparse(const MlaSparseBwdParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    auto kern = mla_sparse_bwd_kernel<decltype(tag)>;
    (void)hipGetLastError();
    hipError_t e = set_dyn_lds_once((const void *)kern, SB_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(p.T, (p.Hq + SB_HB - 1) / SB_HB), dim3(64 * SB_NW), SB_LDS, s, p);
    return hipGetLastError();
  });
}

}  // namespace fa
