// fa_mla_sparse_probs_kernel.hip -- the main attention's probability mass on every listed key, summed over heads: entry point
// fa_mla_sparse_head_probs (include/fa_mi355.h). probs[t][j] = sum_h exp(scale q[t,h] . row(x_j) - lse[t,h]),
// the target of the indexer's KL loss (fa_mla_indexer_loss_sparse) before its normalisation.
//
// One launch, one workgroup of FOUR WAVES per (token, chunk of 64-key tiles). A tile is the 64 rows of 64 list entries, staged by
// fa_mla_sparse_kernel.hip's scheme into fa_mla_body.h's image (wave w stages rows 16 w .. 16 w + 15: one descriptor per latent row on
// the row's 64-bit address, num_records = 0 for an entry behind n_t or outside the pool; the rotary 128 bytes through registers),
// double buffered. No PV product, no workspace: all that leaves a tile is 64 floats.
//   * THE SCORE TILE has HEADS as the rows of v_mfma_f32_16x16x32 (A = 16 heads of Q~ = round(scale . log2 e . Q), the sparse backward's
//     rounding, so P here is the P that call uses) and KEYS as its columns (B = 16 rows of the image): lane (c, g) ends up with heads
//     4 g + i (i < 4) of a 16-head tile against key c. The head sum of a lane is then a chain of adds over its accumulator registers, the
//     sum over g two cross-lane adds; the key, which is the output, never leaves its lane column.
//   * A WAVE holds the Q~ rows of a BLOCK OF 32 HEADS as A operands for the whole chunk: 2 x 18 fragments, 144 registers (the sparse
//     backward's budget). NHB = 1, 2 or 4 such blocks cover the call's heads (Hq <= 32, <= 64, <= 128; a host scalar), and the four waves
//     are (head block hw = w % NHB, key part kw = w / NHB): a wave takes the NHB 16-key tiles NHB kw .. NHB kw + NHB - 1 of every tile.
//     So at Hq = 128 a wave sees all 64 keys under its own 32 heads, at Hq <= 32 the four waves split the tile's keys under the same
//     heads -- no wave idles at any head count, and every K fragment read from LDS feeds two products. Padding heads hold zero fragments
//     and add exactly 0.
//   * P = exp2(S~ - lse . log2 e) on the accumulators. The sum over a wave's 32 heads in a fixed order (head tile, i, then g), the waves'
//     partials [head block][key] through a small LDS area that is double buffered like the image, and in the NEXT iteration, behind its
//     barrier, wave 0 adds the NHB partials of each key in head-block order and stores 64 consecutive floats, predicated on j < n_t:
//     ONE BARRIER PER TILE, no atomics, bitwise reproducible.
//   * THE CHUNK RULE is mla_sparse_probs_chunk_tiles, below: host scalars only. A workgroup whose chunk starts behind n_t leaves in front
//     of the first barrier, as a whole; n_t = 0 is recognised by the integer.
#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types

constexpr int HP_NW = 4;                          // waves of a workgroup
constexpr int HP_HT = 2, HP_HB = 16 * HP_HT;      // 16-head tiles / heads of a wave's block
constexpr int HP_PART = 2 * MLA_IMG;              // the partials behind the double buffer: [2][4 head blocks][64 keys] floats
constexpr int HP_LDS = HP_PART + 2 * HP_NW * BN * 4;
static_assert(HP_LDS <= 160 * 1024, "LDS of gfx950");

// THE CHUNK RULE. A chunk is `chunk_tiles` consecutive 64-key tiles of a list; an item is (token, chunk). One workgroup lives on a compute
// unit (146 KiB of LDS), so 512 items give each of the 256 units two; a chunk must not be so short that the 144 KiB of Q a workgroup
// loads weigh against the 72 KiB tiles it reads: at least 8 tiles wherever the list has them. So: as few chunks as give 512 items, never
// more than floor(tiles / 8). Training chunks (T in the thousands) run one chunk per token.
int mla_sparse_probs_chunk_tiles(int T, int topk) {
  const long long nT = ((long long)topk + BN - 1) / BN;
  const long long want = (512 + (long long)T - 1) / T, most = std::max(1LL, nT / 8);
  const long long nch = std::min(want, most);
  return (int)((nT + nch - 1) / nch);
}

template <typename Tag, int NHB>
__global__ __launch_bounds__(64 * HP_NW) void mla_headsum_probs_kernel(MlaSparseProbsParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int NW = HP_NW;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int KTW = NHB;                             // 16-key tiles of a 64-key tile this wave multiplies
  constexpr int RW = BN / NW;                          // rows (= list entries) of a tile this wave stages
  static_assert(RW == 16 && (NHB == 1 || NHB == 2 || NHB == 4), "sixteen entries per wave; head blocks x key parts = four waves");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int hw = w & (NHB - 1), kw = w / NHB;
  const int b = blockIdx.x;  // the token
  const int Nk = p.counts ? min(max(__builtin_amdgcn_readfirstlane(p.counts[b]), 0), p.topk) : p.topk;  // n_t
  const int t0 = blockIdx.y * p.chunk_tiles;
  if (t0 * BN >= Nk) return;  // the chunk starts behind the list's last entry (workgroup-uniform; n_t = 0 leaves here)
  const int t1 = min(t0 + p.chunk_tiles, (Nk + BN - 1) / BN);

  // ---- Q~ of the wave's 32 heads as A operands: lane (c, g) holds head 32 hw + 16 ht + c, elements 32 ks + 8 g .. + 7; and the LSE (log2
  // units) of the heads its accumulators will hold, 32 hw + 16 ht + 4 g + i
  const float c2 = p.scale * 1.4426950408889634f;
  vec8 qf[HP_HT][KSL + KSR];
  float lse2[HP_HT][4];
  bool hok[HP_HT][4];
#pragma unroll
  for (int ht = 0; ht < HP_HT; ++ht) {
    const int h = HP_HB * hw + 16 * ht + c;
    const elem *qp = (const elem *)p.q + (long long)b * p.q_bs + (long long)h * p.q_hs + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KSL + KSR; ++ks) {
      u32x4 t = {0u, 0u, 0u, 0u};
      if (h < p.Hq) t = *reinterpret_cast<const u32x4 *>(qp + 32 * ks);
      qf[ht][ks] = __builtin_bit_cast(vec8, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[ht][ks][j] = (elem)((float)qf[ht][ks][j] * c2);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ha = HP_HB * hw + 16 * ht + 4 * g + i;
      hok[ht][i] = ha < p.Hq;
      lse2[ht][i] = hok[ht][i] ? p.lse[(long long)b * p.Hq + ha] * 1.4426950408889634f : 0.0f;
    }
  }

  // ---- per-lane read offsets of the B operand: row 16 kt + c of the image, chunk 4 ks + g under the part's swizzle (fa_mla_body.h part 1)
  const int fc = mla_swz(c);
  unsigned kl[4], kr[KSR];
#pragma unroll
  for (int j = 0; j < 4; ++j) kl[j] = (unsigned)(c * MLA_LRB + (((4 * j + g) ^ fc) << 4));
#pragma unroll
  for (int j = 0; j < KSR; ++j) kr[j] = (unsigned)(MLA_LAT + c * MLA_RRB + (((4 * j + g) ^ ((c >> 1) & 7)) << 4));

  // ---- staging (fa_mla_sparse_kernel.hip's): this wave moves rows jr0 .. jr0 + 15 of a tile
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
    if (lane < RW && j < Nk) ev = list[j];  // nothing behind n_t is read
  };
  u32x4 rot[RW / 8];
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const unsigned lbase = (unsigned)(__UINTPTR_TYPE__)smem + buf * MLA_IMG;
    const unsigned ll = lbase + jr0 * MLA_LRB;
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const int x = __builtin_amdgcn_readlane(ev, j);
      const bool ok = (unsigned)x < (unsigned)p.num_slots;  // behind the count (-1) or outside the pool: zeros, no address from x
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

  // the store of a finished tile: wave 0, lane j adds the head blocks' partials of key j in block order
  float *out = p.probs + (long long)b * p.probs_stride;
  typedef __attribute__((address_space(3))) float lds_float;
  auto emit = [&](int t) __attribute__((always_inline)) {
    const lds_float *part = (const lds_float *)(smem + HP_PART) + ((t - t0) & 1) * NW * BN;
    float s = part[lane];
#pragma unroll
    for (int k = 1; k < NHB; ++k) s += part[k * BN + lane];
    if (t * BN + lane < Nk) out[t * BN + lane] = s;
  };

  fetch_entries(t0);
  // iteration t: wait for tile t, send for tile t + 1, store tile t - 1, run tile t, write tile t + 1's rotary chunks; the first only stages
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces, rotary writes and partials have landed
    __builtin_amdgcn_s_barrier();                                // everyone's have, and everyone has left iteration t - 1
    const int nb = (t + 1 - t0) & 1;
    if (t + 1 < t1) stage(t + 1, nb);
    if (t > t0 && w == 0) emit(t - 1);
    if (t >= t0) {
      const lds_char *img = smem + ((t - t0) & 1) * MLA_IMG;
      // ---- S = Q~ . K^T (log2 units): acc[ht][k][i] = S[head 32 hw + 16 ht + 4 g + i][key 16 (KTW kw + k) + c]
      f32x4 acc[HP_HT][KTW];
#pragma unroll
      for (int ht = 0; ht < HP_HT; ++ht)
#pragma unroll
        for (int k = 0; k < KTW; ++k) acc[ht][k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < KSL + KSR; ++ks)
#pragma unroll
        for (int k = 0; k < KTW; ++k) {
          const int kt = KTW * kw + k;
          const lds_char *kp = ks < KSL ? img + kl[ks & 3] + ((ks >> 2) << 8) + kt * 16 * MLA_LRB : img + kr[ks < KSL ? 0 : ks - KSL] + kt * 16 * MLA_RRB;
          const vec8 kf = __builtin_bit_cast(vec8, lds_read_b128(kp));
#pragma unroll
          for (int ht = 0; ht < HP_HT; ++ht) acc[ht][k] = M::mfma(qf[ht][ks], kf, acc[ht][k]);
        }
      // ---- P and the sum over the wave's heads: head tile, i, then g -- a fixed order
      lds_float *part = (lds_float *)(smem + HP_PART) + (((t - t0) & 1) * NW + hw) * BN;
#pragma unroll
      for (int k = 0; k < KTW; ++k) {
        float s = 0.0f;
#pragma unroll
        for (int ht = 0; ht < HP_HT; ++ht)
#pragma unroll
          for (int i = 0; i < 4; ++i) s += hok[ht][i] ? __builtin_amdgcn_exp2f(acc[ht][k][i] - lse2[ht][i]) : 0.0f;
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g == 0) part[16 * (KTW * kw + k) + c] = s;
      }
    }
    if (t + 1 < t1) write_rot(nb);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (w == 0) emit(t1 - 1);
}

// One launch: T x nchunks workgroups of four waves under the double buffer and the partials
hipError_t launch_mla_sparse_head_probs(const MlaSparseProbsParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    (void)hipGetLastError();
    auto go = [&](auto kern) {
      hipError_t e = set_dyn_lds_once((const void *)kern, HP_LDS);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, dim3(p.T, p.nchunks), dim3(64 * HP_NW), HP_LDS, s, p);
      return hipGetLastError();
    };
    return p.Hq <= HP_HB       ? go(mla_headsum_probs_kernel<Tag, 1>)
           : p.Hq <= 2 * HP_HB ? go(mla_headsum_probs_kernel<Tag, 2>)
                               : go(mla_headsum_probs_kernel<Tag, 4>);
  });
}

}  // namespace fa
