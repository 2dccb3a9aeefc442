// fa_mla_sparse_kv8_scaled_kernel.hip -- the absorbed latent-attention decode over a per-token list of keys of a pool of 656-BYTE ROWS
// (512 e4m3 latent bytes, four fp32 scales, one per 128 latent elements, and 64 bf16 rotary elements -- the layout FlashMLA reads and
// vLLM names fp8_ds_mla): entry point fa_fwd_mla_decode_sparse_kv8_scaled.
//
// fa_mla_sparse_kv8_kernel.hip's four-wave workgroup over one shared double buffer, staged through registers into the wide kernel's bf16
// image, with ONE difference: what a wave's sixteen rows of a tile are read from and how they become bf16. Everything from LDS onwards is
// the wide kernel's text (fa_mla_body.h parts 0 - 3 with CAUSAL = false, b = the token, Nq = 1, Nk = n_t), the workspace format and the
// bf16 combine kernel are unchanged. O and LSE are therefore the bits of fa_fwd_mla_decode_sparse (bf16) on a pool that holds, for
// every row, latent element d as bf16_rne(fp32(e4m3 byte d) * s_{d / 128}) -- one fp32 multiply, one rounding to bf16 -- and the rotary
// elements as they stand.
//   * THE ROW: bytes 0 .. 511 latent e4m3, 512 .. 527 the scales s_0 .. s_3, 528 .. 655 rotary bf16. Row and page strides are bytes,
//     multiples of 16: every chunk below is 16-byte aligned, every scale 4-byte aligned.
//   * ALWAYS FOUR WAVES, one instantiation (bf16 queries, no causal form). Wave w stages rows 16 w .. 16 w + 15 of every tile, that is
//     list entries 64 t + 16 w + i, i = 0 .. 15, in eighteen loads per lane:
//       LATENT  eight 16-byte loads under fa_mla_sparse_kv8_kernel.hip's map: load i, lane -> row 2 i + lane / 32, e4m3 chunk lane % 32;
//       SCALE   the sixteen elements of chunk e lie wholly in group e / 8: ONE predicated dword at byte 512 + 4 (e / 8) of the same row,
//               issued with the chunk under the chunk's predicate -- eight per lane. (The other form was compiled next to this one:
//               the wave's sixty-four scales in ONE dword load, lane -> row lane / 4, scale lane % 4, handed out by eight
//               ds_bpermute in front of the writes. It holds one scale register across the arithmetic in place of eight and came out
//               at 256 VGPRs + 227 AGPRs against this form's 256 + 234, neither with scratch. Both fit the 512 registers of the one
//               wave per SIMD that the 144-KiB buffer allows, so the count decides nothing here; this file is the per-lane dword,
//               which puts no LDS round trip between the arithmetic of tile t and the writes of tile t + 1. See DESIGN.md 4.7v.)
//       ROTARY  the row holds bf16 already: 16 rows x 8 chunks = two 16-byte loads per lane under fa_mla_sparse_kernel.hip's map (load
//               k, lane -> row 8 k + lane / 8, chunk lane % 8 at byte 528), written unwidened at chunk ^ ((row >> 1) & 7) of the
//               head_dim-64 K image.
//   * DEQUANTISING, per dword of four codes: v_cvt_pk_f32_fp8 twice (exact), v_mul_f32 by the chunk's scale (one rounding to fp32; no
//     product is subnormal for 2^-64 <= |s| <= 2^64), v_cvt_pk_bf16_f32 (round to nearest even) -- into the e4m3 kernel's two
//     ds_write_b128 per load at its destination arithmetic. A NaN code or a NaN scale of a named row comes out NaN. The multiply is a
//     plain `*` under -ffp-contract=off: nothing fuses into it.
//   * THE ENTRIES, THE ROW ADDRESSES, THE ONE BARRIER PER TILE AND ITS UNIFORMITY are fa_mla_sparse_kv8_kernel.hip's, in its words: one
//     predicated dword of entries per wave, fetched one tile ahead (-1 behind the count); each lane takes ITS ROW's entry out of the entry
//     register (ds_bpermute: ten per tile, eight latent + two rotary), tests it with the one unsigned compare and forms
//     kv + (x >> lp) * page_stride + (x & (P - 1)) * row_stride for its loads under that predicate: an invalid entry gives zeros and
//     makes no load and no address -- its scale is then 0 and the chunk 0 * 0 = +0. The raw loads of tile t + 1 go out behind the barrier
//     of iteration t, the body's part 2 runs on tile t, then the registers are dequantised and written into the other buffer.
//   * REGISTERS: 32 latent + 8 scale + 8 rotary staging dwords per lane live across part 2, against the e4m3 kernel's 36. The compiled
//     kernel holds them without scratch, 256 VGPRs + 234 AGPRs (profiles/r34/mla_sparse_kv8_scaled_kernel_resources.log).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types, the launch tail

constexpr int MLA_SCALED_NW = 4;                        // waves of a workgroup, for every head count
constexpr int MLA_SCALED_SC = MLA_DV;                   // byte of a row's first scale
constexpr int MLA_SCALED_ROT = MLA_DV + 16;             // byte of a row's first rotary element
constexpr int MLA_SCALED_ROW = MLA_SCALED_ROT + MLA_RRB;  // 656
static_assert(MLA_SCALED_ROW == 656, "512 e4m3 + 4 fp32 + 64 bf16");

// 8 e4m3 (two dwords) of one scale group -> 8 bf16 (one 16-byte chunk): bf16_rne(fp32(code) * s), two roundings
__device__ __forceinline__ u32x4 mla_scaled_dequant8(unsigned w0, unsigned w1, float s) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  u32x4 out;
  const unsigned w[2] = {w0, w1};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    bf16x2 a, b;
    a[0] = (__bf16)(lo[0] * s); a[1] = (__bf16)(lo[1] * s);
    b[0] = (__bf16)(hi[0] * s); b[1] = (__bf16)(hi[1] * s);
    out[2 * j] = __builtin_bit_cast(unsigned, a);
    out[2 * j + 1] = __builtin_bit_cast(unsigned, b);
  }
  return out;
}

// workgroup (token, s) x row block wb, wave w: heads 16 (4 wb + w) + c of the token, entries of tiles [t0, t1) of its list
__global__ __launch_bounds__(64 * MLA_SCALED_NW) void mla_sparse_kv8_scaled_partial_kernel(MlaSparseParams p) {
  using M = ML16<BF16>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr bool CAUSAL = false;  // visibility is the list
  constexpr int NW = MLA_SCALED_NW;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // rows (= list entries) of a tile this wave stages: 16
  constexpr int NLL = RW / 2;                          // latent loads per lane and tile (two rows each), a scale dword with each
  constexpr int NRL = RW / 8;                          // rotary loads per lane and tile (eight rows each)
  static_assert(RW == 16, "sixteen entries per wave: one per lane of the first sixteen, two rotary pieces of eight rows");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;  // buffer u: latent part at u * MLA_IMG, rotary part behind it; shared by the NW waves

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, item = blockIdx.x, rb = blockIdx.y * NW + w;  // rb: the wave's 16-row slot
  const int b = item / S, s = item - b * S;                        // b: the token
  const int R = p.Hq * p.Nq;
  const bool live = rb < p.RBLK;  // wave-uniform; false: sixteen padding rows, a slot the workspace does not have
  const int Nk = p.counts ? min(max(__builtin_amdgcn_readfirstlane(p.counts[b]), 0), p.topk) : p.topk;  // n_t: entries of this token's list
  const int coff = Nk - p.Nq;
  const int nT = (Nk + BN - 1) / BN;
  const int t0 = (int)((long long)s * nT / S), t1 = (int)((long long)(s + 1) * nT / S);

#define FA_MLA_BODY_PART 1  // the Q fragments qf[] (pre-scaled; zeros in padding rows), the row limit rlim, the LDS read offsets
#include "fa_mla_body.h"

  // ---- staging: this wave moves rows jr0 .. jr0 + 15 of a tile (jr0 is a multiple of 16: the swizzle of row jr0 + j is that of row j).
  // latent load i: lane -> row 2 i + hi, hi = lane / 32, e4m3 chunk e = lane % 32 -> bf16 chunks 2 e, 2 e + 1 at ((2 e) & 15) ^ f(2 i + hi)
  // and that ^ 1 in 16-chunk group e / 8. f(2 i + hi) = (hi << 1) ^ C_i with C_i = (4 i & 12) ^ 9 (i >> 2) a constant of the load: one
  // per-lane offset, everything else is compile-time (fa_mla_sparse_kv8_kernel.hip's arithmetic)
  const int jr0 = RW * w;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const int hi = lane >> 5, le = lane & 31;
  const unsigned dst_l = (unsigned)(jr0 * MLA_LRB + hi * MLA_LRB + ((le >> 3) << 8) + ((((2 * le) & 15) ^ (hi << 1)) << 4));
  // rotary load k: lane -> row 8 k + drow, bf16 chunk dpc at byte 528 of the row (fa_mla_sparse_kernel.hip's map)
  const int drow = lane >> 3, dpc = lane & 7;
  // the lane's chunk, scale and rotary chunk of its row, from the pool's base: the row's offset is added per load
  const char *src_l = (const char *)p.kv + le * 16, *src_s = (const char *)p.kv + (MLA_SCALED_SC + 4 * (le >> 3));
  const char *src_r = (const char *)p.kv + (MLA_SCALED_ROT + dpc * 16);
  const unsigned rsb = (unsigned)p.row_stride;  // bytes; the rows of one page stay below 2 GiB
  const int *list = p.indices + (long long)b * p.idx_stride;

  // ev: lane i < 16 holds the entry of this wave's row i of the next tile to load, -1 behind the count; loaded one tile ahead
  int ev = -1;
  auto fetch_entries = [&](int t) __attribute__((always_inline)) {
    const int j = t * BN + jr0 + lane;
    ev = -1;
    if (lane < RW && j < Nk) ev = list[j];
  };
  u32x4 raw[NLL], rot[NRL];
  float sc[NLL];
  // the byte offset of slot x in the pool (x valid: page < num_pages, one page stays below 2 GiB)
  auto slot_off = [&](int x) __attribute__((always_inline)) {
    return (unsigned long long)((unsigned)x >> lp) * (unsigned long long)p.page_stride + (unsigned)(x & PM) * rsb;
  };
  // this wave's rows of the tile whose entries ev holds -> raw[], sc[], rot[]: every lane takes its rows' entries out of ev -- all ten
  // permutes first, under one wait, then the loads, each under its row's predicate. An entry behind the count (-1) or outside the pool:
  // zeros, no address, no load
  auto load_raw = [&]() __attribute__((always_inline)) {
    int xs[NLL + NRL];
#pragma unroll
    for (int i = 0; i < NLL; ++i) xs[i] = __shfl(ev, 2 * i + hi, 64);
#pragma unroll
    for (int k = 0; k < NRL; ++k) xs[NLL + k] = __shfl(ev, 8 * k + drow, 64);
#pragma unroll
    for (int i = 0; i < NLL; ++i) {
      raw[i] = u32x4{0u, 0u, 0u, 0u};
      sc[i] = 0.0f;
      if ((unsigned)xs[i] < (unsigned)p.num_slots) {
        const unsigned long long off = slot_off(xs[i]);
        raw[i] = *reinterpret_cast<const u32x4 *>(src_l + off);
        sc[i] = *reinterpret_cast<const float *>(src_s + off);
      }
    }
#pragma unroll
    for (int k = 0; k < NRL; ++k) {
      rot[k] = u32x4{0u, 0u, 0u, 0u};
      if ((unsigned)xs[NLL + k] < (unsigned)p.num_slots) rot[k] = *reinterpret_cast<const u32x4 *>(src_r + slot_off(xs[NLL + k]));
    }
  };
  // raw[], sc[], rot[] -> buffer buf: the latent chunks dequantised, the rotary chunks as they are
  auto write_tile = [&](int buf) __attribute__((always_inline)) {
    lds_char *img = smem + buf * MLA_IMG;
#pragma unroll
    for (int i = 0; i < NLL; ++i) {
      const int ci = ((4 * i) & 12) ^ (9 * (i >> 2));  // C_i
      const unsigned a = (dst_l ^ (unsigned)(ci << 4)) + (unsigned)(2 * i * MLA_LRB);
      lds_write_b128(img + a, mla_scaled_dequant8(raw[i][0], raw[i][1], sc[i]));
      lds_write_b128(img + (a ^ 16u), mla_scaled_dequant8(raw[i][2], raw[i][3], sc[i]));
    }
#pragma unroll
    for (int k = 0; k < NRL; ++k) {
      const int row = jr0 + 8 * k + drow;
      lds_write_b128(img + (unsigned)(MLA_LAT + row * MLA_RRB + ((dpc ^ ((row >> 1) & 7)) << 4)), rot[k]);
    }
  };

  f32x4 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[dt][i] = 0.0f;
  float m = -INFINITY, l = 0.0f;

  // the prologue: tile t0 into buffer 0. Every wave of the workgroup takes the same branch and runs the same iterations (see the head)
  if (t0 < t1) {
    fetch_entries(t0);
    load_raw();
    fetch_entries(t0 + 1);
    write_tile(0);
  }
  for (int t = t0; t < t1; ++t) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's writes of tile t have landed, its reads of tile t - 1 are back
    __builtin_amdgcn_s_barrier();                       // everyone's have
    if (t + 1 < t1) load_raw();                         // (ev: the entries of tile t + 1)
    if (live) {
#define FA_MLA_BODY_PART 2  // tile t: 18 k-steps of scores, the mask, the online softmax, 64 PV steps
#include "fa_mla_body.h"
    }
    if (t + 1 < t1) {
      write_tile((t + 1 - t0) & 1);
      fetch_entries(t + 2);  // (behind the writes; positions >= n_t are not read)
    }
  }

  if (live) {
#define FA_MLA_BODY_PART 3  // the partial (O . l, m, l) -> workspace slot (item, rb)
#include "fa_mla_body.h"
  }
}

// One call: the partial kernel over T . S items x ceil(RBLK / 4) row blocks of four waves, then fa_mla_kernel.hip's bf16 combine kernel
// over the output rows (pc: the call as that kernel sees it, B = T, Nq = 1), on the same stream
hipError_t launch_mla_decode_sparse_kv8_scaled(const MlaSparseParams &p, const MlaDecodeParams &pc, hipStream_t s) {
  return launch_mla_partial_and_combine(mla_sparse_kv8_scaled_partial_kernel, dim3(p.T * p.S, (p.RBLK + MLA_SCALED_NW - 1) / MLA_SCALED_NW),
                                        MLA_SCALED_NW, p, pc, FA_DTYPE_BF16, s);
}

}  // namespace fa
