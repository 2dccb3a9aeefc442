// fa_mla_kv8_kernel.hip -- the absorbed latent-attention decode over an e4m3 latent pool: entry point fa_fwd_mla_decode_paged_kv8.
//
// fa_mla_wide_kernel.hip's four-wave workgroup over one shared double buffer, with ONE difference: the pool holds OCP e4m3 bytes (576 per
// key), so a tile cannot be moved by LDS-DMA. It is staged through registers, as fa_decode_kernel.hip (widen8) and the KV8 mode of
// fa_mfma_kernel.hip (fp8x8_to_bf16) stage theirs: raw 16-byte loads, widened exactly to bf16 (every e4m3 value, subnormals and -0
// included, is a bf16 value), written into THE SAME IMAGE under the same two swizzles. Everything from LDS onwards is the wide kernel's
// text (fa_mla_body.h parts 0 - 3), the workspace format and the combine kernel are unchanged: O and LSE are the bits of
// fa_fwd_mla_decode_paged_wide (bf16) on the pool widened element by element.
//   * ALWAYS FOUR WAVES. Wave w stages rows 16 w .. 16 w + 15 of every tile: 16 x 576 bytes = nine 16-byte loads per lane, eight latent
//     (32 chunks per row, two rows per load: lane -> row 2 i + lane / 32, chunk lane % 32) and one rotary (4 chunks per row: lane -> row
//     lane / 4, chunk lane % 4 behind the row's 512 latent bytes). Sixteen rows lie inside one page for every page size: one range-checked
//     descriptor per wave and tile, num_records = (valid rows - 1) * row_stride + 576 bytes, 0 for a page past L_b or an index outside the
//     pool, the whole offset in voffset. (Two waves would hold 72 staging registers next to the body's: no two-wave form. For <= 32 rows
//     the split rule is still fed one workgroup row block, as the wide call's two-wave form feeds it: the same S.)
//   * e4m3 chunk e of a latent row becomes bf16 chunks 2 e and 2 e + 1: two ds_write_b128 at (2 e) ^ f(row & 15) and (2 e + 1) ^ f(row & 15)
//     within the row's 16-chunk group -- the second address is the first ^ 16. The rotary chunk likewise under chunk ^ ((row >> 1) & 7).
//   * ONE BARRIER PER TILE, at the top of iteration t: s_waitcnt lgkmcnt(0) (this wave's LDS writes of tile t have landed and its reads
//     of tile t - 1 have returned), then the raw s_barrier (everyone's have). Then the raw loads of tile t + 1 go out into registers, the
//     body's part 2 runs on tile t, and last the registers are widened and written into the other buffer, which nobody reads before the
//     next barrier. The prologue loads and writes tile t0.
//   * BARRIER UNIFORMITY: as in fa_mla_paged_partial.inc. (b, s), Nk and [t0, t1) are the same in all waves of a workgroup; every wave runs
//     every iteration; a wave whose 16 rows are all padding stages its share, meets every barrier, skips the arithmetic, stores nothing.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types, the launch tail

constexpr int MLA_KV8_NW = 4;  // waves of a workgroup, for every row count

// 8 e4m3 (two dwords) -> 8 bf16 (one 16-byte chunk): exact (bf16 = the upper half of the fp32 pattern; fa_decode_kernel.hip's widen8)
__device__ __forceinline__ u32x4 mla_widen8(unsigned w0, unsigned w1) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  unsigned r[4];
  const unsigned w[2] = {w0, w1};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    const float a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];  // (scalar temporaries: bit_cast on a vector element expression reads element 0)
    r[2 * j] = (__builtin_bit_cast(unsigned, a0) >> 16) | (__builtin_bit_cast(unsigned, a1) & 0xffff0000u);
    r[2 * j + 1] = (__builtin_bit_cast(unsigned, b0) >> 16) | (__builtin_bit_cast(unsigned, b1) & 0xffff0000u);
  }
  return u32x4{r[0], r[1], r[2], r[3]};
}

// workgroup (b, s) x row block wb, wave w: rows r = 16 (4 wb + w) + c of the packed block, keys of tiles [t0, t1) of sequence b
template <bool CAUSAL>
__global__ __launch_bounds__(64 * MLA_KV8_NW) void mla_kv8_partial_kernel(MlaDecodeParams p) {
  using M = ML16<BF16>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int NW = MLA_KV8_NW;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // rows of a tile this wave stages: 16
  constexpr int NLL = RW / 2;                          // latent loads per lane and tile (two rows each); one rotary load besides
  static_assert(RW == 16, "sixteen rows per wave: inside one page of every size, one rotary load of 64 chunks");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;  // buffer u: latent part at u * MLA_IMG, rotary part behind it; shared by the NW waves

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, item = blockIdx.x, rb = blockIdx.y * NW + w;  // rb: the wave's 16-row slot
  const int b = item / S, s = item - b * S;
  const int R = p.Hq * p.Nq;
  const bool live = rb < p.RBLK;  // wave-uniform; false: sixteen padding rows, a slot the workspace does not have
  const int Nk = min(max(__builtin_amdgcn_readfirstlane(p.seqlens[b]), 0), p.max_pages << p.lp);  // keys of this workgroup's sequence
  const int coff = Nk - p.Nq;
  const int nT = (Nk + BN - 1) / BN;
  const int t0 = (int)((long long)s * nT / S), t1 = (int)((long long)(s + 1) * nT / S);

#define FA_MLA_BODY_PART 1  // the Q fragments qf[] (pre-scaled; zeros in padding rows), the row limit rlim, the LDS read offsets
#include "fa_mla_body.h"

  // ---- staging: this wave moves rows jr0 .. jr0 + 15 of a tile (jr0 is a multiple of 16: the swizzle of row jr0 + j is that of row j).
  // latent load i: lane -> row 2 i + hi, hi = lane / 32, e4m3 chunk e = lane % 32 -> bf16 chunks 2 e, 2 e + 1 at ((2 e) & 15) ^ f(2 i + hi)
  // and that ^ 1 in 16-chunk group e / 8. f(2 i + hi) = (hi << 1) ^ C_i with C_i = (4 i & 12) ^ 9 (i >> 2) a constant of the load: one
  // per-lane offset, everything else is compile-time
  const int jr0 = RW * w;
  const int hi = lane >> 5, le = lane & 31;
  const unsigned rsb = (unsigned)p.row_stride;  // the pool's row stride in bytes (e4m3: elements are bytes)
  const unsigned src_l = (unsigned)hi * rsb + (unsigned)le * 16;
  const unsigned dst_l = (unsigned)(jr0 * MLA_LRB + hi * MLA_LRB + ((le >> 3) << 8) + ((((2 * le) & 15) ^ (hi << 1)) << 4));
  // rotary load: lane -> row rr = lane / 4, e4m3 chunk lane % 4 at byte 512 of the row -> bf16 chunks 2 e, 2 e + 1 of the head_dim-64 K
  // image, chunk ^ ((row >> 1) & 7)
  const int rr = lane >> 2, re = lane & 3;
  const unsigned src_r = (unsigned)rr * rsb + (unsigned)(MLA_DV + re * 16);
  const unsigned dst_r = (unsigned)(MLA_LAT + (jr0 + rr) * MLA_RRB + (((2 * re) ^ ((rr >> 1) & 7)) << 4));

  // ---- pg holds the table entry of this wave's rows of the next tile to load, fetched one tile ahead. The table is read through the
  // constant address space: no kernel of the call writes it, the index is wave-uniform, so the fetch is a scalar load that the vector
  // memory counter, which tells when the raw loads are back, never sees
  const int lp = p.lp;
  int pg = -1;
  auto fetch_page = [&](int t) __attribute__((always_inline)) {
    typedef const __attribute__((address_space(4))) int *const_int_ptr;
    const_int_ptr tbl = (const_int_ptr)(__UINTPTR_TYPE__)(p.block_table + (long long)b * p.bt_stride);
    pg = tbl[min((t * BN + jr0) >> lp, p.max_pages - 1)];  // (never past the row's max_pages entries)
  };
  u32x4 raw[NLL + 1];
  // this wave's rows of tile t -> raw[]: one descriptor, built on the page's 64-bit base with a range that covers only the page's valid rows
  auto load_raw = [&](int t) __attribute__((always_inline)) {
    const int P = 1 << lp, key0 = (t * BN + jr0) & -P;           // first key of the page this wave reads
    const unsigned row0 = (unsigned)((t * BN + jr0) & (P - 1));  // this wave's first slot in it
    const int page = __builtin_amdgcn_readfirstlane(pg);
    const int nv = min(Nk - key0, P);                                  // valid rows of the page
    const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;  // an index outside the pool reads as zeros
    const long long off = ok ? (long long)page * p.page_stride : 0;
    const unsigned nrec = ok ? (unsigned)(nv - 1) * rsb + MLA_DQK : 0u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.kv + off), 0, nrec, 0x00020000);
    const unsigned so = row0 * rsb;  // (the whole offset in voffset: inside the range check)
#pragma unroll
    for (int i = 0; i < NLL; ++i) raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, so + (unsigned)(2 * i) * rsb + src_l, 0, 0);
    raw[NLL] = __builtin_amdgcn_raw_buffer_load_b128(rs, so + src_r, 0, 0);
  };
  // raw[] -> buffer buf, widened
  auto write_tile = [&](int buf) __attribute__((always_inline)) {
    lds_char *img = smem + buf * MLA_IMG;
#pragma unroll
    for (int i = 0; i < NLL; ++i) {
      const int ci = ((4 * i) & 12) ^ (9 * (i >> 2));  // C_i
      const unsigned a = (dst_l ^ (unsigned)(ci << 4)) + (unsigned)(2 * i * MLA_LRB);
      lds_write_b128(img + a, mla_widen8(raw[i][0], raw[i][1]));
      lds_write_b128(img + (a ^ 16u), mla_widen8(raw[i][2], raw[i][3]));
    }
    lds_write_b128(img + dst_r, mla_widen8(raw[NLL][0], raw[NLL][1]));
    lds_write_b128(img + (dst_r ^ 16u), mla_widen8(raw[NLL][2], raw[NLL][3]));
  };

  f32x4 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[dt][i] = 0.0f;
  float m = -INFINITY, l = 0.0f;

  // the prologue: tile t0 into buffer 0. Every wave of the workgroup takes the same branch and runs the same iterations (see the head)
  if (t0 < t1) {
    fetch_page(t0);
    load_raw(t0);
    fetch_page(t0 + 1);
    write_tile(0);
  }
  for (int t = t0; t < t1; ++t) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's writes of tile t have landed, its reads of tile t - 1 are back
    __builtin_amdgcn_s_barrier();                       // everyone's have
    if (t + 1 < t1) load_raw(t + 1);
    if (live) {
#define FA_MLA_BODY_PART 2  // tile t: 18 k-steps of scores, the mask, the online softmax, 64 PV steps
#include "fa_mla_body.h"
    }
    if (t + 1 < t1) {
      write_tile((t + 1 - t0) & 1);
      fetch_page(t + 2);  // (behind the writes: the wait at the top of the next iteration covers it)
    }
  }

  if (live) {
#define FA_MLA_BODY_PART 3  // the partial (O . l, m, l) -> workspace slot (item, rb)
#include "fa_mla_body.h"
  }
}

// the wide call's sizes: the split rule fed ceil(rows / 64) workgroup row blocks gives the wide call's S for every legal row count
// (<= 32 rows: one block there as here)
long long mla_decode_kv8_workspace_bytes(int B, int Hq, int Nq, int Nk) { return mla_decode_wide_workspace_bytes(B, Hq, Nq, Nk); }

// One call: the partial kernel over B . S items x ceil(RBLK / 4) row blocks of four waves, then fa_mla_kernel.hip's bf16 combine kernel
// over the output rows, on the same stream
hipError_t launch_mla_decode_paged_kv8(const MlaDecodeParams &p, hipStream_t s) {
  auto go = [&](auto partial) {
    return launch_mla_partial_and_combine(partial, dim3(p.B * p.S, (p.RBLK + MLA_KV8_NW - 1) / MLA_KV8_NW), MLA_KV8_NW, p, p, FA_DTYPE_BF16, s);
  };
  return p.is_causal ? go(mla_kv8_partial_kernel<true>) : go(mla_kv8_partial_kernel<false>);
}

}  // namespace fa
