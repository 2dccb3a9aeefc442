// fa_mla_wide_kernel.hip -- the absorbed latent-attention decode for up to 128 packed query rows: entry point fa_fwd_mla_decode_paged_wide.
//
// fa_mla_kernel.hip gives every 16 packed rows a one-wave item of their own that streams the sequence's 72-KiB tiles through a private
// double buffer: 32 rows stream every latent row twice, and the one wave issues all 72 LDS-DMA pieces of a tile between its own 200 LDS
// reads and 136 MFMAs. Here a WORKGROUP of NW waves (2 up to 32 rows, 4 above) shares ONE double buffer:
//   * wave w of row block wb IS that one-wave item on rows r = 16 (wb NW + w) + c = h * Nq + iq: the text of fa_mla_body.h, so the same
//     Q~ fragments, the same 18 k-steps in the same order, the same mask, online softmax, 64 PV steps and partial store -- the same bits;
//   * the image and its two swizzles are fa_mla_kernel.hip's (every wave's read pattern is the one whose conflict-freedom is argued at
//     the head of that file); each latent row is streamed once for 16 NW query rows;
//   * wave w stages latent rows (64 / NW) w .. + 64 / NW - 1 of every tile and the rotary pieces over the same rows: 16 + 2 pieces with
//     NW = 4 (all inside ONE page for every page size: one descriptor per wave and tile), 32 + 4 with NW = 2 (two pages of 16, else one).
//     The descriptor rules are unchanged: the whole offset in voffset, num_records over the page's valid rows only, 0 for a page past L_b or
//     an index outside the pool; table entries fetched one tile ahead and clamped to max_pages - 1;
//   * ONE BARRIER PER TILE, at the top of iteration t: s_waitcnt vmcnt(0) (this wave's pieces of tile t have landed), then s_barrier
//     (everyone's have, and everyone has left iteration t - 1, whose buffer tile t + 1 is about to overwrite), then tile t + 1 is staged.
//     The barrier is the raw instruction behind the explicit wait: nothing else is drained.
//   * BARRIER UNIFORMITY. (b, s) and with them Nk, [t0, t1) come from blockIdx.x and scalars: the same in all waves of a workgroup. The
//     loop runs t = t0 - 1 .. t1 - 1 in every wave -- once for an empty split -- and nothing leaves it early. A wave whose 16 rows are all
//     padding (slot >= RBLK) stages its share of every tile and meets every barrier; it skips the arithmetic under a wave-uniform branch
//     and stores nothing: its workspace slot does not exist.
//   * the workspace keeps fa_mla_kernel.hip's format, [B . S][RBLK = ceil(Hq Nq / 16)][MLA_IST] with wave w of block wb on 16-row slot
//     wb NW + w, so that file's combine kernel serves this call unchanged (launch_mla_combine).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

// the tile's shape and image: fa_mla_kernel.hip's constants (stated in each file; fa_mla_body.h is written against them)
constexpr int MLA_DQK = 576, MLA_DV = 512, MLA_DR = MLA_DQK - MLA_DV;
constexpr int MLA_LRB = MLA_DV * 2, MLA_RRB = MLA_DR * 2;              // row bytes of the latent / rotary part
constexpr int MLA_LAT = BN * MLA_LRB, MLA_ROT = BN * MLA_RRB;          // bytes of a tile's two parts
constexpr int MLA_IMG = MLA_LAT + MLA_ROT;                             // one tile: 72 KiB
constexpr size_t mla_lds_bytes() { return 2 * (size_t)MLA_IMG; }       // the double buffer
constexpr int MLA_IST = 16 * (MLA_DV + 2);                             // floats of one 16-row slot's partial: [16][512] O . l, then [16][2] (m, l)
__host__ __device__ constexpr int mla_swz(int r) { return (((r & 7) << 1) ^ (9 * ((r >> 3) & 1))) & 15; }

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"

// workgroup (b, s) x row block wb, wave w: rows r = 16 (wb NW + w) + c of the packed block, keys of tiles [t0, t1) of sequence b
template <typename Tag, bool CAUSAL, int NW>
__global__ __launch_bounds__(64 * NW) void mla_wide_partial_kernel(MlaDecodeParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // latent rows (= 1-KiB pieces) of a tile this wave stages; RW / 8 rotary pieces
  static_assert(NW == 2 || NW == 4, "two or four waves: 32 or 16 rows of a tile each, whole 8-row rotary pieces");

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

  // ---- LDS-DMA: this wave moves rows jr0 .. jr0 + RW - 1 of a tile, the chunk swizzle sits on the source address (jr0 is a multiple of
  // 16: the swizzle of row jr0 + j is that of row j, and rotary piece jr0 / 8 + j has the parity of j).
  // latent piece = one row of the tile: lane -> chunk lane ^ f(row & 15); rotary piece = eight rows: lane -> row lane / 8,
  // chunk (lane % 8) ^ ((row >> 1) & 7) behind the row's 512 latent elements
  const int jr0 = RW * w;
  const unsigned dma_l0 = (unsigned)lane << 4;
  const int drow = lane >> 3, dpc = lane & 7;
  const unsigned dma_r0 = (unsigned)(MLA_LRB + ((dpc ^ (drow >> 1)) << 4));

  // ---- pg[] holds the table entries of this wave's rows of the next tile to stage (max(1, RW / P) pages: two with NW = 2 and pages of
  // 16, one otherwise), loaded one tile ahead
  const int lp = p.lp;
  const unsigned rsb = (unsigned)p.row_stride * 2;  // the pool's row stride in bytes
  const unsigned dma_rrow = (unsigned)drow * rsb;
  constexpr int MAXPG = RW / 16;
  int pg[MAXPG];
#pragma unroll
  for (int k = 0; k < MAXPG; ++k) pg[k] = -1;
  auto fetch_pages = [&](int t) __attribute__((always_inline)) {
    const int *tbl = p.block_table + (long long)b * p.bt_stride;
    const int i0 = (t * BN + jr0) >> lp, npg = max(1, RW >> lp);  // (pages of 64 keys and more: the tile's one page)
#pragma unroll
    for (int k = 0; k < MAXPG; ++k) pg[k] = k < npg ? tbl[min(i0 + k, p.max_pages - 1)] : -1;  // (never past the row's max_pages entries)
  };
  // stage this wave's rows of tile t into buffer buf. LPC = min(lp, 6): the rows' max(1, RW / 2^LPC) pages are compile-time entries of
  // pg[], one descriptor each, built on the page's 64-bit base with a range that covers only the page's valid rows
  auto stage = [&](auto lpc, int t, int buf) __attribute__((always_inline)) {
    constexpr int LPC = decltype(lpc)::value, NPG = (RW >> LPC) > 0 ? (RW >> LPC) : 1, PM = (1 << LPC) - 1;
    const int P = 1 << lp, key0 = (t * BN + jr0) & -P;  // first key of the first page this wave reads
    const unsigned row0 = (unsigned)((t * BN + jr0) & (P - 1));  // this wave's first slot in it (0 where the wave's rows fill whole pages)
    __amdgpu_buffer_rsrc_t rs[NPG];
#pragma unroll
    for (int k = 0; k < NPG; ++k) {
      const int page = __builtin_amdgcn_readfirstlane(pg[k]);
      const int nv = min(Nk - (key0 + k * P), P);  // valid rows of the page
      const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;  // an index outside the pool reads as zeros
      const long long off = ok ? (long long)page * p.page_stride : 0;
      const unsigned nrec = ok ? (unsigned)(nv - 1) * rsb + MLA_DQK * 2 : 0u;
      rs[k] = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.kv + off * 2), 0, nrec, 0x00020000);
    }
    const unsigned lbase = (unsigned)(__UINTPTR_TYPE__)smem + buf * MLA_IMG;
    const unsigned ll = lbase + jr0 * MLA_LRB, lr = lbase + MLA_LAT + (jr0 >> 3) * 1024;  // this wave's first latent / rotary piece
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const unsigned so = (row0 + (unsigned)(NPG > 1 ? (j & PM) : j)) * rsb;  // (the whole offset in voffset: inside the range check)
      const unsigned vo = so + (dma_l0 ^ (unsigned)(mla_swz(j & 15) << 4));
      const unsigned ld = ll + j * MLA_LRB;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs[NPG > 1 ? (j >> LPC) : 0]) : "memory");
    }
#pragma unroll
    for (int j = 0; j < RW / 8; ++j) {
      const unsigned so = (row0 + (unsigned)(NPG > 1 ? ((8 * j) & PM) : 8 * j)) * rsb + dma_rrow;
      const unsigned vo = so + (dma_r0 ^ (unsigned)((j & 1) << 6));  // ((row >> 1) & 7) gains 4 on odd pieces
      const unsigned ld = lr + j * 1024;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs[NPG > 1 ? ((8 * j) >> LPC) : 0]) : "memory");
    }
    fetch_pages(t + 1);
  };

  f32x4 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[dt][i] = 0.0f;
  float m = -INFINITY, l = 0.0f;

  if (t0 < t1) fetch_pages(t0);
  // iteration t: wait for tile t, stage tile t + 1 under its arithmetic; iteration t0 - 1 only stages tile t0 (one staging site).
  // Every wave of the workgroup runs every iteration and meets the barrier in each: see the head of the file
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of tile t have landed
    __builtin_amdgcn_s_barrier();                     // everyone's have, and everyone is done reading the buffer tile t + 1 overwrites
    if (t + 1 < t1) {
      const int nb = (t + 1 - t0) & 1;
      if (lp == 4) stage(std::integral_constant<int, 4>{}, t + 1, nb);
      else if (lp == 5) stage(std::integral_constant<int, 5>{}, t + 1, nb);
      else stage(std::integral_constant<int, 6>{}, t + 1, nb);
    }
    if (t >= t0 && live) {
#define FA_MLA_BODY_PART 2  // tile t: 18 k-steps of scores, the mask, the online softmax, 64 PV steps
#include "fa_mla_body.h"
    }
  }

  if (live) {
#define FA_MLA_BODY_PART 3  // the partial (O . l, m, l) -> workspace slot (item, rb)
#include "fa_mla_body.h"
  }
}

long long mla_decode_wide_workspace_bytes(int B, int Hq, int Nq, int Nk) {
  const int rows = Hq * Nq, rblk = (rows + 15) / 16, nw = mla_wide_waves(rows);
  return (long long)B * mla_decode_splits(B, (rblk + nw - 1) / nw, Nk) * rblk * MLA_IST * 4;
}

// One call: the partial kernel over B . S items x ceil(RBLK / NW) row blocks of NW waves, then fa_mla_kernel.hip's combine kernel over
// the output rows, on the same stream
hipError_t launch_mla_decode_paged_wide(const MlaDecodeParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    auto go = [&](auto partial, int nw) {
      (void)hipGetLastError();
      hipError_t e = set_dyn_lds_once((const void *)partial, (int)mla_lds_bytes());
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(partial, dim3(p.B * p.S, (p.RBLK + nw - 1) / nw), dim3(64 * nw), mla_lds_bytes(), s, p);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
      return launch_mla_combine(p, dtype, s);
    };
    if (mla_wide_waves(p.Hq * p.Nq) == 2) return p.is_causal ? go(mla_wide_partial_kernel<Tag, true, 2>, 2) : go(mla_wide_partial_kernel<Tag, false, 2>, 2);
    return p.is_causal ? go(mla_wide_partial_kernel<Tag, true, 4>, 4) : go(mla_wide_partial_kernel<Tag, false, 4>, 4);
  });
}

}  // namespace fa
