// fa_mla_paged_partial.inc -- the body of the partial kernel of the absorbed latent-attention decode over a paged 16-bit pool, as TEXT that
// mla_partial_kernel (fa_mla_kernel.hip: NW = 1, one wave per item, a private double buffer) and mla_wide_partial_kernel
// (fa_mla_wide_kernel.hip: NW = 2 or 4 waves over one shared double buffer) include, in the manner of fa_bwd_dq_body.inc and fa_mla_body.h.
// Text and not a function called from two thin kernels: as an inlined function template, its parameters by reference or by value, the same
// statements came out with other registers and a few instructions fewer or more in every one of the twelve kernels.
// In scope: Tag, CAUSAL, NW (a constant expression), p (MlaDecodeParams), and the macro FA_MLA_PG_DECL, which declares int pg[MAXPG] with
// every entry -1; the text undefines it. (The one statement whose spelling the compiler is sensitive to: see the two definitions.)
//
// Workgroup (b, s) x row block blockIdx.y, wave w: rows r = 16 rb + c = h * Nq + iq of the packed block, rb = blockIdx.y * NW + w the wave's
// 16-row slot, keys of tiles [t0, t1) of sequence b. What a wave does with its 16 rows from LDS onwards is fa_mla_body.h, parts 1 - 3.
//   * STAGING, the memory-safety boundary of the call. Wave w moves latent rows jr0 = (64 / NW) w .. + 64 / NW - 1 of every tile (one 1-KiB
//     LDS-DMA piece per row) and the rotary pieces over the same rows (eight rows per piece): 64 + 8 pieces with NW = 1, 32 + 4 with NW = 2,
//     16 + 2 with NW = 4. The rows lie in max(1, (64 / NW) / P) pages of P = 2^lp keys: four at most (NW = 1, pages of 16), one for every
//     page size with NW = 4. Each page gets ONE descriptor, built on the page's 64-bit base, with num_records = (valid rows - 1) *
//     row_stride + 1152 bytes -- the page's rows below L_b only -- and 0 for a page past L_b or an index outside the pool: such pieces land
//     as hardware zeros and no address is formed from the index. The whole offset of a piece sits in voffset, inside the range check. The
//     table entries are fetched one tile ahead, the table index clamped to max_pages - 1. The chunk swizzles of the image (the head of
//     fa_mla_kernel.hip) sit on the source offsets.
//   * ONE BARRIER PER TILE (NW > 1), at the top of iteration t: s_waitcnt vmcnt(0) (this wave's pieces of tile t have landed), then
//     s_barrier (everyone's have, and everyone has left iteration t - 1, whose buffer tile t + 1 is about to overwrite), then tile t + 1 is
//     staged. The barrier is the raw instruction behind the explicit wait: nothing else is drained. With NW = 1 the wave issued every piece
//     itself and the wait alone serves.
//   * BARRIER UNIFORMITY. (b, s) and with them Nk, [t0, t1) come from blockIdx.x and scalars: the same in all waves of a workgroup. The
//     loop runs t = t0 - 1 .. t1 - 1 in every wave -- once for an empty split -- and nothing leaves it early. A wave whose 16 rows are all
//     padding (slot >= RBLK; NW > 1 only: the one-wave grid has RBLK row blocks) stages its share of every tile and meets every barrier; it
//     skips the arithmetic under a wave-uniform branch and stores nothing: its workspace slot does not exist.
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // latent rows (= 1-KiB pieces) of a tile this wave stages; RW / 8 rotary pieces
  static_assert(NW == 1 || NW == 2 || NW == 4, "one, two or four waves: 64, 32 or 16 rows of a tile each, whole 8-row rotary pieces");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;  // buffer u: latent part at u * MLA_IMG, rotary part behind it; shared by the NW waves

  const int lane = NW > 1 ? threadIdx.x & 63 : threadIdx.x;
  const int w = NW > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, item = blockIdx.x, rb = blockIdx.y * NW + w;  // rb: the wave's 16-row slot
  const int b = item / S, s = item - b * S;
  const int R = p.Hq * p.Nq;
  const bool live = NW == 1 || rb < p.RBLK;  // wave-uniform; false: sixteen padding rows, a slot the workspace does not have
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

  // ---- pg[] holds the table entries of this wave's rows of the next tile to stage (max(1, RW / P) pages), loaded one tile ahead
  const int lp = p.lp;
  const unsigned rsb = (unsigned)p.row_stride * 2;  // the pool's row stride in bytes
  const unsigned dma_rrow = (unsigned)drow * rsb;
  constexpr int MAXPG = RW / 16;
  FA_MLA_PG_DECL
#undef FA_MLA_PG_DECL
  auto fetch_pages = [&](int t) __attribute__((always_inline)) {
    const int *tbl = p.block_table + (long long)b * p.bt_stride;
    const int i0 = (t * BN + jr0) >> lp, npg = max(1, RW >> lp);  // (pages of RW keys and more: the one page of the wave's rows)
#pragma unroll
    for (int k = 0; k < MAXPG; ++k) pg[k] = k < npg ? tbl[min(i0 + k, p.max_pages - 1)] : -1;  // (never past the row's max_pages entries)
  };
  // stage this wave's rows of tile t into buffer buf. LPC = min(lp, 6): the rows' max(1, RW / 2^LPC) pages are compile-time entries of
  // pg[], one descriptor each, built on the page's 64-bit base with a range that covers only the page's valid rows
  auto stage = [&](auto lpc, int t, int buf) __attribute__((always_inline)) {
    constexpr int LPC = decltype(lpc)::value, NPG = (RW >> LPC) > 0 ? (RW >> LPC) : 1, PM = (1 << LPC) - 1;
    const int P = 1 << lp, key0 = (t * BN + jr0) & -P;  // first key of the first page this wave reads
    // this wave's first slot in it: 0 where the wave's rows fill whole pages. (Spelled as a constant for the one wave that stages whole
    // tiles; the same condition for NW > 1, (RW >> LPC) > 0, is also right and moves those kernels by an instruction each)
    const unsigned row0 = (NW == 1 && LPC < 6) ? 0u : (unsigned)((t * BN + jr0) & (P - 1));
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
  // Every wave of the workgroup runs every iteration and meets the barrier in each: see the head of the text
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of tile t have landed
    if constexpr (NW > 1) __builtin_amdgcn_s_barrier();  // everyone's have, and everyone is done reading the buffer tile t + 1 overwrites
    if (t + 1 < t1) {
      const int nb = (t + 1 - t0) & 1;
      if (lp == 4) stage(std::integral_constant<int, 4>{}, t + 1, nb);
      else if (lp == 5) stage(std::integral_constant<int, 5>{}, t + 1, nb);
      else stage(std::integral_constant<int, 6>{}, t + 1, nb);
    }
    if (t < t0 || !live) continue;
#define FA_MLA_BODY_PART 2  // tile t: 18 k-steps of scores, the mask, the online softmax, 64 PV steps
#include "fa_mla_body.h"
  }

  if (live) {
#define FA_MLA_BODY_PART 3  // the partial (O . l, m, l) -> workspace slot (item, rb)
#include "fa_mla_body.h"
  }
