// fa_mla_kernel.hip -- absorbed multi-head latent attention, decode form, over a paged latent cache: entry point fa_fwd_mla_decode_paged.
//
// Every query head of a sequence reads ONE shared latent row per key: 576 elements, of which all 576 take part in the score product
// (512 of compressed KV plus 64 of rotary key) and the first 512 are the value. This is fa_decode_kernel.hip's paged decode with one
// pool, two head dims and one LDS image for both products; what it keeps of that kernel, line for line where the shapes allow:
//   * the packed row block: r = h * Nq + iq (every query head shares the one latent "key head": G = Hq), 16 rows per item;
//   * the keys of a sequence SPLIT over S one-wave items (no barrier anywhere), 64-key tiles streamed through a private double buffer
//     in LDS by LDS-DMA, 16x16x32 MFMA, the exact online softmax, the pre-scaled query operand Q~ = round(scale . log2(e) . Q);
//   * per-page range-checked descriptors with the whole offset in voffset (rows >= L_b, pages outside the pool: hardware zeros),
//     table entries fetched one tile ahead and clamped to max_pages - 1;
//   * partial (O . l, m, l) in the caller's workspace, a second launch that combines the S partials of a row by their maxima.
// What is new:
//   * THE IMAGE. A 64-key tile is a latent part [64][512] (rows of 1024 B: one 1-KiB LDS-DMA piece per row) and a rotary part [64][64]
//     (rows of 128 B, eight rows per piece: the head_dim-64 K image of fa_decode_kernel.hip), both staged from the same 1152-byte pool
//     row. The score product runs 16 + 2 k-steps over both parts (ds_read_b128), the PV product reads 32 d-tiles from the latent part
//     alone (ds_read_b64_tr_b16): 72 KiB per tile, 144 KiB double-buffered, one item per CU.
//   * ONE SWIZZLE FOR BOTH READ PATTERNS of the latent part: 16-byte chunk ^ f(row & 15), f(r) = ((r & 7) << 1) ^ (9 . (r >> 3)),
//     on the low four chunk bits (a row is 64 chunks; rows start 256 dwords apart, i.e. all on bank 0 of the 64-dword modulus).
//       - score product: lane (c, g) reads row 16 kt + c, chunk (4 ks + g) ^ f(c). ds_read_b128 is served in four groups of 16 lanes,
//         each group c in {0-3, 12-15} of an even g with c in {4-11} of the odd g beside it (or the other way round). f is a
//         permutation of 0..15 and maps {4..11} onto {8..15}, a set closed under ^ 1, so the two halves of a group land on
//         disjoint chunk sets: 16 distinct chunks of one 256-byte window, every bank once. Conflict-free.
//       - PV product: lane (g, vq, vp) reads 8 bytes of row 4 g + vq, chunk pair dt. ds_read_b64_tr_b16 is served in two groups of 32
//         lanes: rows 0..7, then rows 8..15; f(r) >> 1 is a bijection of each onto 0..7, so eight rows' 32-byte pairs tile one
//         256-byte window. Conflict-free.
//     fa_decode_kernel.hip's K swizzle (chunk ^ row & 15) puts rows 2i, 2i + 1 on one chunk pair (two-way on every PV read); its V
//     swizzle (chunk ^ (row & 7) << 1) puts rows c, c + 8 on one chunk (two-way on every score read). A second copy does not fit.
//   * ROWS 17..32 are two 16-row items over the same keys (blockIdx.y: the row block). A 32-row item would hold 256 accumulator and
//     144 query-fragment registers before a single score or address: no room in the 512-entry file without scratch.
//     (fa_mla_wide_kernel.hip, fa_fwd_mla_decode_paged_wide: two or four such items as the waves of ONE workgroup over a shared tile, up
//     to 128 rows. What a wave does with its 16 rows is the text of fa_mla_body.h, included below and there.)
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

#ifndef FA_MLA_MIN_TILES
#define FA_MLA_MIN_TILES 4  // 64-key tiles per item at least, so that an item's prologue amortises (the decode's constant)
#endif
#ifndef FA_MLA_ROUNDS
#define FA_MLA_ROUNDS 1  // rounds of the chip's 256 item slots (144 KiB of LDS: one item per CU) the splits aim for
#endif

namespace fa {

constexpr int MLA_DQK = 576, MLA_DV = 512, MLA_DR = MLA_DQK - MLA_DV;
constexpr int MLA_LRB = MLA_DV * 2, MLA_RRB = MLA_DR * 2;              // row bytes of the latent / rotary part
constexpr int MLA_LAT = BN * MLA_LRB, MLA_ROT = BN * MLA_RRB;          // bytes of a tile's two parts
constexpr int MLA_IMG = MLA_LAT + MLA_ROT;                             // one tile: 72 KiB
constexpr size_t mla_lds_bytes() { return 2 * (size_t)MLA_IMG; }       // the double buffer
constexpr int MLA_IST = 16 * (MLA_DV + 2);                             // floats of one item's partial: [16][512] O . l, then [16][2] (m, l)

// the latent part's swizzle (see the head of the file)
__host__ __device__ constexpr int mla_swz(int r) { return (((r & 7) << 1) ^ (9 * ((r >> 3) & 1))) & 15; }

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the types; parts 1 - 3 are the text of one wave's work, shared with fa_mla_wide_kernel.hip

// item (b, s) x row block rb: rows r = 16 rb + c = h * Nq + iq of the packed block, keys of tiles [t0, t1) of sequence b
template <typename Tag, bool CAUSAL>
__global__ __launch_bounds__(64) void mla_partial_kernel(MlaDecodeParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;  // buffer u: latent part at u * MLA_IMG, rotary part behind it

  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, item = blockIdx.x, rb = blockIdx.y;
  const int b = item / S, s = item - b * S;
  const int R = p.Hq * p.Nq;
  const int Nk = min(max(__builtin_amdgcn_readfirstlane(p.seqlens[b]), 0), p.max_pages << p.lp);  // keys of this item's sequence
  const int coff = Nk - p.Nq;
  const int nT = (Nk + BN - 1) / BN;
  const int t0 = (int)((long long)s * nT / S), t1 = (int)((long long)(s + 1) * nT / S);

#define FA_MLA_BODY_PART 1  // the Q fragments qf[] (pre-scaled), the row limit rlim, the LDS read offsets kl[], kr[], vl[]
#include "fa_mla_body.h"

  // ---- LDS-DMA: this wave moves every piece of a tile, the chunk swizzle sits on the source address.
  // latent piece j = row j of the tile: lane -> chunk lane ^ f(j & 15); rotary piece j = rows 8 j .. 8 j + 7: lane -> row lane / 8,
  // chunk (lane % 8) ^ ((row >> 1) & 7) behind the row's 512 latent elements
  const unsigned dma_l0 = (unsigned)lane << 4;
  const int drow = lane >> 3, dpc = lane & 7;
  const unsigned dma_r0 = (unsigned)(MLA_LRB + ((dpc ^ (drow >> 1)) << 4));

  // ---- pg[] holds the table entries of the next tile to stage (its pages: max(1, 64 / P), at most four), loaded one tile ahead
  const int lp = p.lp;
  const unsigned rsb = (unsigned)p.row_stride * 2;  // the pool's row stride in bytes
  const unsigned dma_rrow = (unsigned)drow * rsb;
  int pg[4] = {-1, -1, -1, -1};
  auto fetch_pages = [&](int t) __attribute__((always_inline)) {
    const int *tbl = p.block_table + (long long)b * p.bt_stride;
    const int i0 = (t * BN) >> lp, npg = max(1, BN >> lp);
#pragma unroll
    for (int k = 0; k < 4; ++k) pg[k] = k < npg ? tbl[min(i0 + k, p.max_pages - 1)] : -1;  // (never past the row's max_pages entries)
  };
  // stage tile t into buffer buf. LPC = min(lp, 6): the tile's 64 / 2^LPC pages are compile-time entries of pg[], one descriptor each,
  // built on the page's 64-bit base with a range that covers only the page's valid rows
  auto stage = [&](auto lpc, int t, int buf) __attribute__((always_inline)) {
    constexpr int LPC = decltype(lpc)::value, NPG = BN >> LPC, PM = (1 << LPC) - 1;
    const int P = 1 << lp, key0 = (t * BN) & -P;  // first key of the tile's first page
    const unsigned row0 = LPC == 6 ? (unsigned)((t * BN) & (P - 1)) : 0u;  // the tile's first slot in it (pages of 64 keys and more)
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
#pragma unroll
    for (int j = 0; j < BN; ++j) {
      const unsigned so = (row0 + (unsigned)(j & PM)) * rsb;  // (the whole offset in voffset: inside the range check)
      const unsigned vo = so + (dma_l0 ^ (unsigned)(mla_swz(j & 15) << 4));
      const unsigned ld = lbase + j * MLA_LRB;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs[j >> LPC]) : "memory");
    }
#pragma unroll
    for (int j = 0; j < BN / 8; ++j) {
      const unsigned so = (row0 + (unsigned)((8 * j) & PM)) * rsb + dma_rrow;
      const unsigned vo = so + (dma_r0 ^ (unsigned)((j & 1) << 6));  // ((row >> 1) & 7) gains 4 on odd pieces
      const unsigned ld = lbase + MLA_LAT + j * 1024;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs[(8 * j) >> LPC]) : "memory");
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
  // iteration t: wait for tile t, stage tile t + 1 under its arithmetic; iteration t0 - 1 only stages tile t0 (one staging site)
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t has landed (this wave issued every piece of it: no barrier needed)
    if (t + 1 < t1) {
      const int nb = (t + 1 - t0) & 1;
      if (lp == 4) stage(std::integral_constant<int, 4>{}, t + 1, nb);
      else if (lp == 5) stage(std::integral_constant<int, 5>{}, t + 1, nb);
      else stage(std::integral_constant<int, 6>{}, t + 1, nb);
    }
    if (t < t0) continue;
#define FA_MLA_BODY_PART 2  // tile t: 18 k-steps of scores, the mask, the online softmax, 64 PV steps
#include "fa_mla_body.h"
  }

#define FA_MLA_BODY_PART 3  // the partial (O . l, m, l) -> workspace slot (item, rb)
#include "fa_mla_body.h"
}

// one wave per output row (b, h, iq): fa_decode_kernel.hip's paged combine at 512 columns. Lanes take the splits' (m, l) pairs in
// parallel, the weights 2^(m_s - M) go through LDS, and thread d folds columns d + 64 e, e = 0..7, of the S partial rows: eight loads
// in flight, the splits in ascending order (bitwise reproducible). A row that saw no visible key (L_b = 0, or causal with
// i + L_b < Nq) has lsum = 0: O = 0 exactly and LSE = -inf. Rows of 512 are written, never 576.
template <typename Tag>
__global__ __launch_bounds__(64) void mla_combine_kernel(MlaDecodeParams p) {
  using elem = typename ML16<Tag>::elem;
  constexpr int NE = MLA_DV / 64;
  __shared__ float wgt[256];
  const int lane = threadIdx.x;
  const int row_id = blockIdx.x;  // (b * Hq + h) * Nq + iq
  const int iq = row_id % p.Nq, bh = row_id / p.Nq;
  const int h = bh % p.Hq, b = bh / p.Hq;
  const int r = h * p.Nq + iq, rb = r >> 4, rr = r & 15;
  const int S = p.S;  // <= 256
  const size_t sst = (size_t)p.RBLK * MLA_IST;  // floats between two splits' partials of one row block
  const float *w0 = p.ws + ((size_t)b * S * p.RBLK + rb) * MLA_IST;
  const float *ml = w0 + 16 * MLA_DV + 2 * rr;
  float ms[4], ls[4];
  float M = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int s = lane + 64 * e;
    ms[e] = s < S ? ml[(size_t)s * sst] : -INFINITY;
    ls[e] = s < S ? ml[(size_t)s * sst + 1] : 0.0f;
    M = fmaxf(M, ms[e]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
  float lsum = 0.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float f = (ms[e] == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(ms[e] - M);  // a split that saw no visible key weighs nothing
    wgt[lane + 64 * e] = f;
    lsum += ls[e] * f;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
  __syncthreads();
  float acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = 0.0f;
  const float *wr = w0 + rr * MLA_DV + lane;
  for (int s = 0; s < S; ++s) {
    float x[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) x[e] = wr[(size_t)s * sst + 64 * e];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] += x[e] * wgt[s];
  }
  const bool dead = !(lsum > 0.0f);
  const float inv = dead ? 0.0f : 1.0f / lsum;
  elem *op = (elem *)p.o + (long long)b * p.o_bs + (long long)h * p.o_hs + (long long)iq * p.o_rs;
#pragma unroll
  for (int e = 0; e < NE; ++e) op[lane + 64 * e] = (elem)(acc[e] * inv);
  if (p.lse != nullptr && lane == 0) p.lse[row_id] = dead ? -INFINITY : (M + log2f(lsum)) * 0.6931471805599453f;
}

// ---------------------------------------------------------------------------
bool mla_decode_supported(int dtype, int Dqk, int Dv) {
  return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && Dqk == MLA_DQK && Dv == MLA_DV;
}

// splits per sequence: the decode's rule. One round of the chip's item slots (144 KiB of LDS: one item per CU) over the B . RBLK
// (sequence, row block) pairs, at least FA_MLA_MIN_TILES 64-key tiles per item, at most 256. Nk is the CAPACITY: host scalars only.
int mla_decode_splits(int B, int rblk, int Nk) {
  const int nT = (Nk + BN - 1) / BN;
  const long long want = (long long)FA_MLA_ROUNDS * 256, pairs = (long long)B * rblk;
  long long S = (want + pairs - 1) / pairs;
  S = std::min<long long>(S, std::max(1, nT / FA_MLA_MIN_TILES));
  return (int)std::max<long long>(1, std::min<long long>(S, 256));
}

long long mla_decode_workspace_bytes(int B, int Hq, int Nq, int Nk) {
  const int rblk = (Hq * Nq + 15) / 16;
  return (long long)B * mla_decode_splits(B, rblk, Nk) * rblk * MLA_IST * 4;
}

// the combine kernel over the output rows of one call (this file's partial kernels and fa_mla_wide_kernel.hip's write the same workspace)
hipError_t launch_mla_combine(const MlaDecodeParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    hipLaunchKernelGGL(mla_combine_kernel<decltype(tag)>, dim3(p.B * p.Hq * p.Nq), dim3(64), 0, s, p);
    return hipGetLastError();
  });
}

// One call: the partial kernel over B . S items x RBLK row blocks, then the combine kernel over the output rows, on the same stream
hipError_t launch_mla_decode_paged(const MlaDecodeParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    auto go = [&](auto partial) {
      (void)hipGetLastError();
      hipError_t e = set_dyn_lds_once((const void *)partial, (int)mla_lds_bytes());
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(partial, dim3(p.B * p.S, p.RBLK), dim3(64), mla_lds_bytes(), s, p);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
      return launch_mla_combine(p, dtype, s);
    };
    return p.is_causal ? go(mla_partial_kernel<Tag, true>) : go(mla_partial_kernel<Tag, false>);
  });
}

}  // namespace fa
