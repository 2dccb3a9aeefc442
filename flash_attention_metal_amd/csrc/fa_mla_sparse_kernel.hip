// fa_mla_sparse_kernel.hip -- the absorbed latent-attention decode over a per-token list of keys: entry point fa_fwd_mla_decode_sparse.
//
// fa_mla_wide_kernel.hip's four-wave workgroup over one shared double buffer, with the item (token, split) in place of (sequence, split)
// and ONE difference: the 64 rows of a tile are not 64 consecutive rows of a page but the rows of 64 list entries, each a SLOT
// x = page * P + row of the pool, anywhere in it. Everything from LDS onwards is the wide kernel's text (fa_mla_body.h parts 0 - 3 with
// CAUSAL = false, b = the token, Nq = 1, Nk = n_t), the workspace format and the combine kernel are unchanged: O and LSE are the bits of
// fa_fwd_mla_decode_paged_wide on a pool of 64-row pages into which every token's listed rows were copied in list order.
//   * ALWAYS FOUR WAVES (the split rule is fed one workgroup row block up to 64 heads and two above, as the wide call's: the same S). Wave
//     w stages rows 16 w .. 16 w + 15 of every tile, that is list entries 64 t + 16 w + i, i = 0 .. 15.
//   * THE ENTRIES of a tile are one predicated dword load per wave: lane i < 16 holds entry 64 t + 16 w + i, or -1 where that position is
//     >= n_t -- positions behind the count are never read, let alone positions >= topk. They are fetched one tile ahead. An entry is
//     VALID when 0 <= x < num_pages * P (one unsigned compare; -1 fails it).
//   * LATENT PART, LDS-DMA as in the wide kernel, one piece = one row of the tile: lane -> chunk lane ^ f(row & 15) on the source offset.
//     Each row gets its OWN descriptor, built on the row's 64-bit address kv + ((x >> lp) * page_stride + (x & (P - 1)) * row_stride),
//     num_records = 1152 for a valid entry and 0 otherwise (the piece then lands as zeros and no address is formed from x). The entry
//     comes out of its lane by v_readlane: wave-uniform, sixteen descriptors per wave and tile.
//   * ROTARY PART through registers: a 1-KiB rotary piece is eight rows, which here lie in eight places. Lane -> row lane / 8 of the piece,
//     chunk lane % 8; the lane takes its row's entry from the entry register (ds_bpermute), forms the row's 64-bit address and loads 16
//     bytes under a predicate (an invalid entry: zeros, no load). Two such loads per lane and tile go out behind the latent pieces of
//     tile t + 1; their two ds_write_b128, at chunk ^ ((row >> 1) & 7) of the head_dim-64 K image, stand BEHIND the arithmetic of tile t,
//     as fa_mla_kv8_kernel.hip orders its writes.
//   * ONE BARRIER PER TILE, at the top of iteration t: s_waitcnt vmcnt(0) lgkmcnt(0) (this wave's pieces of tile t have landed, its
//     rotary writes of tile t too, and its reads of tile t - 1 are back), then the raw s_barrier (everyone's have, and everyone has left
//     iteration t - 1, whose buffer tile t + 1 is about to overwrite). Iteration t0 - 1 only stages tile t0: one staging site.
//   * BARRIER UNIFORMITY: as in fa_mla_paged_partial.inc. (token, s) and with them Nk, [t0, t1) come from blockIdx.x and scalars: the same
//     in all waves of a workgroup. Every wave runs every iteration -- once for an empty split -- and nothing leaves the loop early. A wave
//     whose 16 rows are all padding (slot >= RBLK) stages its share, meets every barrier, skips the arithmetic and stores nothing.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types, the launch tail

constexpr int MLA_SPARSE_NW = 4;  // waves of a workgroup, for every head count

// workgroup (token, s) x row block wb, wave w: heads 16 (4 wb + w) + c of the token, entries of tiles [t0, t1) of its list
template <typename Tag>
__global__ __launch_bounds__(64 * MLA_SPARSE_NW) void mla_sparse_partial_kernel(MlaSparseParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr bool CAUSAL = false;  // visibility is the list
  constexpr int NW = MLA_SPARSE_NW;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // rows (= list entries) of a tile this wave stages: 16; RW / 8 rotary pieces
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

  // ---- staging: this wave moves rows jr0 .. jr0 + 15 of a tile (jr0 is a multiple of 16: the swizzle of row jr0 + j is that of row j)
  const int jr0 = RW * w;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const unsigned dma_l0 = (unsigned)lane << 4;  // latent piece: lane -> chunk lane ^ f(row & 15), on the source offset
  const int drow = lane >> 3, dpc = lane & 7;   // rotary piece: lane -> row drow of the piece, chunk dpc behind the row's 512 latent elements
  const int *list = p.indices + (long long)b * p.idx_stride;
  // byte offset of slot x in the pool (x valid: page < num_pages, one page stays below 2 GiB)
  auto slot_off = [&](int x) __attribute__((always_inline)) { return ((long long)(x >> lp) * p.page_stride + (long long)(x & PM) * p.row_stride) * 2; };

  // ev: lane i < 16 holds the entry of this wave's row i of the next tile to stage, -1 behind the count; loaded one tile ahead
  int ev = -1;
  auto fetch_entries = [&](int t) __attribute__((always_inline)) {
    const int j = t * BN + jr0 + lane;
    ev = -1;
    if (lane < RW && j < Nk) ev = list[j];
  };
  u32x4 rot[RW / 8];
  // stage this wave's rows of tile t: sixteen latent pieces by LDS-DMA into buffer buf, the rotary chunks into rot[]
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const unsigned lbase = (unsigned)(__UINTPTR_TYPE__)smem + buf * MLA_IMG;
    const unsigned ll = lbase + jr0 * MLA_LRB;  // this wave's first latent piece
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
    fetch_entries(t + 1);
  };
  // rot[] -> the rotary part of buffer buf: row jr0 + 8 k + drow, chunk dpc ^ ((row >> 1) & 7)
  auto write_rot = [&](int buf) __attribute__((always_inline)) {
    lds_char *img = smem + buf * MLA_IMG;
#pragma unroll
    for (int k = 0; k < RW / 8; ++k) {
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

  if (t0 < t1) fetch_entries(t0);
  // iteration t: wait for tile t, send for tile t + 1, run tile t, write tile t + 1's rotary chunks; iteration t0 - 1 only stages tile t0.
  // Every wave of the workgroup runs every iteration and meets the barrier in each: see the head of the file
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's pieces and rotary writes of tile t have landed
    __builtin_amdgcn_s_barrier();                                // everyone's have, and everyone is done reading the buffer tile t + 1 overwrites
    const int nb = (t + 1 - t0) & 1;
    if (t + 1 < t1) stage(t + 1, nb);
    if (t >= t0 && live) {
#define FA_MLA_BODY_PART 2  // tile t: 18 k-steps of scores, the mask, the online softmax, 64 PV steps
#include "fa_mla_body.h"
    }
    if (t + 1 < t1) write_rot(nb);
  }

  if (live) {
#define FA_MLA_BODY_PART 3  // the partial (O . l, m, l) -> workspace slot (item, rb)
#include "fa_mla_body.h"
  }
}

// the wide call's size at B = T, Nq = 1 and a capacity of `cap` keys
long long mla_decode_sparse_workspace_bytes(int T, int Hq, int cap) { return mla_decode_wide_workspace_bytes(T, Hq, 1, cap); }

// One call: the partial kernel over T . S items x ceil(RBLK / 4) row blocks of four waves, then fa_mla_kernel.hip's combine kernel over
// the output rows (pc: the call as that kernel sees it, B = T, Nq = 1), on the same stream
hipError_t launch_mla_decode_sparse(const MlaSparseParams &p, const MlaDecodeParams &pc, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return launch_mla_partial_and_combine(mla_sparse_partial_kernel<decltype(tag)>, dim3(p.T * p.S, (p.RBLK + MLA_SPARSE_NW - 1) / MLA_SPARSE_NW),
                                          MLA_SPARSE_NW, p, pc, dtype, s);
  });
}

}  // namespace fa
