// fa_mla_sparse_kv8_kernel.hip -- the absorbed latent-attention decode over a per-token list of keys of an e4m3 latent pool: entry point
// fa_fwd_mla_decode_sparse_kv8.
//
// fa_mla_kv8_kernel.hip's four-wave workgroup over one shared double buffer, staged through registers and widened exactly to bf16 into the
// wide kernel's image, with the item (token, split) of fa_mla_sparse_kernel.hip in place of (sequence, split) and ONE difference from each
// parent: the wave's sixteen rows of a tile are the rows of sixteen list entries, each a SLOT x = page * P + row of a pool of BYTES,
// anywhere in it. Everything from LDS onwards is the wide kernel's text (fa_mla_body.h parts 0 - 3 with CAUSAL = false, b = the token,
// Nq = 1, Nk = n_t), the workspace format and the bf16 combine kernel are unchanged. O and LSE are therefore the bits of
// fa_fwd_mla_decode_sparse (bf16) on the pool widened element by element, and of fa_fwd_mla_decode_paged_kv8 on an e4m3 pool of 64-row
// pages into which every token's listed rows were copied in list order.
//   * ALWAYS FOUR WAVES, one instantiation (bf16 queries, no causal form). Wave w stages rows 16 w .. 16 w + 15 of every tile, that is
//     list entries 64 t + 16 w + i, i = 0 .. 15: 16 x 576 bytes = nine 16-byte loads per lane under fa_mla_kv8_kernel.hip's lane maps,
//     eight latent (lane -> row 2 i + lane / 32, chunk lane % 32) and one rotary (lane -> row lane / 4, chunk lane % 4 behind the row's
//     512 latent bytes). write_tile and the LDS destination arithmetic are that file's: the image is the twin's.
//   * THE ENTRIES of a tile are one predicated dword load per wave, fa_mla_sparse_kernel.hip's: lane i < 16 holds entry 64 t + 16 w + i,
//     or -1 where that position is >= n_t -- positions behind the count are never read, let alone positions >= topk. They are fetched
//     one tile ahead. An entry is VALID when 0 <= x < num_pages * P (one unsigned compare; -1 fails it).
//   * THE ROW ADDRESSES. The sixteen rows lie in sixteen places, two rows share a load and the pool may exceed 4 GiB: no descriptor, but
//     per-lane 64-bit addresses. Each lane takes ITS ROW's entry out of the entry register (ds_bpermute), tests it, and forms
//     kv + (x >> lp) * page_stride + (x & (P - 1)) * row_stride -- bytes, no * 2 -- for one 16-byte load under that predicate. An invalid
//     entry gives zeros and makes no load and no address. (The other form, the 64-bit offset computed once in lanes 0 .. 15 and both
//     halves permuted, was compiled next to this one: eighteen permutes per tile in place of nine and 256 VGPRs + 220 AGPRs against this
//     form's 256 + 218, neither with scratch. The address here is a shift, an and, a 32-bit multiply for the row inside its page and a
//     64-bit multiply-add for the page. This file is the per-load form, by the register count.)
//   * ONE BARRIER PER TILE, at the top of iteration t: s_waitcnt lgkmcnt(0) (this wave's LDS writes of tile t have landed, its reads of
//     tile t - 1 and its permutes have returned), then the raw s_barrier (everyone's have). Then the raw loads of tile t + 1 go out into
//     registers, the body's part 2 runs on tile t, and last the registers are widened and written into the other buffer, which nobody
//     reads before the next barrier; the entries of tile t + 2 are sent for behind the writes. The prologue loads and writes tile t0. The
//     permutes that hand out the entries stand behind the wait that covers the entry load (the compiler's vmcnt on the entry register).
//   * BARRIER UNIFORMITY: as in both parents. (token, s) and with them Nk, [t0, t1) come from blockIdx.x and scalars: the same in all waves
//     of a workgroup. Every wave runs every iteration and nothing leaves the loop early. A wave whose 16 rows are all padding (slot >=
//     RBLK) stages its share, meets every barrier, skips the arithmetic and stores nothing.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types, the launch tail

constexpr int MLA_SPARSE_KV8_NW = 4;  // waves of a workgroup, for every head count

// 8 e4m3 (two dwords) -> 8 bf16 (one 16-byte chunk): exact (fa_mla_kv8_kernel.hip's mla_widen8, the same statements)
__device__ __forceinline__ u32x4 mla_sparse_widen8(unsigned w0, unsigned w1) {
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

// workgroup (token, s) x row block wb, wave w: heads 16 (4 wb + w) + c of the token, entries of tiles [t0, t1) of its list
__global__ __launch_bounds__(64 * MLA_SPARSE_KV8_NW) void mla_sparse_kv8_partial_kernel(MlaSparseParams p) {
  using M = ML16<BF16>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr bool CAUSAL = false;  // visibility is the list
  constexpr int NW = MLA_SPARSE_KV8_NW;
  constexpr int KSL = MLA_DV / 32, KSR = MLA_DR / 32;  // k-steps of the score product over the latent / rotary part
  constexpr int DT = MLA_DV / 16;                      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;                          // 16-key tiles per 64-key tile
  constexpr int RW = BN / NW;                          // rows (= list entries) of a tile this wave stages: 16
  constexpr int NLL = RW / 2;                          // latent loads per lane and tile (two rows each); one rotary load besides
  static_assert(RW == 16, "sixteen entries per wave: one per lane of the first sixteen, one rotary load of 64 chunks");

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
  // per-lane offset, everything else is compile-time (fa_mla_kv8_kernel.hip's arithmetic)
  const int jr0 = RW * w;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const int hi = lane >> 5, le = lane & 31;
  const unsigned dst_l = (unsigned)(jr0 * MLA_LRB + hi * MLA_LRB + ((le >> 3) << 8) + ((((2 * le) & 15) ^ (hi << 1)) << 4));
  // rotary load: lane -> row rr = lane / 4, e4m3 chunk lane % 4 at byte 512 of the row -> bf16 chunks 2 e, 2 e + 1 of the head_dim-64 K
  // image, chunk ^ ((row >> 1) & 7)
  const int rr = lane >> 2, re = lane & 3;
  const unsigned dst_r = (unsigned)(MLA_LAT + (jr0 + rr) * MLA_RRB + (((2 * re) ^ ((rr >> 1) & 7)) << 4));
  // the lane's chunk of its row, from the pool's base: the row's offset is added per load
  const char *src_l = (const char *)p.kv + le * 16, *src_r = (const char *)p.kv + (MLA_DV + re * 16);
  const unsigned rsb = (unsigned)p.row_stride;  // bytes (e4m3: elements are bytes); the rows of one page stay below 2 GiB
  const int *list = p.indices + (long long)b * p.idx_stride;

  // ev: lane i < 16 holds the entry of this wave's row i of the next tile to load, -1 behind the count; loaded one tile ahead
  int ev = -1;
  auto fetch_entries = [&](int t) __attribute__((always_inline)) {
    const int j = t * BN + jr0 + lane;
    ev = -1;
    if (lane < RW && j < Nk) ev = list[j];
  };
  u32x4 raw[NLL + 1];
  // 16 bytes at `src` + the byte offset of slot x, or zeros where x is behind the count (-1) or outside the pool: no address, no load
  auto load_row = [&](int x, const char *src) __attribute__((always_inline)) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if ((unsigned)x < (unsigned)p.num_slots)
      v = *reinterpret_cast<const u32x4 *>(src + ((unsigned long long)((unsigned)x >> lp) * (unsigned long long)p.page_stride + (unsigned)(x & PM) * rsb));
    return v;
  };
  // this wave's rows of the tile whose entries ev holds -> raw[]: every lane takes its rows' entries out of ev -- all nine permutes first,
  // under one wait, then the nine loads, each under its own predicate
  auto load_raw = [&]() __attribute__((always_inline)) {
    int xs[NLL + 1];
#pragma unroll
    for (int i = 0; i < NLL; ++i) xs[i] = __shfl(ev, 2 * i + hi, 64);
    xs[NLL] = __shfl(ev, rr, 64);
#pragma unroll
    for (int i = 0; i < NLL; ++i) raw[i] = load_row(xs[i], src_l);
    raw[NLL] = load_row(xs[NLL], src_r);
  };
  // raw[] -> buffer buf, widened
  auto write_tile = [&](int buf) __attribute__((always_inline)) {
    lds_char *img = smem + buf * MLA_IMG;
#pragma unroll
    for (int i = 0; i < NLL; ++i) {
      const int ci = ((4 * i) & 12) ^ (9 * (i >> 2));  // C_i
      const unsigned a = (dst_l ^ (unsigned)(ci << 4)) + (unsigned)(2 * i * MLA_LRB);
      lds_write_b128(img + a, mla_sparse_widen8(raw[i][0], raw[i][1]));
      lds_write_b128(img + (a ^ 16u), mla_sparse_widen8(raw[i][2], raw[i][3]));
    }
    lds_write_b128(img + dst_r, mla_sparse_widen8(raw[NLL][0], raw[NLL][1]));
    lds_write_b128(img + (dst_r ^ 16u), mla_sparse_widen8(raw[NLL][2], raw[NLL][3]));
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
hipError_t launch_mla_decode_sparse_kv8(const MlaSparseParams &p, const MlaDecodeParams &pc, hipStream_t s) {
  return launch_mla_partial_and_combine(mla_sparse_kv8_partial_kernel, dim3(p.T * p.S, (p.RBLK + MLA_SPARSE_KV8_NW - 1) / MLA_SPARSE_KV8_NW),
                                        MLA_SPARSE_KV8_NW, p, pc, FA_DTYPE_BF16, s);
}

}  // namespace fa
