// fa_mla_indexer_kv8_kernel.hip -- the indexer's logits over e4m3 index keys with one fp32 scale per key: entry points
// fa_mla_indexer_logits_paged_kv8 and (in front of the unchanged select kernel of fa_mla_indexer_kernel.hip) fa_mla_indexer_topk_paged_kv8.
//
//   logit[t][j] = k_scale(b, j) * sum_h w[t][h] max(0, q_idx[t, h, :] . k_idx(b, j)[:]),  j < v_t,  q_idx and k_idx e4m3 bytes.
//
// Items (sequence, token block, chunk), the early exits in front of the first barrier, one barrier per tile behind s_waitcnt vmcnt(0),
// the table entry fetched one tile ahead and the per-key store predicate are fa_mla_indexer_kernel.hip's rules; the chunk rule is its
// mla_indexer_chunk_tiles. What is this kernel's own:
//   * THE SCORE TILE is ONE v_mfma_f32_16x16x128_f8f6f4 (both operands e4m3, unit E8M0 scales 0x7f) per 16 heads x 16 keys: the whole
//     128-column dot in an instruction, Hi / 16 instructions per column block where the 16-bit kernel issues Hi / 4. Heads are the rows
//     (A = the query), keys the columns (B = the key tile): lane (c, g) = (lane % 16, lane / 16) ends up with heads 16 m + 4 g + i of
//     key c, so the head sum stays Hi / 4 v_max / v_fma pairs in the lane plus two cross-lane adds over g.
//   * THE K-ORDER. Lane (c, g) feeds the instruction 32 bytes of row c; WHICH 32 of the 128 columns they are is free as long as A and B
//     agree, because the instruction sums over all of them. Both operands take bytes 32 g .. 32 g + 31 of their row in memory order:
//     two adjacent 16-byte reads, from global memory for the query (once per item) and from LDS for a key.
//   * THE QUERY of a token is Hi / 16 such fragments: 32 VGPRs at Hi = 64, half the 16-bit kernel's.
//   * THE TILE is 64 keys x 128 bytes = 8 KiB, double-buffered in 16 KiB of LDS, staged once per four-wave workgroup by LDS-DMA. Wave w
//     moves rows 16 w .. 16 w + 15 in TWO 1-KiB pieces of eight rows (lane l of a piece: row l / 8, 16-byte position l % 8) under one
//     descriptor on the page's 64-bit base whose range ends behind the page's last row below L_b: 0 bytes for a page past L_b or an
//     entry outside the pool, so such rows land as zeros and no address is formed from the entry.
//   * THE IMAGE: row r of the tile at r * 128 bytes, so TWO rows span the 64 banks (256 bytes) and an even and an odd row never meet.
//     A B-operand read has the sixteen lanes of one g read the SAME chunk index (2 g, then 2 g + 1) of sixteen consecutive rows: rows
//     of equal parity, eight of them, would all hit one 16-byte bank group. So chunk k of row r sits at position k ^ ((r >> 1) & 7):
//     the eight rows of one parity take eight different positions, the sixteen lanes cover sixteen different bank groups, all 64
//     banks once per read. The swizzle is put on the SOURCE offset of the DMA (position pos of row r is filled from chunk
//     pos ^ ((r >> 1) & 7)); the read applies the same xor.
//   * THE SCALE of key j reaches the lane that stores logit j (g = 0, column c of its block) by a PREDICATED GLOBAL LOAD one tile ahead:
//     predicated on j < v_t and a page entry inside the pool, so a scale no visible key names is never read. The other way, a row of
//     the LDS image, would cost a second descriptor and DMA per page and piece for 64 bytes, and hand every wave scales it does not
//     store; here sixteen lanes read one 64-byte segment and the latency hides behind the tile's own vmcnt(0). The scale multiplies
//     the finished head sum once, in front of the predicated store. A wave's column blocks are not the rows it stages when TB > 1, so
//     it fetches the table entries of its TB column blocks themselves, two tiles ahead.
#include <type_traits>

#include "fa_mla_indexer_common.h"  // IdxSeq, idx_seq, idx_visible

namespace fa {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int IDX8_RB = 128;              // bytes of a key row: 128 e4m3 columns
constexpr int IDX8_TILE = BN * IDX8_RB;   // one 64-key tile: 8 KiB
constexpr int IDX8_NW = 4;                // waves of a workgroup

// D = A(e4m3, 16 heads x 128) . B(e4m3, 128 x 16 keys) + C with unit scales (E8M0 0x7f = 2^0): an exact e4m3 product, fp32 from there
__device__ __forceinline__ f32x4 idx8_mfma(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}
__device__ __forceinline__ i32x8 idx8_join(u32x4 a, u32x4 b) {
  return i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

template <int HI, int TB>
__global__ __launch_bounds__(64 * IDX8_NW) void mla_indexer_kv8_logits_kernel(MlaIndexerKv8Params pp) {
  const MlaIndexerParams &p = pp.p;
  constexpr int MT = HI / 16;         // 16-head row tiles of the score tile: one instruction each
  constexpr int CBS = IDX8_NW / TB;   // stride of a wave's column blocks; it takes TB of the four

  __shared__ __attribute__((aligned(16))) char smem_generic[2 * IDX8_TILE];
  lds_char *smem = (lds_char *)smem_generic;

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  int x = blockIdx.x;
  const int ch = x % p.nchunks;
  x /= p.nchunks;
  const int tb = x % p.nblk, b = x / p.nblk;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const IdxSeq sq = idx_seq(p.cu_q, p.seqlens, b, p.total_q, p.max_q, p.max_pages << lp);
  const int i0 = tb * TB;
  if (i0 >= sq.Lq) return;  // the block owns no token
  const int vmax = idx_visible(sq, min(i0 + TB - 1, sq.Lq - 1));
  const int t0 = ch * p.chunk_tiles;
  if (t0 * BN >= vmax) return;  // the chunk starts behind the block's last visible key
  const int t1 = min(t0 + p.chunk_tiles, (vmax + BN - 1) / BN);

  // ---- this wave's token: its visible count, its query fragments (bytes 32 g .. 32 g + 31 of head 16 m + c) and its head weights
  const int it = i0 + w % TB;
  const int v = it < sq.Lq ? idx_visible(sq, it) : 0;
  const bool work = v > t0 * BN;  // wave-uniform
  const long long tok = sq.sq + it;
  i32x8 qf[MT];
  float wv[MT][4];
  {
    const char *qp = (const char *)p.q + tok * p.q_rs + 32 * g;
    const float *wp = p.w + tok * p.w_rs + 4 * g;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      u32x4 lo = {0u, 0u, 0u, 0u}, hi = lo;
      if (work) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(qp + (long long)(16 * m + c) * p.q_hs);
        lo = src[0];
        hi = src[1];
      }
      qf[m] = idx8_join(lo, hi);
#pragma unroll
      for (int i = 0; i < 4; ++i) wv[m][i] = work ? wp[16 * m + i] : 0.0f;
    }
  }
  float *out = p.logits + tok * p.logits_stride;

  // ---- staging: rows 16 w .. 16 w + 15 of a tile, one page, one descriptor, two pieces of eight rows
  const unsigned rsb = (unsigned)p.row_stride;  // the pool's row stride, bytes
  const int *tbl = p.block_table + (long long)b * p.bt_stride;
  int pg = -1;  // the table entry of this wave's rows of the next tile to stage
  auto fetch_page = [&](int t) __attribute__((always_inline)) { pg = tbl[min((t * BN + 16 * w) >> lp, p.max_pages - 1)]; };
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const int key0 = t * BN + 16 * w, row0 = key0 & PM;
    const int page = __builtin_amdgcn_readfirstlane(pg);
    const int nv = min(sq.L - (key0 - row0), PM + 1);  // rows of the page below L_b
    const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;
    const long long off = ok ? (long long)page * p.page_stride : 0;
    const unsigned nrec = ok ? (unsigned)(nv - 1) * rsb + IDX8_RB : 0u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + off), 0, nrec, 0x00020000);
    const unsigned ll = (unsigned)(__UINTPTR_TYPE__)smem + buf * IDX8_TILE + 16 * w * IDX8_RB;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned r = 8 * j + (lane >> 3);  // the row among the wave's sixteen: ((16 w + r) >> 1) & 7 = r >> 1
      const unsigned vo = ((unsigned)row0 + r) * rsb + ((((unsigned)lane & 7) ^ (r >> 1)) << 4);
      const unsigned ld = ll + j * 1024;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs) : "memory");
    }
    fetch_page(t + 1);
  };

  // ---- scales: the table entries of this wave's column blocks of tile t, then the scale of key t * 64 + 16 cb + c into the storing lane
  int spg[TB];
  float sn[TB];  // the scales of the tile behind the current one
  auto fetch_scale_pages = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < TB; ++k) spg[k] = tbl[min((t * BN + 16 * (w / TB + k * CBS)) >> lp, p.max_pages - 1)];
  };
  auto load_scales = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < TB; ++k) {
      const int j = t * BN + 16 * (w / TB + k * CBS) + c, page = spg[k];
      sn[k] = 0.0f;
      if (g == 0 && j < v && (unsigned)page < (unsigned)p.num_pages) sn[k] = pp.k_scale[(long long)page * pp.scale_page_stride + (j & PM)];
    }
  };
#pragma unroll
  for (int k = 0; k < TB; ++k) sn[k] = 0.0f;

  fetch_page(t0);
  fetch_scale_pages(t0);
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of tile t have landed
    __builtin_amdgcn_s_barrier();                     // everyone's have, and everyone is done reading the buffer tile t + 1 overwrites
    float sc[TB];  // the scales of tile t
#pragma unroll
    for (int k = 0; k < TB; ++k) sc[k] = sn[k];
    if (t + 1 < t1) {
      stage(t + 1, (t + 1 - t0) & 1);
      load_scales(t + 1);
      fetch_scale_pages(t + 2);
    }
    if (t < t0 || v <= t * BN) continue;  // (wave-uniform) the staging iteration, or a tile this token sees nothing of
    const lds_char *img = smem + ((t - t0) & 1) * IDX8_TILE;
#pragma unroll
    for (int k = 0; k < TB; ++k) {
      const int cb = w / TB + k * CBS, kb = t * BN + 16 * cb;
      if (kb >= v) continue;  // (wave-uniform)
      const lds_char *row = img + (16 * cb + c) * IDX8_RB;
      const int sx = c >> 1;  // ((16 cb + c) >> 1) & 7
      const i32x8 kf = idx8_join(lds_read_b128(row + (((2 * g) ^ sx) << 4)), lds_read_b128(row + (((2 * g + 1) ^ sx) << 4)));
      f32x4 acc[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[m] = idx8_mfma(qf[m], kf, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
      float s = 0.0f;  // heads 16 m + 4 g + i of key kb + c
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) s = __builtin_fmaf(wv[m][i], __builtin_fmaxf(acc[m][i], 0.0f), s);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (g == 0 && kb + c < v) out[kb + c] = s * sc[k];
    }
  }
}

// ---- the launch: the 16-bit call's grid, host scalars alone
hipError_t launch_mla_indexer_logits_kv8(const MlaIndexerKv8Params &pp, int Hi, hipStream_t s) {
  (void)hipGetLastError();
  const MlaIndexerParams &p = pp.p;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)p.B * p.nblk * p.nchunks)), dim3(64 * IDX8_NW), 0, s, pp);
    return hipGetLastError();
  };
  auto by_tb = [&](auto hi) {
    constexpr int HI = decltype(hi)::value;
    return p.tb == 4 ? go(mla_indexer_kv8_logits_kernel<HI, 4>) : p.tb == 2 ? go(mla_indexer_kv8_logits_kernel<HI, 2>) : go(mla_indexer_kv8_logits_kernel<HI, 1>);
  };
  return Hi == 64 ? by_tb(std::integral_constant<int, 64>{}) : by_tb(std::integral_constant<int, 32>{});
}

}  // namespace fa
