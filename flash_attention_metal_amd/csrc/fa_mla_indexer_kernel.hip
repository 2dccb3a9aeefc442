// fa_mla_indexer_kernel.hip -- the indexer in front of the sparse latent-attention decode: entry points fa_mla_indexer_logits_paged,
// fa_mla_indexer_select and fa_mla_indexer_topk_paged (the first two in a row). Two kernels, both new.
//
// THE LOGITS KERNEL  logit[t][j] = sum_h w[t][h] max(0, q_idx[t, h, :] . k_idx(b, j)[:]),  j < v_t  (fp32 from the matrix core onwards).
//   * THE SCORE TILE of v_mfma_f32_16x16x32 has HEADS as its 16 rows (A = the token's query, 16 heads x 32 columns a step) and KEYS as
//     its 16 columns (B = a column block of the key tile): lane (c, g) = (lane % 16, lane / 16) ends up with the dots of heads
//     16 m + 4 g + i (m < Hi / 16, i < 4) against key c of the block. The head sum is then Hi / 4 v_max / v_fma pairs in the lane over
//     its accumulator registers, against Hi / 4 values of w held in registers, plus two cross-lane adds over g. The key, which is the
//     output, never leaves its lane column.
//   * THE QUERY of a token, Hi x 128, is the A operand of every product of the wave: Hi / 16 x 4 fragments of 16 bytes, 64 VGPRs at
//     Hi = 64, loaded once.
//   * A WORKGROUP is four waves over an item (sequence b, block of TB tokens, key chunk), TB in {1, 2, 4} from max_seqlen_q. Every
//     64-key tile of the chunk (16 KiB) is staged ONCE into LDS for the four waves, double-buffered, by LDS-DMA. Wave w moves rows
//     16 w .. 16 w + 15 of a tile in four 1-KiB pieces of four rows; they lie in one page (P >= 16), under ONE descriptor built on the
//     page's 64-bit base whose range covers the page's rows below L_b only -- 0 bytes for a page past L_b or an entry outside the pool:
//     such rows land as zeros and no address is formed from the entry (the rule of fa_mla_paged_partial.inc). The whole offset of a piece
//     sits in voffset, inside the range check; table entries are fetched one tile ahead, the table index clamped to max_pages - 1.
//   * THE IMAGE: row r of the tile at r * 256 bytes, its 16-byte chunk k at position k ^ (r & 15), the swizzle put on the SOURCE offset
//     of the DMA. A B-operand read is row 16 cb + c, chunk 4 ks + g: the sixteen lanes of one g hit sixteen different chunk positions,
//     that is all 64 banks once.
//   * WAVE w takes token w % TB of the block and the column blocks w / TB + k (4 / TB), k < TB, of every tile: in decode (TB = 1) the four
//     waves split a tile's keys, in a prefill chunk (TB = 4) four tokens share every byte of every tile.
//   * ONE BARRIER PER TILE, at the top of iteration t: s_waitcnt vmcnt(0) (this wave's pieces of tile t have landed), then s_barrier
//     (everyone's have, and everyone has left iteration t - 1, whose buffer tile t + 1 is about to overwrite).
//   * BARRIER UNIFORMITY: (b, token block, chunk) and the tile range [t0, t1) come from blockIdx.x and scalars. An item whose block owns
//     no token or whose chunk starts behind the last visible key of the block leaves in front of the first barrier, as a whole
//     workgroup. Every other wave runs every iteration; one whose token sees none of a tile's keys skips the arithmetic.
//   * STORES are predicated per key on j < v_t: nothing else of the logits buffer is written.
//   * THE CHUNK RULE is mla_indexer_chunk_tiles, below: host scalars only.
//
// THE SELECT KERNEL  one workgroup of 256 threads per (sequence, token of the sequence); a token nobody owns leaves at once.
//   * v <= topk: the list is positions 0 .. v - 1 and the logits are not read.
//   * otherwise the threshold comes from a radix select, most significant byte first, on the order-preserving integer image of the
//     logit (-0 counted as +0): four passes over the row, each a 256-bin histogram in LDS (LDS atomics only) over the keys that match
//     the prefix so far, a workgroup scan over the bins from the top, and the remaining rank carried down. After four passes the
//     threshold T is a whole 32-bit image and `need` says how many keys EQUAL to T are taken.
//   * one ordered emission pass: per 256 keys a workgroup scan of (greater than T, equal to T) packed in one int; a key is taken if it
//     is greater, or equal with fewer than `need` equals in front of it; it lands at (greater in front) + min(equals in front, need):
//     ascending position, no sort, no global atomic. The pass stops once topk entries are out.
//   * every comparison is on the integer image, so any bits -- NaN included -- give topk distinct visible positions.
#include <algorithm>
#include <type_traits>

#include "fa_mla_indexer_common.h"  // IdxSeq, idx_seq, idx_visible

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // ML16 and f32x4: the 16x16x32 matrix-core types of the family

constexpr int IDX_D = 128;              // columns of an index query / key
constexpr int IDX_RB = IDX_D * 2;       // bytes of a key row
constexpr int IDX_TILE = BN * IDX_RB;   // one 64-key tile: 16 KiB
constexpr int IDX_NW = 4;               // waves of a workgroup
constexpr int IDX_KS = IDX_D / 32;      // k-steps of a dot

// ---- the host rules, on scalars alone
int mla_indexer_token_block(int max_seqlen_q) { return max_seqlen_q >= 4 ? 4 : max_seqlen_q >= 2 ? 2 : 1; }
// THE CHUNK RULE. A chunk is `chunk_tiles` consecutive 64-key tiles of a sequence; an item is (sequence, token block, chunk). Two pulls:
// a decode step on few long sequences must still fill the chip -- 1024 items, four workgroups on each of 256 compute units -- and a
// chunk must not be so short that the 16 KiB query a wave loads per item weighs against the keys it reads: at least 8 tiles wherever
// the capacity has them. So: as few chunks as give 1024 items, never more than floor(tiles / 8).
int mla_indexer_chunk_tiles(int B, int max_seqlen_q, int page_size, int max_pages_per_seq) {
  const int tb = mla_indexer_token_block(max_seqlen_q);
  const long long nT = ((long long)page_size * max_pages_per_seq + BN - 1) / BN;
  const long long items = (long long)B * ((max_seqlen_q + tb - 1) / tb);
  const long long want = (1024 + items - 1) / items, most = std::max(1LL, nT / 8);
  const long long nch = std::min(want, most);
  return (int)((nT + nch - 1) / nch);
}

template <typename Tag, int HI, int TB>
__global__ __launch_bounds__(64 * IDX_NW) void mla_indexer_logits_kernel(MlaIndexerParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int MT = HI / 16;        // 16-head row tiles of the score tile
  constexpr int CBS = IDX_NW / TB;   // stride of a wave's column blocks; it takes TB of the four

  __shared__ __attribute__((aligned(16))) char smem_generic[2 * IDX_TILE];
  lds_char *smem = (lds_char *)smem_generic;

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  int x = blockIdx.x;
  const int ch = x % p.nchunks;
  x /= p.nchunks;
  const int tb = x % p.nblk, b = x / p.nblk;
  const int lp = p.lp;
  const IdxSeq sq = idx_seq(p.cu_q, p.seqlens, b, p.total_q, p.max_q, p.max_pages << lp);
  const int i0 = tb * TB;
  if (i0 >= sq.Lq) return;  // the block owns no token
  const int vmax = idx_visible(sq, min(i0 + TB - 1, sq.Lq - 1));
  const int t0 = ch * p.chunk_tiles;
  if (t0 * BN >= vmax) return;  // the chunk starts behind the block's last visible key (t0 * 64 < capacity + 64 <= 2^30 + 64)
  const int t1 = min(t0 + p.chunk_tiles, (vmax + BN - 1) / BN);

  // ---- this wave's token: its visible count, its query fragments and its head weights
  const int it = i0 + w % TB;
  const int v = it < sq.Lq ? idx_visible(sq, it) : 0;
  const bool work = v > t0 * BN;  // wave-uniform
  const long long tok = sq.sq + it;
  vec8 qf[MT][IDX_KS];
  float wv[MT][4];
  {
    const elem *qp = (const elem *)p.q + tok * p.q_rs + 8 * g;
    const float *wp = p.w + tok * p.w_rs + 4 * g;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int ks = 0; ks < IDX_KS; ++ks) {
        u32x4 t = {0u, 0u, 0u, 0u};
        if (work) t = *reinterpret_cast<const u32x4 *>(qp + (long long)(16 * m + c) * p.q_hs + 32 * ks);
        qf[m][ks] = __builtin_bit_cast(vec8, t);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) wv[m][i] = work ? wp[16 * m + i] : 0.0f;
    }
  }
  float *out = p.logits + tok * p.logits_stride;

  // ---- staging: rows 16 w .. 16 w + 15 of a tile, one page, one descriptor, four pieces of four rows
  const unsigned rsb = (unsigned)p.row_stride * 2;  // the pool's row stride in bytes
  const int *tbl = p.block_table + (long long)b * p.bt_stride;
  int pg = -1;  // the table entry of this wave's rows of the next tile to stage
  auto fetch_page = [&](int t) __attribute__((always_inline)) { pg = tbl[min((t * BN + 16 * w) >> lp, p.max_pages - 1)]; };
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
    const int P = 1 << lp, key0 = t * BN + 16 * w, row0 = key0 & (P - 1);
    const int page = __builtin_amdgcn_readfirstlane(pg);
    const int nv = min(sq.L - (key0 - row0), P);  // rows of the page below L_b
    const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;
    const long long off = ok ? (long long)page * p.page_stride : 0;
    const unsigned nrec = ok ? (unsigned)(nv - 1) * rsb + IDX_RB : 0u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + off * 2), 0, nrec, 0x00020000);
    const unsigned ll = (unsigned)(__UINTPTR_TYPE__)smem + buf * IDX_TILE + 16 * w * IDX_RB;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = 4 * j + (lane >> 4);  // the row among the wave's sixteen: (16 w + r) & 15 = r
      const unsigned vo = ((unsigned)row0 + r) * rsb + ((((unsigned)lane & 15) ^ r) << 4);
      const unsigned ld = ll + j * 1024;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ld), "v"(vo), "s"(rs) : "memory");
    }
    fetch_page(t + 1);
  };

  fetch_page(t0);
  for (int t = t0 - 1; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of tile t have landed
    __builtin_amdgcn_s_barrier();                     // everyone's have, and everyone is done reading the buffer tile t + 1 overwrites
    if (t + 1 < t1) stage(t + 1, (t + 1 - t0) & 1);
    if (t < t0 || v <= t * BN) continue;  // (wave-uniform) the staging iteration, or a tile this token sees nothing of
    const lds_char *img = smem + ((t - t0) & 1) * IDX_TILE;
#pragma unroll
    for (int k = 0; k < TB; ++k) {
      const int cb = w / TB + k * CBS, kb = t * BN + 16 * cb;
      if (kb >= v) continue;  // (wave-uniform)
      vec8 kf[IDX_KS];
#pragma unroll
      for (int ks = 0; ks < IDX_KS; ++ks)
        kf[ks] = __builtin_bit_cast(vec8, lds_read_b128(img + (16 * cb + c) * IDX_RB + (((4 * ks + g) ^ c) << 4)));
      f32x4 acc[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < IDX_KS; ++ks) acc[m] = M::mfma(qf[m][ks], kf[ks], acc[m]);
      }
      float s = 0.0f;  // heads 16 m + 4 g + i of key kb + c
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) s = __builtin_fmaf(wv[m][i], __builtin_fmaxf(acc[m][i], 0.0f), s);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (g == 0 && kb + c < v) out[kb + c] = s;
    }
  }
}

// ---- the select kernel (idx_block_scan and idx_image: fa_mla_indexer_common.h)
__global__ __launch_bounds__(IDX_SEL_THREADS) void mla_indexer_select_kernel(MlaIndexerSelectParams p) {
  __shared__ int hist[256];
  __shared__ int ws[IDX_SEL_THREADS / 64];
  __shared__ int pick[2];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.max_q, i = blockIdx.x - b * p.max_q;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const IdxSeq sq = idx_seq(p.cu_q, p.seqlens, b, p.total_q, p.max_q, p.max_pages << lp);
  if (i >= sq.Lq) return;  // nobody's token
  const int v = idx_visible(sq, i), topk = p.topk;
  const long long tok = sq.sq + i;
  int *out = p.indices + tok * p.idx_stride;
  const int *tbl = p.block_table + (long long)b * p.bt_stride;
  // position j < v <= L_b -> its slot (j >> lp < max_pages), -1 under a table entry outside the pool
  auto slot = [&](int j) __attribute__((always_inline)) {
    const int page = tbl[j >> lp];
    return (unsigned)page < (unsigned)p.num_pages ? (page << lp) + (j & PM) : -1;
  };
  if (tid == 0) p.counts[tok] = min(topk, v);
  if (v <= topk) {  // everything visible is taken: the logits are not read
    for (int j = tid; j < v; j += IDX_SEL_THREADS) out[j] = slot(j);
    return;
  }
  const float *row = p.logits + tok * p.logits_stride;

  // ---- the threshold: four passes, most significant byte first
  unsigned T = 0;
  int need = topk;  // the rank still looked for among the keys that match the prefix
  for (int pass = 0; pass < 4; ++pass) {
    const int sh = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < v; j += IDX_SEL_THREADS) {
      const unsigned u = idx_image(row[j]);
      if (pass == 0 || (u >> (sh + 8)) == (T >> (sh + 8))) atomicAdd(&hist[(u >> sh) & 255], 1);
    }
    __syncthreads();
    const int bin = 255 - tid, n = hist[bin];  // thread order = bins from the top: the scan counts the keys in greater bins
    int total;
    const int above = idx_block_scan(n, total, ws);
    if (above < need && need <= above + n) {  // exactly one thread: the matching keys number at least `need`
      pick[0] = bin;
      pick[1] = need - above;
    }
    __syncthreads();
    T |= (unsigned)pick[0] << sh;
    need = pick[1];
    __syncthreads();  // (hist and pick are rewritten by the next pass)
  }

  // ---- the emission: every key greater than T and the first `need` keys equal to it, in ascending position
  int ng = 0, ne = 0;  // greater / equal keys in front of this round's 256
  for (int j0 = 0; j0 < v; j0 += IDX_SEL_THREADS) {
    const int j = j0 + tid;
    int gt = 0, eq = 0;
    if (j < v) {
      const unsigned u = idx_image(row[j]);
      gt = u > T;
      eq = u == T;
    }
    int total;
    const int ex = idx_block_scan(gt | (eq << 16), total, ws);  // (at most 256 of either: sixteen bits each)
    const int g0 = ng + (ex & 0xffff), e0 = ne + (ex >> 16);
    if (gt || (eq && e0 < need)) out[g0 + min(e0, need)] = slot(j);
    ng += total & 0xffff;
    ne += total >> 16;
    if (ng + min(ne, need) >= topk) break;  // (workgroup-uniform) the list is complete
  }
}

// ---- launches. Both grids depend on host scalars alone
hipError_t launch_mla_indexer_logits(const MlaIndexerParams &p, int Hi, int dtype, hipStream_t s) {
  (void)hipGetLastError();
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)p.B * p.nblk * p.nchunks)), dim3(64 * IDX_NW), 0, s, p);
    return hipGetLastError();
  };
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    auto by_tb = [&](auto hi) {
      constexpr int HI = decltype(hi)::value;
      return p.tb == 4 ? go(mla_indexer_logits_kernel<Tag, HI, 4>) : p.tb == 2 ? go(mla_indexer_logits_kernel<Tag, HI, 2>) : go(mla_indexer_logits_kernel<Tag, HI, 1>);
    };
    return Hi == 64 ? by_tb(std::integral_constant<int, 64>{}) : by_tb(std::integral_constant<int, 32>{});
  });
}
hipError_t launch_mla_indexer_select(const MlaIndexerSelectParams &p, hipStream_t s) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(mla_indexer_select_kernel, dim3((unsigned)((long long)p.B * p.max_q)), dim3(IDX_SEL_THREADS), 0, s, p);
  return hipGetLastError();
}

}  // namespace fa
