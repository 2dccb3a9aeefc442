// fa_mla_kernel.hip -- absorbed multi-head latent attention, decode form, over a paged latent cache: entry point fa_fwd_mla_decode_paged.
//
// Every query head of a sequence reads ONE shared latent row per key: 576 elements, of which all 576 take part in the score product
// (512 of compressed KV plus 64 of rotary key) and the first 512 are the value. This is fa_decode_kernel.hip's paged decode with one
// pool, two head dims and one LDS image for both products; what it keeps of that kernel, line for line where the shapes allow:
//   * the packed row block: r = h * Nq + iq (every query head shares the one latent "key head": G = Hq), 16 rows per item;
//   * the keys of a sequence SPLIT over S one-wave items (no barrier anywhere), 64-key tiles streamed through a private double buffer
//     in LDS by LDS-DMA, 16x16x32 MFMA, the exact online softmax, the pre-scaled query operand Q~ = round(scale . log2(e) . Q);
//   * per-page range-checked descriptors (rows >= L_b, pages outside the pool: hardware zeros), table entries fetched one tile ahead: the
//     rules stand at the head of fa_mla_paged_partial.inc, the text of the partial kernel, with the staging they govern;
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
//     to 128 rows. Both partial kernels are one text, fa_mla_paged_partial.inc, at NW = 1, 2 or 4 waves; what a wave does with its 16
//     rows from LDS onwards is the text of fa_mla_body.h, whose part 0 states the image's constants for every file of the family.)
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

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types, the launch tail

// item (b, s) x row block rb: rows r = 16 rb + c = h * Nq + iq of the packed block, keys of tiles [t0, t1) of sequence b. The body is
// the text fa_mla_wide_kernel.hip's kernel includes, at one wave: no barrier, no padding wave, the whole tile staged by this wave
template <typename Tag, bool CAUSAL>
__global__ __launch_bounds__(64) void mla_partial_kernel(MlaDecodeParams p) {
  constexpr int NW = 1;
// (this spelling and not the wide file's loop: with the loop these four kernels come out 16 or 17 instructions apart, in the scalar
// prologue that fetches the first table entries)
#define FA_MLA_PG_DECL int pg[4] = {-1, -1, -1, -1};
#include "fa_mla_paged_partial.inc"
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
    auto go = [&](auto partial) { return launch_mla_partial_and_combine(partial, dim3(p.B * p.S, p.RBLK), 1, p, p, dtype, s); };
    return p.is_causal ? go(mla_partial_kernel<Tag, true>) : go(mla_partial_kernel<Tag, false>);
  });
}

}  // namespace fa
