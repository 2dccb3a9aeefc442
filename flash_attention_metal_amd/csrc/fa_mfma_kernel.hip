// fa_mfma_kernel.hip -- the operator on the CDNA4 matrix cores.
//
// Replaces /root/reference/kernels.metal:600-883 (flash_attention_v4_half_kernel)
// and :177-455 (flash_attention_simd_kernel): same math -- tiled QK^T ->
// online softmax -> PV, causal predicate `key > query -> masked`
// (kernels.metal:748), whole-tile skip (kernels.metal:682), L = m + ln(l)
// (kernels.metal:862-864) -- nothing else is shared with it. fp32 accumulators
// for S, O, m, l (the reference accumulates S and O in half).
//
// Structure (one workgroup = 4 waves = 128 query rows of one (batch, head)):
//   * each wave owns 32 query rows; its Q fragments stay in registers
//   * K/V tiles of 64 keys are double-buffered in LDS: the next tile's
//     128-bit buffer loads are issued before the current tile's arithmetic and
//     written to the other buffer after it; one barrier per tile
//   * S^T = K.Q^T with v_mfma_f32_32x32x16 ("swapped" product): the query index
//     lands on the lane, the 32 key scores of a block in that lane's 16
//     accumulator registers (+16 in lane^32), so row max / row sum are
//     in-register reductions plus ONE v_permlane32_swap -- no LDS round trip
//   * P^T feeds the PV product straight from those registers as the B operand
//     (k order inside a step is the accumulator's row order; V^T is read from
//     LDS in the same order with ds_read_b64_tr_b16, so V stays row-major)
//   * O^T accumulates in 16*(D/32) registers; the O rescale is skipped when no
//     row max in the wave moved (exact: alpha == 1)
//   * K rows are XOR-swizzled in LDS for conflict-free ds_read_b128, V rows for
//     conflict-free transposed reads
//   * epilogue: O tile -> LDS -> whole 128-byte rows, 16 B per lane
//   * grid: 1-D, heads dealt to XCDs (blocks b and b+8 share an L2) so one
//     head's K/V stays in one L2; causal q-blocks heaviest first
#include <stdlib.h>

#include <algorithm>

#include "fa_mfma_common.h"

#ifndef FA_DEFER_THR
#define FA_DEFER_THR 8.0f  // log2 units: P values are bounded by 2^8 between rescales (0 = rescale whenever a max moved)
#endif
#ifndef FA_PRESCALE
#define FA_PRESCALE 1  // 1 (f16/bf16): Q~ = round(scale.log2e.Q) once per block and -m (log2 units) as the C operand of each score chain: P = exp2(S') with no FMA
#endif
#ifndef FA_MAIN_OCC4
#define FA_MAIN_OCC4 1  // 1: the plain 128-row kernel at head_dim 64 (16-bit inputs, pre-scaled operand) gives up the V^T prefetch below and
                        // fits 128 registers: FOUR workgroups per CU instead of three. Config 3 +2.6 %, N=8192 +2.7 %, non-causal N=4096
                        // +1.6 %, N<=2048 -0.3..-1.7 % (profiles/r03/ab_four_waves_per_simd.log). Round 3 first tried four with the prefetch
                        // in place and spilled 150-210 B; the split / 64-row / exact forms keep the prefetch and three.
#endif
#ifndef FA_MFMA_DMA
#define FA_MFMA_DMA 1  // 1 (f16/bf16, head_dim 32/64/128): K/V tiles go global -> LDS by LDS-DMA (buffer_load ... lds), no staging registers, no
                       // ds_write: config 3 +6.7 %, head_dim 128 +9..11 %, bit-identical outputs (profiles/r03/ab_mfma_lds_dma.log); 0 = register staging
#endif
#ifndef FA_LAK
#define FA_LAK (D == 128 ? 4 : 2)  // head dims other than 64: K fragments are read this many MFMAs ahead of their use (head_dim 128: 4 since the
#endif                             // LDS-DMA staging freed the registers: +1..2 %, profiles/r03/ab_dma_knobs.log)
#ifndef FA_LAV
#define FA_LAV (D == 128 ? 4 : 2)  // ... and V^T fragments
#endif

namespace fa {

// Which (dtype, head_dim) the pre-scaled query operand exists for: fp8 Q cannot carry the factor (3 mantissa bits), and
// head_dim 256 has no 16 registers to spare for the row-constant tuple.
template <typename Tag, int D>
constexpr bool prescale_applies() {
  return (FA_PRESCALE != 0) && !std::is_same<Tag, FP8>::value && D <= 128;
}

// head dims: 32, 64, 96, 128, 256 (scope row f3). LDS rows keep a power-of-two pitch (head_dim 96 rows sit in
// 256-byte slots) so the XOR swizzles stay inside a row; head_dim 256 needs the whole register file
// (128 accumulators for O^T alone): one workgroup per CU there.
// SPLIT = 2 ("split2" kernel, for grids that leave most of the chip idle): eight waves per workgroup, waves 0-3 and 4-7
// take the even and the odd KV tiles of the same 128 query rows -- each half with its own K/V buffers, staging and
// (m, l, O^T) -- and merge once through LDS by their reference maxima. Halves the sequential tile count of a block.
// PRESC: the pre-scaled query operand (see PRE below); false = every score scaled in fp32 (variant mfma_exact).
// ROWS: query rows per workgroup, 128 (four row groups of 32 = four waves per split) or 64 (two): "h64s2" = 64 rows x 2 splits
// is a four-wave workgroup whose wave pairs take the even / odd KV tiles -- twice the workgroups and half the sequential
// tiles of a block, for causal grids whose critical path is the heaviest q block (N <= 2048 at 64 heads).
// the instantiations of the plain kernel that run four workgroups per CU (FA_MAIN_OCC4)
template <typename Tag, int D, bool PRESC>
constexpr bool main_kernel_occ4() {
  return (FA_MAIN_OCC4 != 0) && D == 64 && PRESC && prescale_applies<Tag, D>();
}

// PT = VarlenParams ("varlen" mode, fa_fwd_varlen): the "batch" index of the block map selects a sequence of a packed
// [total, heads, D] batch; its lengths come from the cu_seqlens tables in device memory and take the place of N / Nk, its rows are
// addressed with a run-time pitch. Everything from LDS onwards -- images, swizzles, MFMA order, softmax -- is the dense kernel's, so a
// sequence comes out bit for bit as the dense kernel computes it alone.
// PT = VarlenPagedParams ("varlen paged" mode, fa_fwd_varlen_paged): the varlen mode's query side, unchanged, over the paged decode's
// key side (fa_decode_kernel.hip, PAGED). The sequence's length L_b comes from seqlens (clamped to the capacity) and takes LK's place;
// every 1-KiB LDS-DMA piece (8 / 4 rows) comes from the page the block table names for it, through a descriptor built on that page's
// 64-bit base whose range covers only the page's valid rows, with the whole in-page offset in voffset. Pages hold >= 16 rows and start
// at multiples of their size, so a piece lies inside ONE page. Each wave loads the table entries of ITS pieces of the next tile one tile
// ahead (one vector load, lane j takes the entry of piece j: NPW = 2 / 4 entries, duplicates when a page holds several pieces; the value
// stays in its register until the NEXT tile's staging makes it wave-uniform). The LDS images are the varlen mode's, and
// rows at or past L_b read as zeros there as here: a sequence comes out bit for bit as fa_fwd_varlen computes it on the gathered cache.
// (overloads, so that the body can name the page tables in an expression both modes compile)
__device__ __forceinline__ int seqlen_paged(const VarlenPagedParams &p, int b) { return p.seqlens[b]; }
__device__ __forceinline__ int seqlen_paged(const Params &, int) { return 0; }
__device__ __forceinline__ int paged_capacity(const VarlenPagedParams &p) { return p.max_pages << p.lp; }
__device__ __forceinline__ int paged_capacity(const Params &) { return 0; }
__device__ __forceinline__ float softcap_of(const VarlenSoftcapParams &p) { return p.softcap; }
__device__ __forceinline__ float softcap_of(const VarlenPagedSoftcapParams &p) { return p.softcap; }
__device__ __forceinline__ float softcap_of(const Params &) { return 0.0f; }
// key-split mode: the workspace's two parts, [S][rows][D] floats of o_s and [S][rows] floats of lse2_s with rows = H . total_q; these two
// give split s's row `row` (= hq . total_q + token, the LSE's index)
template <int D>
__device__ __forceinline__ float *ksplit_o(const VarlenPagedKsplitParams &p, int s, long long row) {
  return p.ws + ((long long)s * p.H * p.total_q + row) * D;
}
template <int D>
__device__ __forceinline__ float *ksplit_lse2(const VarlenPagedKsplitParams &p, int s, long long row) {
  return p.ws + (long long)p.S * p.H * p.total_q * D + (long long)s * p.H * p.total_q + row;
}
// C = softcap . log2(e): a capped score t . softcap in log2 units is t . C (wave-uniform: it lives in a scalar register)
template <typename PT>
__device__ __forceinline__ float softcap_log2(const PT &p) { return softcap_of(p) * 1.4426950408889634f; }
// Dynamic LDS of a workgroup of the body below, the figure every launcher passes: per split the K and V double buffers (K rows of D
// bytes for e4m3 inputs, head_dim 96 rows in 256-byte slots); the epilogue's O tiles sit inside them, and the split merge buffer --
// (16 D/32 + 2) floats per lane of the publishing waves -- behind the O tiles.
// (DV != D, the MLA prefill mode: K rows of D elements in a two-part image, V and O rows of DV)
template <typename Tag, int D, int SPLIT = 1, int ROWS = BM, int DV = D>
constexpr size_t mfma_lds_bytes() {
  constexpr size_t RB = (D == 96) ? 256 : DV * 2, KRB = std::is_same<Tag, FP8>::value ? D : (DV != D) ? D * 2 : RB;
  constexpr size_t otiles = (size_t)ROWS * RB, merge_end = otiles + (size_t)(ROWS / WM) * (16 * (D / 32) + 2) * 64 * 4;
  return std::max(SPLIT * (2 * BN * KRB + 2 * BN * RB), SPLIT == 2 ? merge_end : otiles);
}

template <typename Tag, int D, bool CAUSAL, int SPLIT, bool PRESC, int ROWS = BM, typename PT = Params, int DV = D>
__device__ __forceinline__ void fwd_mfma_body(const PT &p) {
  // MLA (PT = VarlenMlaParams, D = 192, DV = 128; fa_fwd_varlen_mla): the varlen mode with two head dims -- q and k rows of D elements
  // (128 "nope" + 64 rotary), v and o rows of DV -- and a (row, head) stride pair per tensor. Everything from the scores onwards is the
  // head_dim-128 varlen kernel's. The K tile is a two-part LDS image: the nope part [64][128] is the head_dim-128 K image (swizzle chunk ^
  // (row & 15)), the rotary part [64][64] behind it the head_dim-64 K image (chunk ^ ((row >> 1) & 7)); both are staged by LDS-DMA from
  // the same 384-byte key row. A score chain runs the eight nope k-steps in the head_dim-128 kernel's order, then the four rotary ones:
  // with zero rotary columns the call returns fa_fwd_varlen's bits at D = 128.
  constexpr bool MLA = DV != D;
  constexpr int KS_NOPE = MLA ? DV / 16 : D / 16;  // k-steps whose K fragments come from the first part of the K image
  constexpr bool PAGEDV = std::is_base_of<VarlenPagedParams, PT>::value;
  constexpr bool VARLEN = std::is_base_of<VarlenParams, PT>::value;
  // WINDOW (PT = VarlenWindowParams / VarlenPagedWindowParams; fa_fwd_varlen_window, fa_fwd_varlen_paged_window): the varlen modes under
  // a sliding window, key j visible to query i iff i + cl <= j <= i + cu with cl = coff - wl, cu = coff + wr (both bounds run-time
  // scalars, made non-negative by the host). Instantiated with CAUSAL: cu takes coff's place wherever the mask's upper limit is used,
  // and the lower limit is new -- the tile loop starts at the tile of the block's first row's bound, a wave skips tiles wholly below
  // ITS first row's bound, and its first ACTIVE tile takes the exact path.
  constexpr bool WINDOW = std::is_base_of<VarlenWindowParams, PT>::value || std::is_base_of<VarlenPagedWindowParams, PT>::value;
  // SOFTCAP (PT = VarlenSoftcapParams / VarlenPagedSoftcapParams; fa_fwd_varlen_softcap, fa_fwd_varlen_paged_softcap): window mode over
  // capped scores softcap . tanh(scale . s / softcap). The query operand is pre-scaled by 2 log2(e) scale / softcap, so the matrix core
  // delivers y with 2^y = e^(2x), the one exponential tanh needs; the score chains start from zero, not from -m. Per score: t = 1 - 2 /
  // (1 + 2^y), THEN the mask (tanh(-inf) is -1: a key masked before the cap would weigh exp(-softcap)), then P = exp2(fma(t, C, -m)) with
  // C = softcap . log2(e); m stays in log2 units of the capped scores, so everything from P onwards is the window mode's.
  constexpr bool SOFTCAP = std::is_same<PT, VarlenSoftcapParams>::value || std::is_same<PT, VarlenPagedSoftcapParams>::value;
  // SINK (PT = VarlenSinkParams / VarlenPagedSinkParams; fa_fwd_varlen_sink, fa_fwd_varlen_paged_sink): window mode with one more term in
  // every row's denominator, exp(sinks[head]), which carries no value. The tile loop does not know of it: the logit is one wave-uniform
  // scalar load per block, turned to log2 units, and the epilogue folds it into (m, l) by the larger of the row's reference and the sink.
  constexpr bool SINK = std::is_same<PT, VarlenSinkParams>::value || std::is_base_of<VarlenPagedSinkParams, PT>::value;
  // KV8 (PT = VarlenPagedKv8Params / VarlenPagedKv8SinkParams; fa_fwd_varlen_paged_kv8): the paged window / sink mode over pools of OCP
  // e4m3 bytes. K and V tiles cannot travel by LDS-DMA (the LDS image is bf16): every thread loads NCH 16-byte chunks (16 elements) of
  // K and of V into registers through the page's range-checked descriptor, and writes each, widened exactly by fp8x8_to_bf16, as the two
  // bf16 chunks it stands for in the SAME swizzled images. The two LDS buffers and everything from LDS onwards are the bf16 kernel's, so
  // the results are bit for bit those of the paged window / sink kernels on the widened pool.
  constexpr bool KV8 = std::is_same<PT, VarlenPagedKv8Params>::value || std::is_same<PT, VarlenPagedKv8SinkParams>::value;
  // KSPLIT (PT = VarlenPagedKsplitParams; fa_fwd_varlen_paged_split with S >= 2): the paged window mode over ONE of S sub-ranges of the
  // block's tiles. The grid is the block map times S with the split index in blockIdx.y, i.e. outside map_block: the heads of a group
  // keep their places relative to one another inside every split (they share K / V in one XCD's L2), and the splits of a block, which
  // share nothing, lie a whole block map apart. The tile loop runs tiles [t0, t1) of ksplit_tiles; a wave's first tile INSIDE the split
  // takes the exact path. The epilogue writes the normalised state of the block's owned rows to the workspace instead of O / LSE:
  // o_s = acc * (1 / l) in fp32, the existing epilogue's expression before its rounding, and lse2_s = m + log2 l. A row with no visible
  // key in the split has l = 0 over a finite floor or m = -inf: lse2_s = -inf either way, and its o_s (0 * inf) is never read. An empty
  // split and a block without a visible key write lse2_s = -inf alone. The sink is the combine kernel's.
  constexpr bool KSPLIT = std::is_same<PT, VarlenPagedKsplitParams>::value;
  static_assert(!KV8 || std::is_same<Tag, BF16>::value, "KV8 mode: bf16 queries, e4m3 pools widened to bf16");
  static_assert(!WINDOW || CAUSAL, "window mode: the upper bound is the causal one with its own offset");
  static_assert(!MLA || (D == 192 && DV == 128 && std::is_same<PT, VarlenMlaParams>::value), "MLA mode: (192, 128) over VarlenMlaParams");
  static_assert(!VARLEN || (SPLIT == 1 && ROWS == BM && PRESC && !std::is_same<Tag, FP8>::value && (D == 64 || D == 128 || MLA)),
                "varlen mode: the plain 128-row kernel, 16-bit inputs, LDS-DMA staging");
  constexpr int RW = ROWS / WM;   // row groups = waves per split
  constexpr int ST = 64 * RW;     // threads per split (the staging map's width)
  using M = MT<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int GRB16 = D * 2;              // row bytes of a 16-bit row in global memory
  constexpr int RB = (D == 96) ? 256 : DV * 2;  // LDS row pitch (bytes; MLA mode: of a V / O row, and of the K image's nope part)
  constexpr int RBR = 128;                  // MLA mode: row pitch of the K image's rotary part
  constexpr int CPR = DV / 8;               // 16-byte chunks per row that hold data
  constexpr int CPRL = RB / 16;             // 16-byte slots per LDS row (power of two)
  constexpr int KS = D / 16;                // k-steps of the QK^T product
  constexpr int DB = DV / 32;               // 32-wide d blocks of O^T
  constexpr int TILE = BN * RB;             // bytes of one K (or V) tile in LDS
  constexpr bool IS_FP8 = std::is_same<Tag, FP8>::value;  // Q,K,V are e4m3 in HBM, bf16 from LDS onwards
  constexpr int GB = IS_FP8 ? 1 : 2;        // bytes per element in HBM
  constexpr int GRB = KV8 ? D : D * GB;     // global row bytes (of a K / V row; the dense modes: of a Q row too)
  constexpr int GTILE = BN * GRB;           // global bytes of one K (or V) tile
  constexpr int NCH = BN * (GRB / 16) / ST;  // staged 16-byte global chunks per thread per tile
  // (varlen without the mask keeps the prefetch and three workgroups: at 128 registers its extra row pitch and sequence base spill 20 B,
  // some of it reloaded inside the tile loop. The MFMA order is the same in both forms, so the results do not change.)
  // (window mode: three as well -- two more live scalars and a second compare per masked score)
  constexpr bool MAIN4 = (FA_MAIN_OCC4 != 0) && main_kernel_occ4<Tag, D, PRESC>() && SPLIT == 1 && ROWS == BM && !(VARLEN && !CAUSAL) && !WINDOW;
  constexpr bool VPRE = (D == 64) && !IS_FP8 && !MAIN4;  // prefetch V^T fragments under the QK^T MFMAs
  // Pre-scaled operand (f16/bf16): the Q fragments are multiplied by c = scale.log2(e) and rounded back to the input
  // type ONCE per block, and the running reference -m (log2 units) is the C operand of the first MFMA of every score
  // chain, so the matrix core hands out S' = c.q.k - m and P = exp2(S') needs no v_fma (kernels.metal:763-771 scales
  // and subtracts per score). Costs one rounding of c.q (2^-9 relative for bf16, 2^-12 for f16) per operand element:
  // the score error stays a fraction of the P rounding that follows; LSE error scales with the score magnitude
  // (include/fa_mi355.h states the bound).
  constexpr bool PRE = PRESC && (MLA || prescale_applies<Tag, D>());
  // fp8 inputs: the score product runs on v_mfma_scale_f32_32x32x64_f8f6f4 (unit E8M0 scales: an exact e4m3 product
  // at twice the bf16 rate, K = 64 per instruction). K stays e4m3 in LDS (rows of D bytes) and Q stays e4m3 in
  // registers; V is widened to bf16 while it is staged, because P has to be bf16 for the PV product anyway.
  constexpr int KRB = IS_FP8 ? D : RB;      // K row pitch in LDS (bytes)
  constexpr int KTILE = MLA ? BN * (RB + RBR) : BN * KRB;  // bytes of one K tile in LDS
  constexpr int NS8 = IS_FP8 ? D / 64 : 1;  // fp8: 64-wide k-steps of the score product
  typedef int i32x8 __attribute__((ext_vector_type(8)));

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  const int wave_all = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int sp = (SPLIT == 1) ? 0 : (wave_all / RW);  // which KV split this wave works on
  constexpr int GROUP_LDS = 2 * KTILE + 2 * TILE;     // K and V double buffers of one split
  constexpr size_t LDS = mfma_lds_bytes<Tag, D, SPLIT, ROWS, DV>();
  static_assert(SPLIT * GROUP_LDS <= LDS && RW * WM * RB <= LDS, "the launchers' LDS size covers the K / V buffers and the epilogue's O tiles");
  static_assert(SPLIT == 1 || RW * WM * RB + RW * (16 * DB + 2) * 64 * 4 <= LDS, "... and the split merge buffer");
  lds_char *smem = (lds_char *)smem_generic + sp * GROUP_LDS;
  lds_char *Kbuf = smem;              // [2][BN][KRB], rows swizzled
  lds_char *Vbuf = smem + 2 * KTILE;  // [2][BN][RB], rows swizzled

  const int tid = threadIdx.x & (ST - 1);  // thread within its split's waves (staging map)
  const int lane = tid & 63;
  const int wave = wave_all & (RW - 1);          // row group: query rows 32*wave .. +31 of the block
  const int r = lane & 31;  // query within the wave / key row within a block
  const int h = lane >> 5;  // lane half

  // ---- block -> (batch*head, q block). blocks b and b+8 share an XCD's L2:
  // deal heads to the 8 residues so a head's K/V stays in one L2.
  int bh, qb;
  map_block<CAUSAL>(blockIdx.x, p, bh, qb);
  long long base, base_kv;
  // varlen only (each use below keeps the dense expression in the other arm of a compile-time choice, so that the dense kernels
  // compile to the code they had before the mode existed):
  int LQ = 0, LK = 0;          // queries and keys of this block's sequence
  unsigned qrb = 0, kvrb = 0;  // row pitch of Q / O and of K / V in global memory, bytes
  long long base_v = 0, base_o = 0;  // MLA mode: V and O have bases and row pitches of their own
  unsigned vrb = 0, orb = 0;
  long long lse_base = 0;      // first LSE element of this block's (head, sequence)
  const int *ptbl = nullptr;   // varlen paged: this sequence's row of the block table
  int cl = 0, cu = 0;          // window mode: key j is visible to row i iff i + cl <= j <= i + cu
  int t_lo = 0, kv_hi = 0;     // window mode: the block's first tile and the end of its key range
  float sink = 0.0f;           // sink mode: sinks[head], natural-log units
#define FA_NQ (VARLEN ? LQ : p.N)
#define FA_NK (VARLEN ? LK : p.Nk)
  if constexpr (VARLEN) {
    // ---- sequence b = the "batch" index. Both cu pairs are wave-uniform (scalar loads); every entry is clamped to [0, total], a
    // non-increasing pair is length 0 and a length stops at max_seqlen, so whatever the tables hold the block stays inside tokens
    // [0, total) of every tensor. The host never sees the lengths: the grid is sized by max_seqlen_q, and a block past its sequence's
    // last row leaves here, in front of every barrier.
    const int b = (int)fdiv((unsigned)bh, p.fd_h), hq = bh - b * p.H;
    const int sq = min(max(p.cu_q[b], 0), p.total_q), eq = min(max(p.cu_q[b + 1], 0), p.total_q);
    // (varlen paged: no key table; the cache length -- with the chunk already appended -- comes from seqlens, clamped to the capacity)
    const int sk = PAGEDV ? 0 : min(max(p.cu_k[PAGEDV ? 0 : b], 0), p.total_k), ek = PAGEDV ? 0 : min(max(p.cu_k[PAGEDV ? 0 : b + 1], 0), p.total_k);
    LQ = min(max(eq - sq, 0), p.N);
    LK = PAGEDV ? min(max(__builtin_amdgcn_readfirstlane(seqlen_paged(p, b)), 0), paged_capacity(p)) : min(max(ek - sk, 0), p.Nk);
    if (qb * ROWS >= LQ) return;
    base = (long long)sq * p.q_rs + (long long)hq * p.head_stride;
    base_kv = (long long)sk * p.kv_rs + (long long)fdiv((unsigned)hq, p.fd_gq) * p.kv_head_stride;  // (varlen paged: the key head's offset inside a page)
    if constexpr (PAGEDV) ptbl = p.block_table + (long long)b * p.bt_stride;
    lse_base = (long long)hq * p.total_q + sq;
    if constexpr (SINK) sink = p.sinks[hq];
    qrb = (unsigned)p.q_rs * 2;
    kvrb = (unsigned)p.kv_rs * (KV8 ? 1 : 2);
    if constexpr (MLA) {
      base_v = (long long)sk * p.v_rs + (long long)fdiv((unsigned)hq, p.fd_gq) * p.v_head_stride;
      base_o = (long long)sq * p.o_rs + (long long)hq * p.o_head_stride;
      vrb = (unsigned)p.v_rs * 2;
      orb = (unsigned)p.o_rs * 2;
    }
    // no key is visible to any row of the block (no keys at all, or causal with Lk < Lq: key j is visible to query i iff
    // j <= i + Lk - Lq): O = 0, LSE = -inf, as the paged decode defines it
    // (window mode: the block's rows see keys [k_lo, kv_hi) together; none when the range is empty: kv_hi = 0 then)
    if constexpr (WINDOW) {
      int k_lo;
      window_key_range(LQ, LK, p.wl, p.wr, qb * ROWS, qb * ROWS + ROWS - 1, k_lo, kv_hi);
      cl = LK - LQ - p.wl;
      cu = LK - LQ + p.wr;
      t_lo = k_lo / BN;
      if (k_lo >= kv_hi) kv_hi = 0;
    }
    if ((WINDOW ? kv_hi : CAUSAL ? min(LK, qb * ROWS + ROWS + LK - LQ) : LK) <= 0) {
      if constexpr (KSPLIT) {  // every split says "no key" for the block's owned rows; the combine kernel writes O = 0 and the LSE
        const int row = qb * ROWS + (int)threadIdx.x;
        if ((int)threadIdx.x < ROWS && row < LQ) *ksplit_lse2<D>(p, (int)blockIdx.y, lse_base + row) = -INFINITY;
        return;
      }
      elem *Oz = (elem *)p.o + (MLA ? base_o : base);
      for (int idx = threadIdx.x; idx < ROWS * CPR; idx += NTHREADS) {
        const int row = qb * ROWS + idx / CPR, ch = idx % CPR;
        if (row < LQ) *reinterpret_cast<u32x4 *>(Oz + (long long)row * (MLA ? (long long)(orb / 2) : p.q_rs) + ch * 8) = u32x4{0u, 0u, 0u, 0u};
      }
      const int row = qb * ROWS + (int)threadIdx.x;
      if (p.lse != nullptr && (int)threadIdx.x < ROWS && row < LQ) p.lse[lse_base + row] = SINK ? sink : -INFINITY;  // (sink mode: the sink alone)
      return;
    }
  } else {
    head_bases(bh, p, base, base_kv);
  }
  // grouped-query heads: query head h reads key/value head h / (H / Hkv); Nk keys per head.
  // Causal with Nq != Nk is bottom-right aligned: key j visible to query i iff j <= i + coff (varlen: coff may be negative).
  const int coff = FA_NK - FA_NQ;
  const int cup = WINDOW ? cu : coff;  // the upper limit's offset
  const int q0 = qb * ROWS;
  const int qw0 = q0 + wave * WM;  // first query row of this wave
  const int qrow = qw0 + r;

  // (varlen: the descriptors end with the last row's D elements, so rows at or past the sequence's end read as zero whatever the pitch)
  const unsigned head_bytes = VARLEN ? (unsigned)(LQ - 1) * qrb + GRB16 : (unsigned)p.N * GRB;
  // (varlen paged: K / V have no descriptor of the whole head, every piece builds its page's; these two stay empty and unused)
  const unsigned kv_head_bytes = PAGEDV ? 0u : VARLEN ? (unsigned)(LK - 1) * kvrb + GRB : (unsigned)p.Nk * GRB;
  const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
      (void *)((const char *)p.q + base * GB), 0, head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
      (void *)((const char *)p.k + (PAGEDV ? 0 : base_kv) * GB), 0, kv_head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
      (void *)((const char *)p.v + (PAGEDV ? 0 : MLA ? base_v : base_kv) * GB), 0, MLA ? (unsigned)(LK - 1) * vrb + DV * 2 : kv_head_bytes, 0x00020000);

  // ---- Q fragments (B operand of K.Q^T): lane (r,h) holds Q[qrow][16ks+8h .. +7].
  // Rows >= N read as zero through the descriptor's range check.
  vec8 qf[IS_FP8 ? 1 : KS];
  i32x8 qf8[NS8];  // fp8: k-step j holds Q[qrow][64j + 32h .. +31] (32 e4m3 values; any k order works as long as K uses the same)
  if constexpr (IS_FP8) {
#pragma unroll
    for (int j = 0; j < NS8; ++j) {
      const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rq, (unsigned)qrow * GRB + 64 * j + 32 * h, 0, 0);
      const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(rq, (unsigned)qrow * GRB + 64 * j + 32 * h + 16, 0, 0);
      qf8[j] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rq, (VARLEN ? (unsigned)qrow * qrb : (unsigned)qrow * GRB16) + (2 * ks + h) * 16, 0, 0);
      qf[ks] = __builtin_bit_cast(vec8, t);
    }
  }

  // ---- per-lane LDS offsets
  // K: ds_read_b128 of row (32kb + r), chunk (2ks + h); swizzle depends on r only
  const int kx = (D == 32) ? ((r >> 2) & 3) : (D == 64) ? ((r >> 1) & 7) : (r & 15);
  int koff[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (MLA && ks >= KS_NOPE) koff[ks] = BN * RB + r * RBR + (((2 * (ks - KS_NOPE) + h) ^ ((r >> 1) & 7)) << 4);  // the rotary part
    else koff[ks] = r * RB + (((2 * ks + h) ^ kx) << 4);
  }
  // bytes between rows r and 32 + r of the K image that k-step ks reads
#define FA_K32(ks) ((MLA && (ks) >= KS_NOPE) ? 32 * RBR : 32 * RB)
  // fp8 K rows are D bytes: the row image equals a 16-bit row of head_dim D/2 (same swizzle family)
  const int kx8 = (D == 64) ? ((r >> 2) & 3) : (D == 128) ? ((r >> 1) & 7) : (r & 15);
  // V: transposed read; 16-lane group g covers d columns 16(g&1).. of block db,
  // lane 4q+pp of the group addresses row (.. + 4h + q), columns 4pp..4pp+3
  const int g1 = (lane >> 4) & 1, vq = (lane >> 2) & 3, vp = lane & 3;
  const int vx = (D == 32) ? 0 : (D == 64) ? (((vq >> 1) & 1) << 2) : (vq << 2);
  int voff[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
    voff[db] = (4 * h + vq) * RB + ((((4 * db) ^ vx) + 2 * g1 + (vp >> 1)) << 4) + 8 * (vp & 1);

  // Absolute LDS addresses of this lane's fragment reads, made opaque ONCE: the dynamic-LDS base is a link-time
  // constant hipcc cannot fold, and with plain offsets it re-added it ("v_add_u32 x, 0, y") six times per tile.
  const lds_char *kptr[KS], *vptr[DB];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kptr[ks] = Kbuf + koff[ks];
    asm volatile("" : "+v"(kptr[ks]));
  }
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    vptr[db] = Vbuf + voff[db];
    asm volatile("" : "+v"(vptr[db]));
  }

  // ---- staging: thread -> NCH 16-byte chunks of the K tile and of the V tile
  // (fp8: a 16-byte global chunk holds 16 elements = chunks 2c and 2c+1 of the bf16 row image in LDS,
  //  each swizzled on its own: st_k/st_v address chunk 2c, st_k1/st_v1 chunk 2c+1)
  constexpr int GCPR = GRB / 16;  // global chunks per row
  int st_g[NCH], st_k[NCH], st_v[NCH], st_k1[IS_FP8 ? NCH : 1], st_v1[IS_FP8 ? NCH : 1];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = tid + i * ST;
    const int row = c / GCPR, gch = c % GCPR;
    st_g[i] = (VARLEN ? (int)(row * kvrb) : row * GRB) + gch * 16;
    const int skx = (D == 32) ? ((row >> 2) & 3) : (D == 64) ? ((row >> 1) & 7) : (row & 15);
    const int svx = (D == 32) ? 0 : (D == 64) ? (((row >> 1) & 1) << 2) : ((row & 3) << 2);
    const int ch = (IS_FP8 || KV8) ? 2 * gch : gch;
    st_v[i] = row * RB + ((ch ^ svx) << 4);
    if constexpr (IS_FP8) {
      const int skx8 = (D == 64) ? ((row >> 2) & 3) : (D == 128) ? ((row >> 1) & 7) : (row & 15);
      st_k[i] = row * KRB + ((gch ^ skx8) << 4);  // raw e4m3 chunk
      st_k1[i] = 0;
      st_v1[i] = row * RB + (((ch + 1) ^ svx) << 4);
    } else {
      st_k[i] = row * RB + ((ch ^ skx) << 4);  // (KV8: K is widened as well; chunk 2c + 1 of either image is the address of 2c XOR 16)
    }
  }

  const int kv_end = WINDOW ? kv_hi : CAUSAL ? min(FA_NK, q0 + ROWS + coff) : FA_NK;  // (varlen: >= 1 here)
  int ks_t0 = 0, ks_t1 = 0;  // key-split mode: this split's tiles of the block's range [t_lo, ceil(kv_end / BN))
  if constexpr (KSPLIT) {
    ksplit_tiles(t_lo, (kv_end + BN - 1) / BN, (int)blockIdx.y, p.S, ks_t0, ks_t1);
    if (ks_t0 >= ks_t1) {  // an empty split (n < S): "no key" for the block's owned rows, in front of every barrier
      const int row = q0 + (int)threadIdx.x;
      if ((int)threadIdx.x < ROWS && row < LQ) *ksplit_lse2<D>(p, (int)blockIdx.y, lse_base + row) = -INFINITY;
      return;
    }
  }
  const int tb = KSPLIT ? ks_t0 : WINDOW ? t_lo : 0;            // the block's first tile (key-split mode: the split's)
  // this wave's first active tile (the exact path's "first tile"; key-split mode: not before the split's first)
  const int tfw = KSPLIT ? max(ks_t0, max(0, qw0 + cl) / BN) : WINDOW ? max(0, qw0 + cl) / BN : sp;
  const int nT = KSPLIT ? ks_t1 : (kv_end + BN - 1) / BN;

  // LDS-DMA staging (FA_MFMA_DMA): wave w of a split moves the 1-KiB pieces w, w + RW, ... of each tile; inside a piece the
  // LDS image is lane-linear, so the chunk swizzle sits on the SOURCE address (one per-lane offset for K, one for V)
  constexpr bool DMA = (FA_MFMA_DMA != 0) && !IS_FP8 && !KV8 && (D == 32 || D == 64 || D == 128 || MLA);
  constexpr int RPP = 1024 / RB;                 // rows per piece
  constexpr int NPW = (BN / RPP) / RW;           // pieces per wave, tile and operand
  unsigned dma_kvo = 0, dma_vvo = 0;
  unsigned dma_kro = 0;  // MLA mode: the rotary part's pieces, 8 rows of 128 bytes from byte 256 of the key row
  constexpr int RPPR = 1024 / RBR, NPWR = (BN / RPPR) / RW;
  if constexpr (MLA) {
    static_assert((RW * RPPR) % 16 == 0 && NPWR >= 1, "the piece stride must keep the swizzle");
    const int row = wave * RPPR + lane / (RBR / 16), pc = lane % (RBR / 16);
    dma_kro = row * kvrb + DV * 2 + ((pc ^ ((row >> 1) & 7)) << 4);
  }
  if constexpr (DMA) {
    static_assert((RW * RPP) % 16 == 0 || D == 32, "the piece stride must keep the swizzle");
    const int row = wave * RPP + lane / CPRL, pc = lane % CPRL;
    const int skx = (D == 32) ? ((row >> 2) & 3) : (D == 64) ? ((row >> 1) & 7) : (row & 15);
    const int svx = (D == 32) ? 0 : (D == 64) ? (((row >> 1) & 1) << 2) : ((row & 3) << 2);
    dma_kvo = VARLEN ? row * kvrb + ((pc ^ skx) << 4) : (unsigned)(row * GRB + ((pc ^ skx) << 4));
    dma_vvo = VARLEN ? row * (MLA ? vrb : kvrb) + ((pc ^ svx) << 4) : (unsigned)(row * GRB + ((pc ^ svx) << 4));
    if constexpr (PAGEDV) {  // the lane's row inside its piece only: the piece's own slot in its page is wave-uniform and added per piece
      dma_kvo = (lane / CPRL) * kvrb + ((pc ^ skx) << 4);
      dma_vvo = (lane / CPRL) * kvrb + ((pc ^ svx) << 4);
    }
  }
  // ---- varlen paged: lane j of pgv = the table entry of the page that holds this wave's piece j of the next tile to stage, loaded one
  // tile ahead: ONE global_load_dword per wave and tile, issued behind the tile's LDS-DMA statements. Nothing reads pgv before the next
  // tile's staging (v_readlane per piece), i.e. behind the vmcnt(0) and the barrier that end this tile: a wait placed at the load would
  // drain the K / V pieces that have just been issued, in front of the tile's MFMAs. A piece starts at key t * BN + (wave + RW * j) * RPP;
  // the index never leaves the row's max_pages entries (a tile may reach past the capacity: those pieces have no valid row and read as
  // zeros whatever the entry says).
  // KV8 mode: the same one tile ahead for the wave's NCH register loads of a tile. Load i of a wave covers the 64 chunks wave * 64 +
  // i * ST .., i.e. RPL = 64 / GCPR whole rows (16 at head_dim 64, 8 at 128) from row wave * RPL + i * (ST / GCPR) of the tile: aligned to
  // RPL <= 16 rows, hence inside ONE page, and the descriptor of a load is wave-uniform.
  constexpr int RPL = 64 / GCPR;
  const unsigned kv8_vo = KV8 ? (unsigned)(lane / GCPR) * kvrb + (lane % GCPR) * 16 : 0u;  // the lane's chunk inside its load's rows
  int pgv = 0;
  auto fetch_pages = [&](int t) __attribute__((always_inline)) {
    if constexpr (KV8) {
      const int kp = t * BN + wave * RPL + (lane & (NCH - 1)) * (ST / GCPR);
      pgv = ptbl[min(kp >> p.lp, p.max_pages - 1)];
    } else if constexpr (PAGEDV) {
      const int kp = t * BN + (wave + RW * (lane & (NPW - 1))) * RPP;
      pgv = ptbl[min(kp >> p.lp, p.max_pages - 1)];
    }
  };
  auto stage_dma = [&](int t, int buf) {  // tile t -> buffer buf (hipcc does not count these loads: the caller waits vmcnt(0))
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      const unsigned soff = VARLEN ? ((unsigned)t * BN + j * (RW * RPP)) * kvrb : (unsigned)t * GTILE + j * (RW * 1024);  // (dense: a piece's RPP rows are 1024 bytes)
      const unsigned lk = (unsigned)(__UINTPTR_TYPE__)Kbuf + buf * KTILE + (wave + RW * j) * 1024;
      const unsigned lv = (unsigned)(__UINTPTR_TYPE__)Vbuf + buf * TILE + (wave + RW * j) * 1024;
      if constexpr (PAGEDV) {
        // this piece's page: a descriptor on the page's 64-bit base (+ the key head) that ends with the last valid row's D elements
        // (rows >= L_b, and every row of a page index outside the pool, read as zeros); the slot's offset goes into voffset
        const int P = 1 << p.lp, kp = t * BN + (wave + RW * j) * RPP;
        const int page = __builtin_amdgcn_readlane(pgv, j);
        const int nv = min(LK - (kp & -P), P);  // valid rows of the page
        const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;
        const long long off = ok ? (long long)page * p.page_stride + base_kv : 0;
        const unsigned nrec = ok ? (unsigned)(nv - 1) * kvrb + GRB16 : 0u;
        const __amdgpu_buffer_rsrc_t rkp = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + off * 2), 0, nrec, 0x00020000);
        const __amdgpu_buffer_rsrc_t rvp = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.v + off * 2), 0, nrec, 0x00020000);
        const unsigned so = (unsigned)(kp & (P - 1)) * kvrb;
        const unsigned vk = dma_kvo + so, vv = dma_vvo + so;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lk), "v"(vk), "s"(rkp) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lv), "v"(vv), "s"(rvp) : "memory");
      } else if constexpr (MLA) {  // the varlen arm below with V at its own pitch
        const unsigned vk = dma_kvo + soff, vv = dma_vvo + ((unsigned)t * BN + j * (RW * RPP)) * vrb;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lk), "v"(vk), "s"(rk) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lv), "v"(vv), "s"(rv) : "memory");
      } else if constexpr (VARLEN) {
        // the whole offset in voffset, i.e. inside the descriptor's range check: what follows a sequence's last key is another sequence
        // or the end of the tensor, and both must read as zeros (the dense kernel's heads end where its descriptors end)
        const unsigned vk = dma_kvo + soff, vv = dma_vvo + soff;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lk), "v"(vk), "s"(rk) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lv), "v"(vv), "s"(rv) : "memory");
      } else {
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lk), "v"(dma_kvo), "s"(rk), "s"(soff) : "memory");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lv), "v"(dma_vvo), "s"(rv), "s"(soff) : "memory");
      }
    }
    if constexpr (MLA) {  // the rotary part, behind the nope part in the K buffer: the same key rows through the same descriptor
#pragma unroll
      for (int j = 0; j < NPWR; ++j) {
        const unsigned lr = (unsigned)(__UINTPTR_TYPE__)Kbuf + buf * KTILE + BN * RB + (wave + RW * j) * 1024;
        const unsigned vr = dma_kro + ((unsigned)t * BN + j * (RW * RPPR)) * kvrb;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lr), "v"(vr), "s"(rk) : "memory");
      }
    }
    if constexpr (PAGEDV) fetch_pages(t + 1);
  };
  // fp8 inputs: the K tile stays raw e4m3 in LDS (rows of D bytes), so IT can travel by LDS-DMA; V is widened to bf16 on the way
  // and keeps the register path
  constexpr bool DMA_K8 = (FA_MFMA_DMA != 0) && IS_FP8;
  constexpr int RPP8 = 1024 / KRB, NPW8 = (BN / RPP8) / RW;  // rows per piece / pieces per wave of an e4m3 K tile
  unsigned dma_k8o = 0;
  if constexpr (DMA_K8) {
    static_assert((RW * RPP8) % 16 == 0 && NPW8 >= 1, "the piece stride must keep the swizzle");
    constexpr int CPR8 = KRB / 16;
    const int row = wave * RPP8 + lane / CPR8, pc = lane % CPR8;
    const int skx8 = (D == 64) ? ((row >> 2) & 3) : (D == 128) ? ((row >> 1) & 7) : (row & 15);
    dma_k8o = (unsigned)(row * GRB + ((pc ^ skx8) << 4));
  }
  auto stage_dma_k8 = [&](int t, int buf) {
#pragma unroll
    for (int j = 0; j < NPW8; ++j) {
      const unsigned soff = (unsigned)t * GTILE + j * (RW * 1024);
      const unsigned lk = (unsigned)(__UINTPTR_TYPE__)Kbuf + buf * KTILE + (wave + RW * j) * 1024;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lk), "v"(dma_k8o), "s"(rk), "s"(soff) : "memory");
    }
  };
  u32x4 kst[NCH], vst[NCH];
  auto stage_load = [&](int t) {
    if constexpr (KV8) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        // this load's page, as in stage_dma's paged arm: a descriptor on the page's 64-bit base (+ the key head) that ends with the last
        // valid row's D BYTES (rows >= L_b, and every row of a page index outside the pool, read as zeros: 0 records); the in-page offset
        // goes into voffset, so no address is formed outside the page's valid rows
        const int P = 1 << p.lp, kp = t * BN + wave * RPL + i * (ST / GCPR);
        const int page = __builtin_amdgcn_readlane(pgv, i);
        const int nv = min(LK - (kp & -P), P);  // valid rows of the page
        const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;
        const long long off = ok ? (long long)page * p.page_stride + base_kv : 0;
        const unsigned nrec = ok ? (unsigned)(nv - 1) * kvrb + GRB : 0u;
        const __amdgpu_buffer_rsrc_t rkp = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + off), 0, nrec, 0x00020000);
        const __amdgpu_buffer_rsrc_t rvp = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.v + off), 0, nrec, 0x00020000);
        const unsigned vo = kv8_vo + (unsigned)(kp & (P - 1)) * kvrb;
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rkp, vo, 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rvp, vo, 0, 0);
      }
      fetch_pages(t + 1);  // behind the tile's loads; nothing reads it before the next tile's stage_load
    } else {
    const unsigned g0 = VARLEN ? (unsigned)t * BN * kvrb : (unsigned)t * GTILE;  // tile t starts at key t*BN
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (!DMA_K8) kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, g0 + st_g[i], 0, 0);
      vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, g0 + st_g[i], 0, 0);
    }
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (IS_FP8) {  // K: raw e4m3; V: e4m3 -> bf16 is exact, 16 elements = two bf16 chunks
        if constexpr (!DMA_K8) lds_write_b128(Kbuf + buf * KTILE + st_k[i], kst[i]);
        lds_write_b128(Vbuf + buf * TILE + st_v[i], fp8x8_to_bf16(u32x2{vst[i][0], vst[i][1]}));
        lds_write_b128(Vbuf + buf * TILE + st_v1[i], fp8x8_to_bf16(u32x2{vst[i][2], vst[i][3]}));
      } else if constexpr (KV8) {  // K and V: e4m3 -> bf16 is exact, 16 elements = two bf16 chunks of the row image
        lds_write_b128(Kbuf + buf * KTILE + st_k[i], fp8x8_to_bf16(u32x2{kst[i][0], kst[i][1]}));
        lds_write_b128(Kbuf + buf * KTILE + (st_k[i] ^ 16), fp8x8_to_bf16(u32x2{kst[i][2], kst[i][3]}));
        lds_write_b128(Vbuf + buf * TILE + st_v[i], fp8x8_to_bf16(u32x2{vst[i][0], vst[i][1]}));
        lds_write_b128(Vbuf + buf * TILE + (st_v[i] ^ 16), fp8x8_to_bf16(u32x2{vst[i][2], vst[i][3]}));
      } else {
        lds_write_b128(Kbuf + buf * KTILE + st_k[i], kst[i]);
        lds_write_b128(Vbuf + buf * TILE + st_v[i], vst[i]);
      }
    }
  };

  f32x16 oacc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[db][i] = 0.0f;
  float m = -INFINITY;     // reference max of this row's scores (may lag the true max by < 2^THR); units: raw scores, PRE: log2 units
  float l = 0.0f;          // this lane half's share of the running sum
  const float c2 = p.scale * 1.4426950408889634f;  // scale * log2(e)
  const float cm = PRE ? 1.0f : c2;                // m's units -> log2 units
  // PRE: -m in all 16 registers of a tuple = the C operand of each score chain's first MFMA (0 until the first tile has
  // set m: the first tile's scores come out raw and go through the exact path)
  f32x16 negm;
#pragma unroll
  for (int i = 0; i < 16; ++i) negm[i] = 0.0f;
  if constexpr (PRE && !SOFTCAP) asm volatile("" : "+v"(negm));  // opaque: else hipcc re-materialises the splat in front of every MFMA

  if constexpr (DMA) {
    if constexpr (PAGEDV) fetch_pages(tb);
    stage_dma(tb + sp, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    if constexpr (DMA_K8) stage_dma_k8(sp, 0);
    if constexpr (KV8) fetch_pages(tb);
    stage_load(KV8 ? tb : sp);  // this split's first tile (past the end of a short head: zeros through the descriptor, never used)
    stage_write(0);
    if constexpr (DMA_K8) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  // Retire the Q-fragment loads HERE: hipcc's waitcnt pass otherwise carries them into the
  // loop as "possibly pending" and drains vmcnt(0) in front of every tile's first MFMAs, i.e.
  // waits for the prefetch it has just issued (seen in the .s as vmcnt(3)..vmcnt(0)).
  if constexpr (IS_FP8) {
#pragma unroll
    for (int j = 0; j < NS8; ++j) asm volatile("" : "+v"(qf8[j]));
  } else {
    if constexpr (PRE) {  // Q~ = round(c.Q), once per block
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (SOFTCAP) qf[ks][j] = (elem)((float)qf[ks][j] * (2.0f * c2 / softcap_of(p)));  // (softcap mode: 2 log2(e) scale / softcap)
          else qf[ks][j] = (elem)((float)qf[ks][j] * c2);
        }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
  }
  __syncthreads();

  const float sum_thr = __builtin_exp2f(FA_DEFER_THR);
  // cold path of the softmax: the scores of the current tile once more (plain product, no prefetching)
  auto recompute_scores = [&](auto bufc, f32x16 (&s)[2], const int kv0, const bool need_mask) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = 0.0f;
      if constexpr (IS_FP8) {
#pragma unroll
        for (int j = 0; j < NS8; ++j) {
          const lds_char *kr = Kbuf + buf * KTILE + (32 * kb + r) * KRB;
          const u32x4 a = lds_read_b128(kr + (((4 * j + 2 * h) ^ kx8) << 4));
          const u32x4 b = lds_read_b128(kr + (((4 * j + 2 * h + 1) ^ kx8) << 4));
          const i32x8 kf8 = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
          s[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf8, qf8[j], s[kb], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const vec8 kf = __builtin_bit_cast(vec8, lds_read_b128(kptr[ks] + buf * KTILE + kb * FA_K32(ks)));
          s[kb] = M::mfma(kf, qf[ks], s[kb]);
        }
      }
    }
    if constexpr (SOFTCAP) {  // the cap, in front of the mask as in the tile
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] = tanh_from_exp2_arg(s[kb][i]);
    }
    if (need_mask) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        int lim = FA_NK - 1 - kv0 - 32 * kb - 4 * h;
        if (CAUSAL) lim = min(lim, qrow + cup - kv0 - 32 * kb - 4 * h);
        const int llo = qrow + cl - kv0 - 32 * kb - 4 * h;  // (window mode)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int kpart = (i & 3) + 8 * (i >> 2);
          s[kb][i] = (kpart > lim || (WINDOW && kpart < llo)) ? -INFINITY : s[kb][i];
        }
      }
    }
  };
  // One KV tile; BUF (the LDS buffer holding tile t) is a compile-time constant so every
  // LDS address is a per-lane base register plus an immediate.
  auto tile = [&](auto bufc, const int t) {
    constexpr int buf = decltype(bufc)::value;
    const int kv0 = t * BN;
    if (t + SPLIT < nT) {  // this split's next tile, in flight under this tile's MFMAs (issuing the LDS-DMA pieces behind the score
      if constexpr (DMA) {  // MFMAs instead was measured: -29 % on causal shapes, profiles/r03/ab_dma_late_and_d128_auto.log)
        stage_dma(t + SPLIT, buf ^ 1);
      } else {
        if constexpr (DMA_K8) stage_dma_k8(t + SPLIT, buf ^ 1);
        stage_load(t + SPLIT);
      }
    }

    // whole-tile skip per wave (kernels.metal:682 with Br = 32): every key of
    // the tile is past this wave's last query row
    // (window mode: or every key of the tile is below this wave's first row's bound)
    const bool wave_active = (SPLIT == 1 || t < nT) && (!CAUSAL || (kv0 <= qw0 + WM - 1 + cup)) && (!WINDOW || (kv0 + BN - 1 >= qw0 + cl));
    if (wave_active) {
      const lds_char *Kt = Kbuf + buf * KTILE;  // (fp8 score path only)
      (void)Kt;
      // ---- S^T = K.Q^T : s[kb][reg] = S[q = r][key = kv0 + 32kb + (reg&3) + 8(reg>>2) + 4h]
      // All K fragment reads are issued before the first MFMA, and (D = 64) the V^T
      // fragments of the PV product are streamed in between the MFMAs, two transposed
      // reads per MFMA: they do not depend on the softmax, so PV finds its operands in
      // registers instead of waiting on LDS per MFMA. sched_barrier pins that order.
      // Wave priority is raised around the two MFMA clusters (+0.4..0.9 % A/B; around the softmax instead: -1..-6 %).
      __builtin_amdgcn_s_setprio(1);
      f32x16 s[2];
      s16x4 vlo[VPRE ? 2 : 1][2][DB], vhi[VPRE ? 2 : 1][2][DB];
      if constexpr (VPRE) {
        vec8 kf[2][KS];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            kf[kb][ks] = __builtin_bit_cast(vec8, lds_read_b128(kptr[ks] + buf * KTILE + kb * 32 * RB));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
          for (int i = 0; i < 16; ++i) s[kb][i] = 0.0f;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            s[kb] = M::mfma(kf[kb][ks], qf[ks], (PRE && !SOFTCAP && ks == 0) ? negm : s[kb]);
            // the V blocks of all 64 keys (prefetching only keys 0..31 here and the rest under the PV MFMAs saved 16 registers
            // and was 0.5-0.9 % slower once LDS-DMA staging had freed them, profiles/r03/ab_knobs_final_build.log)
            constexpr int PER = (2 * 2 * DB) / (2 * KS);  // V block reads per QK MFMA (1 at D=64)
#pragma unroll
            for (int u = 0; u < PER; ++u) {
              const int m = (kb * KS + ks) * PER + u;
              const int vkb = m / (2 * DB), vst = (m / DB) % 2, vdb = m % DB;
              const lds_char *vb = vptr[vdb] + buf * TILE + (32 * vkb + 16 * vst) * RB;
              vlo[vkb][vst][vdb] = lds_read_tr16(vb);
              vhi[vkb][vst][vdb] = lds_read_tr16(vb + 8 * RB);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else if constexpr (IS_FP8) {
        // e4m3 score product: one scaled MFMA per 32 x 32 block and 64 head-dim elements (unit scales: 2^0)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
          for (int i = 0; i < 16; ++i) s[kb][i] = 0.0f;
#pragma unroll
          for (int j = 0; j < NS8; ++j) {
            const lds_char *kr = Kt + (32 * kb + r) * KRB;
            const u32x4 a = lds_read_b128(kr + (((4 * j + 2 * h) ^ kx8) << 4));
            const u32x4 b = lds_read_b128(kr + (((4 * j + 2 * h + 1) ^ kx8) << 4));
            const i32x8 kf8 = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
            s[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf8, qf8[j], s[kb], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
          }
        }
      } else {
        // head_dim 128: 16 K fragments would cost 64 VGPRs if held live; read each one LA MFMAs ahead of
        // its use instead (profile before: 9 % of wave time stalled on LDS issue, 14 % MFMA/VALU co-execution)
        constexpr int NK = 2 * KS, LA = MLA ? 4 : FA_LAK;  // (MLA mode: the head_dim-128 kernel's look-ahead)
        vec8 kf[NK];
        auto kread = [&](int i) { kf[i] = __builtin_bit_cast(vec8, lds_read_b128(kptr[i % KS] + buf * KTILE + (i / KS) * FA_K32(i % KS))); };
#pragma unroll
        for (int i = 0; i < LA; ++i) kread(i);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 zero;
#pragma unroll
        for (int i = 0; i < 16; ++i) zero[i] = 0.0f;
#pragma unroll
        for (int i = 0; i < NK; ++i) {
          s[i / KS] = M::mfma(kf[i], qf[i % KS], (i % KS) == 0 ? (PRE ? (SOFTCAP ? zero : negm) : zero) : s[i / KS]);
          if (i + LA < NK) kread(i + LA);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ---- mask (only on tiles that cross the diagonal or the end of the sequence)
      // (window mode: or holds keys below the wave's last row's bound)
      const bool need_mask = (CAUSAL && (kv0 + BN - 1 > qw0 + cup)) || (kv0 + BN > FA_NK) || (WINDOW && (kv0 < qw0 + WM - 1 + cl));
      if constexpr (SOFTCAP) {  // t = tanh(x) from y = 2 x log2(e); s holds t from here to the exponential
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int i = 0; i < 16; ++i) s[kb][i] = tanh_from_exp2_arg(s[kb][i]);
      }
      if (need_mask) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          // masked iff key > qrow (kernels.metal:748) or key >= N. A 32 x 32 block whose every key is visible to every
          // row of the wave needs no work (wave-uniform test: of the two blocks of a diagonal tile one is of this
          // kind or entirely masked): key offsets inside the block span 0..31, the wave's rows qw0..qw0+31.
          const int xw = min(FA_NK - 1 - kv0 - 32 * kb, CAUSAL ? qw0 + cup - kv0 - 32 * kb : 0x7fffffff);
          if (xw >= 31 && (!WINDOW || kv0 + 32 * kb >= qw0 + WM - 1 + cl)) continue;
          int lim = FA_NK - 1 - kv0 - 32 * kb - 4 * h;
          if (CAUSAL) lim = min(lim, qrow + cup - kv0 - 32 * kb - 4 * h);
          const int llo = qrow + cl - kv0 - 32 * kb - 4 * h;  // (window mode: masked iff key < qrow + cl as well)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int kpart = (i & 3) + 8 * (i >> 2);
            s[kb][i] = (kpart > lim || (WINDOW && kpart < llo)) ? -INFINITY : s[kb][i];
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
      // ---- online softmax, lane-local + one half swap
      const float mc_old = m * c2;  // (unused with PRE)
      (void)mc_old;
      float ls0 = 0.0f, ls1 = 0.0f;
      // Deferred row max (T13) WITHOUT a per-tile max: P = exp2(c.s - c.m) is formed with the running reference m, and
      // the row sums that are needed anyway tell whether m is stale: a lane whose 32 probabilities add up to more than
      // 2^THR (or to +inf) has a score more than 2^THR above m at worst. Only then -- and on the first tile, where m is
      // -inf -- the wave takes the exact path: recompute the scores (they were overwritten by P; K is still in LDS),
      // take the row max, rescale O and l, form P again. Saves the 16 v_max3 + swap + compare of every tile
      // (141 -> 118 VALU per 16 MFMAs at head_dim 64); m, l and O stay mutually consistent, LSE = m.scale + ln(l) is exact.
      bool exact = (t == tfw);  // this split's first tile (window mode: this wave's first active tile)
      if (t != tfw) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if constexpr (SOFTCAP) {  // capped score t . C against the reference (a masked t is -inf: P = 0)
            s[0][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[0][i], softcap_log2(p), -m));
            s[1][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[1][i], softcap_log2(p), -m));
          } else if constexpr (PRE) {  // the matrix core has already subtracted m
            s[0][i] = __builtin_amdgcn_exp2f(s[0][i]);
            s[1][i] = __builtin_amdgcn_exp2f(s[1][i]);
          } else {
            s[0][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[0][i], c2, -mc_old));
            s[1][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[1][i], c2, -mc_old));
          }
          ls0 = (i == 0) ? s[0][i] : ls0 + s[0][i];  // (0 + x is an instruction: -ffp-contract/-0.0 rules keep it)
          ls1 = (i == 0) ? s[1][i] : ls1 + s[1][i];
        }
        exact = __builtin_amdgcn_ballot_w64(ls0 + ls1 > sum_thr) != 0;  // wave-uniform
        if (exact) recompute_scores(bufc, s, kv0, need_mask);
      }
      if (exact) {
        float mx = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(fmaxf(mx, s[0][i]), s[1][i]);  // -> v_max3_f32
        {
          float lo, hi;
          half_pair(mx, lo, hi);
          mx = fmaxf(lo, hi);
        }
        if constexpr (SOFTCAP) mx *= softcap_log2(p);  // the largest t -> log2 units of the capped scores (C > 0; -inf stays -inf)
        // varlen, causal with Lk < Lq: a row that sees no key at all has every score masked. A finite floor keeps its reference
        // finite (-inf - -inf would be a NaN in alpha and in P): its P and l stay exactly 0 and the epilogue writes O = 0, LSE = -inf.
        // Any row with a visible key has a finite max already, so nothing changes for it.
        // (window mode: the later rows of a wave can have every score of the wave's first active tile below their bound. The same floor:
        // their next tile's sums overflow the threshold and take the exact path, which drops the floor for the true maximum.)
        if constexpr (VARLEN && CAUSAL) mx = fmaxf(mx, -3.4028234663852886e38f);
        // the reference moves to the true maximum and O and l are rescaled to it: the 32-multiply O pass that a per-tile maximum
        // with "rescale whenever a max moved" paid in nearly every tile on random data (profiles/r02/ab_sumtrig.log)
        const float m_new = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * cm);
        l *= alpha;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
        m = m_new;
        if constexpr (PRE && !SOFTCAP) {
#pragma unroll
          for (int i = 0; i < 16; ++i) negm[i] = -m_new;
          asm volatile("" : "+v"(negm));
        }
        const float mc = m * cm;
        ls0 = 0.0f;
        ls1 = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if constexpr (SOFTCAP) {  // (s holds t)
            s[0][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[0][i], softcap_log2(p), -mc));
            s[1][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[1][i], softcap_log2(p), -mc));
          } else {
          s[0][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[0][i], cm, -mc));
          s[1][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[1][i], cm, -mc));
          }
          ls0 += s[0][i];
          ls1 += s[1][i];
        }
      }
      l += ls0 + ls1;
      __builtin_amdgcn_s_setprio(1);
      // ---- O^T += V^T.P^T : per 16-key step, P fragment = 8 accumulator registers
      if constexpr (VPRE) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
          for (int st = 0; st < 2; ++st) {
            vec8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (elem)s[kb][8 * st + j];
#pragma unroll
            for (int db = 0; db < DB; ++db) {
              const s16x8 v8 = __builtin_shufflevector(vlo[kb][st][db], vhi[kb][st][db], 0, 1, 2, 3, 4, 5, 6, 7);
              oacc[db] = M::mfma(__builtin_bit_cast(vec8, v8), pf, oacc[db]);
            }
          }
        }
      } else {
        // V^T fragments just in time, LA MFMAs ahead (step j = (kb, st, db))
        constexpr int NV = 2 * 2 * DB, LA = MLA ? 4 : FA_LAV;
        s16x4 wlo[NV], whi[NV];
        auto vread = [&](int j) {
          const lds_char *vb = vptr[j % DB] + buf * TILE + (32 * (j / (2 * DB)) + 16 * ((j / DB) % 2)) * RB;
          wlo[j] = lds_read_tr16(vb);           // keys +4h+0..3   (k elements 0..3)
          whi[j] = lds_read_tr16(vb + 8 * RB);  // keys +8+4h+0..3 (k elements 4..7)
        };
        vec8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[kb][st][j] = (elem)s[kb][8 * st + j];
#pragma unroll
        for (int j = 0; j < LA; ++j) vread(j);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const s16x8 v8 = __builtin_shufflevector(wlo[j], whi[j], 0, 1, 2, 3, 4, 5, 6, 7);
          oacc[j % DB] = M::mfma(__builtin_bit_cast(vec8, v8), pf[j / (2 * DB)][(j / DB) % 2], oacc[j % DB]);
          if (j + LA < NV) vread(j + LA);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (t + SPLIT < nT) {
      if constexpr (DMA) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pieces issued at the top of this tile have landed
      } else {
        stage_write(buf ^ 1);
        if constexpr (DMA_K8) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();
  };
  const int steps = (nT - tb + SPLIT - 1) / SPLIT;  // every wave runs the same number of steps (one barrier each)
  for (int j = 0; j < steps; j += 2) {
    tile(std::integral_constant<int, 0>{}, tb + j * SPLIT + sp);
    if (j + 1 < steps) tile(std::integral_constant<int, 1>{}, tb + (j + 1) * SPLIT + sp);
  }

  if constexpr (SPLIT == 2) {
    // ---- merge the two splits: waves 4-7 publish (O^T, m, l) lane by lane, waves 0-3 fold them into their own by the
    // reference maxima (a split that saw no tile has m = -inf, l = 0: weight 0). The buffer sits behind the epilogue's
    // O tiles; the K/V buffers are free (last step's barrier).
    constexpr int NACC = 16 * DB;
    float *mb = (float *)((lds_char *)smem_generic + RW * WM * RB) + (size_t)wave * (NACC + 2) * 64 + lane;
    if (sp == 1) {
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) mb[(16 * db + i) * 64] = oacc[db][i];
      mb[NACC * 64] = m;
      mb[(NACC + 1) * 64] = l;
    }
    __syncthreads();
    if (sp == 0) {
      const float m1 = mb[NACC * 64], l1 = mb[(NACC + 1) * 64];
      const float mm = fmaxf(m, m1);  // split 0 owns tile 0: m is finite
      const float a0 = __builtin_amdgcn_exp2f((m - mm) * cm), a1 = __builtin_amdgcn_exp2f((m1 - mm) * cm);
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[db][i] = oacc[db][i] * a0 + mb[(16 * db + i) * 64] * a1;
      l = l * a0 + l1 * a1;
      m = mm;
    }
  }

  // ---- epilogue: normalise, LSE, O tile -> LDS -> coalesced 16-byte stores (split2: waves 0-3 only; the others keep
  // the barrier company)
  if constexpr (KSPLIT) {
    // key-split mode: the normalised state of this wave's owned rows goes to the workspace, straight from the registers (lane (r, h) holds
    // d columns 32 db + 8 g4 + 4 h + 0..3 of row r: 16-byte stores, a lane pair fills a 32-byte sector). o_s and lse2_s are the
    // expressions of the epilogue below -- oacc . (1 / l), and m with the logarithm of l, here base 2 -- so a split that holds all the
    // visible keys of a row hands the combine exactly what that epilogue rounds.
    {
      float lo, hi;
      half_pair(l, lo, hi);
      l = lo + hi;
    }
    const float inv_l = 1.0f / l;
    // The f16 epilogue below rounds the EXACT product oacc . (1 / l) to f16 once (hipcc fuses the multiply into v_fma_mixlo_f16); the
    // bf16 one rounds the fp32 product. o_s carries what that rounding sees: bf16, the fp32 product; f16, the product rounded to ODD in
    // fp32 (the residual of the product by one fma; inexact: truncate, set the last bit), from which the combine's one rounding to f16
    // gives the bits of rounding the exact product -- 24 bits are two more than f16 needs for that. One ulp of fp32 instead of a half.
    auto o_of = [&](float a) __attribute__((always_inline)) {
      float pr = a * inv_l;
      if constexpr (std::is_same<Tag, F16>::value) {
        const float res = __builtin_fmaf(a, inv_l, -pr);
        unsigned u = __builtin_bit_cast(unsigned, pr);
        if (res != 0.0f) u = (((res < 0.0f) != (pr < 0.0f)) ? u - 1u : u) | 1u;
        pr = __builtin_bit_cast(float, u);
      }
      return pr;
    };
    if (qrow < LQ) {
      typedef float f32x4 __attribute__((ext_vector_type(4)));
      float *wo = ksplit_o<D>(p, (int)blockIdx.y, lse_base + qrow) + 4 * h;
      if (h == 0) *ksplit_lse2<D>(p, (int)blockIdx.y, lse_base + qrow) = m + __builtin_log2f(l);
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
          *reinterpret_cast<f32x4 *>(wo + 32 * db + 8 * g4) = f32x4{o_of(oacc[db][4 * g4 + 0]), o_of(oacc[db][4 * g4 + 1]),
                                                                   o_of(oacc[db][4 * g4 + 2]), o_of(oacc[db][4 * g4 + 3])};
    }
    return;
  }
  lds_char *Ot = (lds_char *)smem_generic + wave * (WM * RB);  // this wave's [32][D] tile (inside the K buffers)
  if (sp == 0) {
    {
      float lo, hi;
      half_pair(l, lo, hi);
      l = lo + hi;
    }
    // varlen: a row with no visible key (causal with Lk < Lq; an integer test, the object is built without NaN handling)
    // (coff through an opaque copy: hipcc otherwise keeps the loop's qrow + coff alive for this one test -- a spill at 128 registers)
    bool no_key = false;
    if constexpr (VARLEN && CAUSAL) {
      int coff_e = cup;
      asm volatile("" : "+s"(coff_e));
      no_key = qrow + coff_e < 0;
    }
    // sink mode: the row's softmax gets the term 2^s2, s2 = sink . log2(e), against the reference mm = max(m, s2): l' = l 2^(m - mm) +
    // 2^(s2 - mm) and O = oacc . 2^(m - mm) / l'. Neither exponent is positive, so nothing overflows whichever side is far larger; a sink
    // whose 2^(s2 - m) underflows leaves mm = m, a factor of exactly 1 and l' = l + 0: the bits of the call without sinks.
    float o_w = 1.0f;  // the factor 2^(m - mm) on O
    if constexpr (SINK) {
      const float s2 = sink * 1.4426950408889634f;
      const float mm = fmaxf(m, s2);
      o_w = __builtin_amdgcn_exp2f(m - mm);
      l = l * o_w + __builtin_amdgcn_exp2f(s2 - mm);
      m = mm;
    }
    const float inv_l = (VARLEN && CAUSAL) ? (no_key ? 0.0f : (SINK ? o_w * (1.0f / l) : 1.0f / l)) : 1.0f / l;
    if constexpr (VARLEN) {
      if (p.lse != nullptr && h == 0 && qrow < LQ)
        p.lse[lse_base + qrow] = no_key ? (SINK ? sink : -INFINITY) : m * 0.6931471805599453f + logf(l);
    } else {
    if (p.lse != nullptr && h == 0 && qrow < p.N)
      p.lse[(long long)bh * p.N + qrow] = m * (PRE ? 0.6931471805599453f : p.scale) + logf(l);
    }
#pragma unroll
    for (int db = 0; db < DB; ++db) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        // registers 4g4..4g4+3 = d columns 32db + 8g4 + 4h + 0..3 of row r
        elem e0 = (elem)(oacc[db][4 * g4 + 0] * inv_l), e1 = (elem)(oacc[db][4 * g4 + 1] * inv_l);
        elem e2 = (elem)(oacc[db][4 * g4 + 2] * inv_l), e3 = (elem)(oacc[db][4 * g4 + 3] * inv_l);
        u32x2 w;
        w[0] = (unsigned)__builtin_bit_cast(unsigned short, e0) | ((unsigned)__builtin_bit_cast(unsigned short, e1) << 16);
        w[1] = (unsigned)__builtin_bit_cast(unsigned short, e2) | ((unsigned)__builtin_bit_cast(unsigned short, e3) << 16);
        // 16-byte chunk index XOR (r & (CPR-1)) spreads the rows over the banks
        const int col_b = (32 * db + 8 * g4 + 4 * h) * 2;
        const int ch = (col_b >> 4) ^ (r & (CPRL - 1));
        lds_write_b64(Ot + r * RB + (ch << 4) + (col_b & 15), w);
      }
    }
  }
  __syncthreads();
  if (sp == 0) {
    elem *Og = (elem *)p.o + (MLA ? base_o : base);
#pragma unroll
    for (int it = 0; it < WM * CPR / 64; ++it) {
      const int idx = it * 64 + lane;
      const int row = idx / CPR, ch = idx % CPR;
      const u32x4 vv = lds_read_b128(Ot + row * RB + ((ch ^ (row & (CPRL - 1))) << 4));
      if (qw0 + row < FA_NQ)
        *reinterpret_cast<u32x4 *>(Og + (VARLEN ? (long long)(qw0 + row) * (long long)((MLA ? orb : qrb) / 2) : (long long)(qw0 + row) * D) + ch * 8) = vv;
    }
  }
}

#undef FA_NQ
#undef FA_NK
#undef FA_K32

template <typename Tag, int D, bool CAUSAL, bool PRESC>
__global__ __launch_bounds__(NTHREADS, (main_kernel_occ4<Tag, D, PRESC>() ? 4 : D <= 64 ? 3 : D <= 128 ? 2 : 1)) void fwd_mfma_kernel(Params p) {
  fwd_mfma_body<Tag, D, CAUSAL, 1, PRESC>(p);
}

template <typename Tag, int D, bool CAUSAL>
__global__ __launch_bounds__(2 * NTHREADS, 2) void fwd_mfma_split2_kernel(Params p) {
  fwd_mfma_body<Tag, D, CAUSAL, 2, true>(p);
}

template <typename Tag, int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, 2) void fwd_mfma_h64s2_kernel(Params p) {
  fwd_mfma_body<Tag, D, CAUSAL, 2, true, 64>(p);
}

// fa_fwd_varlen: the plain kernel (pre-scaled operand) in varlen mode, at the plain kernel's occupancy (head_dim 64 without the mask:
// three workgroups per CU, see MAIN4)
template <typename Tag, int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, ((main_kernel_occ4<Tag, D, true>() && CAUSAL) ? 4 : D <= 64 ? 3 : 2)) void fwd_mfma_varlen_kernel(VarlenParams p) {
  fwd_mfma_body<Tag, D, CAUSAL, 1, true, BM, VarlenParams>(p);
}

// fa_fwd_varlen_paged: the same kernel in varlen paged mode. The page walk lives in SGPRs: the varlen kernels' occupancy is declared.
template <int D, bool CAUSAL>
constexpr int varlen_paged_occupancy() {
  return D <= 64 ? (CAUSAL ? 4 : 3) : 2;
}
template <typename Tag, int D, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, (varlen_paged_occupancy<D, CAUSAL>())) void fwd_mfma_varlen_paged_kernel(VarlenPagedParams p) {
  fwd_mfma_body<Tag, D, CAUSAL, 1, true, BM, VarlenPagedParams>(p);
}

// fa_fwd_varlen_window / fa_fwd_varlen_paged_window: the two varlen modes in window mode, at the occupancy of the unmasked varlen kernels
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_window_kernel(VarlenWindowParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenWindowParams>(p);
}
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_window_paged_kernel(VarlenPagedWindowParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenPagedWindowParams>(p);
}

// fa_fwd_varlen_sink / fa_fwd_varlen_paged_sink: the two window kernels in sink mode, at their occupancy
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_sink_kernel(VarlenSinkParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenSinkParams>(p);
}
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_sink_paged_kernel(VarlenPagedSinkParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenPagedSinkParams>(p);
}

// fa_fwd_varlen_softcap / fa_fwd_varlen_paged_softcap: the two window kernels in softcap mode, at their occupancy
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_softcap_kernel(VarlenSoftcapParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenSoftcapParams>(p);
}
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_softcap_paged_kernel(VarlenPagedSoftcapParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenPagedSoftcapParams>(p);
}

// fa_fwd_varlen_paged_kv8: the paged window / sink kernels in KV8 mode (bf16 queries, e4m3 pools), at their occupancy: the 8 / 16 staging
// registers fit (168 / 222 VGPR, no scratch)
template <int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_kv8_kernel(VarlenPagedKv8Params p) {
  fwd_mfma_body<BF16, D, true, 1, true, BM, VarlenPagedKv8Params>(p);
}
template <int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_kv8_sink_kernel(VarlenPagedKv8SinkParams p) {
  fwd_mfma_body<BF16, D, true, 1, true, BM, VarlenPagedKv8SinkParams>(p);
}

// fa_fwd_varlen_paged_split (S >= 2): the paged window kernel in key-split mode, at its occupancy; grid = the block map x S
template <typename Tag, int D>
__global__ __launch_bounds__(NTHREADS, (D <= 64 ? 3 : 2)) void fwd_mfma_ksplit_paged_kernel(VarlenPagedKsplitParams p) {
  fwd_mfma_body<Tag, D, true, 1, true, BM, VarlenPagedKsplitParams>(p);
}

// fa_fwd_varlen_mla: the varlen kernel in MLA mode, (192, 128). 80 KiB of LDS: two workgroups fill a CU's 160 KiB, and the registers
// are declared for two.
template <typename Tag, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, 2) void fwd_mfma_mla_kernel(VarlenMlaParams p) {
  fwd_mfma_body<Tag, 192, CAUSAL, 1, true, BM, VarlenMlaParams, 128>(p);
}

// ... and its second launch, on the partial's own block map (one workgroup per (sequence, head, 128 rows), the same cu_seqlens_q lookup
// and clamps: what the partials wrote is what is read, and only owned tokens of O / LSE are written). Thread t takes 8 d columns of rows
// t / (D / 8), + 256 / (D / 8), ... of the block. Per row, over the splits in order (no atomics: bitwise reproducible):
//   M = max_s lse2_s;  w_s = 2^(lse2_s - M);  W = sum_s w_s;  O = (sum_s w_s o_s) (1 / W);  LSE = (M + log2 W) ln 2.
// A split with lse2_s = -inf is SKIPPED, its o_s never loaded (stale workspace, or the 0 . inf of a row without a key in the split). The
// sums start from -0, the one value x + (-0) = x holds for bit for bit: a row whose keys all lie in one split has w = 1, W = 1 and comes
// out as o_s rounded to the type once -- the un-split kernel's bits. M = -inf (no split saw a key): O = 0 exactly, LSE = -inf.
// SINK (sinks != nullptr at launch): decode_combine_sink_kernel's merge behind the reduction: s2 = sink . log2(e), Mm = max(M, s2),
// W' = W 2^(M - Mm) + 2^(s2 - Mm), O = acc 2^(M - Mm) / W', LSE = (Mm + log2 W') ln 2. Neither exponent is positive; a sink whose term
// underflows leaves Mm = M, a factor of exactly 1 and W' = W + 0; a dead row gets LSE = sinks[h] bit for bit.
template <typename Tag, int D, bool SINK>
__global__ __launch_bounds__(NTHREADS) void ksplit_combine_kernel(VarlenPagedKsplitParams p) {
  using elem = typename MT<Tag>::elem;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  constexpr int CPR = D / 8, RPP = NTHREADS / CPR;  // 16-byte output chunks per row, rows per pass
  int bh, qb;
  map_block<true>(blockIdx.x, p, bh, qb);
  const int b = (int)fdiv((unsigned)bh, p.fd_h), hq = bh - b * p.H;
  const int sq = min(max(p.cu_q[b], 0), p.total_q), eq = min(max(p.cu_q[b + 1], 0), p.total_q);
  const int LQ = min(max(eq - sq, 0), p.N);
  const long long lse_base = (long long)hq * p.total_q + sq;
  const long long rows = (long long)p.H * p.total_q;
  const float *wl = ksplit_lse2<D>(p, 0, 0);
  const float *wo = ksplit_o<D>(p, 0, 0);
  const int S = p.S, ch = (int)threadIdx.x % CPR;
  float sink = 0.0f;
  if constexpr (SINK) sink = p.sinks[hq];
  elem *Og = (elem *)p.o + (long long)sq * p.q_rs + (long long)hq * p.head_stride;
  for (int row = qb * BM + (int)threadIdx.x / CPR; row < min(LQ, qb * BM + BM); row += RPP) {
    const float *rl = wl + lse_base + row;
    // eight splits' loads in flight at a time (one dependent read per split made the decode's combine cost more than its partial kernel)
    float M = -INFINITY;
    for (int s0 = 0; s0 < S; s0 += 8) {
      float l2[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) l2[u] = s0 + u < S ? rl[(long long)(s0 + u) * rows] : -INFINITY;
#pragma unroll
      for (int u = 0; u < 8; ++u) M = fmaxf(M, l2[u]);
    }
    float W = -0.0f, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = -0.0f;
    for (int s0 = 0; s0 < S; s0 += 8) {
      float l2[8];
      f32x4 x0[8], x1[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) l2[u] = s0 + u < S ? rl[(long long)(s0 + u) * rows] : -INFINITY;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        x0[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        x1[u] = x0[u];
        if (l2[u] != -INFINITY) {  // a split without a key for this row is selected away: never loaded, never multiplied
          const float *ro = wo + ((long long)(s0 + u) * rows + lse_base + row) * D + ch * 8;
          x0[u] = *reinterpret_cast<const f32x4 *>(ro);
          x1[u] = *reinterpret_cast<const f32x4 *>(ro + 4);
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {  // in split order
        if (l2[u] == -INFINITY) continue;
        const float w = __builtin_amdgcn_exp2f(l2[u] - M);
        W += w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i] += w * x0[u][i];
          acc[4 + i] += w * x1[u][i];
        }
      }
    }
    const bool dead = M == -INFINITY;
    float inv, lse;
    if constexpr (SINK) {
      const float s2 = sink * 1.4426950408889634f;
      const float Mm = dead ? s2 : fmaxf(M, s2);
      const float ow = dead ? 0.0f : __builtin_amdgcn_exp2f(M - Mm);
      const float Wt = (dead ? 0.0f : W * ow) + __builtin_amdgcn_exp2f(s2 - Mm);
      inv = ow * (1.0f / Wt);
      lse = dead ? sink : (Mm + __builtin_log2f(Wt)) * 0.6931471805599453f;
    } else {
      inv = dead ? 0.0f : 1.0f / W;
      lse = dead ? -INFINITY : (M + __builtin_log2f(W)) * 0.6931471805599453f;
    }
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const elem e0 = dead ? (elem)0.0f : (elem)(acc[2 * i] * inv), e1 = dead ? (elem)0.0f : (elem)(acc[2 * i + 1] * inv);
      out[i] = (unsigned)__builtin_bit_cast(unsigned short, e0) | ((unsigned)__builtin_bit_cast(unsigned short, e1) << 16);
    }
    *reinterpret_cast<u32x4 *>(Og + (long long)row * p.q_rs + ch * 8) = out;
    if (p.lse != nullptr && ch == 0) p.lse[lse_base + row] = lse;
  }
}

// ---------------------------------------------------------------------------
bool mfma_supported(int dtype, int D) {
  if (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) return D == 32 || D == 64 || D == 96 || D == 128 || D == 256;
  return dtype == FA_DTYPE_FP8_E4M3 && (D == 64 || D == 128 || D == 256);  // an fp8 row must fill whole 16-byte chunks per thread
}

// Every launcher below: launch_blocks (fa_mfma_common.h) with the kernel, its block height and threads, mfma_lds_bytes and a head group.
template <typename Tag, int D, bool CAUSAL, bool PRESC>
static hipError_t launch_one_(const Params &p, hipStream_t s) {
  int head_group = causal_head_group(p, D, std::is_same<Tag, FP8>::value ? 1 : 2);
#ifdef FA_DEBUG_KNOBS  // scheduling experiments only: never compiled into the shipped library
  static const int env_head_group = [] { const char *e = getenv("FA_HEAD_GROUP"); return e ? atoi(e) : -1; }();
  if (env_head_group >= 0) head_group = env_head_group;
#ifdef FA_FORCE_HEAD_GROUP  // compile-time form for tools/ab.py (several builds side by side in one process share the environment)
  head_group = FA_FORCE_HEAD_GROUP;
#endif
#endif
  return launch_blocks(fwd_mfma_kernel<Tag, D, CAUSAL, PRESC>, p, BM, NTHREADS, mfma_lds_bytes<Tag, D>(), head_group, s);
}

// p.exact (variant mfma_exact) selects the instantiation without the pre-scaled operand; where the pre-scaling does not
// exist (fp8, head_dim 256) there is only that one.
template <typename Tag, int D, bool CAUSAL>
static hipError_t launch_one(const Params &p, hipStream_t s) {
  if constexpr (prescale_applies<Tag, D>()) {
    if (!p.exact) return launch_one_<Tag, D, CAUSAL, true>(p, s);
  }
  return launch_one_<Tag, D, CAUSAL, false>(p, s);
}

// The varlen modes: one block per (sequence, head, 128 rows up to max_seqlen_q) -- the host does not know the lengths; blocks past the
// end of their sequence return at once. p.N / p.Nk hold max_seqlen_q / max_seqlen_k (varlen paged: the capacity): the issue order
// (map_block) and the causal head groups are those of a dense batch of B sequences of these lengths. Window mode takes the causal
// order: heaviest-first is harmless where the blocks weigh the same.
template <typename Tag, int D, typename PT, typename K>
static hipError_t launch_varlen_one(K kern, const PT &p, hipStream_t s) {
  return launch_blocks(kern, p, BM, NTHREADS, mfma_lds_bytes<Tag, D>(), causal_head_group(p, D, 2), s);
}

bool mfma_varlen_supported(int dtype, int D) { return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && (D == 64 || D == 128); }

hipError_t launch_mfma_varlen(const VarlenParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim_causal<64, 128>(p.D, p.is_causal, [&](auto d, auto c) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_varlen_kernel<decltype(tag), d(), c()>, p, s); });
  });
}

bool mfma_varlen_mla_supported(int dtype, int Dqk, int Dv) { return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && Dqk == 192 && Dv == 128; }

// (causal_head_group sized by the mean of the K and V row: the issue order only, never the results)
hipError_t launch_mfma_varlen_mla(const VarlenMlaParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    constexpr size_t lds = mfma_lds_bytes<Tag, 192, 1, BM, 128>();
    const int hg = causal_head_group(p, 160, 2);
    if (p.is_causal) return launch_blocks(fwd_mfma_mla_kernel<Tag, true>, p, BM, NTHREADS, lds, hg, s);
    return launch_blocks(fwd_mfma_mla_kernel<Tag, false>, p, BM, NTHREADS, lds, hg, s);
  });
}

bool mfma_varlen_paged_supported(int dtype, int D, int page_size) { return mfma_varlen_supported(dtype, D) && page_size_ok(page_size); }

hipError_t launch_mfma_varlen_paged(const VarlenPagedParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim_causal<64, 128>(p.D, p.is_causal, [&](auto d, auto c) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_varlen_paged_kernel<decltype(tag), d(), c()>, p, s); });
  });
}

hipError_t launch_mfma_varlen_window(const VarlenWindowParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_window_kernel<decltype(tag), d()>, p, s); });
  });
}

hipError_t launch_mfma_varlen_paged_window(const VarlenPagedWindowParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_window_paged_kernel<decltype(tag), d()>, p, s); });
  });
}

hipError_t launch_mfma_varlen_sink(const VarlenSinkParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_sink_kernel<decltype(tag), d()>, p, s); });
  });
}

hipError_t launch_mfma_varlen_paged_sink(const VarlenPagedSinkParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_sink_paged_kernel<decltype(tag), d()>, p, s); });
  });
}

hipError_t launch_mfma_varlen_softcap(const VarlenSoftcapParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_softcap_kernel<decltype(tag), d()>, p, s); });
  });
}

hipError_t launch_mfma_varlen_paged_softcap(const VarlenPagedSoftcapParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) { return launch_varlen_one<decltype(tag), d()>(fwd_mfma_softcap_paged_kernel<decltype(tag), d()>, p, s); });
  });
}

bool mfma_varlen_paged_kv8_supported(int q_dtype, int kv_dtype, int D, int page_size) {
  return q_dtype == FA_DTYPE_BF16 && kv_dtype == FA_DTYPE_FP8_E4M3 && (D == 64 || D == 128) && page_size_ok(page_size);
}

// (causal_head_group sized for rows of one byte: the issue order only, never the results)
hipError_t launch_mfma_varlen_paged_kv8(const VarlenPagedSinkParams &p, bool with_sink, hipStream_t s) {
  return with_dim<64, 128>(p.D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    const int hg = causal_head_group(p, D, 1);
    if (with_sink) {
      VarlenPagedKv8SinkParams pk;
      static_cast<VarlenPagedSinkParams &>(pk) = p;
      return launch_blocks(fwd_mfma_kv8_sink_kernel<D>, pk, BM, NTHREADS, mfma_lds_bytes<BF16, D>(), hg, s);
    }
    VarlenPagedKv8Params pk;
    static_cast<VarlenPagedWindowParams &>(pk) = p;
    return launch_blocks(fwd_mfma_kv8_kernel<D>, pk, BM, NTHREADS, mfma_lds_bytes<BF16, D>(), hg, s);
  });
}

// Splits per 128-row block of fa_fwd_varlen_paged_split: the smallest count with blocks * S >= FA_KSPLIT_SLOTS, but so that a split of a
// block that spans the whole capacity keeps FA_KSPLIT_MIN_TILES 64-key tiles -- a split pays the block's prologue (Q fragments, pre-scale,
// first tile's latency) and 128 (D + 1) floats of workspace traffic.
// FA_KSPLIT_SLOTS = 256 CUs x 2 workgroups at BOTH head dims. The head_dim 64 kernels run three per CU, and 768 was the first value; measured
// on the tool's whole head_dim 64 grid (profiles/r22/bench_varlen_paged_split_d64.log): with 512 blocks (16 x 8 heads x 4, 4 x 32 x 4,
// 16 x 32 x 1) 768 asks for S = 2, i.e. 1024 half-length workgroups in two rounds where the un-split call needs one: 1.09 to 1.24 of its
// time; and one sequence of 8 heads x 512 queries got S = 24 where 8 to 16 is best (1.5 at 8k keys, 1.11 at 32k). With 512 no shape of that
// grid is slower than the un-split call and the worst distance to the best S measured is 1.17.
// FA_KSPLIT_MIN_TILES = 4, the decode's: it binds at 8k keys and a chunk of 8 only (S = 32 where 16 is best, within 3 %); 8 gives the same
// choices on that grid, 16 is worse (S = 8 at 8k keys: 1.25 of the best).
#ifndef FA_KSPLIT_SLOTS
#define FA_KSPLIT_SLOTS 512
#endif
#ifndef FA_KSPLIT_MIN_TILES
#define FA_KSPLIT_MIN_TILES 4
#endif
int varlen_paged_ksplit_splits(int B, int Hq, int max_seqlen_q, int D, int page_size, int max_pages_per_seq) {
  const long long blocks = (long long)B * Hq * (((long long)max_seqlen_q + BM - 1) / BM), slots = FA_KSPLIT_SLOTS;
  (void)D;
  const long long cap_tiles = ((long long)page_size * max_pages_per_seq + BN - 1) / BN;
  long long S = (slots + blocks - 1) / blocks;
  S = std::min<long long>(S, std::max<long long>(1, cap_tiles / FA_KSPLIT_MIN_TILES));
  return (int)std::max<long long>(1, std::min<long long>(S, FA_VARLEN_PAGED_MAX_SPLITS));
}

// the pair of launches on one stream: partials on the block map x S (blockIdx.y = the split), then the combine on the block map
hipError_t launch_mfma_varlen_paged_ksplit(const VarlenPagedKsplitParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim<64, 128>(p.D, [&](auto d) {
      using Tag = decltype(tag);
      constexpr int D = decltype(d)::value;
      const int hg = causal_head_group(p, D, 2);
      hipError_t e = launch_blocks(fwd_mfma_ksplit_paged_kernel<Tag, D>, p, BM, NTHREADS, mfma_lds_bytes<Tag, D>(), hg, s, 0, p.S);
      if (e != hipSuccess) return e;
      if (p.sinks != nullptr) return launch_blocks(ksplit_combine_kernel<Tag, D, true>, p, BM, NTHREADS, 0, hg, s);
      return launch_blocks(ksplit_combine_kernel<Tag, D, false>, p, BM, NTHREADS, 0, hg, s);
    });
  });
}

bool mfma_h64s2_supported(int dtype, int D) { return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && D == 64; }

// (the two split forms: one global head group)
hipError_t launch_mfma_h64s2(const Params &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    return with_dim_causal<64>(p.D, p.is_causal, [&](auto d, auto c) {
      return launch_blocks(fwd_mfma_h64s2_kernel<decltype(tag), d(), c()>, p, 64, NTHREADS, mfma_lds_bytes<decltype(tag), d(), 2, 64>(), 0, s);
    });
  });
}

bool mfma_split2_supported(int dtype, int D) {
  return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16 || dtype == FA_DTYPE_FP8_E4M3) && (D == 64 || D == 128);
}

hipError_t launch_mfma_split2(const Params &p, int dtype, hipStream_t s) {
  auto go = [&](auto tag) {
    return with_dim_causal<64, 128>(p.D, p.is_causal, [&](auto d, auto c) {
      return launch_blocks(fwd_mfma_split2_kernel<decltype(tag), d(), c()>, p, BM, 2 * NTHREADS, mfma_lds_bytes<decltype(tag), d(), 2>(), 0, s);
    });
  };
  return dtype == FA_DTYPE_FP8_E4M3 ? go(FP8{}) : with_tag(dtype, go);
}

template <typename Tag, int... Ds>
static hipError_t launch_dt(const Params &p, hipStream_t s) {
  return with_dim_causal<Ds...>(p.D, p.is_causal, [&](auto d, auto c) { return launch_one<Tag, d(), c()>(p, s); });
}

hipError_t launch_mfma(const Params &p, int dtype, hipStream_t s) {
  if (dtype == FA_DTYPE_FP8_E4M3) return launch_dt<FP8, 64, 128, 256>(p, s);  // (an fp8 row of head_dim 32 / 96 has no kernel)
  return dtype == FA_DTYPE_F16 ? launch_dt<F16, 32, 64, 96, 128, 256>(p, s) : launch_dt<BF16, 32, 64, 96, 128, 256>(p, s);
}

}  // namespace fa
