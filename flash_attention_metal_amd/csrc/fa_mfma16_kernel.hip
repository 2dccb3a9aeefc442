// fa_mfma16_kernel.hip -- the operator on v_mfma_f32_16x16x32_{bf16,f16} (variant "mfma16").
//
// Same math and the same workgroup shape as fa_mfma_kernel.hip (replaces /root/reference/kernels.metal:600-883: tiled
// QK^T -> online softmax -> PV, causal predicate `key > query -> masked` kernels.metal:748, L = m + ln(l)
// kernels.metal:862-864), but every matrix product runs on the 16x16x32 instruction instead of 32x32x16. Why a second
// kernel for the same work: on random data the chip is power-limited under these loops and holds a higher clock on
// the 16x16x32 shape (MI355X_MICROARCH.md, DVFS give-back item 7: 1.12-1.15x the FLOP/s of the 32x32x16 loop at equal
// cycles per FLOP; cdna_hip_programming.md rule 28) -- so cycles per FLOP do not decide which is faster, wall does.
//
// Structure (one workgroup = 4 waves = 128 query rows of one (batch, head); a wave owns 32 rows = TWO 16-row query tiles,
// so every K / V^T fragment read from LDS still feeds two MFMAs -- LDS traffic per FLOP equals the 32x32x16 kernel's):
//   * S^T = K.Q^T per 16 keys x 16 queries ("swapped" product): lane (c = lane & 15, g = lane >> 4) holds the scores of
//     query c of each query tile against keys 16kt + 4g + i (i = register) -- a lane serves TWO query rows, 16 scores each
//     per 64-key tile; row max / row sum are in-register reductions, the four lanes of a row (g = 0..3) meet only on the
//     rare exact path and in the epilogue
//   * pre-scaled query operand Q~ = round(scale.log2e.Q) and the running reference -m as the C operand of the first MFMA
//     of every score chain (4 registers per query tile instead of 16): P = exp2(S') with no FMA. f16: the packed probabilities'
//     exponent bits decide per tile whether m is stale (threshold 2^4; bf16 at head_dim 128: 2^8), and a stale tile is done again on the
//     true maxima. bf16 at head_dim 64 and its padded head dims (LAZY):
//     no per-tile test -- bf16 P' keeps its 8 bits at any scale, so a stale m loses nothing; the row sums the matrix core delivers are
//     looked at inside the NEXT tile's PV product (one compare in an MFMA gap, the verdict scalar), a sum of 2^20 and more takes an exact
//     power of two out of O, the sum and m behind that product, and a sum that left the trusted range (2^64 and more, inf, NaN) makes the
//     workgroup run once more on the exact path (slow mode)
//   * P^T feeds PV straight from the score registers: the B operand's k index (8g + j) is key 16(j >> 2) + 4g + (j & 3) of a
//     32-key step, and V^T is read with ds_read_b64_tr_b16 in the same order (V stays row-major in HBM and LDS)
//   * K/V tiles of 64 keys double-buffered in LDS, global -> LDS by LDS-DMA with the chunk swizzle on the source address;
//     one barrier per tile; images: K chunk ^ ((row >> 1) & 7), V chunk ^ (((row >> 1) & 3) << 1) at head_dim 64 (both
//     conflict-free for these reads: checked on the CPU by tests/test_lds_images.py)
//   * epilogue: O tile -> LDS -> whole rows, 16 B per lane; LSE = m.ln2 + ln(l)
#include <stdlib.h>

#include <algorithm>

#include "fa_mfma_common.h"

#ifndef FA16_DEFER_THR
#define FA16_DEFER_THR 8.0f  // log2 units: P <= 2^8 between rescales
#endif
#ifndef FA16_LAK
#define FA16_LAK (D == 128 ? 3 : 2)  // K fragments are read this many fragments (each feeds two MFMAs) ahead of their use (head_dim 128: 3,
                                    // config 4 +1.5 % over 2, profiles/r04/ab_mfma16_d128_knobs.log)
#endif
#ifndef FA16_LAV
#define FA16_LAV (D == 128 ? 3 : 2)  // ... and V^T fragments
#endif
#ifndef FA16_PRIO
#define FA16_PRIO 1  // 1: wave priority raised around the MFMA clusters
#endif
#ifndef FA16_ONES
#define FA16_ONES 1  // 1: the row sums come out of the matrix core (a fifth "d tile" of ones in the PV product: +4 MFMAs per 64-key tile) and
                     // the staleness test reads the exponent bits of the packed probabilities (8 v_or3 instead of 32 v_add): the loop is
                     // VALU-issue-bound with the matrix pipe half idle, so VALU is traded for MFMA; 0: row sums by v_add, tested against 2^THR
#endif
#ifndef FA16_LAZY
#define FA16_LAZY 1  // bf16 at head_dim 64 with FA16_ONES: 1 = the reference is renewed lazily from the row sums of the PREVIOUS tile (see tile()); 0 = the per-tile
                     // test of the packed exponent bits, as f16; 2 = no test at all (TIMING ONLY, the ceiling of 1: wrong for rows that rise)
#endif
#ifndef FA16_LAZY_THR
#define FA16_LAZY_THR 0x1p20f  // LAZY: a row whose sum reached this is renormalised by an exact power of two behind the PV product of the tile that looks at it
#endif
#ifndef FA16_LAZY_POISON
#define FA16_LAZY_POISON 0x1p64f  // LAZY: a row sum at or above this (inf and NaN included) is not trusted: the block runs again in slow mode
#endif
#ifndef FA16_LOOK
#define FA16_LOOK 1  // LAZY, where the row sums are looked at: 1 = in the PV product, behind its first MFMAs (the sums have no pending writer there),
                     // the repair behind the product's last MFMA; 0 = in front of the tile, directly behind the barrier (round 11's form: a VALU
                     // read of the youngest matrix results and a branch on it in front of the score MFMAs); 3 = nowhere (TIMING ONLY)
#endif
#ifndef FA16_COLD
#define FA16_COLD 3  // LAZY, what parts the code behind the score MFMAs: 3 = the mask's branch alone, on a scalar sign bit -- slow mode enters the exact
                     // path at the head of the tile, through the redo flag; 0 = slow mode's exit and the mask's branch one behind the other, the
                     // mask flag through a VGPR (round 11's form); 2 = 0 without the slow-mode exit (TIMING ONLY)
#endif
#ifndef FA16_TAIL
#define FA16_TAIL 1  // LAZY: 1 = the block's last barrier and the test of the last tile's sums in front of it stand behind the tile loop; 0 = inside
                     // the last unit, on a condition every tile's tail evaluates (round 11's form)
#endif
#ifndef FA16_HALVES
#define FA16_HALVES 0  // 1: the hot pass works on one 32-key half at a time (16 live score registers instead of 32)
#endif
#ifndef FA16_BN128
#define FA16_BN128 64  // keys per staged tile of the head_dim-128 instantiation (64: 64 KiB of LDS, two workgroups per CU; 32: 32 KiB)
#endif
#ifndef FA16_OCC128
#define FA16_OCC128 2  // workgroups per CU the head_dim-128 kernel is compiled for (2: 256 registers, 3: 168)
#endif
#ifndef FA16_SUB8
#define FA16_SUB8 1  // tiles per staged unit (barrier) of the eight-wave head_dim-64 instantiation: 1, or 2 (64 KiB of LDS)
#endif
#ifndef FA16_OCC
#define FA16_OCC 4  // workgroups per CU the head_dim-64 kernel is compiled for (128 registers)
#endif

namespace fa {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename Tag> struct MT16;
template <> struct MT16<BF16> {
  using elem = __bf16;
  using vec8 = bf16x8;
  __device__ static __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MT16<F16> {
  using elem = _Float16;
  using vec8 = f16x8;
  __device__ static __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// value of lane ^ 16 / lane ^ 32 (rare path and epilogue only: ds_bpermute, no LDS memory)
__device__ __forceinline__ float xlane(float x, int mask) { return __shfl_xor(x, mask, 64); }

// PAD: head dims other than 64 / 128 (any multiple of 8 below 128 that has no kernel of its own: 40, 48, 72, 80, 112, ...) run this
// instantiation on ZERO-PADDED rows, as the backward does (fa_bwd_kernels.hip, FA_BWD_PAD): rows keep their packed pitch of p.D elements
// in global memory, the LDS images and register fragments have the kernel's pitch, and every 16-byte chunk at or past column p.D is
// fetched from an offset outside the buffer descriptor's range, which reads as zeros for register loads and LDS-DMA alike. The padding
// adds 0 to every score and its O columns are never stored.
// Dynamic LDS of a workgroup of the body below: the K and V double buffers of SUB tiles each (the epilogue's O tiles sit inside them)
// and, for the lazy kernels, the flag word behind them
template <typename Tag, int D, int SUB>
constexpr size_t mfma16_lds_bytes() {
  constexpr bool lazy = std::is_same<Tag, BF16>::value && D == 64 && (FA16_ONES != 0) && (FA16_LAZY == 1);
  return 4 * SUB * (size_t)(D == 128 ? FA16_BN128 : BN) * D * 2 + (lazy ? 16 : 0);
}

template <typename Tag, int D, bool CAUSAL, int RW, bool PAD, int SUB>
__device__ __forceinline__ void fwd_mfma16_body(const Params &p) {
  using M = MT16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int BMR = RW * WM;     // query rows of the block (RW waves of 32)
  constexpr int RB = D * 2;        // row bytes (global and LDS)
  constexpr int CPR = D / 8;       // 16-byte chunks per row
  constexpr int KS = D / 32;       // 32-wide k-steps of the score product
  constexpr int DT = D / 16;       // 16-wide d tiles of O^T
  constexpr int BNK = (D == 128) ? FA16_BN128 : BN;  // keys per staged tile
  constexpr int KT = BNK / 16;     // 16-key tiles per KV tile
  constexpr int NKP = KT / 2;      // 32-key k-steps of the PV product
  constexpr int TILE = BNK * RB;   // bytes of one K (or V) tile
  static_assert(D == 64 || D == 128, "head dims of the 16x16x32 kernel");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;
  // SUB = 2: a staged unit is a PAIR of tiles (one barrier and one staging pass per 128 keys; slots 2 buf + sub) -- affordable where the
  // workgroups are 256 rows high (two per CU: 2 x 64 KiB of LDS)
  lds_char *Kbuf = smem;                   // [2 SUB][BN][RB], chunks swizzled
  lds_char *Vbuf = smem + 2 * SUB * TILE;  // [2 SUB][BN][RB], chunks swizzled

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int c = lane & 15;  // query within a query tile / key row within a key tile / d within a d tile
  const int g = lane >> 4;  // 16-lane group

  int bh, qb;
  map_block<CAUSAL>(blockIdx.x, p, bh, qb);
  long long base, base_kv;
  head_bases(bh, p, base, base_kv);
  const int coff = p.Nk - p.N;  // causal, Nq != Nk: bottom-right aligned (key j visible to query i iff j <= i + coff)
  const int q0 = qb * BMR;
  const int qw0 = q0 + wave * WM;

  const int GRB = PAD ? p.D * 2 : RB;  // row bytes in global memory
  auto gcol = [&](int chunk) -> unsigned { return (!PAD || chunk * 8 < p.D) ? (unsigned)chunk * 16 : 0x80000000u; };  // (heads below 2 GiB: fa_fwd)
  const unsigned head_bytes = (unsigned)p.N * GRB, kv_head_bytes = (unsigned)p.Nk * GRB;
  const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.q + base * 2), 0, head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + base_kv * 2), 0, kv_head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.v + base_kv * 2), 0, kv_head_bytes, 0x00020000);

  // ---- Q fragments (B operand of K.Q^T): lane (c, g) holds Q[qw0 + 16qt + c][32ks + 8g .. +7]; rows >= N read as zero
  vec8 qf[2][KS];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rq, (unsigned)(qw0 + 16 * qt + c) * GRB + gcol(4 * ks + g), 0, 0);
      qf[qt][ks] = __builtin_bit_cast(vec8, t);
    }

  // ---- per-lane LDS addresses (absolute, opaque to hipcc: the dynamic-LDS base is a link-time constant it cannot fold)
  // K: ds_read_b128 of row (16kt + c), chunk (4ks + g); the swizzle depends on c only
  const int kx = (D == 64) ? ((c >> 1) & 7) : c;
  const lds_char *kptr[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kptr[ks] = Kbuf + c * RB + (((4 * ks + g) ^ kx) << 4);
    asm volatile("" : "+v"(kptr[ks]));
  }
  // V: transposed read; lane 4q + pp of a 16-lane group addresses row (.. + 4g + q), columns 16dt + 4pp .. +3
  const int vq = c >> 2, vp = c & 3;
  const int vrow = 4 * g + vq;
  const int vx = (D == 64) ? (((vrow >> 1) & 3) << 1) : ((vrow & 7) << 1);
  const lds_char *vptr[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    vptr[dt] = Vbuf + vrow * RB + ((((2 * dt) ^ vx) + (vp >> 1)) << 4) + 8 * (vp & 1);
    asm volatile("" : "+v"(vptr[dt]));
  }

  const int kv_end = CAUSAL ? min(p.Nk, q0 + BMR + coff) : p.Nk;
  const int nT = (kv_end + BNK - 1) / BNK;

  // ---- LDS-DMA staging: wave w moves the 1-KiB pieces w, w + 4, ... of each tile; inside a piece the LDS image is
  // lane-linear, so the chunk swizzle sits on the SOURCE address (one per-lane offset for K, one for V)
  constexpr int RPP = 1024 / RB;        // rows per piece
  constexpr int NPW = (BNK / RPP) / RW;  // pieces per wave, tile and operand
  static_assert((RW * RPP) % 16 == 0, "the piece stride must keep the swizzle");
  unsigned dma_kvo, dma_vvo;
  {
    const int row = wave * RPP + lane / CPR, pc = lane % CPR;
    const int skx = (D == 64) ? ((row >> 1) & 7) : (row & 15);
    const int svx = (D == 64) ? (((row >> 1) & 3) << 1) : ((row & 7) << 1);
    dma_kvo = (unsigned)(row * GRB) + gcol(pc ^ skx);
    dma_vvo = (unsigned)(row * GRB) + gcol(pc ^ svx);
  }
  auto stage_dma = [&](int t, int buf) {  // tile t -> buffer buf (hipcc does not count these loads: the caller waits vmcnt(0))
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      const unsigned soff = PAD ? (unsigned)(t * BNK + j * RW * RPP) * GRB : (unsigned)t * TILE + j * (RW * 1024);
      const unsigned lk = (unsigned)(__UINTPTR_TYPE__)Kbuf + buf * TILE + (wave + RW * j) * 1024;
      const unsigned lv = (unsigned)(__UINTPTR_TYPE__)Vbuf + buf * TILE + (wave + RW * j) * 1024;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lk), "v"(dma_kvo), "s"(rk), "s"(soff) : "memory");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lv), "v"(dma_vvo), "s"(rv), "s"(soff) : "memory");
    }
  };

  f32x4 oacc[DT][2];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int i = 0; i < 4; ++i) oacc[dt][qt][i] = 0.0f;
  constexpr bool ONES = (FA16_ONES != 0);
  // LAZY (bf16 only): no staleness test in the hot pass at all. bf16 probabilities carry fp32's exponent range, so P' = exp2(S - m) keeps its
  // 8 bits at ANY scale and O / the row sums are fp32: a stale reference loses nothing, it only has to be corrected before something
  // overflows -- from the row sums the matrix core has already delivered, one tile later (tile()). f16 P' has 5 exponent bits: not for it.
  // Head_dim 64 only: head_dim 128 is bound by the matrix pipe, not by the vector-issue port, and measured 0.6 % SLOWER without the test
  // (config 4 shard, profiles/r11/ab_lazy.log) -- it keeps the per-tile test.
  constexpr bool LAZY = ONES && std::is_same<Tag, BF16>::value && D == 64 && (FA16_LAZY != 0);
  constexpr bool LAZY_TEST = LAZY && (FA16_LAZY == 1);
  constexpr bool LOOK_PV = LAZY_TEST && (FA16_LOOK == 1), LOOK_FRONT = LAZY_TEST && (FA16_LOOK == 0);
  constexpr bool COLD3 = LAZY_TEST && (FA16_COLD == 3);
  constexpr bool TAIL_OUT = LAZY_TEST && (FA16_TAIL == 1);
  static_assert(4 * SUB * TILE + (LAZY_TEST ? 4 : 0) <= mfma16_lds_bytes<Tag, D, SUB>() && RW * WM * RB <= 4 * SUB * TILE,
                "the launcher's LDS size covers the K / V buffers, the flag word and the epilogue's O tiles");
  lds_char *poison_flag = smem + 4 * SUB * TILE;  // LAZY: one word behind the K / V buffers, the workgroup's OR of the waves' poison flags
  int slow = 0;    // LAZY, wave-uniform: this is the block's second run -- every tile takes the exact path (true maxima) before its hot pass
  // ONES: probabilities are formed against a reference BIAS log2 units ABOVE the row maximum found when the reference was last set
  // (P' = P / 2^BIAS <= 2^-BIAS then), so that "some score has since risen THR = BIAS + 1 above that maximum" reads "some P' >= 2",
  // i.e. "the top exponent bit of some packed P' is set" -- an OR over the 16 packed registers instead of 32 additions. bf16 keeps
  // fp32's exponent range (BIAS 7: THR 8 as before); f16 loses probabilities below 2^-24, so its reference sits only 3 above (THR 4).
  constexpr float BIAS = !ONES ? 0.0f : std::is_same<Tag, F16>::value ? 3.0f : 7.0f;
  constexpr float FIRST_SUM_FLOOR = std::is_same<Tag, F16>::value ? 1.0f : 0x1p-64f;  // see tile(): the first tile starts over below it
  // (the reference of row (16qt + c) itself -- log2 units: a stale row max + BIAS -- lives negated in negm[qt] below)
  float l[2] = {0.0f, 0.0f};            // !ONES: this lane's share of the row sums
  f32x4 lacc[2];                        // ONES: the row sums, complete, in every register of the tuple (accumulator of the ones tile)
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int i = 0; i < 4; ++i) lacc[qt][i] = 0.0f;
  vec8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (elem)1.0f;
  if constexpr (ONES) asm volatile("" : "+v"(ones));
  const float c2 = p.scale * 1.4426950408889634f;  // scale * log2(e)
  // minus the reference in the 4 registers of a tuple per query tile = the C operand of each score chain's first MFMA. It starts at
  // BIAS (ONES: an assumed row maximum of 0, see tile()) / at -inf (sums by v_add: the first tile sets it from the true maxima)
  f32x4 negm[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) negm[qt][i] = ONES ? -BIAS : INFINITY;
    asm volatile("" : "+v"(negm[qt]));  // opaque: else hipcc re-materialises the splat in front of every MFMA
  }

  if constexpr (LAZY_TEST) {
    if (threadIdx.x == 0) lds_write_b32(poison_flag, 0u);
  }
  stage_dma(0, 0);
  if constexpr (SUB == 2) {
    if (1 < nT) stage_dma(1, 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // Q~ = round(c.Q), once per block; retire the Q loads HERE (hipcc otherwise carries them into the loop as "possibly pending")
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[qt][ks][j] = (elem)((float)qf[qt][ks][j] * c2);
      asm volatile("" : "+v"(qf[qt][ks]));
    }
  __syncthreads();

  const float sum_thr = __builtin_exp2f(FA16_DEFER_THR);
  // element (kt, i) of query tile qt is masked iff 16kt + i > lim[qt] (key > query + coff, or key >= Nk); NKT key tiles from tile K0 on
  auto apply_mask = [&](auto k0c, auto &s, const int kv0) __attribute__((always_inline)) {
    constexpr int K0 = decltype(k0c)::value;
    constexpr int NKT = sizeof(s) / sizeof(s[0]);
    int g4 = 4 * g;
    asm volatile("" : "+v"(g4));  // pins the limits and the 32 compares inside the caller's `if (need_mask)`: hipcc otherwise hoists them in front of EVERY tile
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      int lim = p.Nk - 1 - kv0 - g4;
      if (CAUSAL) lim = min(lim, qw0 + 16 * qt + c + coff - kv0 - g4);
#pragma unroll
      for (int k2 = 0; k2 < NKT; ++k2)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[k2][qt][i] = (16 * (K0 + k2) + i > lim) ? -INFINITY : s[k2][qt][i];
    }
  };
  // mask only on tiles that cross the diagonal or the end of the sequence (re-evaluated from scalars at every use: carried as a
  // bool across the passes of a tile hipcc kept it in a VGPR, v_cndmask + v_cmp per tile)
  auto needs_mask = [&](const int kv0) __attribute__((always_inline)) { return (CAUSAL && (kv0 + BNK - 1 > qw0 + coff)) || (kv0 + BNK > p.Nk); };
  // S^T = K.Q^T + C for NKT key tiles from tile K0 on: s[k2][qt][i] = S[query 16qt + c][key kv0 + 16(K0 + k2) + 4g + i] + c_[qt];
  // K fragments read LA ahead of their use
  auto score_group = [&](auto bufc, auto k0c, auto &s, const f32x4 c0, const f32x4 c1) __attribute__((always_inline)) {
    constexpr int buf = decltype(bufc)::value;
    constexpr int K0 = decltype(k0c)::value;
    constexpr int NKT = sizeof(s) / sizeof(s[0]);
    constexpr int NK = NKT * KS, LA = (FA16_LAK < NK) ? FA16_LAK : NK;
    vec8 kf[NK];
    auto kread = [&](int i) { kf[i] = __builtin_bit_cast(vec8, lds_read_b128(kptr[i % KS] + buf * TILE + (K0 + i / KS) * 16 * RB)); };
#pragma unroll
    for (int i = 0; i < LA; ++i) kread(i);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int k2 = i / KS, ks = i % KS;
      s[k2][0] = M::mfma(kf[i], qf[0][ks], ks == 0 ? c0 : s[k2][0]);
      s[k2][1] = M::mfma(kf[i], qf[1][ks], ks == 0 ? c1 : s[k2][1]);
      if (i + LA < NK) kread(i + LA);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // pack the probabilities of NKT key tiles (from K0 on) into the PV operands pf[kp][qt] (k-step kp = two key tiles), rounded to
  // the input type; ONES: OR the packed words into `bits`
  auto pack_group = [&](auto k0c, auto &s, vec8 (&pf)[NKP][2], unsigned &bits) __attribute__((always_inline)) {
    constexpr int K0 = decltype(k0c)::value;
    constexpr int NKT = sizeof(s) / sizeof(s[0]);
#pragma unroll
    for (int kp = 0; kp < NKT / 2; ++kp)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[K0 / 2 + kp][qt][j] = (elem)s[2 * kp + (j >> 2)][qt][j & 3];
        if constexpr (ONES && !LAZY) {
          const u32x4 w = __builtin_bit_cast(u32x4, pf[K0 / 2 + kp][qt]);
          bits |= w[0] | w[1] | w[2] | w[3];
        }
      }
  };
  // the hot pass over NKT key tiles: P = exp2(S') -> pf (and `bits`, or the row sums ls)
  // (LAZY, `leave`: slow mode's way into the exact path -- the pass is left behind its score MFMAs, where the mask's branch already
  // parts the code, and the tile comes back after the true maxima; returns true then)
  // (COLD3: `masked` is the tile's mask flag as a scalar sign bit and nothing leaves here -- a tile off the diagonal crosses one scalar
  // compare and branch between its score MFMAs and its exponentials)
  auto hot_group = [&](auto bufc, auto k0c, auto nktc, const int kv0, vec8 (&pf)[NKP][2], unsigned &bits, float (&ls)[2],
                       const bool leave, const int masked) __attribute__((always_inline)) -> bool {
    constexpr int NKT = decltype(nktc)::value;
    f32x4 s[NKT][2];
    score_group(bufc, k0c, s, negm[0], negm[1]);
    if constexpr (COLD3) {
      if (masked < 0) apply_mask(k0c, s, kv0);
    } else {
      if constexpr (LAZY_TEST && FA16_COLD != 2) {
        if (__builtin_expect(leave, 0)) return true;
      }
      if (needs_mask(kv0)) apply_mask(k0c, s, kv0);
    }
#if FA16_PRIO
    if constexpr (decltype(k0c)::value + NKT == KT) __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
    for (int k2 = 0; k2 < NKT; ++k2)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          s[k2][qt][i] = __builtin_amdgcn_exp2f(s[k2][qt][i]);
          if constexpr (!ONES) ls[qt] = (decltype(k0c)::value == 0 && k2 == 0 && i == 0) ? s[k2][qt][i] : ls[qt] + s[k2][qt][i];
        }
    pack_group(k0c, s, pf, bits);
    return false;
  };
  // the row maxima of the raw scores of NKT key tiles, into mx[qt] (this lane's keys)
  auto max_group = [&](auto bufc, auto k0c, auto nktc, const int kv0, float (&mx)[2], const int masked) __attribute__((always_inline)) {
    constexpr int NKT = decltype(nktc)::value;
    f32x4 s[NKT][2], zero;
#pragma unroll
    for (int i = 0; i < 4; ++i) zero[i] = 0.0f;
    score_group(bufc, k0c, s, zero, zero);
    if (COLD3 ? masked < 0 : needs_mask(kv0)) apply_mask(k0c, s, kv0);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int k2 = 0; k2 < NKT; ++k2)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx[qt] = fmaxf(mx[qt], s[k2][qt][i]);
  };
  // row maxima of the raw scores -> new reference: rescale O and the row sums, rewrite the C-operand tuples (first tile and rare path)
  auto new_reference = [&](auto firstc, float (&mx)[2]) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(firstc)::value;  // first tile: O and the row sums are still zero, nothing to rescale
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float v = mx[qt];
      v = fmaxf(v, xlane(v, 16));
      v = fmaxf(v, xlane(v, 32));
      const float m_old = -negm[qt][0];
      const float m_new = FIRST ? v + BIAS : fmaxf(m_old, v + BIAS);  // finite: every row sees key 0 of the first tile
#pragma unroll
      for (int i = 0; i < 4; ++i) negm[qt][i] = -m_new;
      asm volatile("" : "+v"(negm[qt]));
      if constexpr (FIRST) continue;
      const float alpha = __builtin_amdgcn_exp2f(m_old - m_new);
      if constexpr (ONES) {
#pragma unroll
        for (int i = 0; i < 4; ++i) lacc[qt][i] *= alpha;
      } else {
        l[qt] *= alpha;
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) oacc[dt][qt][i] *= alpha;
    }
  };
  // LAZY: the row sums as they stand (every tile before this one is in them: the ones MFMAs of the previous tile retired before the barrier).
  // Compared as unsigned bit patterns, so that inf and NaN of either sign read "large" (-fno-honor-nans: a float compare may lose them).
  // A sum of 2^e.f in [THR, POISON) is renormalised: O and the sum times 2^-e, the reference plus e -- exact, and exactly what a reference
  // e higher would have given from the start. At or above POISON (a score rose more than ~100 log2 units within one tile, or inf / NaN
  // input) nothing is repaired: the wave is poisoned (it says so in the workgroup's flag word at once), walks on so that barriers and staging stay uniform, and the block runs again.
  constexpr unsigned LAZY_THR_BITS = __builtin_bit_cast(unsigned, (float)FA16_LAZY_THR);
  constexpr unsigned LAZY_POISON_BITS = __builtin_bit_cast(unsigned, (float)FA16_LAZY_POISON);
  static_assert(LAZY_THR_BITS < LAZY_POISON_BITS && LAZY_POISON_BITS < 0x7f800000u, "2^-BIAS << THR < POISON < inf");
  // lazy_look: the wave's ballot of "a sum of mine is large" (two VALU; the verdict is scalar). lazy_repair: what a non-zero ballot leads
  // to, from the sums as they stand THEN -- with the look inside the PV product (LOOK_PV) that is one tile more than the look saw: sums
  // only grow, so a row the look found large is large or untrusted now, and a row that meanwhile left the trusted range is poisoned, not scaled.
  auto lazy_look = [&]() __attribute__((always_inline)) -> unsigned long long {
    const unsigned b0 = __builtin_bit_cast(unsigned, lacc[0][0]), b1 = __builtin_bit_cast(unsigned, lacc[1][0]);
    return __builtin_amdgcn_ballot_w64(max(b0, b1) >= LAZY_THR_BITS);
  };
  auto lazy_repair = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const unsigned a = __builtin_bit_cast(unsigned, lacc[qt][0]) & 0x7fffffffu;
      const bool bad = a >= LAZY_POISON_BITS;
      const bool big = !bad && a >= LAZY_THR_BITS;
      const int e = (int)(a >> 23) - 127;
      const float sc = big ? __builtin_bit_cast(float, (unsigned)(127 - e) << 23) : 1.0f;
      const float kf = big ? (float)e : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lacc[qt][i] *= sc;
        negm[qt][i] -= kf;
      }
      asm volatile("" : "+v"(negm[qt]));
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) oacc[dt][qt][i] *= sc;
      if (bad) lds_write_b32(poison_flag, 1u);  // (the flag is read behind the tile loop's last barrier)
    }
  };
  constexpr int G = (FA16_HALVES != 0) ? 2 : 1;  // key-tile groups of the hot pass: 1 = all 16 score MFMAs, then the softmax; 2 = per 32-key half
  using KTG = std::integral_constant<int, KT / G>;
  using K0A = std::integral_constant<int, 0>;
  using K0B = std::integral_constant<int, KT / 2>;

  // One KV tile: P = exp2(S') against the running reference (S' comes out of the matrix core with the reference already subtracted), and
  // a test whether the reference is stale -- ONES: some packed P' has its top exponent bit set (P' >= 2, inf or NaN); else: a lane's 16
  // probabilities of a row add up to more than 2^THR. Only then -- and on the first tile, whose reference is -inf -- the wave takes the
  // rare path: one pass for the row maxima of the raw scores, rescale O and the row sums, and the hot pass AGAIN (a backward branch:
  // the score / P registers of the hot pass never merge with anything the rare path computes -- with the rare path as a forward
  // if / else hipcc parked all 32 P values in scratch on the common path of the non-causal kernel).
  auto tile = [&](auto bufc, auto firstc, const int t) {
    constexpr int buf = decltype(bufc)::value;
    constexpr bool FIRST = decltype(firstc)::value;
    const int kv0 = t * BNK;

    // whole-tile skip per wave (kernels.metal:682 with Br = 32)
    // (non-causal: an always-true scalar hipcc cannot see through -- with the tile body unconditional it schedules across the
    // tile boundary and spills 250-390 B per lane under the 128-register budget; with the branch in place, as in the causal
    // kernel, it fits)
    int always = 1;
    if constexpr (!CAUSAL) asm volatile("" : "+s"(always));
    const bool wave_active = CAUSAL ? (kv0 <= qw0 + WM - 1 + coff) : (always != 0);
    if (wave_active) {
      vec8 pf[NKP][2];  // B operands of the PV product: k-step kp, query tile qt
      float ls[2] = {0.0f, 0.0f};
      // redo (wave-uniform): first the row maxima of the raw scores -> new reference, then the hot pass. The FIRST tile starts without
      // it (ONES): its reference is the constant BIAS, i.e. an assumed row maximum of 0 -- any finite reference is as good as the true
      // maximum as long as no P' reaches 2 (the hot pass's own test) and the rounding of P' to the input type keeps its bits (tested
      // once, behind the first tile's PV product: no row sum below FIRST_SUM_FLOOR) -- which saves every block a whole score pass (16
      // MFMAs, the maxima, their cross-lane steps). (A 16-key reference for the first tile, 4 MFMAs instead of 16, was measured: no gain,
      // profiles/r04/ab_mfma16_first_tile.log.)
      // FIRST_SUM_FLOOR. bf16 has fp32's exponent range: P' keeps its 8 bits down to 2^-126, the floor only catches sums that vanish
      // (2^-64: scores below -2^6). f16 P' is SUBNORMAL below 2^-14 and zero below 2^-25, and the matrix core takes subnormal f16
      // operands as they are (measured: the error grows smoothly with the depth of the scores, profiles/r06/parent_score_range.log): a
      // row whose first 64 scores lie at -11 ... -22 would be summed from probabilities of 0 ... 10 bits, and nothing renews the
      // reference later (no P' >= 2). Measured boundary of the first tile alone (tests/test_gpu_score_range.py, identical keys: every
      // P' of a row rounds the same way): sums of 2^-7.5 and more hold the LSE bar, sums of 2^-8 ... 2^-9 (P' below 2^-14) miss it.
      // A floor just above that, 2^-7, is not enough: a first tile that sums to 2^-6 followed by a thousand keys 8 log2 units lower
      // (P' of 2^-20: five bits) missed the bar by 2.6x (profiles/r06/floor_2m7_tail_case.log) -- the reference stays for the whole
      // row. What a floor F buys: a subnormal P' is rounded by at most 2^-25 absolute, so n keys move a row sum >= F by at most
      // n * 2^-25 / F relative. F = 1: 1.2e-4 at 4096 keys, all roundings in one direction (2^-7: 1.6e-2). (A row that did start
      // over has its largest P' at 2^-3, a sum of 2^-3 at least: the kept first tile is never the weaker of the two.) Ordinary rows
      // (scores around 0) sum to about 8 over 64 keys and never start over; the first rows under the causal mask (fewer than 8
      // visible keys) do, one wave per head.
      // LAZY (bf16): the hot pass has no test, and nothing between the barrier and the first score MFMA touches a vector register. What
      // the tiles BEFORE this one summed to is looked at inside this tile's PV product (LOOK_PV: v_max_u32 + v_cmp into an SGPR pair, in
      // the gap behind the product's first MFMA -- the sums' last writers retired sixteen MFMAs earlier, their next ones follow later in
      // the product); the repair, if any, runs behind the product's last MFMA, from the sums as they stand then. So a rise in tile t is
      // answered behind tile t + 1: the answer is exact whenever it comes (sums only grow, a power of two is a power of two), the lag
      // only decides when a row counts as untrusted -- a sum that goes from below THR past POISON within two tiles (about 44 log2
      // units) instead of one -- and that costs the workgroup its second run, never a wrong result. (Round 11 looked in front of the
      // tile: a VALU read of the youngest matrix results and a branch on it directly behind the barrier; profiles/r20.)
      // The pass below runs scores -> mask -> exp2 -> pack -> PV + ones straight through; between the score MFMAs and the exponentials
      // it crosses ONE scalar compare and branch (the mask's, COLD3). The way back is left for the first tile (the floor) and for slow
      // mode (the second run of a poisoned block), which sets the redo flag at the head of EVERY tile: true maxima first, so every
      // P' <= 2^-BIAS. (In round 11's structure a forward `if (slow)` in front of the pass cost 32-40 B of scratch and slow mode left the
      // pass behind its score MFMAs instead, a second branch on the common path; with the mask flag scalar and the look out of the
      // tile's head, entering through the redo flag costs no scratch and no register: tools/resusage.sh, profiles/r20.)
      if constexpr (LOOK_FRONT && !FIRST) {
        if (__builtin_expect(lazy_look() != 0, 0)) lazy_repair();
      }
      // the tile's mask flag (needs_mask) as a SIGN BIT, scalar end to end: integer arithmetic, pinned -- as the OR of two compares (or
      // as a 0 / 1 value: hipcc turns the shift back into a select) it is formed in the lane-mask domain and goes through a VGPR
      // (v_cndmask + v_cmp) in the header of the redo loop
      int masked = 0;
      if constexpr (COLD3) {
        const int to_diagonal = CAUSAL ? (qw0 + coff) - (kv0 + BNK - 1) : 0, to_end = p.Nk - (kv0 + BNK);  // negative: the tile crosses it
        masked = to_diagonal | to_end;
        asm volatile("" : "+s"(masked));
      }
      unsigned long long look = 0;  // LOOK_PV: the ballot of the look, an SGPR pair across the PV product
      bool redo = (FIRST && !ONES) || (COLD3 && slow != 0);
      for (;;) {
        if (__builtin_expect(redo, 0)) {
          float mx[2] = {-INFINITY, -INFINITY};
          max_group(bufc, K0A{}, std::integral_constant<int, KT / 2>{}, kv0, mx, masked);
          max_group(bufc, K0B{}, std::integral_constant<int, KT / 2>{}, kv0, mx, masked);
          new_reference(firstc, mx);
        }
#if FA16_PRIO
        __builtin_amdgcn_s_setprio(1);
#endif
        unsigned bits = 0;
        if constexpr (LAZY_TEST) {
          if (hot_group(bufc, K0A{}, KTG{}, kv0, pf, bits, ls, !COLD3 && slow != 0 && !redo, masked)) {
            redo = true;
            continue;
          }
        } else {
          hot_group(bufc, K0A{}, KTG{}, kv0, pf, bits, ls, false, 0);
        }
        if constexpr (G == 2) hot_group(bufc, K0B{}, KTG{}, kv0, pf, bits, ls, false, 0);
        bool stale;
        if constexpr (LAZY) stale = false;  // (the test that is not there; written so that the f16 kernels keep their instructions)
        else if constexpr (ONES) stale = __builtin_amdgcn_ballot_w64((bits & 0x40004000u) != 0) != 0;
        else stale = __builtin_amdgcn_ballot_w64(fmaxf(ls[0], ls[1]) > sum_thr) != 0;
        if (__builtin_expect(stale && !redo, 0)) {  // (after a redo every P' <= 2^-BIAS: a second stale reading is inf / NaN input)
          redo = true;
          continue;
        }
        if constexpr (!ONES) {
          l[0] += ls[0];
          l[1] += ls[1];
        }
#if FA16_PRIO
        __builtin_amdgcn_s_setprio(1);
#endif
        // ---- O^T += V^T.P^T, and (ONES) the row sums from a fifth d tile of ones
        {
          constexpr int NV = NKP * DT, LA = FA16_LAV;
          s16x4 wlo[NV], whi[NV];
          auto vread = [&](int j) {  // step j = (kp, dt)
            const lds_char *vb = vptr[j % DT] + buf * TILE + (32 * (j / DT)) * RB;
            wlo[j] = lds_read_tr16(vb);            // keys 32kp + 4g + 0..3       (k elements 0..3)
            whi[j] = lds_read_tr16(vb + 16 * RB);  // keys 32kp + 16 + 4g + 0..3  (k elements 4..7)
          };
#pragma unroll
          for (int j = 0; j < LA; ++j) vread(j);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            const s16x8 v8 = __builtin_shufflevector(wlo[j], whi[j], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) oacc[j % DT][qt] = M::mfma(__builtin_bit_cast(vec8, v8), pf[j / DT][qt], oacc[j % DT][qt]);
            if (j + LA < NV) vread(j + LA);
            if constexpr (ONES) {
              if (j % DT == DT - 1) {
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) lacc[qt] = M::mfma(ones, pf[j / DT][qt], lacc[qt]);
              }
            }
            if constexpr (LOOK_PV && !FIRST) {
              // the look at the row sums, in the gap behind the product's first MFMAs: the sums hold every tile before this one and have
              // no writer pending (this tile's ones MFMAs come later, the previous tile's retired sixteen MFMAs ago)
              if (j == 0) {
                look = lazy_look();
                asm volatile("" : "+s"(look));
              }
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
#if FA16_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        if constexpr (LOOK_PV && !FIRST) {
          // ... and what it leads to, behind the product's last MFMA (never between the MFMAs of one product): one scalar branch
          if (__builtin_expect(look != 0, 0)) lazy_repair();
        }
        if constexpr (FIRST && ONES) {
          // the assumed reference was too HIGH for some row (its first-tile sum is below FIRST_SUM_FLOOR): start the tile over with
          // the true maxima (O and the row sums hold nothing of weight: cleared)
          if (__builtin_expect(!redo && __builtin_amdgcn_ballot_w64(fminf(lacc[0][0], lacc[1][0]) < FIRST_SUM_FLOOR) != 0, 0)) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
              for (int i = 0; i < 4; ++i) lacc[qt][i] = 0.0f;
#pragma unroll
              for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 4; ++i) oacc[dt][qt][i] = 0.0f;
            }
            redo = true;
            continue;
          }
        }
        break;
      }
    }
  };
  // LAZY: the last tile's sums have no tile behind them to be looked at: they are tested in front of the block's last barrier, on which the
  // workgroup's OR of the poison flags rides (a word of LDS, written by poisoned waves only)
  auto tail_test = [&]() __attribute__((always_inline)) {
    const unsigned a0 = __builtin_bit_cast(unsigned, lacc[0][0]) & 0x7fffffffu, a1 = __builtin_bit_cast(unsigned, lacc[1][0]) & 0x7fffffffu;
    if (max(a0, a1) >= LAZY_POISON_BITS) lds_write_b32(poison_flag, 1u);
  };
  // one staged unit (SUB tiles from tile t0 on, in the slots of buffer `buf`): the next unit's tiles go into the other buffer first, in
  // flight under this unit's MFMAs; one wait + barrier at its end
  auto unit = [&](auto bufc, auto firstc, const int t0) {
    constexpr int buf = decltype(bufc)::value;
#pragma unroll
    for (int sub = 0; sub < SUB; ++sub)
      if (t0 + SUB + sub < nT) stage_dma(t0 + SUB + sub, (buf ^ 1) * SUB + sub);
    tile(std::integral_constant<int, buf * SUB>{}, firstc, t0);
    if constexpr (SUB == 2) {
      if (t0 + 1 < nT) tile(std::integral_constant<int, buf * SUB + 1>{}, std::false_type{}, t0 + 1);
    }
    if constexpr (TAIL_OUT) {
      // the block's LAST barrier, and the test in front of it, stand behind the tile loop (below): a tile's tail is one scalar condition
      // around its wait and its barrier (with the test in here, on `last unit && !slow`, hipcc laid three scalar branches into the tail of
      // EVERY tile, in front of the barrier all waves meet at: +0.5 % on configs 3 / non-causal / N = 16384, profiles/r20/ab_tail.log)
      if (t0 + SUB < nT) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    } else {
      if (t0 + SUB < nT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pieces issued at the top of this unit have landed
      if constexpr (LAZY_TEST) {
        if (t0 + SUB >= nT && slow == 0) tail_test();
      }
      __syncthreads();
    }
  };
  // LAZY: a poisoned block (the workgroup's flag word, read behind the last barrier; nothing has been stored yet) runs once more, in
  // slow mode, through the same loops; every other block leaves through the `break`. (The loop ends in front of the epilogue: around
  // it hipcc hoisted the epilogue's addresses over the tile loop, into scratch; and folded into the tile loop as one more way back to
  // tile 0 it cost 220 B.)
  for (;;) {
    unit(std::integral_constant<int, 0>{}, std::true_type{}, 0);
    for (int t = SUB; t < nT; t += 2 * SUB) {
      unit(std::integral_constant<int, 1>{}, std::false_type{}, t);
      if (t + SUB < nT) unit(std::integral_constant<int, 0>{}, std::false_type{}, t + SUB);
    }
    if constexpr (TAIL_OUT) {  // the last unit left its barrier to us
      if (slow == 0) tail_test();
      __syncthreads();
    }
    if constexpr (LAZY_TEST) {
      if (slow == 0) {
        const unsigned f = *reinterpret_cast<const volatile __attribute__((address_space(3))) unsigned *>(poison_flag);
        if (__builtin_expect(__builtin_amdgcn_readfirstlane((int)f) != 0, 0)) {
          // clear the accumulators, take the assumed reference back (the first exact pass replaces it), restage tile 0. Slow mode cannot
          // poison itself (every P' <= 2^-BIAS) -- inf / NaN inputs give inf / NaN rows -- and the second run is the last.
          slow = 1;
#pragma unroll
          for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              lacc[qt][i] = 0.0f;
              negm[qt][i] = -BIAS;
            }
            asm volatile("" : "+v"(negm[qt]));
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
              for (int i = 0; i < 4; ++i) oacc[dt][qt][i] = 0.0f;
          }
          stage_dma(0, 0);
          if constexpr (SUB == 2) {
            if (1 < nT) stage_dma(1, 1);
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          continue;
        }
      }
    }
    break;
  }

  // ---- epilogue: normalise, LSE, O tile -> LDS -> coalesced 16-byte stores
  // (LAZY: the lane's indices once more, opaque -- with the second run's loop in front of it hipcc computes the epilogue's addresses in the
  // prologue and parks them in scratch across the tile loop)
  int elane = lane;
  if constexpr (LAZY_TEST) asm volatile("" : "+v"(elane));
  const int ec = elane & 15, eg = elane >> 4;
  lds_char *Ot = smem + wave * (WM * RB);  // this wave's [32][D] tile (inside the K buffers: free since the last barrier)
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float lt = ONES ? lacc[qt][0] : l[qt];
    if constexpr (!ONES) {
      lt += xlane(lt, 16);
      lt += xlane(lt, 32);
    }
    const float inv_l = __builtin_amdgcn_rcpf(lt);  // v_rcp_f32 (1 ulp): the IEEE division costs ten instructions per row
    const int row = 16 * qt + ec, qrow = qw0 + row;
    // LSE = (reference + log2 l) . ln 2, v_log_f32 straight (l is a sum of probabilities around 2^-BIAS .. 2^THR: no denormals)
    if (p.lse != nullptr && eg == 0 && qrow < p.N)
      p.lse[(long long)bh * p.N + qrow] = (__builtin_amdgcn_logf(lt) - negm[qt][0]) * 0.6931471805599453f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      // registers 0..3 = d columns 16dt + 4g + 0..3 of row (16qt + c); converted as one vector so that hipcc packs pairs
      typedef elem elem4 __attribute__((ext_vector_type(4)));
      elem4 e;
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = (elem)(oacc[dt][qt][i] * inv_l);
      const u32x2 w = __builtin_bit_cast(u32x2, e);
      const int ch = (2 * dt + (eg >> 1)) ^ (row & (CPR - 1));  // chunk XOR row spreads the rows over the banks
      lds_write_b64(Ot + row * RB + (ch << 4) + 8 * (eg & 1), w);
    }
  }
  __syncthreads();
  {
    elem *Og = (elem *)p.o + base;
#pragma unroll
    for (int it = 0; it < WM * CPR / 64; ++it) {
      const int idx = it * 64 + elane;
      const int row = idx / CPR, ch = idx % CPR;
      const u32x4 vv = lds_read_b128(Ot + row * RB + ((ch ^ (row & (CPR - 1))) << 4));
      if (qw0 + row < p.N && (!PAD || ch * 8 < p.D)) *reinterpret_cast<u32x4 *>(Og + (long long)(qw0 + row) * (PAD ? p.D : D) + ch * 8) = vv;
    }
  }
}

template <typename Tag, int D, bool CAUSAL, int RW, bool PAD = false, int SUB = 1>
__global__ __launch_bounds__(64 * RW, (D == 64 ? FA16_OCC : FA16_OCC128)) void fwd_mfma16_kernel(Params p) {
  fwd_mfma16_body<Tag, D, CAUSAL, RW, PAD, SUB>(p);
}

bool mfma16_supported(int dtype, int D) { return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && D >= 8 && D <= 128 && D % 8 == 0; }

template <typename Tag, int D, bool CAUSAL, int RW, bool PAD = false, int SUB = 1>
static hipError_t launch16_one(const Params &p, hipStream_t s) {
  int head_group = causal_head_group(p, D, 2);
#ifdef FA16_FORCE_HEAD_GROUP  // scheduling experiments only (tools/ab.py arms): never defined in the shipped library
  head_group = FA16_FORCE_HEAD_GROUP;
#endif
  return launch_blocks(fwd_mfma16_kernel<Tag, D, CAUSAL, RW, PAD, SUB>, p, RW * WM, 64 * RW, mfma16_lds_bytes<Tag, D, SUB>(), head_group, s);
}

// Waves per workgroup: 4 (128 query rows) or 8 (256 rows, the same 32 rows per wave: eight waves share every K / V tile, so the
// L2 -> LDS stream and its issue slots halve, and a workgroup that is alone on its CU in the launch's tail still runs two waves per SIMD).
// The price is the causal diagonal (a block's lower waves idle through up to seven more tiles' barriers), twice the weight of the
// heaviest block, and a wider spread of launch times on large causal grids. Measured interleaved on warm clocks, medians, bf16 unless
// noted (profiles/r04/ab_mfma16_eight_waves_steady_state.log):
//   non-causal  N = 2048 / 4096 (64 heads) +5.1 / +4.6 %, N = 8192 +4.1 %, 32 heads x 2048 +1.2 % (256 workgroups: level)
//   causal      64 heads x 4096 (config 3) +3.0 %, f16 +3.7 %, x 5120 +1.5 %; but 80 .. 256 heads x 4096 -2.3 .. -6.3 % (best times level),
//               48 heads level, 64 heads x 2048 -4.8 %, x 6144 -0.9 %, x 8192 +0.7 %, x 16384 +0.4 %, 48 heads x 8192 -0.2 %
//   head_dim 128: non-causal 32 heads x 8192 +2.5 %, causal level
// (N = 512, 256 / 512 heads: +3.4 % over four waves) -> eight waves for non-causal grids of at least 512 such workgroups, and under the mask only for the two-round grids of config 3's
// kind (1024 .. 1279 workgroups of 256 rows at 4096 <= N < 6144), where the launch is tail-dominated.
int mfma16_waves(int D, int BH, int N, int Nk, int is_causal) {
#ifdef FA16_FORCE_RW
  return FA16_FORCE_RW;
#endif
  if (D != 64 && D != 128) return 4;  // (padded head dims)
  const long long b256 = (long long)BH * ((N + 255) / 256);
  if (D == 128) return (!is_causal && Nk >= 8192 && b256 >= 1024) ? 8 : 4;
  if (!is_causal) return (Nk >= 512 && b256 >= 512) ? 8 : 4;
  return (Nk >= 4096 && Nk < 6144 && b256 >= 1024 && b256 < 1280) ? 8 : 4;
}

hipError_t launch_mfma16(const Params &p, int dtype, hipStream_t s) {
  const bool w8 = mfma16_waves(p.D, p.B * p.H, p.N, p.Nk, p.is_causal) == 8 && (p.D == 64 || !p.is_causal);
  return with_tag(dtype, [&](auto tag) -> hipError_t {
    using Tag = decltype(tag);
    if (p.D != 64 && p.D != 128) {  // zero-padded rows of the next larger instantiation (four waves)
      if (p.D < 64) return p.is_causal ? launch16_one<Tag, 64, true, 4, true>(p, s) : launch16_one<Tag, 64, false, 4, true>(p, s);
      return p.is_causal ? launch16_one<Tag, 128, true, 4, true>(p, s) : launch16_one<Tag, 128, false, 4, true>(p, s);
    }
    if (p.D == 64) {
      if (w8) return p.is_causal ? launch16_one<Tag, 64, true, 8, false, FA16_SUB8>(p, s) : launch16_one<Tag, 64, false, 8, false, FA16_SUB8>(p, s);
      return p.is_causal ? launch16_one<Tag, 64, true, 4>(p, s) : launch16_one<Tag, 64, false, 4>(p, s);
    }
    if (p.D == 128) {
      if (w8) return launch16_one<Tag, 128, false, 8>(p, s);  // (non-causal only: mfma16_waves)
      return p.is_causal ? launch16_one<Tag, 128, true, 4>(p, s) : launch16_one<Tag, 128, false, 4>(p, s);
    }
    return hipErrorInvalidValue;
  });
}

}  // namespace fa
