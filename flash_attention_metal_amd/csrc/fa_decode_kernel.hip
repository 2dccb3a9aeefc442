// fa_decode_kernel.hip -- few query rows against a long key sequence (decode steps, short chunks), entry point fa_fwd_decode.
//
// Scope row f3 (operator generality; not in the reference, whose operator is square: /root/reference/kernels.metal:606,619). The
// generalised forward fa_fwd_ex launches one workgroup per (batch, QUERY head, 128 query rows): a decode step -- 1..16 queries per
// head, grouped-query heads, thousands of keys -- then runs B.Hq workgroups on 256 CUs, each reading its key head's whole K and V,
// and streams 0.2-0.6 TB/s of an 8 TB/s memory (profiles/r03/decode_steps_splitkv_rule.log). This path is HBM-bound work and is
// laid out as such:
//   * the Hq / Hkv query heads that share a key/value head, times their Nq queries, are PACKED into the rows of one 16- or 32-row
//     query block (R = (Hq / Hkv) . Nq <= 32): K and V of a key head are read once, not once per query head;
//   * the keys of a (batch, key head) are SPLIT over S work items so that B . Hkv . S fills the chip several times over; an item is
//     ONE wave (a 64-thread workgroup: no barrier anywhere) that streams its keys in 64-key tiles through a private double buffer in
//     LDS by LDS-DMA (one tile in flight under the tile being multiplied), multiplies on v_mfma_f32_16x16x32 with the operand maps
//     and LDS images of fa_mfma16_kernel.hip, and keeps an exact online softmax (row maximum per tile: the arithmetic is free here);
//   * each item writes its partial (O . l, m, l) to a caller-owned workspace; a second launch combines the S partials of a row by
//     their maxima: M = max m_s, l = sum l_s 2^(m_s - M), O = sum O_s 2^(m_s - M) / l, LSE = (M + log2 l) ln 2.
// The library allocates nothing (C-ABI): the workspace size comes from fa_fwd_decode_workspace_bytes().
// e4m3 inputs (KV8; dtype FA_DTYPE_FP8_E4M3: Q, K, V e4m3 as in fa_fwd's config-5 family, O bf16): HALF the bytes of the stream this
// path is bound by. K and V tiles travel global -> registers (16 e4m3 per lane and load, the next tile's loads in flight under this
// tile's arithmetic) -> widened EXACTLY to bf16 -> the same swizzled LDS images, so everything behind the staging is the bf16 kernel
// bit for bit (results equal those of the bf16 path on the widened tensors). The widening is VALU work this path has to spare.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

#ifndef FA_DECODE_REGSTAGE
#define FA_DECODE_REGSTAGE 0  // 1 (experiment): 16-bit inputs also travel through registers into ONE LDS image (twice the items per CU), as e4m3 inputs do
#endif
#ifndef FA_DECODE_KV8_DEPTH
#define FA_DECODE_KV8_DEPTH 1  // e4m3 inputs, head_dim 64: tiles waiting in registers (1; 2 measured 0-13 % slower: 160 instead of 128 registers, profiles/r04/decode_ab_kv8_depth.log)
#endif

namespace fa {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename Tag> struct MD16;
template <> struct MD16<BF16> {
  using elem = __bf16;
  using vec8 = bf16x8;
  __device__ static __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MD16<F16> {
  using elem = _Float16;
  using vec8 = f16x8;
  __device__ static __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// item (b, hkv, s): rows r = gi * Nq + iq of the packed block (gi: query head within the group), keys of tiles [t0, t1)
// 8 e4m3 (two dwords) -> 8 bf16 (four dwords = one 16-byte chunk): exact (bf16 = the upper half of the fp32 pattern)
__device__ __forceinline__ u32x4 widen8(unsigned w0, unsigned w1) {
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

// Dynamic LDS of an item: K and V double buffers of 64-key tiles; one image each where the tiles are staged through registers
template <int D, bool KV8>
constexpr size_t decode_lds_bytes() { return ((KV8 || FA_DECODE_REGSTAGE) ? 2 : 4) * (size_t)BN * D * 2; }

// PRM = DecodePagedParams (PAGED: fa_fwd_decode_paged; the DecodeParams instantiations are fa_fwd_decode's kernels, unchanged): the
// item's sequence has its own length L_b
// (read once from device memory, clamped to the capacity p.Nk) in place of Nk, and every K / V piece comes from the page the block
// table names for it, through a descriptor built on that page's 64-bit base whose range covers only the page's valid rows -- so rows
// >= L_b, out-of-range pages and whatever a page holds past L_b read as hardware zeros (the whole offset sits in voffset, inside the
// range check), 32-bit offsets never leave a page, and the pool may exceed 4 GiB. Pages hold >= 16 rows and start at multiples of
// their size: every 1-KiB LDS-DMA piece (4 / 8 rows) and every 16-byte-per-lane register load (<= 16 rows) lies inside ONE page,
// whose table entry is wave-uniform. The entries of the next tile to stage are loaded one tile ahead.
template <typename Tag, int D, int QT, bool CAUSAL, bool KV8, typename PRM = DecodeParams>
__global__ __launch_bounds__(64) void decode_partial_kernel(PRM p) {
  constexpr bool PAGED = std::is_base_of<DecodePagedParams, PRM>::value;
  // WINDOW (PRM = DecodeWindowParams, fa_fwd_decode_paged_window; instantiated with CAUSAL): key j is visible to row iq iff
  // iq + cl <= j <= iq + cu, cl = coff - wl, cu = coff + wr (non-negative bounds from the host). The item's tiles are a share of
  // [t_lo, nT), the tiles that hold the keys rows 0 .. Nq - 1 see together, instead of [0, nT).
  // SOFTCAP (PRM = DecodeSoftcapParams, fa_fwd_decode_paged_softcap): window mode over capped scores softcap . tanh(scale . s / softcap).
  // Q~ carries 2 log2(e) scale / softcap, so the matrix core delivers the argument of tanh's one exponential; t . softcap . log2(e) takes
  // the score's place in front of the mask (tanh(-inf) is -1, not -inf), and everything from the mask onwards is the window mode's.
  constexpr bool SOFTCAP = std::is_same<PRM, DecodeSoftcapParams>::value;
  constexpr bool WINDOW = std::is_same<PRM, DecodeWindowParams>::value || SOFTCAP;
  static_assert(!WINDOW || CAUSAL, "window mode: the upper bound is the causal one with its own offset");
  using M = MD16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int RB = D * 2;       // row bytes
  constexpr int CPR = D / 8;      // 16-byte chunks per row
  constexpr int KS = D / 32;      // 32-wide k-steps of the score product
  constexpr int DT = D / 16;      // 16-wide d tiles of O^T
  constexpr int KT = BN / 16;     // 16-key tiles per 64-key tile
  constexpr int TILE = BN * RB;   // bytes of one K (or V) tile
  constexpr int RPP = 1024 / RB;  // rows per 1-KiB LDS-DMA piece
  constexpr int NP = BN / RPP;    // pieces per tile and operand (all moved by this one wave)

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;
  constexpr bool RS = KV8 || (FA_DECODE_REGSTAGE != 0);  // tiles staged through registers into one LDS image
  lds_char *Kbuf = smem, *Vbuf = smem + (RS ? 1 : 2) * TILE;
  static_assert((RS ? 2 : 4) * TILE == decode_lds_bytes<D, KV8>(), "the launcher's LDS size is the K / V buffers");

  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, item = blockIdx.x;
  const int bkv = item / S, s = item - bkv * S;
  const int b = bkv / p.Hkv, hkv = bkv - b * p.Hkv;
  const int G = p.Hq / p.Hkv, R = G * p.Nq;
  int Nk = p.Nk;  // keys of this item's sequence
  if constexpr (PAGED) Nk = min(max(__builtin_amdgcn_readfirstlane(p.seqlens[b]), 0), p.max_pages << p.lp);
  const int coff = Nk - p.Nq;
  int cl = 0, cup = coff, k_lo = 0, k_hi = Nk;
  if constexpr (WINDOW) {
    cl = coff - p.wl;
    cup = coff + p.wr;
    window_key_range(p.Nq, Nk, p.wl, p.wr, 0, p.Nq - 1, k_lo, k_hi);
    if (k_lo >= k_hi) k_lo = k_hi = 0;
  }
  const int nT = (k_hi + BN - 1) / BN, t_lo = k_lo / BN, nW = nT - t_lo;
  const int t0 = t_lo + (int)((long long)s * nW / S), t1 = t_lo + (int)((long long)(s + 1) * nW / S);

  const long long base_kv = PAGED ? 0 : (long long)b * p.kv_bs + (long long)hkv * p.kv_hs;
  constexpr int EB = KV8 ? 1 : 2;  // bytes per input element
  const unsigned kv_bytes = (unsigned)Nk * D * EB;
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + base_kv * EB), 0, kv_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.v + base_kv * EB), 0, kv_bytes, 0x00020000);

  // ---- Q fragments: lane (c, g) holds row r = 16qt + c of the packed block, elements 32ks + 8g .. +7; pre-scaled Q~ = round(c.Q)
  float c2 = p.scale * 1.4426950408889634f;
  float capc = 0.0f;  // softcap mode: softcap . log2(e)
  if constexpr (SOFTCAP) {
    capc = p.softcap * 1.4426950408889634f;
    c2 = 2.0f * c2 / p.softcap;
  }
  vec8 qf[QT][KS];
  int rlim[QT];  // last visible key of the lane's rows (causal; Nk - 1 otherwise and for padding rows)
  int rlo[QT];   // window mode: their first visible key (0 for padding rows)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int r = 16 * qt + c;
    const int gi = r / p.Nq, iq = r - gi * p.Nq;
    const bool valid = r < R;
    rlim[qt] = (CAUSAL && valid) ? iq + cup : Nk - 1;
    rlo[qt] = (WINDOW && valid) ? iq + cl : 0;
    const long long qoff = (long long)b * p.q_bs + (long long)(hkv * G + gi) * p.q_hs + (long long)iq * D;
    const elem *qp = (const elem *)p.q + qoff;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4 t = {0u, 0u, 0u, 0u};
      if (KV8 && p.q8) {  // e4m3 queries (8 bytes), widened exactly; else (an e4m3 KV cache under 16-bit queries) as the 16-bit path
        if (valid) {
          const u32x2 t8 = *reinterpret_cast<const u32x2 *>((const char *)p.q + qoff + 32 * ks + 8 * g);
          const unsigned w0 = t8[0], w1 = t8[1];
          t = widen8(w0, w1);
        }
      } else {
        if (valid) t = *reinterpret_cast<const u32x4 *>(qp + 32 * ks + 8 * g);
      }
      qf[qt][ks] = __builtin_bit_cast(vec8, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[qt][ks][j] = (elem)((float)qf[qt][ks][j] * c2);
    }
  }

  // ---- per-lane LDS read addresses (images of fa_mfma16_kernel.hip)
  const int kx = (D == 64) ? ((c >> 1) & 7) : c;
  const lds_char *kptr[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) kptr[ks] = Kbuf + c * RB + (((4 * ks + g) ^ kx) << 4);
  const int vq = c >> 2, vp = c & 3, vrow = 4 * g + vq;
  const int vx = (D == 64) ? (((vrow >> 1) & 3) << 1) : ((vrow & 7) << 1);
  const lds_char *vptr[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) vptr[dt] = Vbuf + vrow * RB + ((((2 * dt) ^ vx) + (vp >> 1)) << 4) + 8 * (vp & 1);

  // ---- LDS-DMA: this wave moves every piece of a tile; piece j holds rows RPP j .. RPP j + RPP - 1, the chunk swizzle sits on the
  // source address: K chunk ^ ((row >> 1) & 7) (head_dim 64) / row & 15 (128), V chunk ^ (((row >> 1) & 3) << 1) / ((row & 7) << 1) --
  // the part of the swizzle that depends on the piece is a compile-time XOR of the byte offset
  const int drow = lane / CPR, dpc = lane % CPR;
  const unsigned dma_k0 = (unsigned)(drow * RB + ((dpc ^ ((D == 64) ? ((drow >> 1) & 7) : (drow & 15))) << 4));
  const unsigned dma_v0 = (unsigned)(drow * RB + ((dpc ^ ((D == 64) ? (((drow >> 1) & 3) << 1) : ((drow & 7) << 1))) << 4));

  // ---- PAGED: pg[] holds the table entries of the next tile to stage (its pages: max(1, 64 / P), at most four), loaded one tile
  // ahead; tile_pages() turns them into wave-uniform page offsets and descriptor ranges, page_rsrc() gives the descriptors of the
  // page that holds key kj of the tile and the byte offset of that key's slot in it
  int lp = 0, pg[4] = {-1, -1, -1, -1};
  long long poff[4] = {0, 0, 0, 0};  // elements, page base + key head of entry k
  unsigned prec[4] = {0u, 0u, 0u, 0u}, rsb = 0u;  // descriptor range of entry k (bytes); row stride in bytes
  auto fetch_pages = [&](int t) __attribute__((always_inline)) {
    if constexpr (PAGED) {
      const int *tbl = p.block_table + (long long)b * p.bt_stride;
      const int i0 = (t * BN) >> lp, npg = max(1, BN >> lp);
#pragma unroll
      for (int k = 0; k < 4; ++k) pg[k] = k < npg ? tbl[min(i0 + k, p.max_pages - 1)] : -1;  // (never past the row's max_pages entries)
    }
  };
  auto tile_pages = [&](int t) __attribute__((always_inline)) {
    if constexpr (PAGED) {
      const int P = 1 << lp, key0 = (t * BN) & -P;  // first key of the tile's first page
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int page = __builtin_amdgcn_readfirstlane(pg[k]);
        const int nv = min(Nk - (key0 + k * P), P);  // valid rows of the page
        const bool ok = nv > 0 && (unsigned)page < (unsigned)p.num_pages;  // an index outside the pool reads as zeros
        poff[k] = ok ? (long long)page * p.page_stride + (long long)hkv * p.kv_hs : 0;
        prec[k] = ok ? (unsigned)(nv - 1) * rsb + D * EB : 0u;
      }
    }
  };
  auto page_rsrc = [&](int t, int kj, __amdgpu_buffer_rsrc_t &rkp, __amdgpu_buffer_rsrc_t &rvp) __attribute__((always_inline)) -> unsigned {
    // entry kj >> lp: kj is a compile-time constant, so this selects between (at most) three fixed entries: lp = 4, 5, >= 6
    const int e4 = (kj >> 4) & 3, e5 = (kj >> 5) & 3;
    const long long off = lp == 4 ? poff[e4] : lp == 5 ? poff[e5] : poff[0];
    const unsigned nrec = lp == 4 ? prec[e4] : lp == 5 ? prec[e5] : prec[0];
    rkp = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.k + off * EB), 0, nrec, 0x00020000);
    rvp = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p.v + off * EB), 0, nrec, 0x00020000);
    return (unsigned)((t * BN + kj) & ((1 << lp) - 1)) * rsb;
  };
  unsigned pdma_row = 0u;  // PAGED: drow rows at the pool's row stride
  if constexpr (PAGED) {
    lp = p.lp;
    rsb = (unsigned)p.row_stride * EB;
    pdma_row = (unsigned)drow * rsb;
  }
  auto stage_dma_paged = [&](int t, int buf) __attribute__((always_inline)) {
    tile_pages(t);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const unsigned kxo = (D == 64) ? (unsigned)((j & 1) << 6) : (unsigned)((j & 3) << 6);
      const unsigned vxo = (D == 64) ? 0u : (unsigned)((j & 1) << 7);
      __amdgpu_buffer_rsrc_t rkp, rvp;
      const unsigned so = page_rsrc(t, j * RPP, rkp, rvp) + pdma_row;  // (the whole offset in voffset: inside the range check)
      const unsigned lk = (unsigned)(__UINTPTR_TYPE__)Kbuf + buf * TILE + j * 1024;
      const unsigned lv = (unsigned)(__UINTPTR_TYPE__)Vbuf + buf * TILE + j * 1024;
      const unsigned ko = so + ((dma_k0 % RB) ^ kxo), vo = so + ((dma_v0 % RB) ^ vxo);
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lk), "v"(ko), "s"(rkp) : "memory");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lv), "v"(vo), "s"(rvp) : "memory");
    }
    fetch_pages(t + 1);
  };
  auto stage_dma = [&](int t, int buf) __attribute__((always_inline)) {
    if constexpr (PAGED) {
      stage_dma_paged(t, buf);
      return;
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const unsigned kxo = (D == 64) ? (unsigned)((j & 1) << 6) : (unsigned)((j & 3) << 6);  // ((row >> 1) & 7) gains 4 on odd pieces / (row & 15) gains 4 (j & 3)
      const unsigned vxo = (D == 64) ? 0u : (unsigned)((j & 1) << 7);                        // head_dim 128: (row & 7) gains 4 on odd pieces -> chunk ^ 8
      const unsigned soff = (unsigned)t * TILE + j * 1024;
      const unsigned lk = (unsigned)(__UINTPTR_TYPE__)Kbuf + buf * TILE + j * 1024;
      const unsigned lv = (unsigned)(__UINTPTR_TYPE__)Vbuf + buf * TILE + j * 1024;
      const unsigned ko = dma_k0 ^ kxo, vo = dma_v0 ^ vxo;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lk), "v"(ko), "s"(rk), "s"(soff) : "memory");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lv), "v"(vo), "s"(rv), "s"(soff) : "memory");
    }
  };

  // ---- KV8 staging: tile t = BN x D bytes per operand = NL loads of 16 e4m3 per lane; load i covers row (64 i + lane) 16 / D, bf16
  // chunks 2 ((lane 16 / 8) % CPR') .. +1 -- written into the images above with their swizzles
  constexpr int NL = RS ? D * EB / 16 : 1;
  // DEPTH tiles wait in registers (one; the knob allows two at head_dim 64)
  constexpr int DEPTH = (KV8 && D == 64) ? FA_DECODE_KV8_DEPTH : 1;
  static_assert(EB == 1 || EB == 2, "");
  u32x4 kraw[DEPTH][NL], vraw[DEPTH][NL];
  auto load_raw = [&](int t, auto slotc) __attribute__((always_inline)) {
    constexpr int slot = decltype(slotc)::value;
    if constexpr (PAGED) {  // load i: rows RPL i .. RPL i + RPL - 1 of the tile (<= 16: one page), lane -> row lane / LPR, byte 16 (lane % LPR)
      static_assert(DEPTH == 1, "the paged path stages one tile ahead");
      constexpr int LPR = D * EB / 16, RPL = 64 / LPR;
      tile_pages(t);
      const unsigned lo = (unsigned)(lane / LPR) * rsb + (unsigned)(lane % LPR) * 16;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        __amdgpu_buffer_rsrc_t rkp, rvp;
        const unsigned off = page_rsrc(t, i * RPL, rkp, rvp) + lo;
        kraw[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(rkp, off, 0, 0);
        vraw[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(rvp, off, 0, 0);
      }
      fetch_pages(t + 1);
      return;
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const unsigned off = (unsigned)t * (BN * D * EB) + (unsigned)(i * 64 + lane) * 16;
      kraw[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0);
      vraw[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(rv, off, 0, 0);
    }
  };
  auto write_tile = [&](auto slotc) {  // registers of slot -> the (one) LDS image
    constexpr int slot = decltype(slotc)::value;
    constexpr int buf = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e0 = (i * 64 + lane) * (16 / EB), row = e0 / D, ch = (e0 % D) / 8;  // (e4m3: ch even, chunks ch and ch + 1)
      const int ksw = (D == 64) ? ((row >> 1) & 7) : (row & 15);
      const int vsw = (D == 64) ? (((row >> 1) & 3) << 1) : ((row & 7) << 1);
      if constexpr (KV8) {
        const unsigned k0 = kraw[slot][i][0], k1 = kraw[slot][i][1], k2 = kraw[slot][i][2], k3 = kraw[slot][i][3];
        const unsigned v0 = vraw[slot][i][0], v1 = vraw[slot][i][1], v2 = vraw[slot][i][2], v3 = vraw[slot][i][3];
        lds_write_b128(Kbuf + buf * TILE + row * RB + ((ch ^ ksw) << 4), widen8(k0, k1));
        lds_write_b128(Kbuf + buf * TILE + row * RB + (((ch + 1) ^ ksw) << 4), widen8(k2, k3));
        lds_write_b128(Vbuf + buf * TILE + row * RB + ((ch ^ vsw) << 4), widen8(v0, v1));
        lds_write_b128(Vbuf + buf * TILE + row * RB + (((ch + 1) ^ vsw) << 4), widen8(v2, v3));
      } else {
        lds_write_b128(Kbuf + buf * TILE + row * RB + ((ch ^ ksw) << 4), kraw[slot][i]);
        lds_write_b128(Vbuf + buf * TILE + row * RB + ((ch ^ vsw) << 4), vraw[slot][i]);
      }
    }
  };

  f32x4 oacc[DT][QT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int i = 0; i < 4; ++i) oacc[dt][qt][i] = 0.0f;
  float m[QT], l[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m[qt] = -INFINITY;
    l[qt] = 0.0f;
  }

  // one tile: (KV8) the tile is in the LDS image, register slot `slot` -- which held it -- is free for tile t + DEPTH; slot + 1 holds tile t + 1
  auto step = [&](auto slotc, const int t) {
      constexpr int slot = decltype(slotc)::value;
      // (KV8: ONE LDS image -- the next tile waits in registers and overwrites it behind this tile's arithmetic -- so an item holds half
      // the LDS and twice as many items, i.e. loads, are in flight per CU: the path is bound by tiles in flight, not by bytes)
      const int buf = RS ? 0 : ((t - t0) & 1);
      if constexpr (RS) {
        if (t + DEPTH < t1) load_raw(t + DEPTH, slotc);  // flies under this and the next tile's arithmetic; widened and written behind it
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile t has landed (this wave issued every piece of it: no barrier needed)
        if (t + 1 < t1) stage_dma(t + 1, buf ^ 1);         // the next tile streams under this tile's arithmetic
      }
      const int kv0 = t * BN;
      const unsigned bo = (unsigned)(buf * TILE);
      // ---- S^T = K.Q~^T (log2 units): s[kt][qt][i] = S[row 16qt + c][key kv0 + 16kt + 4g + i]
      f32x4 sc[KT][QT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[kt][qt][i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const vec8 kf = __builtin_bit_cast(vec8, lds_read_b128(kptr[ks] + bo + kt * 16 * RB));
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) sc[kt][qt] = M::mfma(kf, qf[qt][ks], sc[kt][qt]);
        }
      }
      if constexpr (SOFTCAP) {  // the capped scores, log2 units
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[kt][qt][i] = tanh_from_exp2_arg(sc[kt][qt][i]) * capc;
          // (32 packed rows at head_dim 128: one 16-key tile's temporaries at a time, or the kernel no longer fits two waves per SIMD)
          if (D == 128 && QT == 2) __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ---- mask: key > the row's limit (causal, bottom-right aligned) or key >= Nk
      if (kv0 + BN > Nk || (CAUSAL && kv0 + BN - 1 > cup) || (WINDOW && kv0 < p.Nq - 1 + cl)) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          const int lim = min(rlim[qt], Nk - 1) - kv0 - 4 * g;
          const int llo = rlo[qt] - kv0 - 4 * g;  // (window mode)
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[kt][qt][i] = (16 * kt + i > lim || (WINDOW && 16 * kt + i < llo)) ? -INFINITY : sc[kt][qt][i];
        }
      }
      // ---- exact online softmax (a row whose keys are all masked so far keeps m = -inf, l = 0: the guard avoids inf - inf)
      vec8 pf[2][QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        float mx = sc[0][qt][0];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) mx = fmaxf(mx, sc[kt][qt][i]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m[qt], mx);
        const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m[qt] - m_use);
        m[qt] = m_new;
        float ls = 0.0f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[kt][qt][i] = __builtin_amdgcn_exp2f(sc[kt][qt][i] - m_use);
            ls += sc[kt][qt][i];
          }
        l[qt] = l[qt] * alpha + ls;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) oacc[dt][qt][i] *= alpha;
#pragma unroll
        for (int kp = 0; kp < 2; ++kp)
#pragma unroll
          for (int j = 0; j < 8; ++j) pf[kp][qt][j] = (elem)sc[2 * kp + (j >> 2)][qt][j & 3];
      }
      // ---- O^T += V^T.P^T
#pragma unroll
      for (int kp = 0; kp < 2; ++kp)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const lds_char *vb = vptr[dt] + bo + (32 * kp) * RB;
          const s16x4 lo = lds_read_tr16(vb), hi = lds_read_tr16(vb + 16 * RB);
          const s16x8 v8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) oacc[dt][qt] = M::mfma(__builtin_bit_cast(vec8, v8), pf[kp][qt], oacc[dt][qt]);
        }
      if constexpr (RS) {
        if (t + 1 < t1) write_tile(std::integral_constant<int, (slot + 1) % DEPTH>{});  // (one wave, LDS operations in order: this tile's reads are behind us)
      }
  };
  if (t0 < t1) {
    fetch_pages(t0);
    if constexpr (RS) {
      load_raw(t0, std::integral_constant<int, 0>{});
      if constexpr (DEPTH == 2) {
        if (t0 + 1 < t1) load_raw(t0 + 1, std::integral_constant<int, 1>{});
      }
      write_tile(std::integral_constant<int, 0>{});
    } else {
      stage_dma(t0, 0);
    }
    for (int t = t0; t < t1; t += DEPTH) {
      step(std::integral_constant<int, 0>{}, t);
      if constexpr (DEPTH == 2) {
        if (t + 1 < t1) step(std::integral_constant<int, 1>{}, t + 1);
      }
    }
  }

  // ---- partial results -> workspace: [16 QT][D] O (unnormalised, fp32), then [16 QT][2] (m, l)
  float *wo = p.ws + (size_t)item * (16 * QT) * (D + 2);
  float *wm = wo + (16 * QT) * D;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    float lt = l[qt];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const int row = 16 * qt + c;
    if (g == 0) {
      wm[2 * row] = m[qt];
      wm[2 * row + 1] = lt;
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4 *>(wo + row * D + 16 * dt + 4 * g) = oacc[dt][qt];
  }
}

// one wave per output row (b, hq, iq). The S partials of a row are independent reads: lanes take the splits' (m, l) pairs in
// parallel (wave reductions for M and l), the weights 2^(m_s - M) go through LDS, and thread d folds element d (and d + 64) of the S
// partial rows with eight loads in flight (a serial loop over the splits -- one dependent ~0.4 us read each -- cost more than the
// streaming kernel itself: 47 us at S = 128).
// PAGED: a row that saw no visible key at all (L_b = 0, or causal with i + L_b < Nq) has lsum = 0: O = 0 exactly and LSE = -inf
template <typename Tag, int D, int QT, bool PAGED = false>
__global__ __launch_bounds__(64) void decode_combine_kernel(DecodeParams p) {
  using elem = typename MD16<Tag>::elem;
  __shared__ float wgt[256];
  const int lane = threadIdx.x;
  const int row_id = blockIdx.x;  // (b * Hq + hq) * Nq + iq
  const int iq = row_id % p.Nq, bh = row_id / p.Nq;
  const int hq = bh % p.Hq, b = bh / p.Hq;
  const int G = p.Hq / p.Hkv, hkv = hq / G, gi = hq - hkv * G;
  const int r = gi * p.Nq + iq;
  const int S = p.S;  // <= 256
  constexpr int IST = (16 * QT) * (D + 2);
  const float *w0 = p.ws + (size_t)(b * p.Hkv + hkv) * S * IST;
  const float *ml = w0 + (16 * QT) * D + 2 * r;
  float ms[4], ls[4];
  float M = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int s = lane + 64 * e;
    ms[e] = s < S ? ml[(size_t)s * IST] : -INFINITY;
    ls[e] = s < S ? ml[(size_t)s * IST + 1] : 0.0f;
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
  float acc[D / 64];
#pragma unroll
  for (int e = 0; e < D / 64; ++e) acc[e] = 0.0f;
  const float *wr = w0 + r * D + lane;
  int s = 0;
  for (; s + 8 <= S; s += 8) {
    float x[8][D / 64];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int e = 0; e < D / 64; ++e) x[u][e] = wr[(size_t)(s + u) * IST + 64 * e];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int e = 0; e < D / 64; ++e) acc[e] += x[u][e] * wgt[s + u];
  }
  for (; s < S; ++s)
#pragma unroll
    for (int e = 0; e < D / 64; ++e) acc[e] += wr[(size_t)s * IST + 64 * e] * wgt[s];
  const float inv = (PAGED && !(lsum > 0.0f)) ? 0.0f : 1.0f / lsum;
  elem *op = (elem *)p.o + (long long)b * p.q_bs + (long long)hq * p.q_hs + (long long)iq * D;
#pragma unroll
  for (int e = 0; e < D / 64; ++e) op[lane + 64 * e] = (elem)(acc[e] * inv);
  if (p.lse != nullptr && lane == 0) p.lse[row_id] = (PAGED && !(lsum > 0.0f)) ? -INFINITY : (M + log2f(lsum)) * 0.6931471805599453f;
}

// fa_fwd_decode_paged_sink: decode_combine_kernel<.., PAGED = true> with the row's sink logit (sinks[hq], natural-log units) folded in
// behind the reduction of the splits' (M, lsum): s2 = sink . log2(e), Mm = max(M, s2), lsum' = lsum 2^(M - Mm) + 2^(s2 - Mm), O = acc
// 2^(M - Mm) / lsum', LSE = (Mm + log2 lsum') ln 2. Neither exponent is positive: nothing overflows; a sink whose 2^(s2 - M) underflows
// leaves Mm = M, a factor of exactly 1 and lsum' = lsum + 0, the bits of the plain combine. A row whose splits saw no visible key
// (lsum = 0) has the sink alone in its softmax: O = 0 exactly, LSE = sinks[hq] bit for bit.
template <typename Tag, int D, int QT>
__global__ __launch_bounds__(64) void decode_combine_sink_kernel(CombineSinkParams p) {
  using elem = typename MD16<Tag>::elem;
  __shared__ float wgt[256];
  const int lane = threadIdx.x;
  const int row_id = blockIdx.x;  // (b * Hq + hq) * Nq + iq
  const int iq = row_id % p.Nq, bh = row_id / p.Nq;
  const int hq = bh % p.Hq, b = bh / p.Hq;
  const int G = p.Hq / p.Hkv, hkv = hq / G, gi = hq - hkv * G;
  const int r = gi * p.Nq + iq;
  const int S = p.S;  // <= 256
  const float sink = p.sinks[hq];
  constexpr int IST = (16 * QT) * (D + 2);
  const float *w0 = p.ws + (size_t)(b * p.Hkv + hkv) * S * IST;
  const float *ml = w0 + (16 * QT) * D + 2 * r;
  float ms[4], ls[4];
  float M = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int s = lane + 64 * e;
    ms[e] = s < S ? ml[(size_t)s * IST] : -INFINITY;
    ls[e] = s < S ? ml[(size_t)s * IST + 1] : 0.0f;
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
  float acc[D / 64];
#pragma unroll
  for (int e = 0; e < D / 64; ++e) acc[e] = 0.0f;
  const float *wr = w0 + r * D + lane;
  int s = 0;
  for (; s + 8 <= S; s += 8) {
    float x[8][D / 64];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int e = 0; e < D / 64; ++e) x[u][e] = wr[(size_t)(s + u) * IST + 64 * e];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int e = 0; e < D / 64; ++e) acc[e] += x[u][e] * wgt[s + u];
  }
  for (; s < S; ++s)
#pragma unroll
    for (int e = 0; e < D / 64; ++e) acc[e] += wr[(size_t)s * IST + 64 * e] * wgt[s];
  const bool dead = !(lsum > 0.0f);  // (then M = -inf: no exponent is formed from it)
  const float s2 = sink * 1.4426950408889634f;
  const float Mm = dead ? s2 : fmaxf(M, s2);
  const float ow = dead ? 0.0f : __builtin_amdgcn_exp2f(M - Mm);
  const float lt = lsum * ow + __builtin_amdgcn_exp2f(s2 - Mm);
  const float inv = ow * (1.0f / lt);
  elem *op = (elem *)p.o + (long long)b * p.q_bs + (long long)hq * p.q_hs + (long long)iq * D;
#pragma unroll
  for (int e = 0; e < D / 64; ++e) op[lane + 64 * e] = (elem)(acc[e] * inv);
  if (p.lse != nullptr && lane == 0) p.lse[row_id] = dead ? sink : (Mm + log2f(lt)) * 0.6931471805599453f;
}

// ---------------------------------------------------------------------------
bool decode_supported(int dtype, int D) {
  return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16 || dtype == FA_DTYPE_FP8_E4M3) && (D == 64 || D == 128);
}

// splits per (batch, key head): one round of the chip's item slots (an item keeps one tile in flight: 4-5 / 2 items of 16 / 32 KiB per
// CU are what fills the memory pipe), but at least FA_DECODE_MIN_TILES 64-key tiles per item so that its prologue amortises
#ifndef FA_DECODE_MIN_TILES
#define FA_DECODE_MIN_TILES 4  // (2: -20 % at 8 key heads x 16384 keys; 8: +9 % at 32 x 16384 but -25 % at 4096; profiles/r04/decode_ab_split_heuristic.log)
#endif
#ifndef FA_DECODE_ROUNDS
#define FA_DECODE_ROUNDS 1
#endif
int decode_splits(int B, int Hkv, int Nk, int D, int kv8) {
  const int nT = (Nk + BN - 1) / BN;
  const int per_cu = ((D == 64) ? 5 : 2) * ((kv8 || FA_DECODE_REGSTAGE) ? 2 : 1);  // items resident per CU (32 / 64 KiB of LDS each; e4m3 inputs: one image, half)
  const long long want = (long long)FA_DECODE_ROUNDS * 256 * per_cu;
  long long S = (want + (long long)B * Hkv - 1) / ((long long)B * Hkv);
  S = std::min<long long>(S, std::max(1, nT / FA_DECODE_MIN_TILES));
  return (int)std::max<long long>(1, std::min<long long>(S, 256));
}

long long decode_workspace_bytes(int B, int Hq, int Hkv, int Nq, int Nk, int D) {
  const int R = (Hq / Hkv) * Nq, QT = (R + 15) / 16;
  // (sized for the larger of the two split counts -- e4m3 inputs run twice the items -- so that one workspace serves every dtype)
  return (long long)B * Hkv * std::max(decode_splits(B, Hkv, Nk, D, 0), decode_splits(B, Hkv, Nk, D, 1)) * (16 * QT) * (D + 2) * 4;
}

// One call: the partial kernel over the B . Hkv . S items, then the combine kernel over the output rows, on the same stream. PRM picks
// the mode: DecodeParams (dense: the plain combine kernel), DecodePagedParams, DecodeWindowParams (paged combine kernel: empty splits,
// rows with no visible key; window mode has the causal partial kernel only).
template <typename PRM, typename KP, typename KC>
static hipError_t launch_decode_pair(KP partial, KC combine, size_t smem, const PRM &p, hipStream_t s) {
  (void)hipGetLastError();
  if (smem > 48 * 1024) { hipError_t e = set_dyn_lds_once((const void *)partial, (int)smem); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(partial, dim3(p.B * p.Hkv * p.S), dim3(64), smem, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(combine, dim3(p.B * p.Hq * p.Nq), dim3(64), 0, s, (const DecodeParams &)p);
  return hipGetLastError();
}

// fa_fwd_decode_paged_sink: the pair above with the sink combine in the second launch
template <typename Tag, int D, int QT, bool KV8>
static hipError_t launch_decode_sink_q(const DecodeWindowParams &p, const float *sinks, hipStream_t s) {
  auto partial = decode_partial_kernel<Tag, D, QT, true, KV8, DecodeWindowParams>;
  constexpr size_t smem = decode_lds_bytes<D, KV8>();
  (void)hipGetLastError();
  if (smem > 48 * 1024) { hipError_t e = set_dyn_lds_once((const void *)partial, (int)smem); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(partial, dim3(p.B * p.Hkv * p.S), dim3(64), smem, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  CombineSinkParams c;
  (DecodeParams &)c = (const DecodeParams &)p;
  c.sinks = sinks;
  hipLaunchKernelGGL((decode_combine_sink_kernel<Tag, D, QT>), dim3(p.B * p.Hq * p.Nq), dim3(64), 0, s, c);
  return hipGetLastError();
}

template <typename Tag, int D, int QT, bool KV8, typename PRM>
static hipError_t launch_decode_q(const PRM &p, hipStream_t s) {
  constexpr bool PAGED = std::is_base_of<DecodePagedParams, PRM>::value;
  constexpr bool WINDOW = std::is_same<PRM, DecodeWindowParams>::value || std::is_same<PRM, DecodeSoftcapParams>::value;
  auto combine = decode_combine_kernel<Tag, D, QT, PAGED>;
  if constexpr (!WINDOW) {
    if (!p.is_causal) return launch_decode_pair(decode_partial_kernel<Tag, D, QT, false, KV8, PRM>, combine, decode_lds_bytes<D, KV8>(), p, s);
  }
  return launch_decode_pair(decode_partial_kernel<Tag, D, QT, true, KV8, PRM>, combine, decode_lds_bytes<D, KV8>(), p, s);
}

// dtype: of the queries (and of K / V unless kv8); kv8: K and V are e4m3 (dtype FP8: so are the queries; BF16: an e4m3 cache under
// bf16 queries -- the arithmetic, and the output, are bf16 either way)
template <typename PRM>
static hipError_t dispatch_decode(const PRM &p0, int D, int dtype, int kv8, hipStream_t s) {
  PRM p = p0;
  p.q8 = (dtype == FA_DTYPE_FP8_E4M3);
  const int R = (p.Hq / p.Hkv) * p.Nq, QT = (R + 15) / 16;
  auto go = [&](auto tag, auto k8) {
    return with_dim<64, 128>(D, [&](auto d) {
      return QT == 1 ? launch_decode_q<decltype(tag), d(), 1, k8()>(p, s) : launch_decode_q<decltype(tag), d(), 2, k8()>(p, s);
    });
  };
  if (kv8 || dtype == FA_DTYPE_FP8_E4M3) return go(BF16{}, std::true_type{});
  return with_tag(dtype, [&](auto tag) { return go(tag, std::false_type{}); });
}

hipError_t launch_decode(const DecodeParams &p, int D, int dtype, int kv8, hipStream_t s) { return dispatch_decode(p, D, dtype, kv8, s); }
hipError_t launch_decode_paged(const DecodePagedParams &p, int D, int dtype, int kv8, hipStream_t s) { return dispatch_decode(p, D, dtype, kv8, s); }
hipError_t launch_decode_paged_window(const DecodeWindowParams &p, int D, int dtype, int kv8, hipStream_t s) { return dispatch_decode(p, D, dtype, kv8, s); }
hipError_t launch_decode_paged_softcap(const DecodeSoftcapParams &p, int D, int dtype, int kv8, hipStream_t s) { return dispatch_decode(p, D, dtype, kv8, s); }
hipError_t launch_decode_paged_sink(const DecodeWindowParams &p0, const float *sinks, int D, int dtype, int kv8, hipStream_t s) {
  DecodeWindowParams p = p0;
  p.q8 = (dtype == FA_DTYPE_FP8_E4M3);
  const int R = (p.Hq / p.Hkv) * p.Nq, QT = (R + 15) / 16;
  auto go = [&](auto tag, auto k8) {
    return with_dim<64, 128>(D, [&](auto d) {
      return QT == 1 ? launch_decode_sink_q<decltype(tag), d(), 1, k8()>(p, sinks, s) : launch_decode_sink_q<decltype(tag), d(), 2, k8()>(p, sinks, s);
    });
  };
  if (kv8 || dtype == FA_DTYPE_FP8_E4M3) return go(BF16{}, std::true_type{});
  return with_tag(dtype, [&](auto tag) { return go(tag, std::false_type{}); });
}

// fa_kv_append_paged: new K / V rows -> their slots of the page pools, a byte copy (BYTES = element size). One 16-byte chunk per lane and
// step: a workgroup takes APPEND_ROWS new rows of one (sequence, key head), K and V alike. The sequence lookup and its clamps are the
// varlen kernels' (entries to [0, total], a non-increasing pair is length 0, n_b <= max_seqlen_new); token i of sequence b goes to key
// position seqlens[b] - n_b + i -- seqlens is the length AFTER the append -- and is skipped when that position is below 0, at or above
// the capacity, or on a table entry outside [0, num_pages). Nothing else is written. Plain vector loads and stores.
template <int BYTES>
__global__ __launch_bounds__(256) void kv_append_paged_kernel(AppendPagedParams p) {
  const int nblk = (p.max_new + APPEND_ROWS - 1) / APPEND_ROWS;
  const int b = (int)blockIdx.x / nblk, rb = (int)blockIdx.x - b * nblk, hk = blockIdx.y;
  const int s0 = min(max(p.cu_new[b], 0), p.total_new), e0 = min(max(p.cu_new[b + 1], 0), p.total_new);
  const int n = min(max(e0 - s0, 0), p.max_new);
  const long long first = (long long)p.seqlens[b] - n;  // key position of the sequence's first new token
  const long long cap = (long long)p.max_pages << p.lp;
  const int cpr = p.D * BYTES / 16;  // 16-byte chunks per row
  const int *tbl = p.block_table + (long long)b * p.bt_stride;
  for (int idx = threadIdx.x; idx < APPEND_ROWS * cpr; idx += 256) {
    const int i = rb * APPEND_ROWS + idx / cpr, c = idx % cpr;
    if (i >= n) continue;
    const long long pos = first + i;
    if (pos < 0 || pos >= cap) continue;
    const int page = tbl[(int)(pos >> p.lp)];
    if ((unsigned)page >= (unsigned)p.num_pages) continue;
    const long long src = ((long long)(s0 + i) * p.new_rs + (long long)hk * p.new_hs) * BYTES + 16 * c;
    const long long dst = ((long long)page * p.page_stride + (long long)hk * p.head_stride + (pos & ((1 << p.lp) - 1)) * p.row_stride) * BYTES + 16 * c;
    *reinterpret_cast<u32x4 *>((char *)p.k_pages + dst) = *reinterpret_cast<const u32x4 *>((const char *)p.k_new + src);
    *reinterpret_cast<u32x4 *>((char *)p.v_pages + dst) = *reinterpret_cast<const u32x4 *>((const char *)p.v_new + src);
  }
}

// fa_kv_append_paged_quant: the same placement -- sequence lookup, clamps, skipped positions, grid: the lines of the kernel above -- with
// 16-bit new rows (T = _Float16 / __bf16) quantised into e4m3 pools. A lane takes 16 elements: two 16-byte loads, one 16-byte store.
// byte = e4m3_rne(clamp(fp32(x) * mul, -448, 448)): ONE fp32 multiply, the clamp BEFORE the conversion (v_cvt_pk_fp8_f32 gives NaN above
// 448 instead of saturating, see fa_fp8_kernel.hip), the conversion rounds to nearest even, subnormals included, and keeps the sign of -0.
template <typename T>
__device__ __forceinline__ u32x4 quant16_e4m3(u32x4 a, u32x4 b, float mul) {
  u32x4 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned w0 = j < 2 ? a[2 * j] : b[2 * j - 4], w1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned short h = (unsigned short)((e < 2 ? w0 : w1) >> (16 * (e & 1)));
      f[e] = fminf(fmaxf((float)__builtin_bit_cast(T, h) * mul, -448.0f), 448.0f);
    }
    int w;
    asm volatile("" : "=v"(w));  // (the first conversion keeps the other half of its destination: start from an undefined register)
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
    out[j] = (unsigned)w;
  }
  return out;
}
template <typename T>
__global__ __launch_bounds__(256) void kv_quant_append_paged_kernel(AppendPagedParams p, float k_mul, float v_mul) {
  const int nblk = (p.max_new + APPEND_ROWS - 1) / APPEND_ROWS;
  const int b = (int)blockIdx.x / nblk, rb = (int)blockIdx.x - b * nblk, hk = blockIdx.y;
  const int s0 = min(max(p.cu_new[b], 0), p.total_new), e0 = min(max(p.cu_new[b + 1], 0), p.total_new);
  const int n = min(max(e0 - s0, 0), p.max_new);
  const long long first = (long long)p.seqlens[b] - n;  // key position of the sequence's first new token
  const long long cap = (long long)p.max_pages << p.lp;
  const int cpr = p.D / 16;  // 16-byte chunks per row of the POOL (16 elements: 32 bytes of the new row)
  const int *tbl = p.block_table + (long long)b * p.bt_stride;
  for (int idx = threadIdx.x; idx < APPEND_ROWS * cpr; idx += 256) {
    const int i = rb * APPEND_ROWS + idx / cpr, c = idx % cpr;
    if (i >= n) continue;
    const long long pos = first + i;
    if (pos < 0 || pos >= cap) continue;
    const int page = tbl[(int)(pos >> p.lp)];
    if ((unsigned)page >= (unsigned)p.num_pages) continue;
    const long long src = ((long long)(s0 + i) * p.new_rs + (long long)hk * p.new_hs) * 2 + 32 * c;
    const long long dst = (long long)page * p.page_stride + (long long)hk * p.head_stride + (pos & ((1 << p.lp) - 1)) * p.row_stride + 16 * c;
    const u32x4 k0 = *reinterpret_cast<const u32x4 *>((const char *)p.k_new + src), k1 = *reinterpret_cast<const u32x4 *>((const char *)p.k_new + src + 16);
    const u32x4 v0 = *reinterpret_cast<const u32x4 *>((const char *)p.v_new + src), v1 = *reinterpret_cast<const u32x4 *>((const char *)p.v_new + src + 16);
    *reinterpret_cast<u32x4 *>((char *)p.k_pages + dst) = quant16_e4m3<T>(k0, k1, k_mul);
    *reinterpret_cast<u32x4 *>((char *)p.v_pages + dst) = quant16_e4m3<T>(v0, v1, v_mul);
  }
}

hipError_t launch_kv_append_paged_quant(const AppendPagedParams &p, int new_dtype, float k_mul, float v_mul, hipStream_t s) {
  const int nblk = (p.max_new + APPEND_ROWS - 1) / APPEND_ROWS;
  (void)hipGetLastError();
  if (new_dtype == FA_DTYPE_F16) hipLaunchKernelGGL(kv_quant_append_paged_kernel<_Float16>, dim3(p.B * nblk, p.Hkv), dim3(256), 0, s, p, k_mul, v_mul);
  else hipLaunchKernelGGL(kv_quant_append_paged_kernel<__bf16>, dim3(p.B * nblk, p.Hkv), dim3(256), 0, s, p, k_mul, v_mul);
  return hipGetLastError();
}

hipError_t launch_kv_append_paged(const AppendPagedParams &p, int elem_bytes, hipStream_t s) {
  const int nblk = (p.max_new + APPEND_ROWS - 1) / APPEND_ROWS;
  (void)hipGetLastError();
  if (elem_bytes == 1) hipLaunchKernelGGL(kv_append_paged_kernel<1>, dim3(p.B * nblk, p.Hkv), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(kv_append_paged_kernel<2>, dim3(p.B * nblk, p.Hkv), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace fa
