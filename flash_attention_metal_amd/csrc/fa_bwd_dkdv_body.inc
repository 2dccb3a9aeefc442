// fa_bwd_dkdv_body.inc -- the body of the dK/dV kernels (fa_bwd_body.h says how it is used): included inside
//   template <typename Tag, int D, bool CAUSAL, bool PAD> __global__ void kernel(BwdParams or BwdVarlenParams p)
// with FA_BWD_VARLEN defined to 0 or 1, and FA_BWD_WINDOW (varlen only) to 0 or 1: the window mode, whose parameter block is
// BwdWindowParams; FA_BWD_SOFTCAP (window only) to 0 or 1: the softcap mode, BwdSoftcapParams. Their arms are chosen in the preprocessor,
// so that the text the other kernels compile is the text they had.
// dK, dV: workgroup = 128 keys, wave = 32 keys (key on the lane, queries in the registers)
#if FA_BWD_VARLEN
#define FA_VP p
#else
#define FA_VP bwd_no_varlen_params()
#endif
#define FA_NQ (VARLEN ? LQ : p.N)
#define FA_NK (VARLEN ? LK : p.Nk)
  constexpr bool VARLEN = FA_BWD_VARLEN != 0;
  static_assert(!VARLEN || (!PAD && (D == 64 || D == 128) && FA_BWD_DMA != 0), "varlen mode: head_dim 64 / 128, LDS-DMA staging");
  static_assert(FA_BWD_WINDOW == 0 || (VARLEN && CAUSAL), "window mode: on top of the varlen mode");
  static_assert(FA_BWD_SOFTCAP == 0 || FA_BWD_WINDOW != 0, "softcap mode: on top of the window mode");
  FA_BWD_CONSTS(D, bwd_sub_kv(D));
  FA_BWD_PAD(PAD);
  using M = MT<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;
  lds_char *QU = smem;                // [2] Q tile (BT rows): read by rows for S, transposed for dK
  lds_char *OU = smem + 2 * STILE;    // [2] dO tile: read by rows for dP, transposed for dV
  lds_char *ROWS = smem + 4 * STILE;  // [2][2][BT] floats: -lse*log2e, -delta of the tile's query rows (the chains' initial accumulators)
  static_assert(4 * STILE + 2 * 2 * BT * 4 == bwd_dkdv_lds_bytes(D), "the launcher's LDS size is the Q / dO buffers and the row constants");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // varlen: the staging of the row constants names a thread by its wave (a scalar) and its lane, the mask and the final stores form
  // the key row again from the lane: the thread index, the key row and the lane half are then not held across the loops. At
  // head_dim 128 the tile loop takes all 256 registers and they were spilled around it (the dense kernel parks 32 bytes so).
  // (These few places choose in the preprocessor: a choice inside the statement, though constant, changes the block structure the
  // compiler starts from, and with it the dense kernels' operand order.)
#if FA_BWD_VARLEN
#define FA_TID_LT(n) (wave < (n) / 64)
#define FA_TID_ROW (((wave * 64) & (BT - 1)) + lane)
#define FA_TID4 (wave * 256 + lane * 4)
#else
#define FA_TID_LT(n) (tid < (n))
#define FA_TID_ROW (tid & (BT - 1))
#define FA_TID4 tid * 4
#endif
  const int r = lane & 31, h = lane >> 5;
  // one workgroup per (key block, key/value head): it visits the G = H / Hkv query heads that read this head one after the
  // other, so grouped-query dK / dV are summed in registers (kernels.metal has one head count; G = 1 is its case)
  const int BHK = p.B * p.Hkv, G = p.H / p.Hkv;
  const int kvb = blockIdx.x / BHK;  // ascending: under the causal mask the first key blocks see the most queries
  const int bhk = blockIdx.x % BHK, bi = bhk / p.Hkv, hk = bhk % p.Hkv;
  long long base;  // K, V, dK, dV
  // varlen only:
  int LQ = 0, LK = 0;          // queries and keys of this block's sequence (bi)
  int seq_q = 0;               // its first query token
  unsigned qrb = 0, kvrb = 0;  // row pitch of Q / dO and of K / V in global memory, bytes
  if constexpr (VARLEN) {
    // (the tables are read and clamped as in the dQ kernel; a block past its sequence's last key leaves in front of every barrier)
    const int sq = min(max(FA_VP.cu_q[bi], 0), FA_VP.total_q), eq = min(max(FA_VP.cu_q[bi + 1], 0), FA_VP.total_q);
    const int sk = min(max(FA_VP.cu_k[bi], 0), FA_VP.total_k), ek = min(max(FA_VP.cu_k[bi + 1], 0), FA_VP.total_k);
    LQ = min(max(eq - sq, 0), p.N);
    LK = min(max(ek - sk, 0), p.Nk);
    if (kvb * BM >= LK) return;
    seq_q = sq;
    base = (long long)sk * FA_VP.kv_rs + (long long)hk * p.kv_head_stride;
    qrb = (unsigned)FA_VP.q_rs * 2;
    kvrb = (unsigned)FA_VP.kv_rs * 2;
  } else {
    base = (long long)bi * p.kv_batch_stride + (long long)hk * p.kv_head_stride;
  }
  const int k0 = kvb * BM, kw0 = k0 + wave * WM, krow = kw0 + r;

  // (varlen: a sequence without queries stages nothing -- its keys get dK = dV = 0 -- and its query descriptors are empty)
  const unsigned head_bytes = VARLEN ? (LQ > 0 ? (unsigned)(LQ - 1) * qrb + BRB : 0u) : (unsigned)p.N * GRB;
  const unsigned kv_head_bytes = VARLEN ? (unsigned)(LK - 1) * kvrb + BRB : (unsigned)p.Nk * GRB;
  const int coff = FA_NK - FA_NQ;  // (varlen: may be negative)
  __amdgpu_buffer_rsrc_t rq, rdo;  // of the query head being visited (set_head)
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.k + base), 0, kv_head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.v + base), 0, kv_head_bytes, 0x00020000);

  vec8 kf[BKS], vf[BKS];  // B operands: lane (r,h) holds key row krow, columns 16ks+8h..
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks) {
    kf[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rk, (VARLEN ? (unsigned)krow * kvrb : (unsigned)krow * GRB) + gcol(2 * ks + h), 0, 0));
    vf[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rv, (VARLEN ? (unsigned)krow * kvrb : (unsigned)krow * GRB) + gcol(2 * ks + h), 0, 0));
  }
#if FA_BWD_SOFTCAP
  // softcap (see the dQ body): K~ carries 2 log2(e) scale / softcap; the score chain starts from zero and the row's -lse.log2e is applied
  // behind tanh, from the LDS rows that hold it already
  const float c2 = 2.0f * LOG2E * p.scale / p.softcap;
  const float capc = p.cap_log2;  // (softcap . log2(e) from the host: a kernel argument stays in a scalar register, a product formed here in a vector one)
#else
  const float c2 = p.scale * LOG2E;
#endif

  const int kx = u_swz(r);
  const unsigned qu0 = (unsigned)(__UINTPTR_TYPE__)QU;
  unsigned koff[BKS];  // ABSOLUTE LDS addresses in the current Q buffer (the dO image is 2 STILE further)
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks) koff[ks] = qu0 + r * BRB + (((2 * ks + h) ^ kx) << 4);
  const int g1 = (lane >> 4) & 1, vq = (lane >> 2) & 3, vp = lane & 3;
  unsigned voff[NTV][BDB];
#pragma unroll
  for (int tv = 0; tv < NTV; ++tv)
#pragma unroll
    for (int db = 0; db < BDB; ++db) voff[tv][db] = qu0 + tr_off(tv, db, h, g1, vq, vp);
  // Offsets INCLUDING the current buffer's: with the buffer base added at the point of use hipcc kept a second, per-tile copy
  // of all twelve (base + offset) in registers (seen in the ISA, and spilled under the 168-register cap); they flip in place
  unsigned rowoff = (unsigned)(__UINTPTR_TYPE__)ROWS + 4 * h * 4;
  int flip = STILE, flip_rows = 2 * BT * 4;  // to the other buffer and back
  auto at = [](unsigned a) { return (const lds_char *)(__UINTPTR_TYPE__)a; };
  constexpr int NCH = BT * BCPR / NTHREADS;
  int st_g[NCH], st_r[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = tid + i * NTHREADS, row = c / BCPR, ch = c % BCPR;
    st_g[i] = row * BRB + ch * 16;
    st_r[i] = row * BRB + ((ch ^ u_swz(row)) << 4);
  }
  // query tiles of BT rows; under the causal mask only tiles that reach this block's first key
#if FA_BWD_WINDOW
  // window (all wave-uniform, kept in scalar registers; per-lane limits are formed where they are used): key j is seen by queries
  // j - cu <= i <= j - cl, so the walk is the query tiles [t_begin, nTq) of window_query_range of the block's keys -- a last tile as
  // well as a first. No query sees any key of the block: an empty walk, and the zero accumulators are stored.
  const int cl = coff - p.wl, cu = coff + p.wr;
  int w_lo, w_hi;
  window_query_range(LQ, LK, p.wl, p.wr, k0, k0 + BM - 1, w_lo, w_hi);
  const int nTq = w_lo < w_hi ? (w_hi + BT - 1) / BT : 0;
  const int t_begin = w_lo < w_hi ? w_lo / BT : 0;
#define FA_DEAD_OFF cu
#else
  const int nTq = (FA_NQ + BT - 1) / BT;
  const int t_begin = CAUSAL ? max(k0 - coff, 0) / BT : 0;  // the first query that sees key k0 is k0 - coff
#define FA_DEAD_OFF coff
#endif
  static_assert(2 * BT <= NTHREADS, "one thread per staged row constant");

  u32x4 qst[NCH], ost[NCH];
  // threads 0..BT-1: lse of row tid of the next tile; BT..2BT-1: delta of row tid-BT. The RAW loaded value: any arithmetic on it
  // here makes hipcc wait for it -- vmcnt(0), i.e. for the whole tile's loads issued just before -- at the top of every
  // iteration (seen in the ISA: the memory latency was exposed once per tile). It is scaled / negated in stage_write.
  float rowv = 0.0f;
  // (2 BT threads = whole waves: the choice of array is wave-uniform and stays in scalar registers)
  const float *row_src = nullptr;
  auto set_head = [&](int g) {
    const int hq = hk * G + g;
    long long bq, rows0;  // the head's first element of Q / dO, and of lse / delta
    if constexpr (VARLEN) {
      bq = (long long)seq_q * (long long)(qrb / 2) + (long long)hq * p.head_stride;
      rows0 = (long long)hq * FA_VP.total_q + seq_q;
    } else {
      bq = (long long)bi * p.batch_stride + (long long)hq * p.head_stride;
      rows0 = (long long)(bi * p.H + hq) * p.N;
    }
    rq = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.q + bq), 0, head_bytes, 0x00020000);
    rdo = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.d_o + bq), 0, head_bytes, 0x00020000);
#if FA_BWD_VARLEN
    row_src = (wave < BT / 64 ? p.lse : p.delta) + rows0;
#else
    row_src = (__builtin_amdgcn_readfirstlane(tid) < BT ? p.lse : p.delta) + rows0;
#endif
  };
  constexpr bool DMA = FA_BWD_DMA != 0;
  static_assert(DMA || !PAD, "padded head dims are staged by LDS-DMA only");
  // (varlen: dma_off under the run-time pitch -- the row of the piece times the pitch, plus the swizzled chunk)
  auto dma_off_rs = [&](unsigned pitch) {
    const int row = wave * RPP + lane / BCPR, lc = (lane % BCPR) ^ u_swz(row);
    return (unsigned)row * pitch + ((unsigned)lc << 4);
  };
  const unsigned dvo_ = VARLEN ? dma_off_rs(qrb) : PAD ? dma_off_pad(wave, lane) : dma_off(wave, lane);
  // (head_dim 256: a piece is 2 rows and a wave's pieces are 8 rows apart, half the swizzle's period: odd pieces flip bit 1 of the chunk)
  const unsigned dvo1 = dvo_ ^ 32u;
  auto stage_load = [&](int t, int buf) {
    if constexpr (DMA) {  // (hipcc does not count these loads: stage_write waits vmcnt(0))
#pragma unroll
      for (int j = 0; j < NPW; ++j) {
        const unsigned dvo = (BD == 256 && (j & 1)) ? dvo1 : dvo_;
        const unsigned soff = VARLEN ? (unsigned)(t * BT + j * 4 * RPP) * qrb : PAD ? (unsigned)(t * BT + j * 4 * RPP) * GRB : (unsigned)t * STILE + j * 4096;
        const unsigned lq = (unsigned)(__UINTPTR_TYPE__)QU + buf * STILE + (wave + 4 * j) * 1024;
        const unsigned lo = (unsigned)(__UINTPTR_TYPE__)OU + buf * STILE + (wave + 4 * j) * 1024;
        if constexpr (VARLEN) {  // the whole offset in voffset, inside the descriptor's range check (see the dQ kernel)
          // (the scalar part through an opaque copy: hipcc otherwise keeps one loop-invariant dvo + piece offset per piece in vector
          // registers -- spilled at head_dim 128 -- where one v_add with a scalar operand per load does)
          unsigned so = soff;
          asm volatile("" : "+s"(so));
          const unsigned vo = dvo + so;
          asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lq), "v"(vo), "s"(rq) : "memory");
          asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lo), "v"(vo), "s"(rdo) : "memory");
        } else {
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lq), "v"(dvo), "s"(rq), "s"(soff) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lo), "v"(dvo), "s"(rdo), "s"(soff) : "memory");
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        qst[i] = __builtin_amdgcn_raw_buffer_load_b128(rq, (unsigned)t * STILE + st_g[i], 0, 0);
        ost[i] = __builtin_amdgcn_raw_buffer_load_b128(rdo, (unsigned)t * STILE + st_g[i], 0, 0);
      }
    }
    if (FA_TID_LT(2 * BT)) {
      // (varlen: the tile index through an opaque copy -- hipcc otherwise keeps the first tile's 64-bit row index across the query
      // heads of the group in vector registers it does not have at head_dim 128, and spills it)
#if FA_BWD_VARLEN
      int ti = t;
      asm volatile("" : "+s"(ti));
      const int qi = ti * BT + FA_TID_ROW;
#else
      const int qi = t * BT + FA_TID_ROW;
#endif
      rowv = row_src[qi < FA_NQ ? qi : FA_NQ - 1];
    }
  };
  auto stage_write = [&](int buf, int wt) {  // wt = the tile the staged registers hold
    if constexpr (DMA) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        lds_write_b128(QU + buf * STILE + st_r[i], qst[i]);
        lds_write_b128(OU + buf * STILE + st_r[i], ost[i]);
      }
    }
    if (FA_TID_LT(2 * BT)) {  // (the staged registers hold tile wt: its rows past N get p = 0 through -inf)
      const int qi = wt * BT + FA_TID_ROW;
      // (varlen under the mask, Lk < Lq: a row with no visible key -- the forward's integer test; its LSE is -inf and its delta of no
      // use -- is staged like a row past the end: -inf and 0, so the +inf never reaches a score chain and the row adds exactly nothing)
      // (window: the row's upper bound qi + cu takes the place of qi + coff)
      const float v = (VARLEN && CAUSAL) ? (FA_TID_LT(BT) ? ((qi < LQ && qi + FA_DEAD_OFF >= 0) ? -rowv * LOG2E : -INFINITY) : ((qi < LQ && qi + FA_DEAD_OFF >= 0) ? -rowv : 0.0f))
                                         : ((tid < BT) ? (qi < FA_NQ ? -rowv * LOG2E : -INFINITY) : (qi < FA_NQ ? -rowv : 0.0f));
      lds_write_b32(ROWS + buf * (2 * BT * 4) + FA_TID4, __builtin_bit_cast(unsigned, v));
    }
  };

  f32x16 dkacc[BDB], dvacc[BDB];
#pragma unroll
  for (int db = 0; db < BDB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dkacc[db][i] = 0.0f; dvacc[db][i] = 0.0f; }

  set_head(0);
  if (t_begin < nTq) {
    stage_load(t_begin, 0);
    stage_write(0, t_begin);
  }
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks)  // K~ = round(c.K): S' = Q.K~ comes out in log2 units
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[ks][j] = (elem)((float)kf[ks][j] * c2);
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks) asm volatile("" : "+v"(kf[ks]), "+v"(vf[ks]));
  __syncthreads();

  int buf = 0;  // the buffer koff / voff / rowoff point into
  for (int g = 0; g < G; ++g) {
  if (g > 0) {  // next query head of the group (every wave is past the last tile's barrier: both buffers are free)
    set_head(g);
    if (t_begin < nTq) {
      stage_load(t_begin, buf);
      stage_write(buf, t_begin);
    }
    __syncthreads();
  }
  for (int t = t_begin; t < nTq; ++t) {
    if (t + 1 < nTq) stage_load(t + 1, buf ^ 1);
#pragma unroll
    for (int sub = 0; sub < BSUB; ++sub) {
    const int sub_c = sub;
    const int qt0 = t * BT + sub * BN;
    // (window: some query of the sub-tile sees one of this wave's 32 keys -- its last query reaches the first key from below, its first
    // query the last key from above)
#if FA_BWD_WINDOW
    if (qt0 < FA_NQ && qt0 + BN - 1 + cu >= kw0 && qt0 + cl <= kw0 + WM - 1) {
#else
    if (qt0 < FA_NQ && (!CAUSAL || qt0 + BN - 1 + coff >= kw0)) {  // some query of the sub-tile sees this wave's first key
#endif
      // (the buffer's offset is inside koff / voff / rowoff, toggled once per tile: everything added here is an immediate)
      const int QS = sub_c * BTILE, OS = 2 * STILE + sub_c * BTILE;  // Q / dO sub-tile images, relative to koff / voff
      const unsigned rows = rowoff + sub_c * (BN * 4);
      // only sub-tiles that cross the diagonal for this wave need the per-element mask (wave-uniform)
      // (window: either edge crosses it)
#if FA_BWD_WINDOW
      const bool need_mask = (qt0 + cu < kw0 + WM - 1) || (qt0 + BN - 1 + cl > kw0);
#else
      const bool need_mask = CAUSAL && (qt0 + coff < kw0 + WM - 1);
#endif
      // One 32-query half (qb) at a time -- scores, P / dS, then its share of dV / dK -- so that only ONE score and ONE dP tuple
      // are live (round 3 first kept both halves': 212 VGPR, two waves per SIMD; this form fits three).
      static_for<0, 2>([&](auto qbc) {
        constexpr int qb = decltype(qbc)::value;
        f32x16 sq, dpq;
        __builtin_amdgcn_s_setprio(1);  // matrix phases above the other wave's arithmetic (as in the forward kernel)
        // the chains start from the row constants: registers 4g..4g+3 are query rows 32qb + 8g + 4h + 0..3 of the sub-tile
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ql = 32 * qb + 8 * g;  // (+ 4h: in rowoff)
#if FA_BWD_SOFTCAP
          const u32x4 d4 = lds_read_b128(at(rows + BT * 4 + ql * 4));  // (-lse.log2e is applied behind tanh: the score chain starts from zero)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned dw = d4[e];
            sq[4 * g + e] = 0.0f;
            dpq[4 * g + e] = __builtin_bit_cast(float, dw);
          }
#else
          const u32x4 l4 = lds_read_b128(at(rows + ql * 4));
          const u32x4 d4 = lds_read_b128(at(rows + BT * 4 + ql * 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            // (scalar temporaries on purpose: __builtin_bit_cast applied directly to the vector element expression
            //  l4[e] read element 0 for every e -- seen in the IR)
            const unsigned lw = l4[e], dw = d4[e];
            sq[4 * g + e] = __builtin_bit_cast(float, lw);
            dpq[4 * g + e] = __builtin_bit_cast(float, dw);
          }
#endif
        }
        {
          constexpr int NF = 2 * BKS, LA = BD >= 128 ? FA_BWD_KV128_LA : FA_BWD_LA;
          vec8 fr[NF];
          auto fread = [&](auto fc) {  // f = (ks, which): which 0 = Q row fragment, 1 = dO row fragment
            constexpr int f = decltype(fc)::value;
            fr[f] = __builtin_bit_cast(
                vec8, lds_read_b128(at(koff[f / 2] + ((f & 1) ? OS : QS) + qb * 32 * BRB)));
          };
          static_for<0, LA>([&](auto fc) { fread(fc); });
          __builtin_amdgcn_sched_barrier(0);
          static_for<0, NF>([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            if constexpr (f & 1) dpq = M::mfma(fr[f], vf[f / 2], dpq);
            else sq = M::mfma(fr[f], kf[f / 2], sq);
            if constexpr (f + LA < NF) fread(std::integral_constant<int, f + LA>{});
            __builtin_amdgcn_sched_barrier(0);
          });
        }
#if FA_BWD_SOFTCAP
        // the cap, in front of the mask: sq becomes the exponent t . C - lse.log2e (the row's value from LDS; -inf for a dead row or one
        // past the end) and dpq takes the factor 1 - t^2 (a masked element's exponent is set to -inf below; its dpq stays finite)
        // (a few rows at a time and the steps kept apart: left to itself hipcc holds all sixteen t and row values at once and spills around
        // the tile loop. head_dim 64: four rows, the next four's values read one step ahead; head_dim 128: two rows and no step ahead)
        if constexpr (BD >= 128) {
#pragma unroll
          for (int c = 0; c < 8; ++c) {  // registers 2c, 2c + 1 = rows 8 (c / 2) + 2 (c % 2) + 0..1 (+ 4h: in rowoff)
            const u32x2 l2 = *reinterpret_cast<const __attribute__((address_space(3))) u32x2 *>(at(rows + (32 * qb + 8 * (c / 2) + 2 * (c % 2)) * 4));
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const unsigned lw = l2[e];
              const float tq = tanh_from_exp2_arg(sq[2 * c + e]);
              dpq[2 * c + e] *= __builtin_fmaf(-tq, tq, 1.0f);
              asm volatile("" : "+v"(dpq[2 * c + e]));  // (formed here: hipcc otherwise sinks the multiply below the mask and keeps every t)
              sq[2 * c + e] = __builtin_fmaf(tq, capc, __builtin_bit_cast(float, lw));
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          u32x4 l4 = lds_read_b128(at(rows + (32 * qb) * 4));
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            u32x4 l4n = l4;
            if (g < 3) l4n = lds_read_b128(at(rows + (32 * qb + 8 * (g + 1)) * 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const unsigned lw = l4[e];
              const float tq = tanh_from_exp2_arg(sq[4 * g + e]);
              dpq[4 * g + e] *= __builtin_fmaf(-tq, tq, 1.0f);
              asm volatile("" : "+v"(dpq[4 * g + e]));  // (as above)
              sq[4 * g + e] = __builtin_fmaf(tq, capc, __builtin_bit_cast(float, lw));
            }
            __builtin_amdgcn_sched_barrier(0);
            l4 = l4n;
          }
        }
#endif
        // dV / dK fragments of this half (step j = (st, db, which): which 0 = dO^T fragment -> dV, 1 = Q^T fragment -> dK) are
        // read LA2 steps ahead of their MFMA, the first ones before the P / dS arithmetic (they do not depend on it)
        constexpr int NJ = 4 * BDB, LA2 = BD >= 128 ? FA_BWD_KV128_LA2 : FA_BWD_LA2, TV = BD == 64 ? 4 : 2;
        s16x4 tlo[NJ], thi[NJ];
        auto tread = [&](auto jc) {
          constexpr int j = decltype(jc)::value, jj = j / 2, R0 = 32 * qb + 16 * (jj / BDB), db = jj % BDB;
          const int src = (j & 1) ? QS : OS;
          tlo[j] = lds_read_tr16(at(voff[(R0 >> 3) % TV][db] + src + R0 * BRB));
          thi[j] = lds_read_tr16(at(voff[((R0 >> 3) + 1) % TV][db] + src + (R0 + 8) * BRB));
        };
#if FA_BWD_SOFTCAP
        // (head_dim 128: the first transposed reads wait until P and dS are packed -- their four registers are what the cap's arithmetic needs)
        if constexpr (BD < 128) static_for<0, LA2>([&](auto jc) { tread(jc); });
#else
        static_for<0, LA2>([&](auto jc) { tread(jc); });
#endif
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
        if (need_mask) {  // key > query (kernels.metal:748): S' = -inf there. A wave-uniform BRANCH: written as a per-element
          // condition hipcc turned it into 32 compare + select pairs on every tile (seen in the ISA). Register 4g+e holds query
          // qt0 + 32qb + 8g + 4h + e: compared as a constant against ONE per-lane limit (else: sixteen threshold registers)
          // (window: query < key - cu or query > key - cl -> masked; the second limit is the first plus the scalar cu - cl)
#if FA_BWD_WINDOW
          int lane_m = lane;
          asm volatile("" : "+v"(lane_m));
          const int lim = kw0 + (lane_m & 31) - cu - 4 * (lane_m >> 5) - qt0 - 32 * qb;
          const int lim_hi = lim + (cu - cl);
#pragma unroll
          for (int i = 0; i < 16; ++i) sq[i] = (8 * (i >> 2) + (i & 3) < lim || 8 * (i >> 2) + (i & 3) > lim_hi) ? -INFINITY : sq[i];
#else
#if FA_BWD_VARLEN
          int lane_m = lane;
          asm volatile("" : "+v"(lane_m));
          const int lim = kw0 + (lane_m & 31) - coff - 4 * (lane_m >> 5) - qt0 - 32 * qb;
#else
          const int lim = krow - coff - 4 * h - qt0 - 32 * qb;
#endif
#pragma unroll
          for (int i = 0; i < 16; ++i) sq[i] = (8 * (i >> 2) + (i & 3) < lim) ? -INFINITY : sq[i];
#endif
        }
        vec8 pf[2], df[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pv = __builtin_amdgcn_exp2f(sq[i]);  // S' = Q.K~ - lse*log2e came out of the matrix core
          sq[i] = pv;
          dpq[i] = pv * dpq[i];  // dS (without the softmax scale: it goes onto the finished dK)
        }
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            pf[st][j] = (elem)sq[8 * st + j];
            df[st][j] = (elem)dpq[8 * st + j];
          }
        // dV^T += dO^T.P ; dK^T += Q^T.dS   (reduction over this half's 32 query rows)
#if FA_BWD_SOFTCAP
        if constexpr (BD >= 128) {
          __builtin_amdgcn_sched_barrier(0);
          static_for<0, LA2>([&](auto jc) { tread(jc); });
        }
#endif
        __builtin_amdgcn_s_setprio(1);
        static_for<0, NJ>([&](auto jc) {
          constexpr int j = decltype(jc)::value, jj = j / 2, st = jj / BDB, db = jj % BDB;
          const s16x8 a8 = __builtin_shufflevector(tlo[j], thi[j], 0, 1, 2, 3, 4, 5, 6, 7);
          if constexpr (j & 1) dkacc[db] = M::mfma(__builtin_bit_cast(vec8, a8), df[st], dkacc[db]);
          else dvacc[db] = M::mfma(__builtin_bit_cast(vec8, a8), pf[st], dvacc[db]);
          if constexpr (j + LA2 < NJ) tread(std::integral_constant<int, j + LA2>{});
          __builtin_amdgcn_sched_barrier(0);
        });
      });
    }
    }  // sub-tiles
#pragma unroll
    for (int ks = 0; ks < BKS; ++ks) {
      koff[ks] += flip;
      asm volatile("" : "+v"(koff[ks]));
    }
#pragma unroll
    for (int tv = 0; tv < NTV; ++tv)
#pragma unroll
      for (int db = 0; db < BDB; ++db) {
        voff[tv][db] += flip;
        asm volatile("" : "+v"(voff[tv][db]));
      }
    rowoff += flip_rows;
    asm volatile("" : "+v"(rowoff));
    flip = -flip;
    flip_rows = -flip_rows;
    if (t + 1 < nTq) stage_write(buf ^ 1, t + 1);
    __syncthreads();
    buf ^= 1;
  }
  }  // query heads of the group
  // (varlen: the key row formed again from the thread index, so that it is not held -- at head_dim 128: spilled -- across the loops)
#if FA_BWD_VARLEN
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int krow_e = kw0 + (lane_e & 31), h_e = lane_e >> 5;
  if (krow_e < LK) {
    float *dk = p.dk + base + (long long)krow_e * (long long)(kvrb / 2), *dv = p.dv + base + (long long)krow_e * (long long)(kvrb / 2);
#else
  const int h_e = h;
  if (krow < p.Nk) {
    float *dk = p.dk + base + (long long)krow * (PAD ? p.D : BD), *dv = p.dv + base + (long long)krow * (PAD ? p.D : BD);
#endif
#pragma unroll
    for (int db = 0; db < BDB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * db + 8 * g4 + 4 * h_e;
        if (PAD && d0 >= p.D) continue;
        *reinterpret_cast<float4 *>(dk + d0) = make_float4(dkacc[db][4 * g4] * p.scale, dkacc[db][4 * g4 + 1] * p.scale, dkacc[db][4 * g4 + 2] * p.scale,
                                                             dkacc[db][4 * g4 + 3] * p.scale);
        *reinterpret_cast<float4 *>(dv + d0) = make_float4(dvacc[db][4 * g4], dvacc[db][4 * g4 + 1], dvacc[db][4 * g4 + 2], dvacc[db][4 * g4 + 3]);
      }
  }
#undef FA_NQ
#undef FA_NK
#undef FA_VP
#undef FA_TID_LT
#undef FA_TID_ROW
#undef FA_TID4
#undef FA_DEAD_OFF
