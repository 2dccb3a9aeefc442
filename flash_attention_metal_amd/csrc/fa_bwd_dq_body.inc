// fa_bwd_dq_body.inc -- the body of the dQ kernels (fa_bwd_body.h says how it is used): included inside
//   template <typename Tag, int D, bool CAUSAL, bool PAD> __global__ void kernel(BwdParams or BwdVarlenParams p)
// with FA_BWD_VARLEN defined to 0 or 1, and FA_BWD_WINDOW (varlen only) to 0 or 1: the window mode, whose parameter block is
// BwdWindowParams; FA_BWD_SOFTCAP (window only) to 0 or 1: the softcap mode, BwdSoftcapParams. Their arms are chosen in the preprocessor,
// so that the text the other kernels compile is the text they had.
// dQ: workgroup = 128 query rows, wave = 32 rows (query on the lane, keys in the registers)
#if FA_BWD_VARLEN
#define FA_VP p
#else
#define FA_VP bwd_no_varlen_params()
#endif
#define FA_NQ (VARLEN ? LQ : p.N)
#define FA_NK (VARLEN ? LK : p.Nk)
  constexpr bool VARLEN = FA_BWD_VARLEN != 0;
  static_assert(!VARLEN || (!PAD && (D == 64 || D == 128) && FA_BWD_DMA != 0), "varlen mode: head_dim 64 / 128, LDS-DMA staging");
  static_assert(FA_BWD_WINDOW == 0 || (VARLEN && CAUSAL), "window mode: on top of the varlen mode, in the masked kernels' block order");
  static_assert(FA_BWD_SOFTCAP == 0 || FA_BWD_WINDOW != 0, "softcap mode: on top of the window mode");
  FA_BWD_CONSTS(D, bwd_sub_dq(D));
  FA_BWD_PAD(PAD);
  using M = MT<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;
  lds_char *KU = smem;               // [2] K tile of BT rows (read by rows for S, transposed for dQ)
  lds_char *VR = smem + 2 * STILE;   // [2] V tile (read by rows)
  static_assert(4 * STILE == bwd_dq_lds_bytes(D), "the launcher's LDS size is the K / V buffers");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nQ = (p.N + BM - 1) / BM;
  int bh, qb;
  map_block_div<CAUSAL>(blockIdx.x, p.B * p.H, nQ, bh, qb);
  long long base, base_kv;
  // varlen only:
  int LQ = 0, LK = 0;          // queries and keys of this block's sequence
  unsigned qrb = 0, kvrb = 0;  // row pitch of Q / O / dO and of K / V in global memory, bytes
  long long row_base = 0;      // first lse / delta element of this block's (head, sequence)
#if FA_BWD_WINDOW
  // window only (all wave-uniform): key j is visible to query i iff i + cl <= j <= i + cu; [w_lo, w_hi) = the keys this block's rows see
  int cl = 0, cu = 0, w_lo = 0, w_hi = 0;
#endif
  if constexpr (VARLEN) {
    // sequence b = the "batch" index. Both cu pairs are wave-uniform (scalar loads) and clamped exactly as the forward clamps them:
    // every entry to [0, total], a non-increasing pair is length 0, a length stops at max_seqlen -- whatever the tables hold, the
    // block stays inside tokens [0, total) of every tensor. A block past its sequence's last row leaves in front of every barrier.
    const int b = bh / p.H, hq = bh % p.H;
    const int sq = min(max(FA_VP.cu_q[b], 0), FA_VP.total_q), eq = min(max(FA_VP.cu_q[b + 1], 0), FA_VP.total_q);
    const int sk = min(max(FA_VP.cu_k[b], 0), FA_VP.total_k), ek = min(max(FA_VP.cu_k[b + 1], 0), FA_VP.total_k);
    LQ = min(max(eq - sq, 0), p.N);
    LK = min(max(ek - sk, 0), p.Nk);
    if (qb * BM >= LQ) return;
    base = (long long)sq * FA_VP.q_rs + (long long)hq * p.head_stride;
    base_kv = (long long)sk * FA_VP.kv_rs + (long long)(hq / (p.H / p.Hkv)) * p.kv_head_stride;
    row_base = (long long)hq * FA_VP.total_q + sq;
    qrb = (unsigned)FA_VP.q_rs * 2;
    kvrb = (unsigned)FA_VP.kv_rs * 2;
    // no key is visible to any row of the block (no keys at all, or causal with Lk < Lq: key j is visible to query i iff
    // j <= i + Lk - Lq): dQ = 0, and a defined delta for the dK/dV kernel, which discards it by the same integer test
#if FA_BWD_WINDOW
    cl = LK - LQ - p.wl;
    cu = LK - LQ + p.wr;
    window_key_range(LQ, LK, p.wl, p.wr, qb * BM, qb * BM + BM - 1, w_lo, w_hi);
    // (window: the block's key range is empty -- no keys, or every row of the block in front of the first key's band)
    if (w_lo >= w_hi) {
#else
    if ((CAUSAL ? min(LK, qb * BM + BM + LK - LQ) : LK) <= 0) {
#endif
      float *dqz = p.dq + base;
      for (int idx = threadIdx.x; idx < BM * (BD / 4); idx += NTHREADS) {
        const int row = qb * BM + idx / (BD / 4), c4 = idx % (BD / 4);
        if (row < LQ) *reinterpret_cast<float4 *>(dqz + (long long)row * FA_VP.q_rs + c4 * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
      const int row = qb * BM + (int)threadIdx.x;
      if ((int)threadIdx.x < BM && row < LQ) p.delta[row_base + row] = 0.0f;
      return;
    }
  } else {
    base = (long long)(bh / p.H) * p.batch_stride + (long long)(bh % p.H) * p.head_stride;
    base_kv = (long long)(bh / p.H) * p.kv_batch_stride + (long long)((bh % p.H) / (p.H / p.Hkv)) * p.kv_head_stride;
  }
  const int q0 = qb * BM, qw0 = q0 + wave * WM, qrow = qw0 + r;

  // (varlen: the descriptors end with the last row's D elements, so rows at or past the sequence's end read as zeros whatever the
  // pitch -- what follows a sequence is another sequence)
  const unsigned head_bytes = VARLEN ? (unsigned)(LQ - 1) * qrb + BRB : (unsigned)p.N * GRB;
  const unsigned kv_head_bytes = VARLEN ? (unsigned)(LK - 1) * kvrb + BRB : (unsigned)p.Nk * GRB;
  const int coff = FA_NK - FA_NQ;  // (varlen: may be negative)
  const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.q + base), 0, head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.k + base_kv), 0, kv_head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.v + base_kv), 0, kv_head_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rdo = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.d_o + base), 0, head_bytes, 0x00020000);

  vec8 qf[BKS], dof[BKS];  // B operands: lane (r,h) holds row qrow, columns 16ks+8h..
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks) {
    qf[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rq, (VARLEN ? (unsigned)qrow * qrb : (unsigned)qrow * GRB) + gcol(2 * ks + h), 0, 0));
    dof[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rdo, (VARLEN ? (unsigned)qrow * qrb : (unsigned)qrow * GRB) + gcol(2 * ks + h), 0, 0));
  }
  // S' = K.Q~ - lse*log2e straight out of the matrix core (rows past N: -inf, p = 0); dP' = V.dO - delta likewise
  const bool qvalid = qrow < FA_NQ;
  // varlen under the mask, Lk < Lq: a row with no visible key carries LSE = -inf, and +inf as the start of a score chain would meet the
  // mask's -inf. Decided by the forward's integer test (the object is built without NaN handling): such a row starts from -inf like a
  // row past the end, so P = 0, dS = 0 and dQ = 0 exactly, and it adds nothing to anything.
  // (window: the forward's test -- the row's upper bound reaches key 0; its lower bound is never past the last key)
#if FA_BWD_WINDOW
  const bool qlive = qvalid && LK > 0 && qrow + cu >= 0;
#else
  const bool qlive = (VARLEN && CAUSAL) ? (qvalid && qrow + coff >= 0) : qvalid;
#endif
  const float lse2 = qlive ? p.lse[(VARLEN ? row_base : (long long)bh * p.N) + qrow] * LOG2E : INFINITY;
#if FA_BWD_SOFTCAP
  // softcap: the capped score softcap . tanh(x), x = scale . s / softcap, takes the raw score's place. Q~ carries 2 log2(e) scale /
  // softcap, so the matrix core delivers y with 2^y = e^(2x); the score chain starts from zero and the row's -lse.log2e is applied behind
  // tanh: P = exp2(fma(t, C, -lse2)), C = softcap . log2(e). dS gets the factor 1 - t^2 = d(softcap tanh(x)) / d(scale s).
  const float c2 = 2.0f * LOG2E * p.scale / p.softcap;
  const float capc = p.cap_log2;  // (softcap . log2(e) from the host: a kernel argument stays in a scalar register, a product formed here in a vector one)
#else
  const float c2 = p.scale * LOG2E;
#endif
  // delta_i = rowsum(dO o O) (kernels.metal:983-990): this lane holds half of row i's dO (columns 16ks + 8h ..), loads the
  // same half of O, and the two halves of the row meet through one permlane swap; written once for the dK/dV kernel
  float dlt = 0.0f;
  {
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.o + base), 0, head_bytes, 0x00020000);
#pragma unroll
    for (int ks = 0; ks < BKS; ++ks) {
      const vec8 of = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(ro, (VARLEN ? (unsigned)qrow * qrb : (unsigned)qrow * GRB) + gcol(2 * ks + h), 0, 0));
#pragma unroll
      for (int j = 0; j < 8; ++j) dlt = __builtin_fmaf((float)of[j], (float)dof[ks][j], dlt);
    }
    float lo, hi;
    half_pair(dlt, lo, hi);
    dlt = lo + hi;
    if (qvalid && h == 0) p.delta[(VARLEN ? row_base : (long long)bh * p.N) + qrow] = dlt;
  }
  f32x16 nlse, ndlt;  // the row constants, one per lane, in all 16 registers of a tuple: C operands of the chains' first MFMAs
#pragma unroll
#if FA_BWD_SOFTCAP
  for (int i = 0; i < 16; ++i) { nlse[i] = 0.0f; ndlt[i] = -dlt; }  // (the score chain starts from a constant zero tuple: no registers)
  asm volatile("" : "+v"(ndlt));
#else
  for (int i = 0; i < 16; ++i) { nlse[i] = -lse2; ndlt[i] = -dlt; }
  asm volatile("" : "+v"(nlse), "+v"(ndlt));  // opaque: else hipcc re-materialises the splats in front of every MFMA
#endif

  const int kx = u_swz(r);
  // ABSOLUTE LDS addresses in the current K buffer (the V image is 2 STILE further), flipped in place once per tile: with the
  // buffer base added at the point of use hipcc kept a second, per-tile copy of all (base + offset) in registers (seen in the ISA)
  const unsigned ku0 = (unsigned)(__UINTPTR_TYPE__)KU;
  int flip = STILE;
  auto at = [](unsigned a) { return (const lds_char *)(__UINTPTR_TYPE__)a; };
  unsigned koff[BKS];
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks) koff[ks] = ku0 + r * BRB + (((2 * ks + h) ^ kx) << 4);
  const int g1 = (lane >> 4) & 1, vq = (lane >> 2) & 3, vp = lane & 3;
  unsigned voff[NTV][BDB];
#pragma unroll
  for (int tv = 0; tv < NTV; ++tv)
#pragma unroll
    for (int db = 0; db < BDB; ++db) voff[tv][db] = ku0 + tr_off(tv, db, h, g1, vq, vp);
  constexpr int NCH = BT * BCPR / NTHREADS;
  int st_g[NCH], st_r[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = tid + i * NTHREADS, row = c / BCPR, ch = c % BCPR;
    st_g[i] = row * BRB + ch * 16;
    st_r[i] = row * BRB + ((ch ^ u_swz(row)) << 4);
  }
  // (window: the walk is tiles [t0, nT) of the block's key range; buffer parity and the flipped addresses follow the position in the
  // walk -- the prologue stages tile t0 into buffer 0 -- not the tile's absolute index)
#if FA_BWD_WINDOW
  (void)coff;
  const int kv_end = w_hi;
  const int t0 = w_lo / BT;
#define FA_T0 t0
#else
  const int kv_end = CAUSAL ? min(FA_NK, q0 + BM + coff) : FA_NK;  // (varlen: >= 1 here)
#define FA_T0 0
#endif
  const int nT = (kv_end + BT - 1) / BT;

  constexpr bool DMA = FA_BWD_DMA != 0;
  static_assert(DMA || !PAD, "padded head dims are staged by LDS-DMA only");
  // (varlen: dma_off under the run-time pitch -- the row of the piece times the pitch, plus the swizzled chunk)
  auto dma_off_rs = [&](unsigned pitch) {
    const int row = wave * RPP + lane / BCPR, lc = (lane % BCPR) ^ u_swz(row);
    return (unsigned)row * pitch + ((unsigned)lc << 4);
  };
  const unsigned dvo_ = VARLEN ? dma_off_rs(kvrb) : PAD ? dma_off_pad(wave, lane) : dma_off(wave, lane);
  // (head_dim 256: a piece is 2 rows and a wave's pieces are 8 rows apart, half the swizzle's period: odd pieces flip bit 1 of the chunk)
  const unsigned dvo1 = dvo_ ^ 32u;
  // tile t -> buffer buf by LDS-DMA (hipcc does not count these loads: stage_write waits vmcnt(0))
  auto stage_dma = [&](int t, int buf) {
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      const unsigned dvo = (BD == 256 && (j & 1)) ? dvo1 : dvo_;
      const unsigned soff = VARLEN ? (unsigned)(t * BT + j * 4 * RPP) * kvrb : PAD ? (unsigned)(t * BT + j * 4 * RPP) * GRB : (unsigned)t * STILE + j * 4096;
      const unsigned lk = (unsigned)(__UINTPTR_TYPE__)KU + buf * STILE + (wave + 4 * j) * 1024;
      const unsigned lv = (unsigned)(__UINTPTR_TYPE__)VR + buf * STILE + (wave + 4 * j) * 1024;
      if constexpr (VARLEN) {
        // the whole offset in voffset, i.e. inside the descriptor's range check (soffset is outside it): what follows a sequence's last
        // key is another sequence or the end of the tensor, and both must read as zeros
        // (the scalar part through an opaque copy: hipcc otherwise keeps one loop-invariant dvo + piece offset per piece in vector
        // registers -- spilled at head_dim 128 -- where one v_add with a scalar operand per load does)
        unsigned so = soff;
        asm volatile("" : "+s"(so));
        const unsigned vo = dvo + so;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lk), "v"(vo), "s"(rk) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lv), "v"(vo), "s"(rv) : "memory");
      } else {
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lk), "v"(dvo), "s"(rk), "s"(soff) : "memory");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lv), "v"(dvo), "s"(rv), "s"(soff) : "memory");
      }
    }
  };
  u32x4 kst[NCH], vst[NCH];
  auto stage_load = [&](int t, int buf) {
    if constexpr (DMA) {
      stage_dma(t, buf);
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        kst[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, (unsigned)t * STILE + st_g[i], 0, 0);
        vst[i] = __builtin_amdgcn_raw_buffer_load_b128(rv, (unsigned)t * STILE + st_g[i], 0, 0);
      }
    }
  };
  auto stage_write = [&](int buf) {
    if constexpr (DMA) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        lds_write_b128(KU + buf * STILE + st_r[i], kst[i]);
        lds_write_b128(VR + buf * STILE + st_r[i], vst[i]);
      }
    }
  };

  f32x16 dqacc[BDB];
#pragma unroll
  for (int db = 0; db < BDB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dqacc[db][i] = 0.0f;

  stage_load(FA_T0, 0);
  stage_write(0);
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks)  // Q~ = round(c.Q): the very operand the forward multiplied (fa_mfma_kernel.hip)
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[ks][j] = (elem)((float)qf[ks][j] * c2);
#pragma unroll
  for (int ks = 0; ks < BKS; ++ks) asm volatile("" : "+v"(qf[ks]), "+v"(dof[ks]));  // retire the prologue loads
  __syncthreads();

#if FA_BWD_WINDOW
  for (int t = t0; t < nT; ++t) {
    const int buf = (t - t0) & 1;
#else
  for (int t = 0; t < nT; ++t) {
    const int buf = t & 1;
#endif
    if (t + 1 < nT) stage_load(t + 1, buf ^ 1);
#pragma unroll
    for (int sub = 0; sub < BSUB; ++sub) {
    const int kv0 = t * BT + sub * BN;
    // (window: a wave skips a sub-tile wholly outside its own 32 rows' bounds, above or below)
#if FA_BWD_WINDOW
    if (kv0 < kv_end && kv0 <= qw0 + WM - 1 + cu && kv0 + BN - 1 >= qw0 + cl) {
#else
    if (kv0 < kv_end && (!CAUSAL || kv0 <= qw0 + WM - 1 + coff)) {
#endif
      const int KS = sub * BTILE, VS = 2 * STILE + sub * BTILE;  // K / V sub-tile images, relative to koff / voff
      // masked: key > query (causal), and -- the partial last tile -- key >= Nk: those K / V rows arrive as zeros through the
      // descriptor, S' = -lse.log2e there, and with a strongly negative lse P = exp2(S') overflows the cast of dS (inf x 0 = NaN in dQ)
      // (window: two-sided, on sub-tiles that either edge of some row of the wave or the end of the keys crosses)
#if FA_BWD_WINDOW
      const bool need_mask = (kv0 + BN - 1 > qw0 + cu) || (kv0 < qw0 + WM - 1 + cl) || (kv0 + BN > FA_NK);
#else
      const bool need_mask = (CAUSAL && (kv0 + BN - 1 > qw0 + coff)) || (kv0 + BN > FA_NK);
#endif
      // One 32-key half (kb) at a time -- scores, dS, then its share of dQ -- so that only one score and one dP tuple are live
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 sk, dpk;
        __builtin_amdgcn_s_setprio(1);  // matrix phases above the other wave's arithmetic (as in the forward kernel)
        {
          // 2 BKS row fragments (K and V alternating), each read LA products ahead of the MFMA that consumes it
          constexpr int NF = 2 * BKS, LA = FA_BWD_LA;
          vec8 fr[NF];
          auto fread = [&](int f) {  // f = (ks, which): which 0 = K row fragment, 1 = V row fragment
            fr[f] = __builtin_bit_cast(vec8, lds_read_b128(at(koff[f / 2] + ((f & 1) ? VS : KS) + kb * 32 * BRB)));
          };
#pragma unroll
          for (int f = 0; f < LA; ++f) fread(f);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            const int ks = f / 2;
            if (f & 1) dpk = M::mfma(fr[f], dof[ks], ks == 0 ? ndlt : dpk);
            else sk = M::mfma(fr[f], qf[ks], ks == 0 ? nlse : sk);
            if (f + LA < NF) fread(f + LA);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        // dQ^T += K^T.dS^T : step j = (st, db); the transposed K fragments are read LA2 steps ahead of their MFMA, the first
        // ones before the dS arithmetic (they do not depend on it)
        constexpr int NJ = 2 * BDB, LA2 = FA_BWD_LA2, TV = BD == 64 ? 4 : 2;
        s16x4 tlo[NJ], thi[NJ];
        auto tread = [&](int j) {
          const int R0 = 32 * kb + 16 * (j / BDB), db = j % BDB;
          tlo[j] = lds_read_tr16(at(voff[(R0 >> 3) % TV][db] + KS + R0 * BRB));
          thi[j] = lds_read_tr16(at(voff[((R0 >> 3) + 1) % TV][db] + KS + (R0 + 8) * BRB));
        };
#pragma unroll
        for (int j = 0; j < LA2; ++j) tread(j);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
#if FA_BWD_SOFTCAP
        // the cap, in front of the mask: sk becomes the exponent t . C - lse2 and dpk takes the factor 1 - t^2 (a masked element's
        // exponent is set to -inf below; its dpk stays finite, so its dS is exactly 0)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float tq = tanh_from_exp2_arg(sk[i]);
          dpk[i] *= __builtin_fmaf(-tq, tq, 1.0f);
          sk[i] = __builtin_fmaf(tq, capc, -lse2);
        }
#endif
        if (need_mask) {  // key > query -> masked (kernels.metal:748); a wave-uniform branch
          int lim = FA_NK - 1 - kv0 - 32 * kb - 4 * h;
#if FA_BWD_WINDOW
          lim = min(lim, qrow + cu - kv0 - 32 * kb - 4 * h);
          const int lim_lo = qrow + cl - kv0 - 32 * kb - 4 * h;  // key < query + cl -> masked
#pragma unroll
          for (int i = 0; i < 16; ++i) sk[i] = ((i & 3) + 8 * (i >> 2) > lim || (i & 3) + 8 * (i >> 2) < lim_lo) ? -INFINITY : sk[i];
#else
          if (CAUSAL) lim = min(lim, qrow + coff - kv0 - 32 * kb - 4 * h);
#pragma unroll
          for (int i = 0; i < 16; ++i) sk[i] = ((i & 3) + 8 * (i >> 2) > lim) ? -INFINITY : sk[i];
#endif
        }
        // dS^T = P^T o (dP^T - delta) (the softmax scale goes onto the finished dQ): keys in the registers, the query on the lane
#pragma unroll
        for (int i = 0; i < 16; ++i) sk[i] = __builtin_amdgcn_exp2f(sk[i]) * dpk[i];
        vec8 df[2];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int j = 0; j < 8; ++j) df[st][j] = (elem)sk[8 * st + j];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const s16x8 k8 = __builtin_shufflevector(tlo[j], thi[j], 0, 1, 2, 3, 4, 5, 6, 7);
          dqacc[j % BDB] = M::mfma(__builtin_bit_cast(vec8, k8), df[j / BDB], dqacc[j % BDB]);
          if (j + LA2 < NJ) tread(j + LA2);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
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
    flip = -flip;
    if (t + 1 < nT) stage_write(buf ^ 1);
    __syncthreads();
  }
  // dQ^T[d][q]: lane (q = r, h) holds d = 32db + 8g4 + 4h + 0..3 -> one 16-byte store per group
  if (qvalid) {
    float *dq = p.dq + base + (VARLEN ? (long long)qrow * (long long)(qrb / 2) : (long long)qrow * (PAD ? p.D : BD));
#pragma unroll
    for (int db = 0; db < BDB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 w = make_float4(dqacc[db][4 * g4] * p.scale, dqacc[db][4 * g4 + 1] * p.scale, dqacc[db][4 * g4 + 2] * p.scale,
                                     dqacc[db][4 * g4 + 3] * p.scale);
        const int d0 = 32 * db + 8 * g4 + 4 * h;
        if (!PAD || d0 < p.D) *reinterpret_cast<float4 *>(dq + d0) = w;
      }
  }
#undef FA_NQ
#undef FA_NK
#undef FA_VP
#undef FA_T0
