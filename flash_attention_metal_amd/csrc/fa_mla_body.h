// fa_mla_body.h -- what ONE WAVE of the absorbed latent-attention decode does with its 16 packed query rows, as TEXT that the partial
// kernels of the family include into their bodies, in the manner of fa_bwd_dq_body.inc: fa_mla_paged_partial.inc (the paged 16-bit pool:
// fa_mla_kernel.hip's one wave per item over a private double buffer, fa_mla_wide_kernel.hip's two or four waves over one shared double
// buffer), fa_mla_kv8_kernel.hip and fa_mla_sparse_kernel.hip. The same tokens in all, so a wave of any computes the same bits from the
// same tile image. (As inlined functions the same statements came out with other registers and two instructions fewer: text it is.)
// Define FA_MLA_BODY_PART and include; the part undefines it.
//   0  at namespace scope, once per file: the tile's shape and image (MLA_DQK .. MLA_IST, mla_swz), stated here and nowhere else, the MFMA
//      types, and the launch tail of every call of the family (launch_mla_partial_and_combine)
//   1  the query fragments and the per-lane LDS read offsets. In scope: M / vec8 / elem, KSL, KSR, p, b, c, g, R, Nk, coff and
//      rb, the wave's 16-row slot. Declares qf[], rlim, kl[], kr[], vl[]
//   2  one 64-key tile, t, folded into the wave's (oacc[], m, l). In scope besides: DT, KT, smem, t0. The image and its swizzles are
//      described at the head of fa_mla_kernel.hip
//   3  the partial store. In scope: item (b * S + s), rb, oacc[], m, l
#if FA_MLA_BODY_PART == 0
// ---- the tile's shape and image. Parts 1 and 2, every file's staging and the combine kernel are written against these; that the latent
// part's swizzle serves both read patterns without a bank conflict is argued at the head of fa_mla_kernel.hip
constexpr int MLA_DQK = 576, MLA_DV = 512, MLA_DR = MLA_DQK - MLA_DV;
constexpr int MLA_LRB = MLA_DV * 2, MLA_RRB = MLA_DR * 2;              // row bytes of the latent / rotary part (of 16-bit elements)
constexpr int MLA_LAT = BN * MLA_LRB, MLA_ROT = BN * MLA_RRB;          // bytes of a tile's two parts
constexpr int MLA_IMG = MLA_LAT + MLA_ROT;                             // one tile: 72 KiB
constexpr size_t mla_lds_bytes() { return 2 * (size_t)MLA_IMG; }       // the double buffer
constexpr int MLA_IST = 16 * (MLA_DV + 2);                             // floats of one 16-row slot's partial: [16][512] O . l, then [16][2] (m, l)
__host__ __device__ constexpr int mla_swz(int r) { return (((r & 7) << 1) ^ (9 * ((r >> 3) & 1))) & 15; }  // the latent part's swizzle f

// ---- the launch tail of every call: the partial kernel over `grid` workgroups of nw waves under the double buffer, then fa_mla_kernel.hip's
// combine kernel over the output rows of pc (the call as that kernel sees it), on the same stream
template <typename K, typename PT>
inline hipError_t launch_mla_partial_and_combine(K partial, dim3 grid, int nw, const PT &p, const MlaDecodeParams &pc, int dtype, hipStream_t s) {
  (void)hipGetLastError();
  hipError_t e = set_dyn_lds_once((const void *)partial, (int)mla_lds_bytes());
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(partial, grid, dim3(64 * nw), mla_lds_bytes(), s, p);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_mla_combine(pc, dtype, s);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename Tag> struct ML16;
template <> struct ML16<BF16> {
  using elem = __bf16;
  using vec8 = bf16x8;
  __device__ static __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct ML16<F16> {
  using elem = _Float16;
  using vec8 = f16x8;
  __device__ static __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
#elif FA_MLA_BODY_PART == 1
  // ---- Q fragments: lane (c, g) holds row r = 16 rb + c of the packed block, elements 32 ks + 8 g .. + 7; pre-scaled Q~ = round(c2 . Q)
  const float c2 = p.scale * 1.4426950408889634f;
  vec8 qf[KSL + KSR];
  int rlim;  // last visible key of the lane's row (causal; Nk - 1 otherwise and for padding rows)
  {
    const int r = 16 * rb + c;
    const int h = r / p.Nq, iq = r - h * p.Nq;
    const bool valid = r < R;
    rlim = (CAUSAL && valid) ? iq + coff : Nk - 1;
    const elem *qp = (const elem *)p.q + (long long)b * p.q_bs + (long long)h * p.q_hs + (long long)iq * p.q_rs;
#pragma unroll
    for (int ks = 0; ks < KSL + KSR; ++ks) {
      u32x4 t = {0u, 0u, 0u, 0u};
      if (valid) t = *reinterpret_cast<const u32x4 *>(qp + 32 * ks + 8 * g);
      qf[ks] = __builtin_bit_cast(vec8, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[ks][j] = (elem)((float)qf[ks][j] * c2);
    }
  }

  // ---- per-lane LDS read offsets: a few bases, everything else is a compile-time offset
  // score product, latent part: row 16 kt + c, chunk (4 ks + g) ^ f(c) = ((ks >> 2) << 4) | ((4 (ks & 3) + g) ^ f(c))
  const int fc = mla_swz(c);
  unsigned kl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kl[j] = (unsigned)(c * MLA_LRB + (((4 * j + g) ^ fc) << 4));
  // score product, rotary part: the head_dim-64 K image, chunk ^ ((row >> 1) & 7)
  unsigned kr[KSR];
#pragma unroll
  for (int j = 0; j < KSR; ++j) kr[j] = (unsigned)(MLA_LAT + c * MLA_RRB + (((4 * j + g) ^ ((c >> 1) & 7)) << 4));
  // PV product: row 4 g + vq (+ 16, + 32 kp), chunk (2 dt + (vp >> 1)) ^ f(row) = ((dt >> 3) << 4) | ((2 (dt & 7) + (vp >> 1)) ^ f(row))
  const int vq = c >> 2, vp = c & 3, vrow = 4 * g + vq, fv = mla_swz(vrow);
  unsigned vl[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) vl[j] = (unsigned)(vrow * MLA_LRB + (((2 * j + (vp >> 1)) ^ fv) << 4) + 8 * (vp & 1));
#elif FA_MLA_BODY_PART == 2
    const int kv0 = t * BN;
    const lds_char *img = smem + ((t - t0) & 1) * MLA_IMG;
    // ---- S^T = K.Q~^T (log2 units) over 576 columns: sc[kt][i] = S[row c][key kv0 + 16 kt + 4 g + i]
    f32x4 sc[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[kt][i] = 0.0f;
    // (one wave per SIMD and nobody else on the CU: a read that an MFMA waits on exposes its whole latency, so the four reads of k-step
    // ks + 1 are issued in front of the four MFMAs of k-step ks; the scheduling barriers keep the compiler from folding the two groups
    // back into read, wait, multiply on one register quad)
    auto kread = [&](auto ksc, vec8 (&kf)[KT]) __attribute__((always_inline)) {
      constexpr int ks = decltype(ksc)::value;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        if constexpr (ks < KSL) kf[kt] = __builtin_bit_cast(vec8, lds_read_b128(img + kl[ks & 3] + ((ks >> 2) << 8) + kt * 16 * MLA_LRB));
        else kf[kt] = __builtin_bit_cast(vec8, lds_read_b128(img + kr[ks - KSL] + kt * 16 * MLA_RRB));
      }
    };
    auto kmul = [&](auto ksc, const vec8 (&kf)[KT]) __attribute__((always_inline)) {
      constexpr int ks = decltype(ksc)::value;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) sc[kt] = M::mfma(kf[kt], qf[ks], sc[kt]);
    };
    {
      vec8 kfa[KT], kfb[KT];
      kread(std::integral_constant<int, 0>{}, kfa);
      auto pair = [&](auto ksc) __attribute__((always_inline)) {
        constexpr int ks = decltype(ksc)::value;
        kread(std::integral_constant<int, ks + 1>{}, kfb);
        __builtin_amdgcn_sched_barrier(0);
        kmul(std::integral_constant<int, ks>{}, kfa);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ks + 2 < KSL + KSR) kread(std::integral_constant<int, ks + 2>{}, kfa);
        __builtin_amdgcn_sched_barrier(0);
        kmul(std::integral_constant<int, ks + 1>{}, kfb);
        __builtin_amdgcn_sched_barrier(0);
      };
      static_assert((KSL + KSR) % 2 == 0 && KSL + KSR == 18, "nine pairs of k-steps");
      pair(std::integral_constant<int, 0>{}); pair(std::integral_constant<int, 2>{}); pair(std::integral_constant<int, 4>{});
      pair(std::integral_constant<int, 6>{}); pair(std::integral_constant<int, 8>{}); pair(std::integral_constant<int, 10>{});
      pair(std::integral_constant<int, 12>{}); pair(std::integral_constant<int, 14>{}); pair(std::integral_constant<int, 16>{});
    }
    // ---- mask: key > the row's limit (causal, bottom-right aligned) or key >= Nk
    if (kv0 + BN > Nk || (CAUSAL && kv0 + BN - 1 > coff)) {
      const int lim = min(rlim, Nk - 1) - kv0 - 4 * g;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[kt][i] = (16 * kt + i > lim) ? -INFINITY : sc[kt][i];
    }
    // ---- exact online softmax (a row whose keys are all masked so far keeps m = -inf, l = 0: the guard avoids inf - inf)
    vec8 pf[2];
    {
      float mx = sc[0][0];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, sc[kt][i]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m, mx);
      const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m - m_use);
      m = m_new;
      float ls = 0.0f;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sc[kt][i] = __builtin_amdgcn_exp2f(sc[kt][i] - m_use);
          ls += sc[kt][i];
        }
      l = l * alpha + ls;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) oacc[dt][i] *= alpha;
#pragma unroll
      for (int kp = 0; kp < 2; ++kp)
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[kp][j] = (elem)sc[2 * kp + (j >> 2)][j & 3];
    }
    // ---- O^T += V^T.P^T over the latent part's 512 columns: 64 (key pair, d tile) steps in groups of four, the eight transposed reads of
    // group u + 1 in front of the four MFMAs of group u (as above)
    {
      constexpr int GV = 4, NG = 2 * DT / GV;
      auto vread = [&](auto uc, s16x8 (&v8)[GV]) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
#pragma unroll
        for (int e = 0; e < GV; ++e) {
          constexpr int step0 = u * GV;
          const int kp = (step0 + e) / DT, dt = (step0 + e) % DT;
          const lds_char *vb = img + vl[dt & 7] + ((dt >> 3) << 8) + (32 * kp) * MLA_LRB;
          const s16x4 lo = lds_read_tr16(vb), hi = lds_read_tr16(vb + 16 * MLA_LRB);
          v8[e] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
      };
      auto vmul = [&](auto uc, const s16x8 (&v8)[GV]) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
#pragma unroll
        for (int e = 0; e < GV; ++e) {
          constexpr int step0 = u * GV;
          const int kp = (step0 + e) / DT, dt = (step0 + e) % DT;
          oacc[dt] = M::mfma(__builtin_bit_cast(vec8, v8[e]), pf[kp], oacc[dt]);
        }
      };
      s16x8 va[GV], vb2[GV];
      vread(std::integral_constant<int, 0>{}, va);
      auto pair = [&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
        vread(std::integral_constant<int, u + 1>{}, vb2);
        __builtin_amdgcn_sched_barrier(0);
        vmul(std::integral_constant<int, u>{}, va);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (u + 2 < NG) vread(std::integral_constant<int, u + 2>{}, va);
        __builtin_amdgcn_sched_barrier(0);
        vmul(std::integral_constant<int, u + 1>{}, vb2);
        __builtin_amdgcn_sched_barrier(0);
      };
      static_assert(NG == 16, "eight pairs of groups");
      pair(std::integral_constant<int, 0>{}); pair(std::integral_constant<int, 2>{}); pair(std::integral_constant<int, 4>{});
      pair(std::integral_constant<int, 6>{}); pair(std::integral_constant<int, 8>{}); pair(std::integral_constant<int, 10>{});
      pair(std::integral_constant<int, 12>{}); pair(std::integral_constant<int, 14>{});
    }
#elif FA_MLA_BODY_PART == 3
  // ---- partial results -> workspace: [16][512] O (unnormalised, fp32), then [16][2] (m, l)
  float *wo = p.ws + ((size_t)item * p.RBLK + rb) * MLA_IST;
  float *wm = wo + 16 * MLA_DV;
  float lt = l;
  lt += __shfl_xor(lt, 16, 64);
  lt += __shfl_xor(lt, 32, 64);
  if (g == 0) {
    wm[2 * c] = m;
    wm[2 * c + 1] = lt;
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4 *>(wo + c * MLA_DV + 16 * dt + 4 * g) = oacc[dt];
#endif
#undef FA_MLA_BODY_PART
