// fa_bwd_mla_kernels.hip -- the backward of the MLA prefill (fa_bwd_varlen_mla): packed variable-length sequences with two head dims,
// q and k rows of 192 elements (128 "nope" columns, then 64 rotary ones), v / o / dO rows of 128.
//
//   mla_grad_q_kernel    one workgroup per (sequence, query head, 128 query rows up to max_seqlen_q): dQ, and delta for the other kernel
//   mla_grad_kv_kernel   one workgroup per (sequence, key/value head, 128 keys up to max_seqlen_k): dK and dV, summed in registers over the
//                        head's group of query heads in the dense order
//
// The structure is the two-kernel backward of fa_bwd_body.h in its varlen mode (fa_bwd_dq_body.inc / fa_bwd_dkdv_body.inc): the same
// tables and clamping, block maps, LDS-DMA staging, chains and roundings. Those bodies assume ONE head dim for both streamed tiles (one
// tile size, one distance between the two images, one set of row-read offsets), so this is a text of its own beside them and every
// existing kernel keeps its instruction text (profiles/r28/isa_kernel_diff.log).
//
// The LDS image. The 192-wide tile (K in the dQ kernel, Q in the dK/dV kernel) is staged in two parts, as the forward's MLA mode stages
// its keys: the head_dim-128 image of the nope columns (64 rows of 256 bytes) and behind it the head_dim-64 image of the rotary columns
// (64 rows of 128 bytes), each under the backward's own swizzle for that head dim -- the one image serves the row reads (S) and the
// transposed reads (dQ / dK). The 128-wide tile (V / dO) is the head_dim-128 image as it is. One buffer is [nope | rotary | 128-wide]
// = 40 KiB, so that one flip moves every read offset to the other buffer.
//
// The order of the chains (the bit contract of include/fa_mi355.h): the eight nope k-steps of S first, in the head_dim-128 kernels'
// order, then the four rotary ones; dP and both second products in the head_dim-128 kernels' order. With zero rotary columns the rotary
// steps add +0 to finite sums, and dq[:, :128], dk[:, :128] and dv are bit for bit fa_bwd_varlen's at D = 128.
#include "fa_bwd_body.h"

namespace fa {

// one fa_bwd_varlen_mla call: BwdVarlenParams with a (row, head) stride pair per tensor -- q / dq: q_rs / head_stride, k / dk: kv_rs /
// kv_head_stride, v / dv and o / d_o: the four below. D holds 192.
struct BwdMlaParams : BwdVarlenParams {
  long long v_rs, v_head_stride, o_rs, o_head_stride;  // elements
};

constexpr int LG_DQK = 192, LG_DV = 128;
constexpr int LG_NRB = 256, LG_RRB = 128;                            // row bytes of the nope / 128-wide images and of the rotary image
constexpr int LG_IMGN = BN * LG_NRB, LG_IMGR = BN * LG_RRB;          // a 64-row image of either kind
constexpr int LG_WIDE = LG_IMGN + LG_IMGR, LG_BUF = LG_WIDE + LG_IMGN;  // the two-part image; one buffer (both streamed tiles)
constexpr int LG_KSN = 8, LG_KSR = 4, LG_KS = LG_KSN + LG_KSR;       // k-steps over the nope / rotary columns
constexpr int LG_DBN = 4, LG_DBR = 2, LG_DB = LG_DBN + LG_DBR;       // 32-wide output blocks
constexpr size_t mla_grad_q_lds_bytes() { return (size_t)2 * LG_BUF; }
constexpr size_t mla_grad_kv_lds_bytes() { return (size_t)2 * LG_BUF + 2 * 2 * BN * 4; }
// Workgroups per CU the kernels are compiled for. dQ: two (80 KiB of LDS each fill the CU's 160 KiB; 256 registers). dK/dV: one -- 81 KiB
// of LDS, and 160 accumulator registers plus 80 of K~ / V fragments per lane need the 512-register budget (as the dense D = 256 kernels).
constexpr int LG_Q_OCC = 2, LG_KV_OCC = 1;

// the backward's swizzles (FA_BWD_CONSTS) of head_dim 128 and 64: XOR on the 16-byte chunk index of a row
__device__ constexpr int lg_swz_n(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ constexpr int lg_swz_r(int row) { return (((row >> 1) & 1) << 2) | ((row >> 3) & 3); }
// and their transposed-read rules (tr_off there): variant = (R0 >> 3) & 1 (nope part) or (R0 >> 3) & 3 (rotary part)
__device__ constexpr int lg_tr_n(int variant, int db, int h, int g1, int vq, int vp) {
  return (4 * h + vq) * LG_NRB + ((((4 * db) + 2 * g1 + (vp >> 1)) ^ lg_swz_n(8 * variant + 4 * h + vq)) << 4) + 8 * (vp & 1);
}
__device__ constexpr int lg_tr_r(int variant, int db, int h, int g1, int vq, int vp) {
  return (4 * h + vq) * LG_RRB + ((((4 * db) + 2 * g1 + (vp >> 1)) ^ lg_swz_r(8 * variant + 4 * h + vq)) << 4) + 8 * (vp & 1);
}

#define LG_DMA(lds_, voff_, rsrc_) \
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_), "v"(voff_), "s"(rsrc_) : "memory")

// dQ: workgroup = 128 query rows, wave = 32 rows (query on the lane, keys in the registers)
template <typename Tag, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, LG_Q_OCC) void mla_grad_q_kernel(BwdMlaParams p) {
  using M = MT<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  extern __shared__ __attribute__((aligned(256))) char smem_generic[];  // (256: the read addresses are XORed in place, below)
  lds_char *smem = (lds_char *)smem_generic;  // [2] buffers of [K nope | K rotary | V]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nQ = (p.N + BM - 1) / BM;
  int bh, qb;
  map_block_div<CAUSAL>(blockIdx.x, p.B * p.H, nQ, bh, qb);
  // sequence b = the "batch" index. Both cu pairs are wave-uniform (scalar loads) and clamped exactly as the forward clamps them:
  // every entry to [0, total], a non-increasing pair is length 0, a length stops at max_seqlen -- whatever the tables hold, the
  // block stays inside tokens [0, total) of every tensor. A block past its sequence's last row leaves in front of every barrier.
  const int b = bh / p.H, hq = bh % p.H;
  const int sq = min(max(p.cu_q[b], 0), p.total_q), eq = min(max(p.cu_q[b + 1], 0), p.total_q);
  const int sk = min(max(p.cu_k[b], 0), p.total_k), ek = min(max(p.cu_k[b + 1], 0), p.total_k);
  const int LQ = min(max(eq - sq, 0), p.N);
  const int LK = min(max(ek - sk, 0), p.Nk);
  if (qb * BM >= LQ) return;
  const int hk = hq / (p.H / p.Hkv);
  const long long base_q = (long long)sq * p.q_rs + (long long)hq * p.head_stride;
  const long long base_o = (long long)sq * p.o_rs + (long long)hq * p.o_head_stride;
  const long long base_k = (long long)sk * p.kv_rs + (long long)hk * p.kv_head_stride;
  const long long base_v = (long long)sk * p.v_rs + (long long)hk * p.v_head_stride;
  const long long row_base = (long long)hq * p.total_q + sq;  // first lse / delta element of this block's (head, sequence)
  const unsigned qrb = (unsigned)p.q_rs * 2, orb = (unsigned)p.o_rs * 2, krb = (unsigned)p.kv_rs * 2, vrb = (unsigned)p.v_rs * 2;
  // no key is visible to any row of the block (no keys at all, or causal with Lk < Lq: key j is visible to query i iff
  // j <= i + Lk - Lq): dQ = 0, and a defined delta for the dK/dV kernel, which discards it by the same integer test
  if ((CAUSAL ? min(LK, qb * BM + BM + LK - LQ) : LK) <= 0) {
    float *dqz = p.dq + base_q;
    for (int idx = threadIdx.x; idx < BM * (LG_DQK / 4); idx += NTHREADS) {
      const int row = qb * BM + idx / (LG_DQK / 4), c4 = idx % (LG_DQK / 4);
      if (row < LQ) *reinterpret_cast<float4 *>(dqz + (long long)row * p.q_rs + c4 * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const int row = qb * BM + (int)threadIdx.x;
    if ((int)threadIdx.x < BM && row < LQ) p.delta[row_base + row] = 0.0f;
    return;
  }
  const int q0 = qb * BM, qw0 = q0 + wave * WM, qrow = qw0 + r;

  // the descriptors end with the last row's 192 (q, k) or 128 (v, o, dO) elements, per tensor and per pitch, so rows at or past the
  // sequence's end read as zeros whatever the pitch -- what follows a sequence is another sequence
  const unsigned q_bytes = (unsigned)(LQ - 1) * qrb + LG_DQK * 2, o_bytes = (unsigned)(LQ - 1) * orb + LG_DV * 2;
  const unsigned k_bytes = (unsigned)(LK - 1) * krb + LG_DQK * 2, v_bytes = (unsigned)(LK - 1) * vrb + LG_DV * 2;
  const int coff = LK - LQ;  // (may be negative)
  const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.q + base_q), 0, q_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.k + base_k), 0, k_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.v + base_v), 0, v_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rdo = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.d_o + base_o), 0, o_bytes, 0x00020000);

  vec8 qf[LG_KS], dof[LG_KSN];  // B operands: lane (r,h) holds row qrow, columns 16ks+8h..
#pragma unroll
  for (int ks = 0; ks < LG_KS; ++ks)
    qf[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rq, (unsigned)qrow * qrb + (2 * ks + h) * 16, 0, 0));
#pragma unroll
  for (int ks = 0; ks < LG_KSN; ++ks)
    dof[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rdo, (unsigned)qrow * orb + (2 * ks + h) * 16, 0, 0));
  // S' = K.Q~ - lse*log2e straight out of the matrix core (rows past the end: -inf, p = 0); dP' = V.dO - delta likewise
  const bool qvalid = qrow < LQ;
  // under the mask, Lk < Lq: a row with no visible key carries LSE = -inf, and +inf as the start of a score chain would meet the mask's
  // -inf. Decided by the forward's integer test (the object is built without NaN handling): such a row starts from -inf like a row
  // past the end, so P = 0, dS = 0 and dQ = 0 exactly, and it adds nothing to anything.
  const bool qlive = CAUSAL ? (qvalid && qrow + coff >= 0) : qvalid;
  const float lse2 = qlive ? p.lse[row_base + qrow] * LOG2E : INFINITY;
  const float c2 = p.scale * LOG2E;
  // delta_i = rowsum(dO o O) over the 128 value columns: this lane holds half of row i's dO (columns 16ks + 8h ..), loads the same half
  // of O, and the two halves of the row meet through one permlane swap; written once for the dK/dV kernel
  float dlt = 0.0f;
  {
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.o + base_o), 0, o_bytes, 0x00020000);
#pragma unroll
    for (int ks = 0; ks < LG_KSN; ++ks) {
      const vec8 of = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(ro, (unsigned)qrow * orb + (2 * ks + h) * 16, 0, 0));
#pragma unroll
      for (int j = 0; j < 8; ++j) dlt = __builtin_fmaf((float)of[j], (float)dof[ks][j], dlt);
    }
    float lo, hi;
    half_pair(dlt, lo, hi);
    dlt = lo + hi;
    if (qvalid && h == 0) p.delta[row_base + qrow] = dlt;
  }
  // the row constants, one per lane: splat into the 16 registers of a tuple in front of each chain (the C operands of the chains' first
  // MFMAs). The head_dim-128 kernel holds both tuples across the loop; here those 32 registers are what two workgroups per CU lack,
  // and 32 moves per 44 MFMAs hide behind the other wave's matrix phase.
  float nl1 = -lse2, nd1 = -dlt;

  // LDS read addresses. The head_dim-128 kernel holds one absolute address per k-step and per (variant, output block) -- here that would
  // be 28 registers, which two workgroups per CU do not have. A k-step only XORs bits 5..7 of the swizzled chunk and an output block bits
  // 6..7, and every base (the dynamic LDS, a buffer, an image) is a multiple of 256: ONE absolute address per row rule and variant is
  // held, flipped in place once per tile, and each read forms address ^ constant -- the constant through an opaque scalar at the point
  // of use, else hipcc forms all 44 results at the head of the tile and holds (spills) them.
  const unsigned ku0 = (unsigned)(__UINTPTR_TYPE__)smem;
  int flip = LG_BUF;
  auto at = [](unsigned a) { return (const lds_char *)(__UINTPTR_TYPE__)a; };
  auto xat = [](unsigned a, unsigned c) {
    if (c == 0) return a;
    unsigned x = c;
    asm volatile("" : "+s"(x));
    return a ^ x;
  };
  unsigned rown = ku0 + r * LG_NRB + ((h ^ lg_swz_n(r)) << 4);            // row reads, nope part and V image: k-step ks is ^ (ks << 5)
  unsigned rowr = ku0 + LG_IMGN + r * LG_RRB + ((h ^ lg_swz_r(r)) << 4);  // row reads, rotary part
  const int g1 = (lane >> 4) & 1, vq = (lane >> 2) & 3, vp = lane & 3;
  unsigned trn[2], trr[4];  // transposed reads per variant, output block 0: block db is ^ (db << 6)
#pragma unroll
  for (int tv = 0; tv < 2; ++tv) trn[tv] = ku0 + lg_tr_n(tv, 0, h, g1, vq, vp);
#pragma unroll
  for (int tv = 0; tv < 4; ++tv) trr[tv] = ku0 + LG_IMGN + lg_tr_r(tv, 0, h, g1, vq, vp);
  static_assert(LG_BUF % 256 == 0 && LG_IMGN % 256 == 0 && LG_WIDE % 256 == 0, "the XORed bits lie below every base");

  const int kv_end = CAUSAL ? min(LK, q0 + BM + coff) : LK;  // (>= 1 here)
  const int nT = (kv_end + BN - 1) / BN;

  // LDS-DMA: wave w moves the 1-KiB pieces w, w + 4, ... of an image; lane L fills LDS bytes [16 L, 16 L + 16) of its piece, whose
  // logical chunk is the physical one XOR the row's swizzle (on the SOURCE address). A piece is 4 rows of a 256-byte image (a wave's
  // pieces 16 rows apart) or 8 rows of the rotary image (32 rows apart): multiples of either swizzle's period.
  unsigned dvo_k, dvo_v, dvo_r;
  {
    const int row = wave * 4 + lane / 16, lc = (lane % 16) ^ lg_swz_n(row);
    dvo_k = (unsigned)row * krb + ((unsigned)lc << 4);
    dvo_v = (unsigned)row * vrb + ((unsigned)lc << 4);
    const int rr = wave * 8 + lane / 8, lr = (lane % 8) ^ lg_swz_r(rr);
    dvo_r = (unsigned)rr * krb + LG_DV * 2 + ((unsigned)lr << 4);
  }
  // tile t -> buffer buf (hipcc does not count these loads: stage_wait waits vmcnt(0)). The whole offset in voffset, i.e. inside the
  // descriptor's range check: what follows a sequence's last key is another sequence or the end of the tensor, and both must read as
  // zeros. (The scalar part through an opaque copy: one v_add with a scalar operand per load, no per-piece vector registers.)
  auto stage_load = [&](int t, int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned sok = (unsigned)(t * BN + j * 16) * krb, sov = (unsigned)(t * BN + j * 16) * vrb;
      asm volatile("" : "+s"(sok), "+s"(sov));
      const unsigned lk = ku0 + buf * LG_BUF + (wave + 4 * j) * 1024;
      const unsigned lv = lk + LG_WIDE;
      const unsigned vk = dvo_k + sok, vv = dvo_v + sov;
      LG_DMA(lk, vk, rk);
      LG_DMA(lv, vv, rv);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned sor = (unsigned)(t * BN + j * 32) * krb;
      asm volatile("" : "+s"(sor));
      const unsigned lr = ku0 + buf * LG_BUF + LG_IMGN + (wave + 4 * j) * 1024;
      const unsigned vr = dvo_r + sor;
      LG_DMA(lr, vr, rk);
    }
  };
  auto stage_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  f32x16 dqacc[LG_DB];
#pragma unroll
  for (int db = 0; db < LG_DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dqacc[db][i] = 0.0f;

  stage_load(0, 0);
  stage_wait();
#pragma unroll
  for (int ks = 0; ks < LG_KS; ++ks)  // Q~ = round(c.Q): the very operand the forward multiplied
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[ks][j] = (elem)((float)qf[ks][j] * c2);
#pragma unroll
  for (int ks = 0; ks < LG_KS; ++ks) asm volatile("" : "+v"(qf[ks]));  // retire the prologue loads
#pragma unroll
  for (int ks = 0; ks < LG_KSN; ++ks) asm volatile("" : "+v"(dof[ks]));
  __syncthreads();

  for (int t = 0; t < nT; ++t) {
    const int buf = t & 1;
    if (t + 1 < nT) stage_load(t + 1, buf ^ 1);
    const int kv0 = t * BN;
    if (!CAUSAL || kv0 <= qw0 + WM - 1 + coff) {
      // masked: key > query (causal), and -- the partial last tile -- key >= Lk: those K / V rows arrive as zeros through the
      // descriptor, S' = -lse.log2e there, and with a strongly negative lse P = exp2(S') overflows the cast of dS (inf x 0 = NaN in dQ)
      const bool need_mask = (CAUSAL && (kv0 + BN - 1 > qw0 + coff)) || (kv0 + BN > LK);
      // One 32-key half (kb) at a time -- scores, dS, then its share of dQ -- so that only one score and one dP tuple are live
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 sk_, dpk, nlse, ndlt;
        asm volatile("" : "+v"(nl1), "+v"(nd1));  // opaque: the splats are formed here, not hoisted
#pragma unroll
        for (int i = 0; i < 16; ++i) { nlse[i] = nl1; ndlt[i] = nd1; }
        __builtin_amdgcn_s_setprio(1);  // matrix phases above the other wave's arithmetic
        {
          // 20 row fragments -- K and V alternating over the eight nope k-steps (the head_dim-128 kernel's order), then the four rotary
          // K fragments -- each read LA products ahead of the MFMA that consumes it
          constexpr int NF = 2 * LG_KSN + LG_KSR, LA = FA_BWD_LA;
          vec8 fr[NF];
          auto fread = [&](int f) {
            if (f < 2 * LG_KSN) fr[f] = __builtin_bit_cast(vec8, lds_read_b128(at(xat(rown, (f / 2) << 5) + ((f & 1) ? LG_WIDE : 0) + kb * 32 * LG_NRB)));
            else fr[f] = __builtin_bit_cast(vec8, lds_read_b128(at(xat(rowr, (f - 2 * LG_KSN) << 5) + kb * 32 * LG_RRB)));
          };
#pragma unroll
          for (int f = 0; f < LA; ++f) fread(f);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            if (f < 2 * LG_KSN) {
              const int ks = f / 2;
              if (f & 1) dpk = M::mfma(fr[f], dof[ks], ks == 0 ? ndlt : dpk);
              else sk_ = M::mfma(fr[f], qf[ks], ks == 0 ? nlse : sk_);
            } else {
              sk_ = M::mfma(fr[f], qf[f - LG_KSN], sk_);
            }
            if (f + LA < NF) fread(f + LA);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        // dQ^T += K^T.dS^T : step j = (st, db), db 0..3 from the nope part and 4..5 from the rotary part; the transposed K fragments
        // are read LA2 steps ahead of their MFMA, the first ones before the dS arithmetic (they do not depend on it)
        constexpr int NJ = 2 * LG_DB, LA2 = FA_BWD_LA2;
        s16x4 tlo[NJ], thi[NJ];
        auto tread = [&](int j) {
          const int R0 = 32 * kb + 16 * (j / LG_DB), db = j % LG_DB;
          if (db < LG_DBN) {
            tlo[j] = lds_read_tr16(at(xat(trn[(R0 >> 3) % 2], db << 6) + R0 * LG_NRB));
            thi[j] = lds_read_tr16(at(xat(trn[((R0 >> 3) + 1) % 2], db << 6) + (R0 + 8) * LG_NRB));
          } else {
            tlo[j] = lds_read_tr16(at(xat(trr[(R0 >> 3) % 4], (db - LG_DBN) << 6) + R0 * LG_RRB));
            thi[j] = lds_read_tr16(at(xat(trr[((R0 >> 3) + 1) % 4], (db - LG_DBN) << 6) + (R0 + 8) * LG_RRB));
          }
        };
#pragma unroll
        for (int j = 0; j < LA2; ++j) tread(j);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
        if (need_mask) {  // key > query -> masked; a wave-uniform branch
          // (the row and the lane half formed again from the lane index, so that they are not held across the loops)
          int lane_m = lane;
          asm volatile("" : "+v"(lane_m));
          int lim = LK - 1 - kv0 - 32 * kb;
          if (CAUSAL) lim = min(lim, qw0 + (lane_m & 31) + coff - kv0 - 32 * kb);
          lim -= 4 * (lane_m >> 5);
#pragma unroll
          for (int i = 0; i < 16; ++i) sk_[i] = ((i & 3) + 8 * (i >> 2) > lim) ? -INFINITY : sk_[i];
        }
        // dS^T = P^T o (dP^T - delta) (the softmax scale goes onto the finished dQ): keys in the registers, the query on the lane
#pragma unroll
        for (int i = 0; i < 16; ++i) sk_[i] = __builtin_amdgcn_exp2f(sk_[i]) * dpk[i];
        vec8 df[2];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int j = 0; j < 8; ++j) df[st][j] = (elem)sk_[8 * st + j];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const s16x8 k8 = __builtin_shufflevector(tlo[j], thi[j], 0, 1, 2, 3, 4, 5, 6, 7);
          dqacc[j % LG_DB] = M::mfma(__builtin_bit_cast(vec8, k8), df[j / LG_DB], dqacc[j % LG_DB]);
          if (j + LA2 < NJ) tread(j + LA2);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    rown += flip; rowr += flip;
    asm volatile("" : "+v"(rown), "+v"(rowr));
#pragma unroll
    for (int tv = 0; tv < 2; ++tv) { trn[tv] += flip; asm volatile("" : "+v"(trn[tv])); }
#pragma unroll
    for (int tv = 0; tv < 4; ++tv) { trr[tv] += flip; asm volatile("" : "+v"(trr[tv])); }
    flip = -flip;
    if (t + 1 < nT) stage_wait();
    __syncthreads();
  }
  // dQ^T[d][q]: lane (q = r, h) holds d = 32db + 8g4 + 4h + 0..3 -> one 16-byte store per group, under q's strides
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int qrow_e = qw0 + (lane_e & 31), h_e = lane_e >> 5;
  if (qrow_e < LQ) {
    float *dq = p.dq + base_q + (long long)qrow_e * p.q_rs;
#pragma unroll
    for (int db = 0; db < LG_DB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 w = make_float4(dqacc[db][4 * g4] * p.scale, dqacc[db][4 * g4 + 1] * p.scale, dqacc[db][4 * g4 + 2] * p.scale,
                                     dqacc[db][4 * g4 + 3] * p.scale);
        *reinterpret_cast<float4 *>(dq + 32 * db + 8 * g4 + 4 * h_e) = w;
      }
  }
}

// dK, dV: workgroup = 128 keys, wave = 32 keys (key on the lane, queries in the registers)
template <typename Tag, bool CAUSAL>
__global__ __launch_bounds__(NTHREADS, LG_KV_OCC) void mla_grad_kv_kernel(BwdMlaParams p) {
  using M = MT<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  constexpr int BT = BN;
  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;  // [2] buffers of [Q nope | Q rotary | dO]
  lds_char *ROWS = smem + 2 * LG_BUF;         // [2][2][BT] floats: -lse*log2e, -delta of the tile's query rows (the chains' initial accumulators)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // one workgroup per (key block, key/value head): it visits the G = H / Hkv query heads that read this head one after the other, so
  // grouped-query dK / dV are summed in registers
  const int BHK = p.B * p.Hkv, G = p.H / p.Hkv;
  const int kvb = blockIdx.x / BHK;  // ascending: under the causal mask the first key blocks see the most queries
  const int bhk = blockIdx.x % BHK, bi = bhk / p.Hkv, hk = bhk % p.Hkv;
  // (the tables are read and clamped as in the dQ kernel; a block past its sequence's last key leaves in front of every barrier)
  const int sq = min(max(p.cu_q[bi], 0), p.total_q), eq = min(max(p.cu_q[bi + 1], 0), p.total_q);
  const int sk = min(max(p.cu_k[bi], 0), p.total_k), ek = min(max(p.cu_k[bi + 1], 0), p.total_k);
  const int LQ = min(max(eq - sq, 0), p.N);
  const int LK = min(max(ek - sk, 0), p.Nk);
  if (kvb * BM >= LK) return;
  const int seq_q = sq;
  const long long base_k = (long long)sk * p.kv_rs + (long long)hk * p.kv_head_stride;
  const long long base_v = (long long)sk * p.v_rs + (long long)hk * p.v_head_stride;
  const unsigned qrb = (unsigned)p.q_rs * 2, orb = (unsigned)p.o_rs * 2, krb = (unsigned)p.kv_rs * 2, vrb = (unsigned)p.v_rs * 2;
  const int k0 = kvb * BM, kw0 = k0 + wave * WM, krow = kw0 + r;

  // (a sequence without queries stages nothing -- its keys get dK = dV = 0 -- and its query descriptors are empty)
  const unsigned q_bytes = LQ > 0 ? (unsigned)(LQ - 1) * qrb + LG_DQK * 2 : 0u, o_bytes = LQ > 0 ? (unsigned)(LQ - 1) * orb + LG_DV * 2 : 0u;
  const unsigned k_bytes = (unsigned)(LK - 1) * krb + LG_DQK * 2, v_bytes = (unsigned)(LK - 1) * vrb + LG_DV * 2;
  const int coff = LK - LQ;        // (may be negative)
  __amdgpu_buffer_rsrc_t rq, rdo;  // of the query head being visited (set_head)
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.k + base_k), 0, k_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.v + base_v), 0, v_bytes, 0x00020000);

  vec8 kf[LG_KS], vf[LG_KSN];  // B operands: lane (r,h) holds key row krow, columns 16ks+8h..
#pragma unroll
  for (int ks = 0; ks < LG_KS; ++ks)
    kf[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rk, (unsigned)krow * krb + (2 * ks + h) * 16, 0, 0));
#pragma unroll
  for (int ks = 0; ks < LG_KSN; ++ks)
    vf[ks] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(rv, (unsigned)krow * vrb + (2 * ks + h) * 16, 0, 0));
  const float c2 = p.scale * LOG2E;

  const unsigned qu0 = (unsigned)(__UINTPTR_TYPE__)smem;
  unsigned koff[LG_KSN], koffr[LG_KSR];  // ABSOLUTE LDS addresses in the current buffer (the dO image is LG_WIDE behind the nope part)
#pragma unroll
  for (int ks = 0; ks < LG_KSN; ++ks) koff[ks] = qu0 + r * LG_NRB + (((2 * ks + h) ^ lg_swz_n(r)) << 4);
#pragma unroll
  for (int ks = 0; ks < LG_KSR; ++ks) koffr[ks] = qu0 + LG_IMGN + r * LG_RRB + (((2 * ks + h) ^ lg_swz_r(r)) << 4);
  const int g1 = (lane >> 4) & 1, vq = (lane >> 2) & 3, vp = lane & 3;
  unsigned voff[2][LG_DBN], voffr[4][LG_DBR];
#pragma unroll
  for (int tv = 0; tv < 2; ++tv)
#pragma unroll
    for (int db = 0; db < LG_DBN; ++db) voff[tv][db] = qu0 + lg_tr_n(tv, db, h, g1, vq, vp);
#pragma unroll
  for (int tv = 0; tv < 4; ++tv)
#pragma unroll
    for (int db = 0; db < LG_DBR; ++db) voffr[tv][db] = qu0 + LG_IMGN + lg_tr_r(tv, db, h, g1, vq, vp);
  unsigned rowoff = (unsigned)(__UINTPTR_TYPE__)ROWS + 4 * h * 4;
  int flip = LG_BUF, flip_rows = 2 * BT * 4;  // to the other buffer and back
  auto at = [](unsigned a) { return (const lds_char *)(__UINTPTR_TYPE__)a; };
  // query tiles of BT rows; under the causal mask only tiles that reach this block's first key
  const int nTq = (LQ + BT - 1) / BT;
  const int t_begin = CAUSAL ? max(k0 - coff, 0) / BT : 0;  // the first query that sees key k0 is k0 - coff
  static_assert(2 * BT <= NTHREADS, "one thread per staged row constant");

  // waves 0 (lse) and 1 (delta) stage the row constants: the RAW loaded value here, scaled / negated in stage_write (arithmetic on it
  // here would make hipcc wait for the whole tile's loads at the top of every iteration)
  float rowv = 0.0f;
  const float *row_src = nullptr;
  auto set_head = [&](int g) {
    const int hq = hk * G + g;
    const long long bq = (long long)seq_q * p.q_rs + (long long)hq * p.head_stride;
    const long long bo = (long long)seq_q * p.o_rs + (long long)hq * p.o_head_stride;
    const long long rows0 = (long long)hq * p.total_q + seq_q;
    rq = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.q + bq), 0, q_bytes, 0x00020000);
    rdo = __builtin_amdgcn_make_buffer_rsrc((void *)((const elem *)p.d_o + bo), 0, o_bytes, 0x00020000);
    row_src = (wave < BT / 64 ? p.lse : p.delta) + rows0;
  };
  unsigned dvo_q, dvo_o, dvo_r;
  {
    const int row = wave * 4 + lane / 16, lc = (lane % 16) ^ lg_swz_n(row);
    dvo_q = (unsigned)row * qrb + ((unsigned)lc << 4);
    dvo_o = (unsigned)row * orb + ((unsigned)lc << 4);
    const int rr = wave * 8 + lane / 8, lr = (lane % 8) ^ lg_swz_r(rr);
    dvo_r = (unsigned)rr * qrb + LG_DV * 2 + ((unsigned)lr << 4);
  }
  auto stage_load = [&](int t, int buf) {  // (the whole offset in voffset, inside the descriptor's range check: see the dQ kernel)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned soq = (unsigned)(t * BT + j * 16) * qrb, soo = (unsigned)(t * BT + j * 16) * orb;
      asm volatile("" : "+s"(soq), "+s"(soo));
      const unsigned lq = qu0 + buf * LG_BUF + (wave + 4 * j) * 1024;
      const unsigned lo = lq + LG_WIDE;
      const unsigned vq_ = dvo_q + soq, vo_ = dvo_o + soo;
      LG_DMA(lq, vq_, rq);
      LG_DMA(lo, vo_, rdo);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned sor = (unsigned)(t * BT + j * 32) * qrb;
      asm volatile("" : "+s"(sor));
      const unsigned lr = qu0 + buf * LG_BUF + LG_IMGN + (wave + 4 * j) * 1024;
      const unsigned vr = dvo_r + sor;
      LG_DMA(lr, vr, rq);
    }
    if (wave < 2 * BT / 64) {
      int ti = t;
      asm volatile("" : "+s"(ti));
      const int qi = ti * BT + lane;
      rowv = row_src[qi < LQ ? qi : LQ - 1];
    }
  };
  auto stage_write = [&](int buf, int wt) {  // wt = the tile the staged value belongs to
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wave < 2 * BT / 64) {  // (rows past the end get p = 0 through -inf)
      const int qi = wt * BT + lane;
      // (under the mask, Lk < Lq: a row with no visible key -- the forward's integer test; its LSE is -inf and its delta of no use -- is
      // staged like a row past the end: -inf and 0, so the +inf never reaches a score chain and the row adds exactly nothing)
      const bool live = CAUSAL ? (qi < LQ && qi + coff >= 0) : (qi < LQ);
      const float v = (wave < BT / 64) ? (live ? -rowv * LOG2E : -INFINITY) : (live ? -rowv : 0.0f);
      lds_write_b32(ROWS + buf * (2 * BT * 4) + wave * 256 + lane * 4, __builtin_bit_cast(unsigned, v));
    }
  };

  f32x16 dkacc[LG_DB], dvacc[LG_DBN];
#pragma unroll
  for (int db = 0; db < LG_DB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dkacc[db][i] = 0.0f;
#pragma unroll
  for (int db = 0; db < LG_DBN; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) dvacc[db][i] = 0.0f;

  set_head(0);
  if (t_begin < nTq) {
    stage_load(t_begin, 0);
    stage_write(0, t_begin);
  }
#pragma unroll
  for (int ks = 0; ks < LG_KS; ++ks)  // K~ = round(c.K): S' = Q.K~ comes out in log2 units
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[ks][j] = (elem)((float)kf[ks][j] * c2);
#pragma unroll
  for (int ks = 0; ks < LG_KS; ++ks) asm volatile("" : "+v"(kf[ks]));
#pragma unroll
  for (int ks = 0; ks < LG_KSN; ++ks) asm volatile("" : "+v"(vf[ks]));
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
      const int qt0 = t * BT;
      if (!CAUSAL || qt0 + BN - 1 + coff >= kw0) {  // some query of the tile sees this wave's first key
        const unsigned rows = rowoff;
        // only tiles that cross the diagonal for this wave need the per-element mask (wave-uniform)
        const bool need_mask = CAUSAL && (qt0 + coff < kw0 + WM - 1);
        // One 32-query half (qb) at a time -- scores, P / dS, then its share of dV / dK -- so that only ONE score and ONE dP tuple are live
        static_for<0, 2>([&](auto qbc) {
          constexpr int qb = decltype(qbc)::value;
          f32x16 sq_, dpq;
          __builtin_amdgcn_s_setprio(1);
          // the chains start from the row constants: registers 4g..4g+3 are query rows 32qb + 8g + 4h + 0..3 of the tile
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) {
            const int ql = 32 * qb + 8 * gg;  // (+ 4h: in rowoff)
            const u32x4 l4 = lds_read_b128(at(rows + ql * 4));
            const u32x4 d4 = lds_read_b128(at(rows + BT * 4 + ql * 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const unsigned lw = l4[e], dw = d4[e];  // (scalar temporaries on purpose: see fa_bwd_dkdv_body.inc)
              sq_[4 * gg + e] = __builtin_bit_cast(float, lw);
              dpq[4 * gg + e] = __builtin_bit_cast(float, dw);
            }
          }
          {
            // 20 row fragments: Q and dO alternating over the eight nope k-steps (the head_dim-128 kernel's order), then the rotary Q ones
            constexpr int NF = 2 * LG_KSN + LG_KSR, LA = FA_BWD_KV128_LA;
            vec8 fr[NF];
            auto fread = [&](auto fc) {
              constexpr int f = decltype(fc)::value;
              if constexpr (f < 2 * LG_KSN) fr[f] = __builtin_bit_cast(vec8, lds_read_b128(at(koff[f / 2] + ((f & 1) ? LG_WIDE : 0) + qb * 32 * LG_NRB)));
              else fr[f] = __builtin_bit_cast(vec8, lds_read_b128(at(koffr[f - 2 * LG_KSN] + qb * 32 * LG_RRB)));
            };
            static_for<0, LA>([&](auto fc) { fread(fc); });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, NF>([&](auto fc) {
              constexpr int f = decltype(fc)::value;
              if constexpr (f >= 2 * LG_KSN) sq_ = M::mfma(fr[f], kf[f - LG_KSN], sq_);
              else if constexpr (f & 1) dpq = M::mfma(fr[f], vf[f / 2], dpq);
              else sq_ = M::mfma(fr[f], kf[f / 2], sq_);
              if constexpr (f + LA < NF) fread(std::integral_constant<int, f + LA>{});
              __builtin_amdgcn_sched_barrier(0);
            });
          }
          // dV / dK fragments of this half. Step j = (st, i): i = 0..7 alternates dO^T (-> dV) and Q^T (-> dK) over output blocks 0..3 of
          // the 256-byte images, in the head_dim-128 kernel's order; i = 8, 9 are the rotary part's two dK blocks. Read LA2 steps ahead.
          constexpr int NI = 2 * LG_DBN + LG_DBR, NJ = 2 * NI, LA2 = FA_BWD_KV128_LA2;
          s16x4 tlo[NJ], thi[NJ];
          auto tread = [&](auto jc) {
            constexpr int j = decltype(jc)::value, st = j / NI, i = j % NI, R0 = 32 * qb + 16 * st;
            if constexpr (i < 2 * LG_DBN) {
              constexpr int db = i / 2, src = (i & 1) ? 0 : LG_WIDE;
              tlo[j] = lds_read_tr16(at(voff[(R0 >> 3) % 2][db] + src + R0 * LG_NRB));
              thi[j] = lds_read_tr16(at(voff[((R0 >> 3) + 1) % 2][db] + src + (R0 + 8) * LG_NRB));
            } else {
              constexpr int db = i - 2 * LG_DBN;
              tlo[j] = lds_read_tr16(at(voffr[(R0 >> 3) % 4][db] + R0 * LG_RRB));
              thi[j] = lds_read_tr16(at(voffr[((R0 >> 3) + 1) % 4][db] + (R0 + 8) * LG_RRB));
            }
          };
          static_for<0, LA2>([&](auto jc) { tread(jc); });
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_setprio(0);
          if (need_mask) {  // key > query: S' = -inf there. A wave-uniform BRANCH; register 4g+e holds query qt0 + 32qb + 8g + 4h + e,
            // compared as a constant against ONE per-lane limit
            int lane_m = lane;
            asm volatile("" : "+v"(lane_m));
            const int lim = kw0 + (lane_m & 31) - coff - 4 * (lane_m >> 5) - qt0 - 32 * qb;
#pragma unroll
            for (int i = 0; i < 16; ++i) sq_[i] = (8 * (i >> 2) + (i & 3) < lim) ? -INFINITY : sq_[i];
          }
          vec8 pf[2], df[2];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float pv = __builtin_amdgcn_exp2f(sq_[i]);  // S' = Q.K~ - lse*log2e came out of the matrix core
            sq_[i] = pv;
            dpq[i] = pv * dpq[i];  // dS (without the softmax scale: it goes onto the finished dK)
          }
#pragma unroll
          for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              pf[st][j] = (elem)sq_[8 * st + j];
              df[st][j] = (elem)dpq[8 * st + j];
            }
          // dV^T += dO^T.P ; dK^T += Q^T.dS   (reduction over this half's 32 query rows)
          __builtin_amdgcn_s_setprio(1);
          static_for<0, NJ>([&](auto jc) {
            constexpr int j = decltype(jc)::value, st = j / NI, i = j % NI;
            const s16x8 a8 = __builtin_shufflevector(tlo[j], thi[j], 0, 1, 2, 3, 4, 5, 6, 7);
            if constexpr (i >= 2 * LG_DBN) dkacc[LG_DBN + i - 2 * LG_DBN] = M::mfma(__builtin_bit_cast(vec8, a8), df[st], dkacc[LG_DBN + i - 2 * LG_DBN]);
            else if constexpr (i & 1) dkacc[i / 2] = M::mfma(__builtin_bit_cast(vec8, a8), df[st], dkacc[i / 2]);
            else dvacc[i / 2] = M::mfma(__builtin_bit_cast(vec8, a8), pf[st], dvacc[i / 2]);
            if constexpr (j + LA2 < NJ) tread(std::integral_constant<int, j + LA2>{});
            __builtin_amdgcn_sched_barrier(0);
          });
        });
      }
#pragma unroll
      for (int ks = 0; ks < LG_KSN; ++ks) {
        koff[ks] += flip;
        asm volatile("" : "+v"(koff[ks]));
      }
#pragma unroll
      for (int ks = 0; ks < LG_KSR; ++ks) {
        koffr[ks] += flip;
        asm volatile("" : "+v"(koffr[ks]));
      }
#pragma unroll
      for (int tv = 0; tv < 2; ++tv)
#pragma unroll
        for (int db = 0; db < LG_DBN; ++db) {
          voff[tv][db] += flip;
          asm volatile("" : "+v"(voff[tv][db]));
        }
#pragma unroll
      for (int tv = 0; tv < 4; ++tv)
#pragma unroll
        for (int db = 0; db < LG_DBR; ++db) {
          voffr[tv][db] += flip;
          asm volatile("" : "+v"(voffr[tv][db]));
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
  // dK under k's strides (192 wide), dV under v's (128 wide): lane (key = r, h) holds d = 32db + 8g4 + 4h + 0..3
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int krow_e = kw0 + (lane_e & 31), h_e = lane_e >> 5;
  if (krow_e < LK) {
    float *dk = p.dk + base_k + (long long)krow_e * p.kv_rs, *dv = p.dv + base_v + (long long)krow_e * p.v_rs;
#pragma unroll
    for (int db = 0; db < LG_DB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * db + 8 * g4 + 4 * h_e;
        *reinterpret_cast<float4 *>(dk + d0) = make_float4(dkacc[db][4 * g4] * p.scale, dkacc[db][4 * g4 + 1] * p.scale, dkacc[db][4 * g4 + 2] * p.scale,
                                                             dkacc[db][4 * g4 + 3] * p.scale);
      }
#pragma unroll
    for (int db = 0; db < LG_DBN; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d0 = 32 * db + 8 * g4 + 4 * h_e;
        *reinterpret_cast<float4 *>(dv + d0) = make_float4(dvacc[db][4 * g4], dvacc[db][4 * g4 + 1], dvacc[db][4 * g4 + 2], dvacc[db][4 * g4 + 3]);
      }
  }
  (void)r; (void)krow;
}

bool bwd_varlen_mla_supported(int dtype, int Dqk, int Dv) {
  return (dtype == FA_DTYPE_F16 || dtype == FA_DTYPE_BF16) && Dqk == LG_DQK && Dv == LG_DV;
}

// One call: dQ first -- it leaves delta in the workspace for the dK/dV kernel -- then dK/dV on the same stream, one error check at the
// end. max_q / max_k size the grids (host scalars only: the call can be captured in a graph).
hipError_t launch_bwd_varlen_mla(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                                 float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                                 int total_k, int max_q, int max_k, float scale, long long q_rs, long long q_hs, long long k_rs,
                                 long long k_hs, long long v_rs, long long v_hs, long long o_rs, long long o_hs, int causal, int dtype,
                                 hipStream_t s) {
  BwdMlaParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.d_o = d_o; p.lse = lse;
  p.dq = dq; p.dk = dk; p.dv = dv; p.delta = ws;
  p.B = B; p.H = H; p.N = max_q; p.D = LG_DQK; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_hs; p.is_causal = causal;
  p.Hkv = Hkv; p.Nk = max_k; p.kv_batch_stride = 0; p.kv_head_stride = k_hs;
  p.cu_q = cu_q; p.cu_k = cu_k; p.total_q = total_q; p.total_k = total_k; p.q_rs = q_rs; p.kv_rs = k_rs;
  p.v_rs = v_rs; p.v_head_stride = v_hs; p.o_rs = o_rs; p.o_head_stride = o_hs;
  auto launch = [&](auto kq, auto kk) {
    const int nBq = (max_q + BM - 1) / BM, nBk = (max_k + BM - 1) / BM;
    const size_t smem_q = mla_grad_q_lds_bytes(), smem_kv = mla_grad_kv_lds_bytes();
    hipError_t e = set_dyn_lds_once((const void *)kk, (int)smem_kv);
    if (e != hipSuccess) return e;
    e = set_dyn_lds_once((const void *)kq, (int)smem_q);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();  // do not report an older sticky error as this launch's
    hipLaunchKernelGGL(kq, dim3(nBq * B * H), dim3(NTHREADS), smem_q, s, p);
    hipLaunchKernelGGL(kk, dim3(nBk * B * Hkv), dim3(NTHREADS), smem_kv, s, p);
    return hipGetLastError();
  };
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    return causal ? launch(mla_grad_q_kernel<Tag, true>, mla_grad_kv_kernel<Tag, true>)
                  : launch(mla_grad_q_kernel<Tag, false>, mla_grad_kv_kernel<Tag, false>);
  });
}

}  // namespace fa
