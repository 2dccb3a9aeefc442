// fa_mla_indexer_loss_kernel.hip -- the indexer's training loss over a per-token list of keys and its gradients: entry point
// fa_mla_indexer_loss_sparse (include/fa_mi355.h).
//   s_hj = q_idx[t,h] . k_idx(x_j),  I_j = sum_h w[t,h] max(0, s_hj),  pi = softmax_j I,  tau = target / sum target,
//   loss[t] = KL(tau || pi),  g_j = u_t (pi_j - tau_j),  and dw, dq_idx, dk_idx from G_hj = g_j w_h [s_hj > 0].
//
// One launch, ONE WORKGROUP OF FOUR WAVES PER TOKEN, two passes over the token's list. No key split: training chunks hold thousands of
// tokens.
//   * A TILE is the 64 index-key rows (256 bytes each) of 64 list entries: 16 KiB, double buffered, in the logits kernel's image (row r at
//     r * 256, its 16-byte chunk k at position k ^ (r & 15)). A 256-byte row fills only 16 of the 64 lanes of an LDS-DMA instruction, so
//     the rows go THROUGH REGISTERS instead, as the rotary bytes of the latent tiles do: wave w moves rows 16 w .. 16 w + 15 in four
//     instructions of four rows, every lane one 16-byte chunk on the row's own 64-bit address; the loads of tile t + 1 are issued at the
//     head of iteration t and written to LDS at its end. An entry behind n_t or outside the pool forms no address: its chunks are zeros.
//     The slot of every row (-1 where no gradient may leave) stands next to the tile.
//   * THE QUERY of the token, Hi x 128, is the A operand of the score product in both passes: Hi / 16 x 4 fragments, 64 registers at
//     Hi = 64, loaded once (the logits kernel's arrangement: lane (c, g) ends up with heads 16 m + 4 g + i against key c).
//   * PASS 1: wave w takes keys 16 w .. 16 w + 15 of every tile: score MFMAs, relu, the weighted head sum in the lane plus two cross-lane
//     adds, I_j into an LDS row of IL_MAXK floats. Then the workgroup's max, sum of exponentials and sum of targets (wave butterflies,
//     then the four waves' values in wave order: a fixed order), the loss, and g_j written over I_j in place. A loss-only call stops here.
//   * PASS 2 stages the tiles again and recomputes S the same way (the same bits: the mask [s > 0] is pass 1's). PHASE A: G rounded to the
//     type into an exchange area in two forms, [head][key] and [key][head]; dw accumulates g_j max(0, s_hj) in the lane. One barrier.
//     PHASE B, by columns: wave w owns columns 32 w .. 32 w + 31. dq^T[column][head] += K^T . G^T over the tile's 64 keys: transposed
//     reads of the image (ds_read_b64_tr_b16) as A, G by [head][key] as B in the key order those reads imply. PHASE C, the same columns:
//     dk[key][column] = G^T . Q contracts over all Hi heads (Q by columns in registers, Hi / 32 k-steps), so the sum over heads is complete
//     before ONE fp32 atomic add per (listed row, column).
//   * REPRODUCIBILITY: loss, dq and dw are sums in a fixed order; dk is accumulated by atomics in an order that varies from run to run.
//   * BARRIERS: every wave meets every barrier: the token, n_t and the target's sum are workgroup-uniform.
#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // ML16 and f32x4: the 16x16x32 matrix-core types of the family

constexpr int IL_D = 128;             // columns of an index query / key
constexpr int IL_RB = IL_D * 2;       // bytes of a key row
constexpr int IL_TILE = BN * IL_RB;   // one 64-key tile: 16 KiB
constexpr int IL_NW = 4;              // waves of a workgroup
constexpr int IL_KS = IL_D / 32;      // k-steps of a dot
constexpr int IL_MAXK = 4096;         // list entries the LDS row of I / g holds: the call's topk limit
constexpr int IL_HMAX = 64;           // most index heads
constexpr int IL_TRB = BN * 2 + 8;    // row bytes of G by [head][key] (padded against bank conflicts)
constexpr int IL_KRB = IL_HMAX * 2 + 16;  // row bytes of G by [key][head]
// LDS: the double buffer, the row of I / g, the two buffers' slots, the exchange area, the reductions' scratch and dw's partials
constexpr int IL_ROW = 2 * IL_TILE;
constexpr int IL_SLOT = IL_ROW + IL_MAXK * 4;
constexpr int IL_GT = IL_SLOT + 2 * BN * 4;
constexpr int IL_GK = IL_GT + IL_HMAX * IL_TRB;
constexpr int IL_RED = IL_GK + BN * IL_KRB;
constexpr int IL_DW = IL_RED + 16 * 4;
constexpr int IL_LDS = IL_DW + IL_NW * IL_HMAX * 4;
static_assert(IL_LDS <= 80 * 1024 && IL_GT % 16 == 0 && IL_GK % 16 == 0 && IL_KRB % 16 == 0, "two workgroups per compute unit; 16-byte reads");

int mla_indexer_loss_max_topk() { return IL_MAXK; }

typedef __attribute__((address_space(3))) float il_lds_float;
__device__ __forceinline__ u32x2 il_read_b64(const lds_char *p) { return *reinterpret_cast<const __attribute__((address_space(3))) u32x2 *>(p); }

// the workgroup's max / sum of one value per thread: a butterfly in the wave, then the four waves' values in wave order. `red` holds four
// floats; two barriers, met by every thread
template <bool MAX>
__device__ __forceinline__ float il_block_reduce(float x, il_lds_float *red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float y = __shfl_xor(x, d, 64);
    x = MAX ? fmaxf(x, y) : x + y;
  }
  __syncthreads();  // (the previous reduction's reads are over)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int k = 1; k < IL_NW; ++k) r = MAX ? fmaxf(r, red[k]) : r + red[k];
  return r;
}

template <typename Tag, int HI>
__global__ __launch_bounds__(64 * IL_NW) void mla_idxloss_kernel(MlaIndexerLossParams p) {
  using M = ML16<Tag>;
  using vec8 = typename M::vec8;
  using elem = typename M::elem;
  typedef elem elem4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) elem lds_elem;
  constexpr int MT = HI / 16;  // 16-head row tiles of the score tile
  constexpr int KH = HI / 32;  // k-steps of the product that contracts over heads
  constexpr int NW = IL_NW;
  static_assert(HI <= IL_HMAX && HI % 32 == 0, "32 or 64 index heads");

  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  lds_char *smem = (lds_char *)smem_generic;
  il_lds_float *irow = (il_lds_float *)(smem + IL_ROW), *red = (il_lds_float *)(smem + IL_RED);

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;  // the token
  const int Nk = p.counts ? min(max(__builtin_amdgcn_readfirstlane(p.counts[b]), 0), p.topk) : p.topk;  // n_t
  const int nT = (Nk + BN - 1) / BN;
  const bool grads = p.dq != nullptr;
  float *dqr = p.dq + (long long)b * p.q_rs, *dwr = p.dw + (long long)b * p.w_rs;
  const float *tgt = p.target + (long long)b * p.target_stride;

  // a token without a loss: loss 0, zero dq and dw rows, nothing for dk
  auto leave_zero = [&]() __attribute__((always_inline)) {
    if (tid == 0) p.loss[b] = 0.0f;
    if (grads) {
      for (int e = tid; e < HI * (IL_D / 4); e += 64 * NW)
        *reinterpret_cast<f32x4 *>(dqr + (long long)(e / (IL_D / 4)) * p.q_hs + 4 * (e % (IL_D / 4))) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (tid < HI) dwr[tid] = 0.0f;
    }
  };
  if (Nk == 0) {  // recognised by the integer
    leave_zero();
    return;
  }

  // ---- the token's query fragments and head weights (the logits kernel's): heads 16 m + c as A rows; w of heads 16 m + 4 g + i
  vec8 qf[MT][IL_KS];
  float wv[MT][4];
  {
    const elem *qp = (const elem *)p.q + (long long)b * p.q_rs + 8 * g;
    const float *wp = p.w + (long long)b * p.w_rs + 4 * g;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int ks = 0; ks < IL_KS; ++ks)
        qf[m][ks] = __builtin_bit_cast(vec8, *reinterpret_cast<const u32x4 *>(qp + (long long)(16 * m + c) * p.q_hs + 32 * ks));
#pragma unroll
      for (int i = 0; i < 4; ++i) wv[m][i] = wp[16 * m + i];
    }
  }

  // ---- staging through registers: instruction k of wave w moves rows 16 w + 4 k + g of a tile, lane chunk c
  const int jr0 = 16 * w;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const int *list = p.indices + (long long)b * p.idx_stride;
  auto slot_off = [&](int x) __attribute__((always_inline)) { return ((long long)(x >> lp) * p.page_stride + (long long)(x & PM) * p.row_stride) * 2; };
  int ev = -1;
  auto fetch_entries = [&](int t) __attribute__((always_inline)) {
    const int j = t * BN + jr0 + lane;
    ev = -1;
    if (lane < 16 && j < Nk) ev = list[j];  // nothing behind n_t is read
  };
  u32x4 st[4];
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = __shfl(ev, 4 * k + g, 64);
      st[k] = u32x4{0u, 0u, 0u, 0u};
      if ((unsigned)x < (unsigned)p.num_slots) st[k] = *reinterpret_cast<const u32x4 *>((const char *)p.k + slot_off(x) + c * 16);
    }
    if (lane < 16) lds_write_b32(smem + IL_SLOT + (buf * BN + jr0 + lane) * 4, (unsigned)ev < (unsigned)p.num_slots ? (unsigned)ev : ~0u);
    fetch_entries(t + 1);
  };
  auto write_staged = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = 4 * k + g;  // (16 w + r) & 15 = r
      lds_write_b128(smem + buf * IL_TILE + (jr0 + r) * IL_RB + ((c ^ r) << 4), st[k]);
    }
  };
  // S of the wave's sixteen keys of the tile in `img`: acc[m][i] = s[head 16 m + 4 g + i][key 16 w + c]
  auto scores = [&](const lds_char *img, f32x4 (&acc)[MT]) __attribute__((always_inline)) {
    vec8 kf[IL_KS];
#pragma unroll
    for (int ks = 0; ks < IL_KS; ++ks) kf[ks] = __builtin_bit_cast(vec8, lds_read_b128(img + (jr0 + c) * IL_RB + (((4 * ks + g) ^ c) << 4)));
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < IL_KS; ++ks) acc[m] = M::mfma(qf[m][ks], kf[ks], acc[m]);
    }
  };

  // ---- pass 1: I_j into the row
  fetch_entries(0);
  for (int t = -1; t < nT; ++t) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // tile t is in LDS, and everyone has left iteration t - 1
    const int nb = (t + 1) & 1;
    if (t + 1 < nT) stage(t + 1, nb);
    if (t >= 0) {
      f32x4 acc[MT];
      scores(smem + (t & 1) * IL_TILE, acc);
      float s = 0.0f;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) s = __builtin_fmaf(wv[m][i], __builtin_fmaxf(acc[m][i], 0.0f), s);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (g == 0) irow[t * BN + jr0 + c] = s;  // (t * 64 + 63 < IL_MAXK: the call's topk limit)
    }
    if (t + 1 < nT) write_staged(nb);
  }

  // ---- the softmax over j < n_t, the target's sum, the loss (natural units, fp32)
  float mx = -INFINITY, ts = 0.0f;
  __syncthreads();
  for (int j = tid; j < Nk; j += 64 * NW) {
    mx = fmaxf(mx, irow[j]);
    ts += tgt[j];
  }
  mx = il_block_reduce<true>(mx, red);
  ts = il_block_reduce<false>(ts, red);
  if (!(ts > 0.0f)) {  // a target row whose sum is 0 (workgroup-uniform)
    leave_zero();
    return;
  }
  float z = 0.0f;
  for (int j = tid; j < Nk; j += 64 * NW) z += expf(irow[j] - mx);
  z = il_block_reduce<false>(z, red);
  const float lz = logf(z), u = p.loss_grad ? p.loss_grad[b] : 1.0f;
  float ls = 0.0f;
  for (int j = tid; j < Nk; j += 64 * NW) {
    const float d = irow[j] - mx, tau = tgt[j] / ts;
    if (tau > 0.0f) ls += tau * (logf(tau) - (d - lz));
    irow[j] = u * (expf(d) / z - tau);  // g_j, over I_j
  }
  ls = il_block_reduce<false>(ls, red);
  if (tid == 0) p.loss[b] = ls;
  if (!grads) return;

  // ---- pass 2. Q by columns for the product over heads: lane (c, g) holds heads 32 kh + 8 g .. + 7 at column 32 w + 16 dl + c
  vec8 qT[2][KH];
  {
    const elem *qb = (const elem *)p.q + (long long)b * p.q_rs + 32 * w + c;
#pragma unroll
    for (int dl = 0; dl < 2; ++dl)
#pragma unroll
      for (int kh = 0; kh < KH; ++kh)
#pragma unroll
        for (int j = 0; j < 8; ++j) qT[dl][kh][j] = qb[(long long)(32 * kh + 8 * g + j) * p.q_hs + 16 * dl];
  }
  // dq^T of the wave's columns: dqacc[dl][m][i] = dq[head 16 m + c][column 32 w + 16 dl + 4 g + i]
  f32x4 dqacc[2][MT];
  float dwacc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int dl = 0; dl < 2; ++dl) dqacc[dl][m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) dwacc[m][i] = 0.0f;
  }
  // per-lane offsets: the transposed reads' row 4 g + (c >> 2) and 8-byte piece c & 3 of a 16-column tile; the exchange area's rows
  const int vq = c >> 2, vp = c & 3, vrow = 4 * g + vq;
  const unsigned gt_w = (unsigned)(IL_GT + (4 * g) * IL_TRB + 2 * (jr0 + c));  // phase A: heads 16 m + 4 g + i, key 16 w + c
  const unsigned gk_w = (unsigned)(IL_GK + (jr0 + c) * IL_KRB + 2 * (4 * g));  // phase A: key 16 w + c, heads 16 m + 4 g ..
  const unsigned gt_r = (unsigned)(IL_GT + c * IL_TRB + 8 * g);                // phase B: head 16 m + c, keys 4 g ..
  const unsigned gk_r = (unsigned)(IL_GK + c * IL_KRB + 16 * g);               // phase C: key 16 kt + c, heads 8 g ..

  __syncthreads();  // g_j of every j stands in the row
  fetch_entries(0);
  for (int t = -1; t < nT; ++t) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int nb = (t + 1) & 1;
    if (t + 1 < nT) stage(t + 1, nb);
    if (t >= 0) {
      const lds_char *img = smem + (t & 1) * IL_TILE;
      // ---- phase A: S again, G = g_j w_h [s > 0] rounded to the type in both forms, dw in the lane
      {
        f32x4 acc[MT];
        scores(img, acc);
        const int j = t * BN + jr0 + c;
        const float gj = j < Nk ? irow[j] : 0.0f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          elem4 g4;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float s = acc[m][i];
            dwacc[m][i] = __builtin_fmaf(gj, __builtin_fmaxf(s, 0.0f), dwacc[m][i]);
            g4[i] = (elem)(s > 0.0f ? gj * wv[m][i] : 0.0f);
            *reinterpret_cast<lds_elem *>(smem + gt_w + (16 * m + i) * IL_TRB) = g4[i];
          }
          lds_write_b64(smem + gk_w + 32 * m, __builtin_bit_cast(u32x2, g4));
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // ---- phase B: dq^T += K^T . G^T. B: lane (c, g) holds G[head 16 m + c] at keys 32 kp + 16 (j >> 2) + 4 g + (j & 3), the order in
      // which the transposed reads deliver K
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        vec8 gb[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const lds_char *x = smem + gt_r + m * 16 * IL_TRB + 64 * kp;
          const u32x2 lo = il_read_b64(x), hi = il_read_b64(x + 32);
          gb[m] = __builtin_bit_cast(vec8, u32x4{lo[0], lo[1], hi[0], hi[1]});
        }
#pragma unroll
        for (int dl = 0; dl < 2; ++dl) {
          const int rr = 32 * kp + vrow;  // (rr + 16) & 15 = rr & 15: both reads under one swizzle
          const lds_char *vb = img + rr * IL_RB + (((2 * (2 * w + dl) + (vp >> 1)) ^ (rr & 15)) << 4) + 8 * (vp & 1);
          const s16x4 lo = lds_read_tr16(vb), hi = lds_read_tr16(vb + 16 * IL_RB);
          const vec8 kt8 = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
          for (int m = 0; m < MT; ++m) dqacc[dl][m] = M::mfma(kt8, gb[m], dqacc[dl][m]);
        }
      }
      // ---- phase C: dk[key][column] = G^T . Q over all heads, one atomic add per (listed row, column)
#pragma unroll
      for (int kt = 0; kt < BN / 16; ++kt) {
        vec8 ag[KH];
#pragma unroll
        for (int kh = 0; kh < KH; ++kh) ag[kh] = __builtin_bit_cast(vec8, lds_read_b128(smem + gk_r + kt * 16 * IL_KRB + 64 * kh));
        const u32x4 xs = lds_read_b128(smem + IL_SLOT + ((t & 1) * BN + 16 * kt + 4 * g) * 4);  // the slots of keys 16 kt + 4 g + i
        float *rowp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int x = (int)xs[i];
          rowp[i] = x < 0 ? nullptr : p.dk + ((long long)(x >> lp) * p.dk_page_stride + (long long)(x & PM) * p.dk_row_stride) + 32 * w + c;
        }
#pragma unroll
        for (int dl = 0; dl < 2; ++dl) {
          f32x4 out = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int kh = 0; kh < KH; ++kh) out = M::mfma(ag[kh], qT[dl][kh], out);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (rowp[i]) unsafeAtomicAdd(rowp[i] + 16 * dl, out[i]);
        }
      }
    }
    if (t + 1 < nT) write_staged(nb);
  }

  // ---- dq under q_idx's element strides: lane (c, g) writes columns 32 w + 16 dl + 4 g .. + 3 of head 16 m + c
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int dl = 0; dl < 2; ++dl) *reinterpret_cast<f32x4 *>(dqr + (long long)(16 * m + c) * p.q_hs + 32 * w + 16 * dl + 4 * g) = dqacc[dl][m];
  // ---- dw: the lane's sums over its keys, the sixteen key lanes by a butterfly, the four waves in wave order
  il_lds_float *dwp = (il_lds_float *)(smem + IL_DW);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float x = dwacc[m][i];
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
      if (c == 0) dwp[w * IL_HMAX + 16 * m + 4 * g + i] = x;
    }
  __syncthreads();
  if (tid < HI) dwr[tid] = ((dwp[tid] + dwp[IL_HMAX + tid]) + dwp[2 * IL_HMAX + tid]) + dwp[3 * IL_HMAX + tid];
}

// One launch: T workgroups of four waves
hipError_t launch_mla_indexer_loss(const MlaIndexerLossParams &p, int Hi, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    (void)hipGetLastError();
    auto go = [&](auto kern) {
      hipError_t e = set_dyn_lds_once((const void *)kern, IL_LDS);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, dim3(p.T), dim3(64 * IL_NW), IL_LDS, s, p);
      return hipGetLastError();
    };
    return Hi == 64 ? go(mla_idxloss_kernel<Tag, 64>) : go(mla_idxloss_kernel<Tag, 32>);
  });
}

}  // namespace fa
