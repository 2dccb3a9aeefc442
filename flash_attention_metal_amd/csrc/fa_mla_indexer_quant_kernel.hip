// fa_mla_indexer_quant_kernel.hip -- the input stage of the e4m3 indexer: the two kernels that WRITE what fa_mla_indexer_logits_paged_kv8
// reads. Entry points fa_mla_indexer_k_append_paged_quant (new index keys -> e4m3 bytes and one fp32 scale per key, in their slots of the
// index cache) and fa_mla_indexer_q_quant (index queries -> e4m3 bytes, the per-(token, head) scale folded into the head weights).
//   * THE ROW RULE (include/fa_mi355.h, "The MLA indexer's input stage") is one text, idxq_row, for both kernels: widen to fp32, seven
//     butterfly stages and one multiply by fp32(128^-0.5) when rotating, amax, the exponent, the codes. Every step is the single IEEE fp32
//     operation the header names, in its order: nothing here may reassociate, contract or run on the matrix core.
//   * ONE WAVE PER ROW, four rows per workgroup, no LDS and no barrier; every early exit is wave-uniform, so all 64 lanes are active in
//     every cross-lane step.
//   * LANE MAP: lane l holds elements 2 l and 2 l + 1 of the row -- one 4-byte load per lane, 256 contiguous bytes per wave. Bit 0 of
//     the element index is in-lane, bit s >= 1 is bit s - 1 of the lane id: butterfly stage 0 is in-lane, stage s >= 1 pairs lane l with
//     lane l ^ 2^(s-1). The lane whose bit is set holds the UPPER element of the pair and computes partner - own, as partner + (-own):
//     one sign flip by xor and one add, the same bits as the subtraction; the lower lane computes partner + own (addition commutes).
//   * THE EXCHANGE per stage (lane_xor): ^1 and ^2 are one DPP quad_perm each; ^4 is quad_perm [3, 2, 1, 0] then row_half_mirror
//     (i ^ 3 ^ 7); ^8 is row_mirror then row_half_mirror (i ^ 15 ^ 7); ^16 is v_permlane16_swap_b32 and ^32 v_permlane32_swap_b32, each
//     with both operands the value, followed by one select on the lane's bit (after the swap the first operand holds the lower partner's
//     value in both lanes of a pair, the second the upper one's: fa_mfma_common.h half_pair).
//   * AMAX by integer max on the fp32 bits (non-negative floats order as integers) over the same exchanges; after it every lane holds the
//     row's max and derives the exponent by fa_mla_kv_append_paged_scaled's integer rule, so e is wave-uniform without a broadcast.
//   * THE STORE: a lane converts its two elements with one v_cvt_pk_fp8_f32 (the clamp in front: the instruction gives NaN above 448, not
//     saturation), fetches lane l ^ 1's two bytes by one quad_perm, and the EVEN lanes store four bytes each: 32 stores of 4 bytes, 128
//     contiguous bytes per row. Lane 0 stores the scale (keys) or the folded weight (queries). Plain vector stores, no atomics.
#include "fa_mfma_common.h"

namespace fa {

constexpr int IDXQ_ROWS = 4;  // rows (= waves) per workgroup

// the value lane (l ^ M) holds, for every lane l of the wave
template <int M>
__device__ __forceinline__ int lane_xor(int x, int lane) {
  if constexpr (M == 1) return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]
  if constexpr (M == 2) return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);  // quad_perm [2, 3, 0, 1]
  if constexpr (M == 4)  // quad_perm [3, 2, 1, 0], then row_half_mirror
    return __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, x, 0x1B, 0xF, 0xF, true), 0x141, 0xF, 0xF, true);
  if constexpr (M == 8)  // row_mirror, then row_half_mirror
    return __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true), 0x141, 0xF, 0xF, true);
  if constexpr (M == 16 || M == 32) {
    // (inline asm and the s_nop: see half_pair in fa_mfma_common.h)
    int a = x, b = x;
    if constexpr (M == 16) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    else asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return (lane & M) ? a : b;
  }
}

// one butterfly stage across lanes: (lower, upper) <- (lower + upper, lower - upper), two elements per lane
template <int M>
__device__ __forceinline__ void butterfly(float (&x)[2], int lane) {
  const unsigned flip = (lane & M) ? 0x80000000u : 0u;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float partner = __builtin_bit_cast(float, lane_xor<M>(__builtin_bit_cast(int, x[j]), lane));
    x[j] = partner + __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x[j]) ^ flip);
  }
}

// The row rule on the lane's two 16-bit elements `in` (element 2 l in the low half). Returns the row's exponent e (the same in every
// lane); `word` is, in the even lanes, the four code bytes of elements 2 l .. 2 l + 3.
template <int DT, bool ROTATE>
__device__ __forceinline__ int idxq_row(unsigned in, int lane, unsigned &word) {
  float x[2];
  if constexpr (DT == FA_DTYPE_BF16) {
    x[0] = __builtin_bit_cast(float, in << 16);
    x[1] = __builtin_bit_cast(float, in & 0xffff0000u);
  } else {
    x[0] = (float)__builtin_bit_cast(_Float16, (unsigned short)(in & 0xffffu));
    x[1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(in >> 16));
  }
  if constexpr (ROTATE) {
    const float a = x[0] + x[1], b = x[0] - x[1];  // stage 0, in-lane
    x[0] = a;
    x[1] = b;
    butterfly<1>(x, lane);
    butterfly<2>(x, lane);
    butterfly<4>(x, lane);
    butterfly<8>(x, lane);
    butterfly<16>(x, lane);
    butterfly<32>(x, lane);
    const float c = 0.088388347648318440550f;  // fp32(128^-0.5) = 0x3DB504F3
    x[0] *= c;
    x[1] *= c;
  }
  int amax = max((int)(__builtin_bit_cast(unsigned, x[0]) & 0x7fffffffu), (int)(__builtin_bit_cast(unsigned, x[1]) & 0x7fffffffu));
  amax = max(amax, lane_xor<1>(amax, lane));
  amax = max(amax, lane_xor<2>(amax, lane));
  amax = max(amax, lane_xor<4>(amax, lane));
  amax = max(amax, lane_xor<8>(amax, lane));
  amax = max(amax, lane_xor<16>(amax, lane));
  amax = max(amax, lane_xor<32>(amax, lane));
  // the smallest e in [-32, 32] with amax <= 1.75 * 2^(8 + e): fa_mla_append_scaled_kernel.hip's rule
  const int e = min(max((amax >> 23) - 127 - 8 + ((amax & 0x7fffff) > 0x600000 ? 1 : 0), -32), 32);
  const float inv = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);  // 2^-e
  const float f0 = fminf(fmaxf(x[0] * inv, -448.0f), 448.0f), f1 = fminf(fmaxf(x[1] * inv, -448.0f), 448.0f);
  int cw;
  asm volatile("" : "=v"(cw));  // (the conversion keeps the other half of its destination: start from an undefined register)
  cw = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, cw, false);
  word = ((unsigned)cw & 0xffffu) | ((unsigned)lane_xor<1>(cw, lane) << 16);
  return e;
}

// fa_mla_indexer_k_append_paged_quant. Placement is fa_mla_kv_append_paged_scaled's, line for line.
template <int DT, bool ROTATE>
__global__ __launch_bounds__(64 * IDXQ_ROWS) void idxq_key_rows_kernel(MlaIndexerKQuantParams q) {
  const AppendPagedParams &p = q.a;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nblk = (p.max_new + IDXQ_ROWS - 1) / IDXQ_ROWS;
  const int b = (int)blockIdx.x / nblk, rb = (int)blockIdx.x - b * nblk;
  const int s0 = min(max(p.cu_new[b], 0), p.total_new), e0 = min(max(p.cu_new[b + 1], 0), p.total_new);
  const int n = min(max(e0 - s0, 0), p.max_new);
  const long long first = (long long)p.seqlens[b] - n;  // key position of the sequence's first new token
  const long long cap = (long long)p.max_pages << p.lp;
  const int i = rb * IDXQ_ROWS + w;  // the wave's new row: everything up to the load is wave-uniform
  if (i >= n) return;
  const long long pos = first + i;
  if (pos < 0 || pos >= cap) return;
  const int page = p.block_table[(long long)b * p.bt_stride + (int)(pos >> p.lp)];
  if ((unsigned)page >= (unsigned)p.num_pages) return;
  const int row = (int)(pos & ((1 << p.lp) - 1));
  const char *src = (const char *)p.k_new + (long long)(s0 + i) * p.new_rs * 2;
  char *dst = (char *)p.k_pages + ((long long)page * p.page_stride + (long long)row * p.row_stride);  // byte strides
  unsigned word;
  const int e = idxq_row<DT, ROTATE>(*reinterpret_cast<const unsigned *>(src + 4 * lane), lane, word);
  if (!(lane & 1)) *reinterpret_cast<unsigned *>(dst + 2 * lane) = word;
  if (lane == 0) *reinterpret_cast<unsigned *>(q.k_scale + ((long long)page * q.scale_page_stride + row)) = (unsigned)(127 + e) << 23;
}

// fa_mla_indexer_q_quant: row r of total_q * Hi is (token r / Hi, head r % Hi)
template <int DT, bool ROTATE>
__global__ __launch_bounds__(64 * IDXQ_ROWS) void idxq_query_rows_kernel(MlaIndexerQQuantParams q) {
  const int lane = threadIdx.x & 63;
  const unsigned r = blockIdx.x * IDXQ_ROWS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= q.rows) return;  // wave-uniform
  const unsigned t = r / (unsigned)q.Hi, h = r - t * (unsigned)q.Hi;
  const char *src = (const char *)q.q + ((long long)t * q.q_rs + (long long)h * q.q_hs) * 2;
  char *dst = (char *)q.q_out + ((long long)t * q.qo_rs + (long long)h * q.qo_hs);  // byte strides
  unsigned word;
  const int e = idxq_row<DT, ROTATE>(*reinterpret_cast<const unsigned *>(src + 4 * lane), lane, word);
  if (!(lane & 1)) *reinterpret_cast<unsigned *>(dst + 2 * lane) = word;
  if (lane == 0) {  // (w_out may be head_w: this lane alone reads and writes the element)
    const float wv = q.head_w[(long long)t * q.w_rs + h] * q.w_mul;                                       // one rounded multiply
    q.w_out[(long long)t * q.wo_rs + h] = wv * __builtin_bit_cast(float, (unsigned)(127 + e) << 23);  // times 2^e: exact
  }
}

template <template <int, bool> class Launch, class Params>
static hipError_t idxq_dispatch(const Params &q, int dtype, int rotate, dim3 grid, hipStream_t s) {
  (void)hipGetLastError();
  if (dtype == FA_DTYPE_BF16) rotate ? Launch<FA_DTYPE_BF16, true>::go(q, grid, s) : Launch<FA_DTYPE_BF16, false>::go(q, grid, s);
  else rotate ? Launch<FA_DTYPE_F16, true>::go(q, grid, s) : Launch<FA_DTYPE_F16, false>::go(q, grid, s);
  return hipGetLastError();
}
template <int DT, bool ROTATE>
struct IdxqKeyLaunch {
  static void go(const MlaIndexerKQuantParams &q, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((idxq_key_rows_kernel<DT, ROTATE>), grid, dim3(64 * IDXQ_ROWS), 0, s, q);
  }
};
template <int DT, bool ROTATE>
struct IdxqQueryLaunch {
  static void go(const MlaIndexerQQuantParams &q, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((idxq_query_rows_kernel<DT, ROTATE>), grid, dim3(64 * IDXQ_ROWS), 0, s, q);
  }
};

hipError_t launch_mla_indexer_k_quant(const MlaIndexerKQuantParams &q, int new_dtype, int rotate, hipStream_t s) {
  const int nblk = (q.a.max_new + IDXQ_ROWS - 1) / IDXQ_ROWS;
  return idxq_dispatch<IdxqKeyLaunch>(q, new_dtype, rotate, dim3(q.a.B * nblk), s);
}
hipError_t launch_mla_indexer_q_quant(const MlaIndexerQQuantParams &q, int dtype, int rotate, hipStream_t s) {
  return idxq_dispatch<IdxqQueryLaunch>(q, dtype, rotate, dim3((q.rows + IDXQ_ROWS - 1) / IDXQ_ROWS), s);
}

}  // namespace fa
