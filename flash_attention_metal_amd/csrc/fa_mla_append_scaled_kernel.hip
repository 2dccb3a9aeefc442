// fa_mla_append_scaled_kernel.hip -- the quantising append that WRITES the 656-byte rows fa_fwd_mla_decode_sparse_kv8_scaled reads: entry
// point fa_mla_kv_append_paged_scaled. New bf16 rows [total_new, 576] -> bytes 0 .. 655 of their slots of one pool: 512 e4m3 latent
// bytes, four fp32 scales (one per 128 latent elements, a power of two), the 64 rotary elements copied.
//   * PLACEMENT is fa_kv_append_paged's, line for line (fa_decode_kernel.hip): the sequence lookup and its clamps (entries to [0, total],
//     a non-increasing pair is length 0, n_b <= max_seqlen_new); token i of sequence b goes to key position seqlens[b] - n_b + i --
//     seqlens is the length AFTER the append -- and is skipped when that position is below 0, at or above the capacity, or on a table
//     entry outside [0, num_pages). Nothing but bytes 0 .. 655 of a written row is written.
//   * ONE WAVE PER NEW ROW, four rows per workgroup; the grid, B * ceil(max_seqlen_new / 4), depends on host scalars only. The skip is
//     wave-uniform and there is no barrier.
//   * Lane l holds latent chunk l, eight elements (one 16-byte load). A group of 128 elements is sixteen lanes, exactly one DPP row:
//     amax_g is an in-lane max of eight |x|, taken on the fp32 bits (non-negative floats order as integers), then four row-local DPP
//     steps (quad_perm 1-0-3-2 and 2-3-0-1, row_half_mirror, row_mirror) after which every lane of the row holds the row's max.
//   * THE EXPONENT by integer arithmetic on those bits: amax = m * 2^E, 1 <= m < 2, and 448 = 1.75 * 2^8, so the smallest e with
//     amax <= 448 * 2^e is E - 8, plus one where m > 1.75 (mantissa field above 0x600000), clamped to [-32, 32]. Zero and subnormal
//     amax have E = -127: -32. s_g = 2^e_g and 2^-e_g are built from their exponent fields.
//   * THE CODES: e4m3_rne(clamp(fp32(x) * 2^-e_g, -448, 448)) -- fa_kv_append_paged_quant's conversion, the clamp BEFORE
//     v_cvt_pk_fp8_f32 (which gives NaN above 448 instead of saturating); the multiply by a power of two is exact. One 8-byte store per
//     lane; lanes 16 g store s_g at byte 512 + 4 g; lanes 0 .. 7 copy the rotary chunks (16 bytes each) to byte 528. Plain vector stores.
#include "fa_mfma_common.h"

namespace fa {

constexpr int MLA_APPEND_SCALED_ROWS = 4;  // new rows (= waves) per workgroup

__global__ __launch_bounds__(64 * MLA_APPEND_SCALED_ROWS) void mla_kv_append_paged_scaled_kernel(AppendPagedParams p) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nblk = (p.max_new + MLA_APPEND_SCALED_ROWS - 1) / MLA_APPEND_SCALED_ROWS;
  const int b = (int)blockIdx.x / nblk, rb = (int)blockIdx.x - b * nblk;
  const int s0 = min(max(p.cu_new[b], 0), p.total_new), e0 = min(max(p.cu_new[b + 1], 0), p.total_new);
  const int n = min(max(e0 - s0, 0), p.max_new);
  const long long first = (long long)p.seqlens[b] - n;  // key position of the sequence's first new token
  const long long cap = (long long)p.max_pages << p.lp;
  const int i = rb * MLA_APPEND_SCALED_ROWS + w;  // the wave's new row: everything below is wave-uniform up to the loads
  if (i >= n) return;
  const long long pos = first + i;
  if (pos < 0 || pos >= cap) return;
  const int page = p.block_table[(long long)b * p.bt_stride + (int)(pos >> p.lp)];
  if ((unsigned)page >= (unsigned)p.num_pages) return;
  const char *src = (const char *)p.k_new + (long long)(s0 + i) * p.new_rs * 2;                                       // 576 bf16
  char *dst = (char *)p.k_pages + ((long long)page * p.page_stride + (pos & ((1 << p.lp) - 1)) * p.row_stride);  // 656 bytes

  // the lane's eight latent elements as fp32 bits (bf16 -> fp32 is a shift), and their largest magnitude
  const u32x4 in = *reinterpret_cast<const u32x4 *>(src + 16 * lane);
  unsigned xb[8];
  int amax = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    xb[2 * j] = in[j] << 16;
    xb[2 * j + 1] = in[j] & 0xffff0000u;
    amax = max(amax, max((int)(xb[2 * j] & 0x7fffffffu), (int)(xb[2 * j + 1] & 0x7fffffffu)));
  }
  // over the sixteen lanes of the group: every lane ends with the group's max
  amax = max(amax, __builtin_amdgcn_update_dpp(0, amax, 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
  amax = max(amax, __builtin_amdgcn_update_dpp(0, amax, 0x4E, 0xF, 0xF, true));   // quad_perm [2, 3, 0, 1]
  amax = max(amax, __builtin_amdgcn_update_dpp(0, amax, 0x141, 0xF, 0xF, true));  // row_half_mirror
  amax = max(amax, __builtin_amdgcn_update_dpp(0, amax, 0x140, 0xF, 0xF, true));  // row_mirror
  // e_g: the smallest integer in [-32, 32] with amax <= 1.75 * 2^(8 + e_g)
  const int e = min(max((amax >> 23) - 127 - 8 + ((amax & 0x7fffff) > 0x600000 ? 1 : 0), -32), 32);
  const float inv = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);  // 2^-e_g

  u32x2 out;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = fminf(fmaxf(__builtin_bit_cast(float, xb[4 * j + k]) * inv, -448.0f), 448.0f);
    int cw;
    asm volatile("" : "=v"(cw));  // (the first conversion keeps the other half of its destination: start from an undefined register)
    cw = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], cw, false);
    cw = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], cw, true);
    out[j] = (unsigned)cw;
  }
  *reinterpret_cast<u32x2 *>(dst + 8 * lane) = out;
  if ((lane & 15) == 0) *reinterpret_cast<unsigned *>(dst + 512 + 4 * (lane >> 4)) = (unsigned)(127 + e) << 23;  // s_g = 2^e_g
  if (lane < 8) *reinterpret_cast<u32x4 *>(dst + 528 + 16 * lane) = *reinterpret_cast<const u32x4 *>(src + 1024 + 16 * lane);
}

hipError_t launch_mla_kv_append_paged_scaled(const AppendPagedParams &p, hipStream_t s) {
  const int nblk = (p.max_new + MLA_APPEND_SCALED_ROWS - 1) / MLA_APPEND_SCALED_ROWS;
  (void)hipGetLastError();
  hipLaunchKernelGGL(mla_kv_append_paged_scaled_kernel, dim3(p.B * nblk), dim3(64 * MLA_APPEND_SCALED_ROWS), 0, s, p);
  return hipGetLastError();
}

}  // namespace fa
