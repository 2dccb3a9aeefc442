// fa_api.hip -- the C-ABI entry points of include/fa_mi355.h.
// Validation + dispatch only; every kernel lives in its own file.
#include <stdarg.h>
#include <algorithm>
#include <initializer_list>
#include <stdio.h>
#include <string.h>

#include "fa_common.h"

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ---- argument rules shared by the launch entry points: each returns FA_OK, or fails with a message that names the entry point `fn`.
// What the entry points require differently is the caller's argument or a line of its own (making it one rule would change what
// is accepted, which is for a later change):
//  - batch_stride >= head_stride: fa_fwd whenever H > 1, the backward whenever H > 1 (and on k / v whenever Hkv > 1); fa_fwd_exv
//    and the dense and paged decode only when B > 1 as well;
//  - the head-size guards: fa_fwd / fa_fwd_exv (max(Nq, Nk) + 128) * D * in_bytes < 4 GiB, the decode (Nk + 128) * D * 2 < 4 GiB,
//    the backward max(Nq, Nk) * D * 2 < 4 GiB (no +128) and (max(Nq, Nk) + 128) * D * 2 < 2 GiB for its padded head dims, the
//    paged decode 2 GiB per page of one head;
//  - the grid guards: B * H * ceil(Nq / 128) (fa_fwd, fa_fwd_exv) or B * H * ceil(max(Nq, Nk) / 128) (backward) below 2^31;
//    B * Hq * Nq and B * Hkv * 256 for the decodes;
//  - fa_fwd_varlen has row and head strides (no batch): each at least D and a multiple of 8, checked in its own lines; its size guard is
//    (max_seqlen + 128) * row_stride * 2 < 4 GiB per sequence, for q and for k / v; its grid guard B * Hq * ceil(max_seqlen_q / 128);
//  - fa_bwd_varlen and fa_bwd_varlen_window (one bwd_varlen_impl): fa_fwd_varlen's rules, with the grid guard for both of its kernels (B * Hq * ceil(max_seqlen_q / 128) and
//    B * Hkv * ceil(max_seqlen_k / 128));
//  - fa_fwd_varlen_paged: fa_fwd_varlen's rules for q and the grid, page_pool_ok for the pools and tables (the paged decode's rules);
//    fa_kv_append_paged: varlen_strides_ok for the new rows, page_pool_ok, and a grid of B * ceil(max_seqlen_new / 16) x Hkv;
//  - fa_fwd_varlen_paged_kv8: varlen_paged_impl with the pools' own type (strides of 16 elements, a page counted in bytes of 1), its own
//    support table, sinks optional; fa_kv_append_paged_quant: kv_append_impl with e4m3 pools, plus the two multipliers;
//  - the four *_softcap entry points: the impl function, and with it every rule, of their *_window call, plus softcap_ok;
//  - the four *_sink entry points: the impl function, and with it every rule, of their *_window call, plus sinks_ok (and dsinks' alignment);
//  - a missing device: FA_ERR_NO_DEVICE from fa_fwd, FA_ERR_LAUNCH from every other entry point.
#define TRY(check) do { if (const int st_ = (check)) return st_; } while (0)

int nonnull(const char *fn, std::initializer_list<const void *> ptrs) {
  for (const void *p : ptrs)
    if (!p) return fail(FA_ERR_INVALID_ARG, "%s: null pointer", fn);
  return FA_OK;
}
int positive(const char *fn, std::initializer_list<int> sizes) {
  for (int n : sizes)
    if (n < 1) return fail(FA_ERR_INVALID_ARG, "%s: sizes must be >= 1", fn);
  return FA_OK;
}
int grouped(const char *fn, int Hq, int Hkv) {
  return Hkv >= 1 && Hq % Hkv == 0 ? FA_OK : fail(FA_ERR_INVALID_ARG, "%s: Hq=%d must be a multiple of Hkv=%d", fn, Hq, Hkv);
}
int causal_fits(const char *fn, int is_causal, int Nq, int Nk) {
  return !is_causal || Nk >= Nq ? FA_OK
                                : fail(FA_ERR_UNSUPPORTED, "%s: causal needs Nk >= Nq (bottom-right alignment would leave empty rows)", fn);
}
int scale_ok(const char *fn, float scale) {
  return scale > 0.0f ? FA_OK : fail(FA_ERR_INVALID_ARG, "%s: scale=%g must be > 0", fn, (double)scale);
}
int stride_mult(int dtype) { return dtype == FA_DTYPE_FP8_E4M3 ? 16 : 8; }  // elements: keeps every head 16-byte aligned
// one [B, H, N, D] operand under (batch, head) element strides; `what` names it in the message ("" or "key/value ")
int strides_ok(const char *fn, const char *what, int N, int D, long long bs, long long hs, int mult, bool batch_over_head) {
  if (hs < (long long)N * D || bs < 0 || (batch_over_head && bs < hs) || (bs % mult) || (hs % mult))
    return fail(FA_ERR_INVALID_ARG, "%s: bad %sstrides (batch %lld, head %lld): a head holds %lld elements, strides are multiples of %d",
                fn, what, bs, hs, (long long)N * D, mult);
  return FA_OK;
}
// one packed [total, H, D] operand of the varlen entry points under (row, head) element strides: rows and heads may interleave either
// way, so all that is required of a stride is room for one row and 16-byte alignment of every row
int varlen_strides_ok(const char *fn, const char *what, int D, long long rs, long long hs, int mult) {
  if (rs < D || hs < D || (rs % mult) || (hs % mult))
    return fail(FA_ERR_INVALID_ARG, "%s: bad %sstrides (row %lld, head %lld): a row holds %d elements, strides are multiples of %d", fn, what, rs, hs, D, mult);
  return FA_OK;
}
int aligned16(const char *fn, const char *what, std::initializer_list<const void *> ptrs) {
  for (const void *p : ptrs)
    if ((uintptr_t)p & 15) return fail(FA_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned", fn, what);
  return FA_OK;
}
int head_fits(const char *fn, double head_bytes, int gib, const char *why) {
  return head_bytes < gib * 1073741824.0 ? FA_OK : fail(FA_ERR_INVALID_ARG, "%s: one head exceeds %d GiB%s", fn, gib, why);
}
int grid_fits(const char *fn, long long heads, int rows) {  // heads x blocks of 128 rows fit an int
  return heads <= 0x7fffffffLL / ((rows + 127) / 128) ? FA_OK : fail(FA_ERR_INVALID_ARG, "%s: grid too large", fn);
}
// the page pool and its tables, for every entry point that reads or writes one, in three steps (fa_fwd_decode_paged interleaves them with
// its other checks, in the order it has always reported them; page_pool_ok is the three in a row):
//  - block_table_stride covers max_pages_per_seq entries;
int table_stride_ok(const char *fn, long long block_table_stride, int max_pages_per_seq) {
  return block_table_stride >= max_pages_per_seq
             ? FA_OK
             : fail(FA_ERR_INVALID_ARG, "%s: block_table_stride=%lld < max_pages_per_seq=%d", fn, block_table_stride, max_pages_per_seq);
}
//  - the three page strides (elements), and 2 GiB per page of one head (32-bit offsets from the page's own 64-bit base);
int page_strides_ok(const char *fn, int D, int page_size, long long page_stride, long long head_stride, long long row_stride,
                    long long block_table_stride, int kv_dtype) {
  const int ksm = stride_mult(kv_dtype);  // keeps every row 16-byte aligned
  if (row_stride < D || head_stride < D || page_stride < D || (page_stride % ksm) || (head_stride % ksm) || (row_stride % ksm) ||
      block_table_stride > 0x7fffffffLL)
    return fail(FA_ERR_INVALID_ARG, "%s: bad page strides", fn);
  if ((double)page_size * row_stride * (kv_dtype == FA_DTYPE_FP8_E4M3 ? 1 : 2) >= 2147483648.0)
    return fail(FA_ERR_INVALID_ARG, "%s: one page of one head exceeds 2 GiB", fn);
  return FA_OK;
}
//  - int32 tables, and a capacity of at most 2^30 keys.
int page_tables_ok(const char *fn, int page_size, int max_pages_per_seq, const void *block_table, const void *seqlens_k) {
  if (((uintptr_t)block_table | (uintptr_t)seqlens_k) & 3) return fail(FA_ERR_INVALID_ARG, "%s: block_table / seqlens_k must be int32-aligned", fn);
  if ((long long)page_size * max_pages_per_seq > (1 << 30)) return fail(FA_ERR_INVALID_ARG, "%s: capacity above 2^30 keys", fn);
  return FA_OK;
}
int page_pool_ok(const char *fn, int D, int page_size, int max_pages_per_seq, long long page_stride, long long head_stride, long long row_stride,
                 long long block_table_stride, int kv_dtype, const void *block_table, const void *seqlens_k) {
  TRY(table_stride_ok(fn, block_table_stride, max_pages_per_seq));
  TRY(page_strides_ok(fn, D, page_size, page_stride, head_stride, row_stride, block_table_stride, kv_dtype));
  return page_tables_ok(fn, page_size, max_pages_per_seq, block_table, seqlens_k);
}
int log2_of(int page_size) {
  int lp = 0;
  while ((1 << lp) < page_size) ++lp;
  return lp;
}
int workspace_fits(const char *fn, long long bytes, long long need, const char *sizer) {
  return bytes >= need ? FA_OK : fail(FA_ERR_INVALID_ARG, "%s: workspace of %lld bytes, %s() asks for %lld", fn, bytes, sizer, need);
}
// The *_window entry points route by SIGN only: (wl < 0, wr < 0) is the un-windowed call without the mask and (wl < 0, wr == 0) the
// causal one -- the existing kernels, bit for bit; every other pair runs the windowed kernels, however large its values.
enum { WIN_FULL = 0, WIN_CAUSAL = 1, WIN_KERNEL = 2 };
int window_route(int wl, int wr) { return wl < 0 && wr < 0 ? WIN_FULL : wl < 0 && wr == 0 ? WIN_CAUSAL : WIN_KERNEL; }
// what the windowed kernels get: a side that is unbounded (negative) or at least `never` wide becomes `never`, the smallest width that
// cannot bind (wl: the most keys a sequence of the call can hold; wr: the most query rows), so that the kernels' 32-bit coff - wl and
// row + coff + wr cannot wrap
int window_clamp(int w, int never) { return w < 0 || w > never ? never : w; }
// the *_sink entry points: one fp32 logit per query head in device memory, read by the kernels only
int sinks_ok(const char *fn, const float *sinks) {
  if (!sinks) return fail(FA_ERR_INVALID_ARG, "%s: null pointer", fn);
  return (uintptr_t)sinks & 3 ? fail(FA_ERR_INVALID_ARG, "%s: sinks must be fp32-aligned", fn) : FA_OK;
}
// the *_softcap entry points: the cap is a host scalar, finite and greater than 0
int softcap_ok(const char *fn, float softcap) {
  return (std::isfinite(softcap) && softcap > 0.0f) ? FA_OK : fail(FA_ERR_INVALID_ARG, "%s: softcap must be finite and > 0", fn);
}
int launched(const char *fn, hipError_t e) {
  return e == hipSuccess ? FA_OK : fail(FA_ERR_LAUNCH, "%s: launch failed: %s", fn, hipGetErrorString(e));
}
}  // namespace

extern "C" {

const char *fa_last_error(void) { return g_err; }
int fa_version(void) { return FA_MI355_VERSION; }

const char *fa_variant_name(int v) {
  switch (v) {
    case FA_VARIANT_AUTO: return "auto";
    case FA_VARIANT_NAIVE: return "naive";
    case FA_VARIANT_TILED: return "tiled";
    case FA_VARIANT_TILED_V2: return "tiled_v2";
    case FA_VARIANT_MFMA: return "mfma";
    case FA_VARIANT_MFMA_PP: return "mfma_pp";
    case FA_VARIANT_MFMA_SPLITKV: return "mfma_splitkv";
    case FA_VARIANT_MFMA_SPLIT2: return "mfma_split2";
    case FA_VARIANT_MFMA_EXACT: return "mfma_exact";
    case FA_VARIANT_MFMA_H64S2: return "mfma_h64s2";
    case FA_VARIANT_MFMA16: return "mfma16";
    case FA_VARIANT_MFMA_FP8PV: return "mfma_fp8pv";
    default: return "?";
  }
}
const char *fa_dtype_name(int d) {
  switch (d) {
    case FA_DTYPE_F32: return "f32";
    case FA_DTYPE_F16: return "f16";
    case FA_DTYPE_BF16: return "bf16";
    case FA_DTYPE_FP8_E4M3: return "fp8_e4m3";
    default: return "?";
  }
}
int fa_dtype_in_bytes(int d) {
  switch (d) {
    case FA_DTYPE_F32: return 4;
    case FA_DTYPE_F16: case FA_DTYPE_BF16: return 2;
    case FA_DTYPE_FP8_E4M3: return 1;
    default: return 0;
  }
}
int fa_dtype_out_bytes(int d) { return d == FA_DTYPE_FP8_E4M3 ? 2 : fa_dtype_in_bytes(d); }

int fa_supported(int dtype, int variant, int D) {
  switch (variant) {
    case FA_VARIANT_AUTO: return fa_resolve_variant(dtype, D) > 0;
    case FA_VARIANT_NAIVE: return fa::naive_supported(dtype, D);
    case FA_VARIANT_TILED: return fa::tiled_supported(dtype, D);
    case FA_VARIANT_TILED_V2: return fa::tiled_v2_supported(dtype, D);
    case FA_VARIANT_MFMA: return fa::mfma_supported(dtype, D);
    case FA_VARIANT_MFMA_PP: return 0;  // retired in round 4 (tools/experiments/fa_fwd_pp_kernel.hip): the enum value stays reserved
    case FA_VARIANT_MFMA_SPLITKV: return fa::splitkv_supported(dtype, D);
    case FA_VARIANT_MFMA_SPLIT2: return fa::mfma_split2_supported(dtype, D);
    case FA_VARIANT_MFMA_EXACT: return fa::mfma_supported(dtype, D);
    case FA_VARIANT_MFMA_H64S2: return fa::mfma_h64s2_supported(dtype, D);
    case FA_VARIANT_MFMA16: return fa::mfma16_supported(dtype, D);
    case FA_VARIANT_MFMA_FP8PV: return fa::fp8pv_supported(dtype, D);
    default: return 0;
  }
}
int fa_resolve_variant(int dtype, int D) {
  if (fa::mfma_supported(dtype, D)) return FA_VARIANT_MFMA;
  if (fa::mfma16_supported(dtype, D)) return FA_VARIANT_MFMA16;  // 16-bit inputs, the other multiples of 8 up to 128: zero-padded rows
  if (fa::tiled_v2_supported(dtype, D)) return FA_VARIANT_TILED_V2;
  return FA_ERR_UNSUPPORTED;
}

// FA_VARIANT_AUTO of fa_fwd (what fa_resolve_variant_for returns) and of fa_fwd_exv (`ex`). The two rules differ: fa_fwd_exv takes the
// 16x16x32 kernel on thresholds of its own and none of the other forms; making them one would change which kernel runs (a later change).
// fa_fwd chooses between the matrix-core kernels (interleaved A/B on MI355X): the split-KV kernel wins on grids
// far smaller than the chip, the 64-row two-split form and the eight-wave form of the 128-row kernel on grids of up to two / one
// workgroup(s) per CU; everywhere else the 128-row kernel, its 16x16x32 form or (e4m3) the all-fp8 kernel is fastest.
static int route_auto(int dtype, int D, int B, int H, int Nq, int Nk, int is_causal, bool ex) {
  // small grids: fewer 128-row workgroups than a quarter of the CUs (or half, when each would walk >= 32 tiles), as in decode steps:
  // split the keys of every 32-row block over the waves of a workgroup instead (config 2: 15.9 -> 10.6 us; 32 heads x 1 query x 16384
  // keys: 165 -> 55 us, profiles/r03/decode_steps_splitkv_rule.log)
  // (head_dim 64 only: the head_dim-128 instantiation needs more than the 256 registers its eight-wave workgroup leaves a wave and
  // spills 820 B -- 8 heads x 1024: 73 us against 17-20 us for the kernels below, profiles/r03/ab_d128_small_grids.log; it stays
  // reachable by name)
  const long long blocks128 = (long long)B * H * ((Nq + 127) / 128);
  if (D == 64 && fa::splitkv_supported(dtype, D) && Nk > 64 && blocks128 <= 64) return FA_VARIANT_MFMA_SPLITKV;
  const int v = fa_resolve_variant(dtype, D);  // (fa_fwd_exv has refused the head dims without a matrix-core kernel)
  if (v != FA_VARIANT_MFMA) return v;
  if (ex)
    return fa::mfma16_supported(dtype, D) && blocks128 > 512 && Nk >= (D == 64 ? (is_causal ? 1536 : 1024) : (is_causal ? 2048 : 1024))
               ? FA_VARIANT_MFMA16
               : FA_VARIANT_MFMA;
  const int N = Nq;
  // (round 2 sent long head_dim-128 sequences to the paired-block kernel; since the 128-row kernel stages its tiles by
  // LDS-DMA it is 8-10 % ahead there too -- config 4 shard 1295 vs 1181 TFLOP/s, profiles/r03/ab_dma_late_and_d128_auto.log --
  // and round 4 retired FA_VARIANT_MFMA_PP: the kernel is kept under tools/experiments/)
  // head_dim 64, 16-bit inputs, at most two 64-row workgroups per CU: 64-row blocks whose wave pairs take the even / odd
  // tiles -- twice the workgroups and half the sequential tiles (h=8, N=2048 causal: 20.0 (eight-wave form) -> 17.9 us;
  // 64 heads x 256: 6.6 -> 5.9 us; profiles/r03/ab_h64s2.log)
  const long long blocks64 = (long long)B * H * ((N + 63) / 64);
  if (fa::mfma_h64s2_supported(dtype, D) && N >= 256 && blocks64 <= 512) return FA_VARIANT_MFMA_H64S2;
  // up to one 128-row workgroup per CU: the block's tiles are the critical path -- eight waves, even / odd tiles
  // (h=32, N=1024 causal: 16.1 -> 14.2 us; h=8, N=2048: 27.3 -> 22.0 us, split-KV 25.1)
  // (e4m3 inputs at head_dim 128: the all-fp8 kernel is ahead of the eight-wave form except on small grids of long sequences --
  // 32 heads x 512 / 2048: 11.4 -> 10.3 / 36.8 -> 32.7 us, 8 heads x 4096: 50.6 vs 53.6; profiles/r04/auto_check_late.log)
  const bool fp8_d128 = dtype == FA_DTYPE_FP8_E4M3 && D == 128;
  if (fa::mfma_split2_supported(dtype, D) && N >= 512 && blocks128 <= 256 && !(fp8_d128 && N < 4096)) return FA_VARIANT_MFMA_SPLIT2;
  // causal, two workgroups' worth of blocks per CU of which half are light: the heaviest block's 32+ tiles are still the critical
  // path (32 heads x 2048: 28.9 -> 25.9 us at head_dim 64, 45.8 -> 42.5 at 128, fp8 29.3 -> 24.6; at N = 1024 the plain kernel
  // wins again; profiles/r03/auto_check.log)
  // (fp8 inputs at head_dim 64 already from N = 1024: 64 heads x 1024, 16.7 -> 14.7 us)
  const int n_min = (dtype == FA_DTYPE_FP8_E4M3 && D == 64) ? 1024 : 2048;
  if (fa::mfma_split2_supported(dtype, D) && is_causal && N >= n_min && blocks128 <= 512 && !fp8_d128) return FA_VARIANT_MFMA_SPLIT2;
  // head_dim 64, 16-bit inputs, grids that fill the chip: the same workgroup on the 16x16x32 instruction with its row sums on the matrix
  // core -- config 3 +2 %, N >= 4096 non-causal / N >= 8192 causal +4.5..5.7 %; level at N = 2048, 1-2 % behind at N = 1024 (its
  // first tile pays a second score pass) (profiles/r04/ab_mfma16_ones_vs_adds.log)
  // head_dim 128: from N = 8192 on (config 4 shard 1259-1300 -> 1323-1331 TFLOP/s, non-causal N = 8192 +4..5.7 %; level at N <= 4096;
  // profiles/r04/ab_mfma16_d128*.log)
  // (late round 4, on warm clocks, profiles/r04/ab_auto_short_sequences_mfma16.log: with its first tile free of the second score pass it is
  // also ahead from N = 1536 on under the mask (+4 %; level at 1024) and, without the mask, from N = 512 on for grids of at least 512
  // workgroups (+2..6 %, eight waves per workgroup there: mfma16_waves))
  if (fa::mfma16_supported(dtype, D)) {
    // (head_dim 128: since the first tile lost its second score pass it is ahead from N = 2048 on, +5.5..7 % at 4 x 16 heads x 2048 / 4096
    // causal and non-causal; without the mask from 1024 on, +4..5 %; auto_check_late.log)
    const bool take = D == 64 ? (is_causal ? N >= 1536 : (N >= 2048 || (N >= 512 && blocks128 >= 512))) : (is_causal ? N >= 2048 : N >= 1024);
    if (take) return FA_VARIANT_MFMA16;
  }
  // fp8 inputs, head_dim 64, grids that fill the chip: both products on the fp8 matrix pipe (config 5: 1215-1245 -> 1364-1461 TFLOP/s,
  // profiles/r04/ab_fp8pv_*.log). Its probabilities are e4m3 (include/fa_mi355.h, "fp8 probabilities"); FA_VARIANT_MFMA keeps them bf16
  if (fa::fp8pv_supported(dtype, D)) return FA_VARIANT_MFMA_FP8PV;
  return FA_VARIANT_MFMA;
}
int fa_resolve_variant_for(int dtype, int D, int B, int H, int N, int is_causal) {
  return route_auto(dtype, D, B, H, N, N, is_causal, false);
}

const char *fa_fwd_kernel_name(int dtype, int D, int B, int H, int N, int is_causal) {
  static thread_local char name[96];
  const int v = fa_resolve_variant_for(dtype, D, B, H, N, is_causal);
  const char *tag = dtype == FA_DTYPE_F32 ? "float" : dtype == FA_DTYPE_F16 ? "fa::F16" : dtype == FA_DTYPE_BF16 ? "fa::BF16" : "fa::FP8";
  const char *c = is_causal ? "true" : "false";
  switch (v) {
    case FA_VARIANT_MFMA_SPLITKV: snprintf(name, sizeof(name), "fa::fwd_splitkv_kernel<%s, %d, %s>", tag, D, c); break;
    case FA_VARIANT_MFMA_SPLIT2: snprintf(name, sizeof(name), "fa::fwd_mfma_split2_kernel<%s, %d, %s>", tag, D, c); break;
    case FA_VARIANT_MFMA_H64S2: snprintf(name, sizeof(name), "fa::fwd_mfma_h64s2_kernel<%s, %d, %s>", tag, D, c); break;
    case FA_VARIANT_MFMA16:
      // (template arguments as rocprofv3 prints them: dtype, head dim of the instantiation, causal, waves per workgroup, padded rows, tiles per barrier)
      snprintf(name, sizeof(name), "fa::fwd_mfma16_kernel<%s, %d, %s, %d, %s, 1>", tag, (D == 64 || D == 128) ? D : (D < 64 ? 64 : 128), c,
               fa::mfma16_waves(D, B * H, N, N, is_causal), (D == 64 || D == 128) ? "false" : "true");
      break;
    case FA_VARIANT_MFMA_FP8PV: snprintf(name, sizeof(name), "fa::fwd_fp8_kernel<%d, %s>", D, c); break;
    case FA_VARIANT_MFMA:
      snprintf(name, sizeof(name), "fa::fwd_mfma_kernel<%s, %d, %s, %s>", tag, D, c,
               (dtype != FA_DTYPE_FP8_E4M3 && D <= 128) ? "true" : "false");  // pre-scaled operand where it exists
      break;
    case FA_VARIANT_MFMA_EXACT: snprintf(name, sizeof(name), "fa::fwd_mfma_kernel<%s, %d, %s, false>", tag, D, c); break;
    case FA_VARIANT_TILED_V2: snprintf(name, sizeof(name), "fa::tiled_v2_kernel"); break;
    default: name[0] = 0;
  }
  return name;
}

double fa_algorithmic_flops(int B, int H, int N, int D, int is_causal) {
  return (is_causal ? 2.0 : 4.0) * (double)B * H * (double)N * (double)N * D;
}
double fa_algorithmic_bytes(int B, int H, int N, int D, int dtype) {
  return (3.0 * fa_dtype_in_bytes(dtype) + fa_dtype_out_bytes(dtype)) * (double)B * H * N * D +
         4.0 * (double)B * H * N;
}

// the forward launch of fa_fwd and fa_fwd_exv (fa_fwd passes Hkv = H, Nk = N and its strides as the kv strides)
static hipError_t launch_fwd(const void *q, const void *k, const void *v, void *o, float *lse, int B, int Hq, int Hkv, int Nq, int Nk,
                             int D, float scale, long long q_batch_stride, long long q_head_stride, long long kv_batch_stride,
                             long long kv_head_stride, int is_causal, int dtype, int variant, hipStream_t s) {
  fa::Params p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse;
  p.B = B; p.H = Hq; p.N = Nq; p.D = D; p.scale = scale;
  p.batch_stride = q_batch_stride; p.head_stride = q_head_stride;
  p.is_causal = is_causal ? 1 : 0;
  p.Nk = Nk; p.Hkv = Hkv; p.kv_batch_stride = kv_batch_stride; p.kv_head_stride = kv_head_stride;
  p.exact = (variant == FA_VARIANT_MFMA_EXACT);
  switch (variant) {
    case FA_VARIANT_NAIVE: return fa::launch_naive(p, dtype, s);
    case FA_VARIANT_TILED: return fa::launch_tiled(p, dtype, s);
    case FA_VARIANT_TILED_V2: return fa::launch_tiled_v2(p, dtype, s);
    case FA_VARIANT_MFMA_SPLITKV: return fa::launch_splitkv(p, dtype, s);
    case FA_VARIANT_MFMA_SPLIT2: return fa::launch_mfma_split2(p, dtype, s);
    case FA_VARIANT_MFMA_H64S2: return fa::launch_mfma_h64s2(p, dtype, s);
    case FA_VARIANT_MFMA16: return fa::launch_mfma16(p, dtype, s);
    case FA_VARIANT_MFMA_FP8PV: return fa::launch_fp8pv(p, dtype, s);
    default: return fa::launch_mfma(p, dtype, s);  // FA_VARIANT_MFMA, FA_VARIANT_MFMA_EXACT
  }
}

int fa_fwd(const void *q, const void *k, const void *v, void *o, float *lse, int B, int H, int N,
           int D, float scale, long long batch_stride, long long head_stride, int is_causal,
           int dtype, int variant, void *hip_stream) {
  g_err[0] = 0;
  const char *fn = "fa_fwd";
  TRY(nonnull(fn, {q, k, v, o}));
  TRY(positive(fn, {B, H, N, D}));
  TRY(scale_ok(fn, scale));
  if (fa_dtype_in_bytes(dtype) == 0) return fail(FA_ERR_INVALID_ARG, "fa_fwd: bad dtype %d", dtype);
  TRY(strides_ok(fn, "", N, D, batch_stride, head_stride, stride_mult(dtype), H > 1));
  TRY(aligned16(fn, "tensors", {q, k, v, o}));
  // 32-bit byte offsets inside a head; the staging loops may address up to two 64-key tiles past its end (range-checked
  // by the buffer descriptor, but the offset itself must not wrap)
  TRY(head_fits(fn, (double)(N + 128) * D * fa_dtype_in_bytes(dtype), 4, ""));
  // head dims without a kernel of their own run on zero-padded rows whose padding is fetched from offset 2^31 + ... (fa_mfma16_kernel.hip, PAD)
  if (!fa::mfma_supported(dtype, D) && fa::mfma16_supported(dtype, D))
    TRY(head_fits(fn, (double)(N + 128) * D * 2, 2, " (head dims on padded rows)"));
  TRY(grid_fits(fn, (long long)B * H, N));
  if (variant == FA_VARIANT_AUTO) {
    variant = route_auto(dtype, D, B, H, N, N, is_causal, false);
    if (variant < 0)
      return fail(FA_ERR_UNSUPPORTED, "fa_fwd: no kernel for dtype=%s D=%d", fa_dtype_name(dtype), D);
  }
  if (!fa_supported(dtype, variant, D))
    return fail(FA_ERR_UNSUPPORTED, "fa_fwd: variant=%s does not support dtype=%s D=%d",
                fa_variant_name(variant), fa_dtype_name(dtype), D);
  if ((variant == FA_VARIANT_NAIVE || variant == FA_VARIANT_TILED || variant == FA_VARIANT_TILED_V2) &&
      (H > 65535 || B > 65535))
    return fail(FA_ERR_INVALID_ARG, "fa_fwd: B,H must be <= 65535 for variant %s", fa_variant_name(variant));
  const hipError_t e = launch_fwd(q, k, v, o, lse, B, H, H, N, N, D, scale, batch_stride, head_stride, batch_stride, head_stride,
                                  is_causal, dtype, variant, (hipStream_t)hip_stream);
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice)
    return fail(FA_ERR_NO_DEVICE, "fa_fwd: %s", hipGetErrorString(e));
  return launched(fn, e);
}

int fa_fwd_ex(const void *q, const void *k, const void *v, void *o, float *lse, int B, int Hq, int Hkv, int Nq, int Nk,
              int D, float scale, long long q_batch_stride, long long q_head_stride, long long kv_batch_stride,
              long long kv_head_stride, int is_causal, int dtype, void *hip_stream) {
  return fa_fwd_exv(q, k, v, o, lse, B, Hq, Hkv, Nq, Nk, D, scale, q_batch_stride, q_head_stride, kv_batch_stride, kv_head_stride,
                    is_causal, dtype, FA_VARIANT_AUTO, hip_stream);
}

int fa_fwd_exv(const void *q, const void *k, const void *v, void *o, float *lse, int B, int Hq, int Hkv, int Nq, int Nk,
               int D, float scale, long long q_batch_stride, long long q_head_stride, long long kv_batch_stride,
               long long kv_head_stride, int is_causal, int dtype, int variant, void *hip_stream) {
  g_err[0] = 0;
  const char *fn = "fa_fwd_ex";
  TRY(nonnull(fn, {q, k, v, o}));
  TRY(positive(fn, {B, Hq, Hkv, Nq, Nk, D}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(causal_fits(fn, is_causal, Nq, Nk));
  TRY(scale_ok(fn, scale));
  const bool padded_dim = !fa::mfma_supported(dtype, D) && fa::mfma16_supported(dtype, D);  // (zero-padded rows of the 16x16x32 kernel)
  if (!fa::mfma_supported(dtype, D) && !padded_dim)
    return fail(FA_ERR_UNSUPPORTED, "fa_fwd_ex: needs a matrix-core kernel (f16/bf16: D a multiple of 8 up to 128, or 256; fp8: D=64|128|256), got dtype=%s D=%d",
                fa_dtype_name(dtype), D);
  if (padded_dim) TRY(head_fits(fn, (double)(std::max(Nq, Nk) + 128) * D * 2, 2, " (head dims on padded rows)"));
  TRY(strides_ok(fn, "", Nq, D, q_batch_stride, q_head_stride, stride_mult(dtype), Hq > 1 && B > 1));
  TRY(strides_ok(fn, "key/value ", Nk, D, kv_batch_stride, kv_head_stride, stride_mult(dtype), Hkv > 1 && B > 1));
  TRY(aligned16(fn, "tensors", {q, k, v, o}));
  // (as in fa_fwd: the staging loops may address up to two 64-key tiles past the end of a head)
  TRY(head_fits(fn, (double)(std::max(Nq, Nk) + 128) * D * fa_dtype_in_bytes(dtype), 4, ""));
  TRY(grid_fits(fn, (long long)B * Hq, Nq));
  if (variant == FA_VARIANT_AUTO) variant = route_auto(dtype, D, B, Hq, Nq, Nk, is_causal, true);
  // the kernels that take the generalised problem (key/value heads, Nk): the 128-row kernel with / without its pre-scaled operand, its
  // 16x16x32 form, the split-KV kernel
  if (variant != FA_VARIANT_MFMA && variant != FA_VARIANT_MFMA_EXACT && variant != FA_VARIANT_MFMA16 && variant != FA_VARIANT_MFMA_SPLITKV)
    return fail(FA_ERR_UNSUPPORTED, "fa_fwd_ex: variant=%s does not take grouped heads / Nq != Nk (mfma, mfma_exact, mfma16, mfma_splitkv do)",
                fa_variant_name(variant));
  if (!fa_supported(dtype, variant, D))
    return fail(FA_ERR_UNSUPPORTED, "fa_fwd_ex: variant=%s does not support dtype=%s D=%d", fa_variant_name(variant), fa_dtype_name(dtype), D);
  return launched(fn, launch_fwd(q, k, v, o, lse, B, Hq, Hkv, Nq, Nk, D, scale, q_batch_stride, q_head_stride, kv_batch_stride,
                                 kv_head_stride, is_causal, dtype, variant, (hipStream_t)hip_stream));
}

int fa_fwd_varlen_supported(int dtype, int D) { return fa::mfma_varlen_supported(dtype, D); }
// fa_fwd_varlen (window_left = -1, window_right = is_causal ? 0 : -1), fa_fwd_varlen_window and fa_fwd_varlen_sink (`sinks`: its own
// argument; null for the other two): one set of rules, one launch path. With sinks the call always runs the windowed kernels in their
// sink mode, an unbounded side clamped to the never-binding width.
static int varlen_impl(const char *fn, const void *q, const void *k, const void *v, void *o, float *lse, const int *cu_seqlens_q,
                       const int *cu_seqlens_k, int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D,
                       float scale, long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                       int window_left, int window_right, int dtype, void *hip_stream, const float *const *sinks = nullptr,
                       const float *softcap = nullptr) {
  // softcap (fa_fwd_varlen_softcap): like sinks, always the windowed kernels, in their softcap mode
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k, v, o, cu_seqlens_q, cu_seqlens_k}));
  if (sinks) TRY(sinks_ok(fn, *sinks));
  if (softcap) TRY(softcap_ok(fn, *softcap));
  TRY(positive(fn, {B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(scale_ok(fn, scale));
  if (!fa_fwd_varlen_supported(dtype, D))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 and D = 64 | 128, got dtype=%s D=%d", fn, fa_dtype_name(dtype), D);
  if (max_seqlen_q > total_q || max_seqlen_k > total_k)
    return fail(FA_ERR_INVALID_ARG, "%s: max_seqlen (%d, %d) exceeds the token count (%d, %d)", fn, max_seqlen_q, max_seqlen_k, total_q, total_k);
  // a token's head is D contiguous elements; rows and heads may interleave either way ([total, H, D], [H, total, D], views of a packed
  // QKV projection), so all that is required of a stride is room for one row and 16-byte alignment of every row
  TRY(varlen_strides_ok(fn, "", D, q_row_stride, q_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "key/value ", D, kv_row_stride, kv_head_stride, stride_mult(dtype)));
  TRY(aligned16(fn, "tensors", {q, k, v, o}));
  if (((uintptr_t)cu_seqlens_q | (uintptr_t)cu_seqlens_k) & 3) return fail(FA_ERR_INVALID_ARG, "%s: cu_seqlens_q / cu_seqlens_k must be int32-aligned", fn);
  // 32-bit byte offsets inside ONE sequence of one head (its base is a 64-bit address: the tensors themselves may exceed 4 GiB); as in
  // fa_fwd the staging may address up to two 64-key tiles past the end
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)q_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_k + 128) * (double)kv_row_stride * 2, 4, " (one sequence of max_seqlen_k rows)"));
  TRY(grid_fits(fn, (long long)B * Hq, max_seqlen_q));
  const int route = (sinks || softcap) ? WIN_KERNEL : window_route(window_left, window_right);
  fa::VarlenSinkParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse;
  p.B = B; p.H = Hq; p.Hkv = Hkv; p.N = max_seqlen_q; p.Nk = max_seqlen_k; p.D = D; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_head_stride; p.kv_batch_stride = 0; p.kv_head_stride = kv_head_stride;
  p.is_causal = route != WIN_FULL;
  p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
  p.total_q = total_q; p.total_k = total_k;
  p.q_rs = q_row_stride; p.kv_rs = kv_row_stride;
  if (route != WIN_KERNEL) return launched(fn, fa::launch_mfma_varlen(p, dtype, (hipStream_t)hip_stream));
  p.wl = window_clamp(window_left, max_seqlen_k);
  p.wr = window_clamp(window_right, max_seqlen_q);
  if (softcap) {
    fa::VarlenSoftcapParams pc;
    static_cast<fa::VarlenWindowParams &>(pc) = p;
    pc.softcap = *softcap;
    return launched(fn, fa::launch_mfma_varlen_softcap(pc, dtype, (hipStream_t)hip_stream));
  }
  if (!sinks) return launched(fn, fa::launch_mfma_varlen_window(p, dtype, (hipStream_t)hip_stream));
  p.sinks = *sinks;
  return launched(fn, fa::launch_mfma_varlen_sink(p, dtype, (hipStream_t)hip_stream));
}
int fa_fwd_varlen(const void *q, const void *k, const void *v, void *o, float *lse, const int *cu_seqlens_q, const int *cu_seqlens_k,
                  int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                  long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride, int is_causal,
                  int dtype, void *hip_stream) {
  return varlen_impl("fa_fwd_varlen", q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D,
                     scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride, -1, is_causal ? 0 : -1, dtype, hip_stream);
}
// fa_fwd_varlen_mla: fa_fwd_varlen's rules in its order, with the stride, alignment and 4 GiB rules once per tensor (q, k, v, o)
int fa_fwd_varlen_mla_supported(int dtype, int Dqk, int Dv) { return fa::mfma_varlen_mla_supported(dtype, Dqk, Dv); }
int fa_fwd_varlen_mla(const void *q, const void *k, const void *v, void *o, float *lse, const int *cu_seqlens_q, const int *cu_seqlens_k,
                      int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int Dqk, int Dv, float scale,
                      long long q_row_stride, long long q_head_stride, long long k_row_stride, long long k_head_stride,
                      long long v_row_stride, long long v_head_stride, long long o_row_stride, long long o_head_stride, int is_causal,
                      int dtype, void *hip_stream) {
  const char *fn = "fa_fwd_varlen_mla";
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k, v, o, cu_seqlens_q, cu_seqlens_k}));
  TRY(positive(fn, {B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, Dqk, Dv}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(scale_ok(fn, scale));
  if (!fa_fwd_varlen_mla_supported(dtype, Dqk, Dv))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 and (Dqk, Dv) = (192, 128), got dtype=%s Dqk=%d Dv=%d", fn, fa_dtype_name(dtype), Dqk, Dv);
  if (max_seqlen_q > total_q || max_seqlen_k > total_k)
    return fail(FA_ERR_INVALID_ARG, "%s: max_seqlen (%d, %d) exceeds the token count (%d, %d)", fn, max_seqlen_q, max_seqlen_k, total_q, total_k);
  TRY(varlen_strides_ok(fn, "", Dqk, q_row_stride, q_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "key ", Dqk, k_row_stride, k_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "value ", Dv, v_row_stride, v_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "output ", Dv, o_row_stride, o_head_stride, stride_mult(dtype)));
  TRY(aligned16(fn, "tensors", {q, k, v, o}));
  if (((uintptr_t)cu_seqlens_q | (uintptr_t)cu_seqlens_k) & 3) return fail(FA_ERR_INVALID_ARG, "%s: cu_seqlens_q / cu_seqlens_k must be int32-aligned", fn);
  // 32-bit byte offsets inside ONE sequence of one head, per tensor (fa_fwd_varlen's rule)
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)q_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)o_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_k + 128) * (double)k_row_stride * 2, 4, " (one sequence of max_seqlen_k rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_k + 128) * (double)v_row_stride * 2, 4, " (one sequence of max_seqlen_k rows)"));
  TRY(grid_fits(fn, (long long)B * Hq, max_seqlen_q));
  fa::VarlenMlaParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse;
  p.B = B; p.H = Hq; p.Hkv = Hkv; p.N = max_seqlen_q; p.Nk = max_seqlen_k; p.D = Dqk; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_head_stride; p.kv_batch_stride = 0; p.kv_head_stride = k_head_stride;
  p.is_causal = is_causal != 0;
  p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
  p.total_q = total_q; p.total_k = total_k;
  p.q_rs = q_row_stride; p.kv_rs = k_row_stride;
  p.v_rs = v_row_stride; p.v_head_stride = v_head_stride; p.o_rs = o_row_stride; p.o_head_stride = o_head_stride;
  return launched(fn, fa::launch_mfma_varlen_mla(p, dtype, (hipStream_t)hip_stream));
}
int fa_fwd_varlen_window(const void *q, const void *k, const void *v, void *o, float *lse, const int *cu_seqlens_q, const int *cu_seqlens_k,
                         int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                         long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                         int window_left, int window_right, int dtype, void *hip_stream) {
  return varlen_impl("fa_fwd_varlen_window", q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q, total_k, max_seqlen_q,
                     max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride, window_left, window_right, dtype,
                     hip_stream);
}
int fa_fwd_varlen_sink(const void *q, const void *k, const void *v, void *o, float *lse, const int *cu_seqlens_q, const int *cu_seqlens_k,
                       int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                       long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                       int window_left, int window_right, const float *sinks, int dtype, void *hip_stream) {
  return varlen_impl("fa_fwd_varlen_sink", q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q, total_k, max_seqlen_q,
                     max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride, window_left, window_right, dtype,
                     hip_stream, &sinks);
}
int fa_fwd_varlen_softcap(const void *q, const void *k, const void *v, void *o, float *lse, const int *cu_seqlens_q, const int *cu_seqlens_k,
                          int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                          long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                          int window_left, int window_right, float softcap, int dtype, void *hip_stream) {
  return varlen_impl("fa_fwd_varlen_softcap", q, k, v, o, lse, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q, total_k, max_seqlen_q,
                     max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride, window_left, window_right, dtype,
                     hip_stream, nullptr, &softcap);
}
int fa_window_key_range(int Lq, int Lk, int window_left, int window_right, int row_first, int row_last, int *key_lo, int *key_hi) {
  g_err[0] = 0;
  if (!key_lo || !key_hi) return fail(FA_ERR_INVALID_ARG, "fa_window_key_range: null pointer");
  if (Lq < 0 || Lk < 0) return fail(FA_ERR_INVALID_ARG, "fa_window_key_range: lengths must be >= 0");
  fa::window_key_range(Lq, Lk, window_left, window_right, row_first, row_last, *key_lo, *key_hi);
  return FA_OK;
}

int fa_fwd_decode_supported(int dtype, int D, int Hq, int Hkv, int Nq) {
  return fa::decode_supported(dtype, D) && Hq >= 1 && Hkv >= 1 && Nq >= 1 && Hq % Hkv == 0 && (long long)(Hq / Hkv) * Nq <= 32;
}
long long fa_fwd_decode_workspace_bytes(int B, int Hq, int Hkv, int Nq, int Nk, int D) {
  if (B < 1 || Hq < 1 || Hkv < 1 || Nq < 1 || Nk < 1 || (D != 64 && D != 128) || Hq % Hkv) return 0;
  return fa::decode_workspace_bytes(B, Hq, Hkv, Nq, Nk, D);
}
// the decode grid guard and the DecodeParams of the dense and the paged decode alike: everything but how the cache is addressed
// (kv_bs, kv_hs and the page tables, the caller's)
static int decode_params(const char *fn, fa::DecodeParams &p, const void *q, const void *k, const void *v, void *o, float *lse,
                         void *workspace, int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale, long long q_batch_stride,
                         long long q_head_stride, int is_causal, int kv8) {
  if ((long long)B * Hq * Nq > 0x7fffffffLL || (long long)B * Hkv * 256 > 0x7fffffffLL) return fail(FA_ERR_INVALID_ARG, "%s: grid too large", fn);
  p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse; p.ws = (float *)workspace;
  p.B = B; p.Hq = Hq; p.Hkv = Hkv; p.Nq = Nq; p.Nk = Nk; p.scale = scale;
  p.q_bs = q_batch_stride; p.q_hs = q_head_stride;
  p.is_causal = is_causal ? 1 : 0;
  p.S = fa::decode_splits(B, Hkv, Nk, D, kv8);
  return FA_OK;
}
static int decode_impl(const void *q, const void *k, const void *v, void *o, float *lse, int B, int Hq, int Hkv, int Nq, int Nk, int D,
                       float scale, long long q_batch_stride, long long q_head_stride, long long kv_batch_stride, long long kv_head_stride,
                       int is_causal, int dtype, int kv8, void *workspace, long long workspace_bytes, void *hip_stream) {
  g_err[0] = 0;
  const char *fn = "fa_fwd_decode";
  TRY(nonnull(fn, {q, k, v, o, workspace}));
  TRY(positive(fn, {B, Hq, Hkv, Nq, Nk, D}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(causal_fits(fn, is_causal, Nq, Nk));
  TRY(scale_ok(fn, scale));
  if (!fa_fwd_decode_supported(dtype, D, Hq, Hkv, Nq))
    return fail(FA_ERR_UNSUPPORTED, "fa_fwd_decode: needs f16 / bf16 / fp8_e4m3, D = 64 | 128 and (Hq / Hkv) * Nq <= 32 packed query rows; got dtype=%s D=%d "
                "Hq=%d Hkv=%d Nq=%d (use fa_fwd_ex)", fa_dtype_name(dtype), D, Hq, Hkv, Nq);
  TRY(strides_ok(fn, "", Nq, D, q_batch_stride, q_head_stride, stride_mult(dtype), Hq > 1 && B > 1));
  TRY(strides_ok(fn, "key/value ", Nk, D, kv_batch_stride, kv_head_stride, kv8 ? 16 : stride_mult(dtype), Hkv > 1 && B > 1));
  TRY(aligned16(fn, "tensors and workspace", {q, k, v, o, workspace}));
  TRY(head_fits(fn, (double)(Nk + 128) * D * 2, 4, ""));
  TRY(workspace_fits(fn, workspace_bytes, fa::decode_workspace_bytes(B, Hq, Hkv, Nq, Nk, D), "fa_fwd_decode_workspace_bytes"));
  fa::DecodeParams p;
  TRY(decode_params(fn, p, q, k, v, o, lse, workspace, B, Hq, Hkv, Nq, Nk, D, scale, q_batch_stride, q_head_stride, is_causal, kv8));
  p.kv_bs = kv_batch_stride; p.kv_hs = kv_head_stride;
  return launched(fn, fa::launch_decode(p, D, dtype, kv8, (hipStream_t)hip_stream));
}
int fa_fwd_decode(const void *q, const void *k, const void *v, void *o, float *lse, int B, int Hq, int Hkv, int Nq, int Nk, int D,
                  float scale, long long q_batch_stride, long long q_head_stride, long long kv_batch_stride, long long kv_head_stride,
                  int is_causal, int dtype, void *workspace, long long workspace_bytes, void *hip_stream) {
  return decode_impl(q, k, v, o, lse, B, Hq, Hkv, Nq, Nk, D, scale, q_batch_stride, q_head_stride, kv_batch_stride, kv_head_stride, is_causal,
                     dtype, dtype == FA_DTYPE_FP8_E4M3, workspace, workspace_bytes, hip_stream);
}
int fa_fwd_decode_kv8(const void *q, const void *k, const void *v, void *o, float *lse, int B, int Hq, int Hkv, int Nq, int Nk, int D,
                      float scale, long long q_batch_stride, long long q_head_stride, long long kv_batch_stride, long long kv_head_stride,
                      int is_causal, int q_dtype, void *workspace, long long workspace_bytes, void *hip_stream) {
  g_err[0] = 0;
  if (q_dtype != FA_DTYPE_BF16 && q_dtype != FA_DTYPE_FP8_E4M3)
    return fail(FA_ERR_UNSUPPORTED, "fa_fwd_decode_kv8: queries must be bf16 (or e4m3: then this is fa_fwd_decode), got %s", fa_dtype_name(q_dtype));
  return decode_impl(q, k, v, o, lse, B, Hq, Hkv, Nq, Nk, D, scale, q_batch_stride, q_head_stride, kv_batch_stride, kv_head_stride, is_causal,
                     q_dtype, 1, workspace, workspace_bytes, hip_stream);
}

int fa_fwd_decode_paged_supported(int q_dtype, int kv_dtype, int D, int Hq, int Hkv, int Nq, int page_size) {
  const bool pair = (q_dtype == kv_dtype && (q_dtype == FA_DTYPE_F16 || q_dtype == FA_DTYPE_BF16 || q_dtype == FA_DTYPE_FP8_E4M3)) ||
                    (q_dtype == FA_DTYPE_BF16 && kv_dtype == FA_DTYPE_FP8_E4M3);
  return pair && fa::page_size_ok(page_size) && fa_fwd_decode_supported(q_dtype, D, Hq, Hkv, Nq);
}
long long fa_fwd_decode_paged_workspace_bytes(int B, int Hq, int Hkv, int Nq, int D, int page_size, int max_pages_per_seq) {
  if (page_size < 1 || max_pages_per_seq < 1 || (long long)page_size * max_pages_per_seq > (1 << 30)) return 0;
  return fa_fwd_decode_workspace_bytes(B, Hq, Hkv, Nq, page_size * max_pages_per_seq, D);  // the dense decode's at the capacity
}
static int decode_paged_impl(const char *fn, const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                             const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages,
                             int max_pages_per_seq, float scale, long long q_batch_stride, long long q_head_stride, long long kv_page_stride,
                             long long kv_head_stride, long long kv_row_stride, long long block_table_stride, int window_left,
                             int window_right, int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes, void *hip_stream,
                             const float *const *sinks = nullptr, const float *softcap = nullptr) {
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k_pages, v_pages, o, block_table, seqlens_k, workspace}));
  if (sinks) TRY(sinks_ok(fn, *sinks));
  if (softcap) TRY(softcap_ok(fn, *softcap));
  TRY(positive(fn, {B, Hq, Hkv, Nq, D, page_size, num_pages, max_pages_per_seq}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(scale_ok(fn, scale));
  if (!fa_fwd_decode_paged_supported(q_dtype, kv_dtype, D, Hq, Hkv, Nq, page_size))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs (q, kv) dtypes f16/f16, bf16/bf16, e4m3/e4m3 or bf16/e4m3, D = 64 | 128, (Hq / Hkv) * Nq "
                "<= 32 packed query rows and a page size of 16, 32, 64, 128 or 256; got q=%s kv=%s D=%d Hq=%d Hkv=%d Nq=%d page_size=%d",
                fn, fa_dtype_name(q_dtype), fa_dtype_name(kv_dtype), D, Hq, Hkv, Nq, page_size);
  TRY(table_stride_ok(fn, block_table_stride, max_pages_per_seq));
  TRY(strides_ok(fn, "", Nq, D, q_batch_stride, q_head_stride, stride_mult(q_dtype), Hq > 1 && B > 1));
  const int kv8 = kv_dtype == FA_DTYPE_FP8_E4M3;
  TRY(page_strides_ok(fn, D, page_size, kv_page_stride, kv_head_stride, kv_row_stride, block_table_stride, kv_dtype));
  TRY(aligned16(fn, "tensors and workspace", {q, k_pages, v_pages, o, workspace}));
  TRY(page_tables_ok(fn, page_size, max_pages_per_seq, block_table, seqlens_k));
  const int cap = page_size * max_pages_per_seq;
  TRY(workspace_fits(fn, workspace_bytes, fa::decode_workspace_bytes(B, Hq, Hkv, Nq, cap, D), "fa_fwd_decode_paged_workspace_bytes"));
  const int route = (sinks || softcap) ? WIN_KERNEL : window_route(window_left, window_right);
  fa::DecodeWindowParams p;
  // Nk = the capacity, hence the dense decode's split rule there: bit-identical to it on full caches
  TRY(decode_params(fn, p, q, k_pages, v_pages, o, lse, workspace, B, Hq, Hkv, Nq, cap, D, scale, q_batch_stride, q_head_stride, route != WIN_FULL, kv8));
  p.kv_bs = 0; p.kv_hs = kv_head_stride;
  p.block_table = block_table; p.seqlens = seqlens_k;
  p.page_stride = kv_page_stride; p.row_stride = kv_row_stride;
  p.bt_stride = (int)block_table_stride; p.num_pages = num_pages; p.max_pages = max_pages_per_seq;
  p.lp = log2_of(page_size);
  if (route != WIN_KERNEL) return launched(fn, fa::launch_decode_paged(p, D, q_dtype, kv8, (hipStream_t)hip_stream));
  p.wl = window_clamp(window_left, cap);
  p.wr = window_clamp(window_right, Nq);
  if (softcap) {
    fa::DecodeSoftcapParams pc;
    static_cast<fa::DecodePagedParams &>(pc) = p;
    pc.wl = p.wl; pc.wr = p.wr; pc.softcap = *softcap;
    return launched(fn, fa::launch_decode_paged_softcap(pc, D, q_dtype, kv8, (hipStream_t)hip_stream));
  }
  if (!sinks) return launched(fn, fa::launch_decode_paged_window(p, D, q_dtype, kv8, (hipStream_t)hip_stream));
  return launched(fn, fa::launch_decode_paged_sink(p, *sinks, D, q_dtype, kv8, (hipStream_t)hip_stream));
}
int fa_fwd_decode_paged(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *block_table,
                        const int *seqlens_k, int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages, int max_pages_per_seq,
                        float scale, long long q_batch_stride, long long q_head_stride, long long kv_page_stride, long long kv_head_stride,
                        long long kv_row_stride, long long block_table_stride, int is_causal, int q_dtype, int kv_dtype, void *workspace,
                        long long workspace_bytes, void *hip_stream) {
  return decode_paged_impl("fa_fwd_decode_paged", q, k_pages, v_pages, o, lse, block_table, seqlens_k, B, Hq, Hkv, Nq, D, page_size, num_pages,
                           max_pages_per_seq, scale, q_batch_stride, q_head_stride, kv_page_stride, kv_head_stride, kv_row_stride,
                           block_table_stride, -1, is_causal ? 0 : -1, q_dtype, kv_dtype, workspace, workspace_bytes, hip_stream);
}
int fa_fwd_decode_paged_window(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *block_table,
                               const int *seqlens_k, int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages,
                               int max_pages_per_seq, float scale, long long q_batch_stride, long long q_head_stride, long long kv_page_stride,
                               long long kv_head_stride, long long kv_row_stride, long long block_table_stride, int window_left,
                               int window_right, int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes, void *hip_stream) {
  return decode_paged_impl("fa_fwd_decode_paged_window", q, k_pages, v_pages, o, lse, block_table, seqlens_k, B, Hq, Hkv, Nq, D, page_size,
                           num_pages, max_pages_per_seq, scale, q_batch_stride, q_head_stride, kv_page_stride, kv_head_stride, kv_row_stride,
                           block_table_stride, window_left, window_right, q_dtype, kv_dtype, workspace, workspace_bytes, hip_stream);
}
int fa_fwd_decode_paged_sink(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *block_table,
                             const int *seqlens_k, int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages,
                             int max_pages_per_seq, float scale, long long q_batch_stride, long long q_head_stride, long long kv_page_stride,
                             long long kv_head_stride, long long kv_row_stride, long long block_table_stride, int window_left,
                             int window_right, const float *sinks, int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes,
                             void *hip_stream) {
  return decode_paged_impl("fa_fwd_decode_paged_sink", q, k_pages, v_pages, o, lse, block_table, seqlens_k, B, Hq, Hkv, Nq, D, page_size,
                           num_pages, max_pages_per_seq, scale, q_batch_stride, q_head_stride, kv_page_stride, kv_head_stride, kv_row_stride,
                           block_table_stride, window_left, window_right, q_dtype, kv_dtype, workspace, workspace_bytes, hip_stream, &sinks);
}
int fa_fwd_decode_paged_softcap(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *block_table,
                                const int *seqlens_k, int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages,
                                int max_pages_per_seq, float scale, long long q_batch_stride, long long q_head_stride,
                                long long kv_page_stride, long long kv_head_stride, long long kv_row_stride, long long block_table_stride,
                                int window_left, int window_right, float softcap, int q_dtype, int kv_dtype, void *workspace,
                                long long workspace_bytes, void *hip_stream) {
  return decode_paged_impl("fa_fwd_decode_paged_softcap", q, k_pages, v_pages, o, lse, block_table, seqlens_k, B, Hq, Hkv, Nq, D, page_size,
                           num_pages, max_pages_per_seq, scale, q_batch_stride, q_head_stride, kv_page_stride, kv_head_stride, kv_row_stride,
                           block_table_stride, window_left, window_right, q_dtype, kv_dtype, workspace, workspace_bytes, hip_stream, nullptr,
                           &softcap);
}

// ---- fa_fwd_mla_decode_paged, fa_fwd_mla_decode_paged_wide and fa_fwd_mla_decode_paged_kv8: the paged decode's rules on one latent pool.
// q and o carry three strides each (a rule of these calls' own); everything else is the shared helpers, in fa_fwd_decode_paged's order,
// with its statuses and texts. One path for all three: the row limit (32 / 128), the block count the split rule is fed, the launcher
// and, for the e4m3 pool, the dtype pair and the pool's stride multiple are all that differ.
static bool mla_decode_shape_ok(int dtype, int Dqk, int Dv, int Hq, int Nq, int page_size, int max_rows) {
  return fa::mla_decode_supported(dtype, Dqk, Dv) && Hq >= 1 && Nq >= 1 && (long long)Hq * Nq <= max_rows && fa::page_size_ok(page_size);
}
static bool mla_workspace_scalars_ok(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq, int max_rows) {
  return B >= 1 && Hq >= 1 && Nq >= 1 && (long long)Hq * Nq <= max_rows && Dv == 512 && fa::page_size_ok(page_size) && max_pages_per_seq >= 1 &&
         (long long)page_size * max_pages_per_seq <= (1 << 30);
}
int fa_fwd_mla_decode_paged_supported(int dtype, int Dqk, int Dv, int Hq, int Nq, int page_size) {
  return mla_decode_shape_ok(dtype, Dqk, Dv, Hq, Nq, page_size, 32);
}
int fa_fwd_mla_decode_paged_wide_supported(int dtype, int Dqk, int Dv, int Hq, int Nq, int page_size) {
  return mla_decode_shape_ok(dtype, Dqk, Dv, Hq, Nq, page_size, 128);
}
long long fa_fwd_mla_decode_paged_workspace_bytes(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq) {
  if (!mla_workspace_scalars_ok(B, Hq, Nq, Dv, page_size, max_pages_per_seq, 32)) return 0;
  return fa::mla_decode_workspace_bytes(B, Hq, Nq, page_size * max_pages_per_seq);  // the split rule at the capacity: host scalars only
}
long long fa_fwd_mla_decode_paged_wide_workspace_bytes(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq) {
  if (!mla_workspace_scalars_ok(B, Hq, Nq, Dv, page_size, max_pages_per_seq, 128)) return 0;
  return fa::mla_decode_wide_workspace_bytes(B, Hq, Nq, page_size * max_pages_per_seq);
}
// one [B, Hq, Nq, D] operand under (batch, head, row) element strides, rows and heads interleaved either way
static int mla_strides_ok(const char *fn, const char *what, int B, int D, long long bs, long long hs, long long rs) {
  if (rs < D || hs < D || bs < 0 || (B > 1 && bs < D) || (bs % 8) || (hs % 8) || (rs % 8))
    return fail(FA_ERR_INVALID_ARG, "%s: bad %sstrides (batch %lld, head %lld, row %lld): a row holds %d elements, strides are multiples of 8", fn,
                what, bs, hs, rs, D);
  return FA_OK;
}
// The three modes of the one path. MLA_WIDE: workgroups of 2 or 4 waves over a shared tile (fa_mla_wide_kernel.hip), up to 128 rows.
// MLA_ONE: one-wave items, up to 32. MLA_KV8: bf16 queries on an e4m3 pool (fa_mla_kv8_kernel.hip), always four waves, up to 128 rows, the
// wide call's split count and workspace; `dtype` is the queries' and kv_dtype the pool's (the other modes: both are `dtype`)
enum { MLA_ONE = 0, MLA_WIDE = 1, MLA_KV8 = 2 };
static bool mla_kv8_shape_ok(int q_dtype, int kv_dtype, int Dqk, int Dv, int Hq, int Nq, int page_size) {
  return q_dtype == FA_DTYPE_BF16 && kv_dtype == FA_DTYPE_FP8_E4M3 && mla_decode_shape_ok(FA_DTYPE_BF16, Dqk, Dv, Hq, Nq, page_size, 128);
}
static int mla_decode_paged_impl(const char *fn, int mode, const void *q, const void *kv_pages, void *o, float *lse, const int *block_table,
                                 const int *seqlens_k, int B, int Hq, int Nq, int Dqk, int Dv, int page_size, int num_pages,
                                 int max_pages_per_seq, float scale, long long q_batch_stride, long long q_head_stride, long long q_row_stride,
                                 long long o_batch_stride, long long o_head_stride, long long o_row_stride, long long kv_page_stride,
                                 long long kv_row_stride, long long block_table_stride, int is_causal, int dtype, int kv_dtype, void *workspace,
                                 long long workspace_bytes, void *hip_stream) {
  g_err[0] = 0;
  const bool wide = mode != MLA_ONE;  // (the e4m3 mode has the wide call's row limit, split count and workspace)
  const int max_rows = wide ? 128 : 32;
  TRY(nonnull(fn, {q, kv_pages, o, block_table, seqlens_k, workspace}));
  TRY(positive(fn, {B, Hq, Nq, Dqk, Dv, page_size, num_pages, max_pages_per_seq}));
  TRY(scale_ok(fn, scale));
  if (mode == MLA_KV8) {
    if (!mla_kv8_shape_ok(dtype, kv_dtype, Dqk, Dv, Hq, Nq, page_size))
      return fail(FA_ERR_UNSUPPORTED, "%s: needs bf16 queries on an e4m3 pool, (Dqk, Dv) = (576, 512), Hq * Nq <= %d packed query rows and a "
                  "page size of 16, 32, 64, 128 or 256; got q=%s kv=%s Dqk=%d Dv=%d Hq=%d Nq=%d page_size=%d", fn, max_rows,
                  fa_dtype_name(dtype), fa_dtype_name(kv_dtype), Dqk, Dv, Hq, Nq, page_size);
  } else if (!mla_decode_shape_ok(dtype, Dqk, Dv, Hq, Nq, page_size, max_rows))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 (q and the pool alike), (Dqk, Dv) = (576, 512), Hq * Nq <= %d packed query rows and a "
                "page size of 16, 32, 64, 128 or 256; got dtype=%s Dqk=%d Dv=%d Hq=%d Nq=%d page_size=%d", fn, max_rows, fa_dtype_name(dtype),
                Dqk, Dv, Hq, Nq, page_size);
  TRY(table_stride_ok(fn, block_table_stride, max_pages_per_seq));
  TRY(mla_strides_ok(fn, "", B, Dqk, q_batch_stride, q_head_stride, q_row_stride));
  TRY(mla_strides_ok(fn, "output ", B, Dv, o_batch_stride, o_head_stride, o_row_stride));
  // (one latent head: no head stride. An e4m3 pool: strides in elements = bytes, multiples of 16 -- fa_fwd_decode_paged's rule)
  TRY(page_strides_ok(fn, Dqk, page_size, kv_page_stride, kv_row_stride, kv_row_stride, block_table_stride, kv_dtype));
  TRY(aligned16(fn, "tensors and workspace", {q, kv_pages, o, workspace}));
  TRY(page_tables_ok(fn, page_size, max_pages_per_seq, block_table, seqlens_k));
  const int cap = page_size * max_pages_per_seq;
  TRY(workspace_fits(fn, workspace_bytes,
                     mode == MLA_KV8    ? fa::mla_decode_kv8_workspace_bytes(B, Hq, Nq, cap)
                     : mode == MLA_WIDE ? fa::mla_decode_wide_workspace_bytes(B, Hq, Nq, cap)
                                        : fa::mla_decode_workspace_bytes(B, Hq, Nq, cap),
                     mode == MLA_KV8    ? "fa_fwd_mla_decode_paged_kv8_workspace_bytes"
                     : mode == MLA_WIDE ? "fa_fwd_mla_decode_paged_wide_workspace_bytes"
                                        : "fa_fwd_mla_decode_paged_workspace_bytes"));
  const int rblk = (Hq * Nq + 15) / 16;
  if ((long long)B * Hq * Nq > 0x7fffffffLL || (long long)B * 256 * rblk > 0x7fffffffLL) return fail(FA_ERR_INVALID_ARG, "%s: grid too large", fn);
  const int nw = mode == MLA_KV8 ? 4 : fa::mla_wide_waves(Hq * Nq);
  fa::MlaDecodeParams p;
  p.q = q; p.kv = kv_pages; p.o = o; p.lse = lse; p.ws = (float *)workspace;
  p.block_table = block_table; p.seqlens = seqlens_k;
  p.B = B; p.Hq = Hq; p.Nq = Nq; p.RBLK = rblk; p.scale = scale;
  p.S = fa::mla_decode_splits(B, wide ? (rblk + nw - 1) / nw : rblk, cap);  // (the wide and e4m3 calls: workgroup row blocks of 16 NW rows)
  p.q_bs = q_batch_stride; p.q_hs = q_head_stride; p.q_rs = q_row_stride;
  p.o_bs = o_batch_stride; p.o_hs = o_head_stride; p.o_rs = o_row_stride;
  p.page_stride = kv_page_stride; p.row_stride = kv_row_stride;
  p.bt_stride = (int)block_table_stride; p.num_pages = num_pages; p.max_pages = max_pages_per_seq;
  p.lp = log2_of(page_size);
  p.is_causal = is_causal ? 1 : 0;
  return launched(fn, mode == MLA_KV8    ? fa::launch_mla_decode_paged_kv8(p, (hipStream_t)hip_stream)
                      : mode == MLA_WIDE ? fa::launch_mla_decode_paged_wide(p, dtype, (hipStream_t)hip_stream)
                                         : fa::launch_mla_decode_paged(p, dtype, (hipStream_t)hip_stream));
}
int fa_fwd_mla_decode_paged(const void *q, const void *kv_pages, void *o, float *lse, const int *block_table, const int *seqlens_k, int B,
                            int Hq, int Nq, int Dqk, int Dv, int page_size, int num_pages, int max_pages_per_seq, float scale,
                            long long q_batch_stride, long long q_head_stride, long long q_row_stride, long long o_batch_stride,
                            long long o_head_stride, long long o_row_stride, long long kv_page_stride, long long kv_row_stride,
                            long long block_table_stride, int is_causal, int dtype, void *workspace, long long workspace_bytes,
                            void *hip_stream) {
  return mla_decode_paged_impl("fa_fwd_mla_decode_paged", MLA_ONE, q, kv_pages, o, lse, block_table, seqlens_k, B, Hq, Nq, Dqk, Dv, page_size,
                               num_pages, max_pages_per_seq, scale, q_batch_stride, q_head_stride, q_row_stride, o_batch_stride, o_head_stride,
                               o_row_stride, kv_page_stride, kv_row_stride, block_table_stride, is_causal, dtype, dtype, workspace,
                               workspace_bytes, hip_stream);
}
int fa_fwd_mla_decode_paged_wide(const void *q, const void *kv_pages, void *o, float *lse, const int *block_table, const int *seqlens_k, int B,
                                 int Hq, int Nq, int Dqk, int Dv, int page_size, int num_pages, int max_pages_per_seq, float scale,
                                 long long q_batch_stride, long long q_head_stride, long long q_row_stride, long long o_batch_stride,
                                 long long o_head_stride, long long o_row_stride, long long kv_page_stride, long long kv_row_stride,
                                 long long block_table_stride, int is_causal, int dtype, void *workspace, long long workspace_bytes,
                                 void *hip_stream) {
  return mla_decode_paged_impl("fa_fwd_mla_decode_paged_wide", MLA_WIDE, q, kv_pages, o, lse, block_table, seqlens_k, B, Hq, Nq, Dqk, Dv, page_size,
                               num_pages, max_pages_per_seq, scale, q_batch_stride, q_head_stride, q_row_stride, o_batch_stride, o_head_stride,
                               o_row_stride, kv_page_stride, kv_row_stride, block_table_stride, is_causal, dtype, dtype, workspace,
                               workspace_bytes, hip_stream);
}

// fa_fwd_mla_decode_paged_kv8: the wide call on an e4m3 pool under bf16 queries -- the third mode of the path above
int fa_fwd_mla_decode_paged_kv8_supported(int q_dtype, int kv_dtype, int Dqk, int Dv, int Hq, int Nq, int page_size) {
  return mla_kv8_shape_ok(q_dtype, kv_dtype, Dqk, Dv, Hq, Nq, page_size);
}
long long fa_fwd_mla_decode_paged_kv8_workspace_bytes(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq) {
  if (!mla_workspace_scalars_ok(B, Hq, Nq, Dv, page_size, max_pages_per_seq, 128)) return 0;
  return fa::mla_decode_kv8_workspace_bytes(B, Hq, Nq, page_size * max_pages_per_seq);
}
int fa_fwd_mla_decode_paged_kv8(const void *q, const void *kv_pages, void *o, float *lse, const int *block_table, const int *seqlens_k, int B,
                                int Hq, int Nq, int Dqk, int Dv, int page_size, int num_pages, int max_pages_per_seq, float scale,
                                long long q_batch_stride, long long q_head_stride, long long q_row_stride, long long o_batch_stride,
                                long long o_head_stride, long long o_row_stride, long long kv_page_stride, long long kv_row_stride,
                                long long block_table_stride, int is_causal, int q_dtype, int kv_dtype, void *workspace,
                                long long workspace_bytes, void *hip_stream) {
  return mla_decode_paged_impl("fa_fwd_mla_decode_paged_kv8", MLA_KV8, q, kv_pages, o, lse, block_table, seqlens_k, B, Hq, Nq, Dqk, Dv,
                               page_size, num_pages, max_pages_per_seq, scale, q_batch_stride, q_head_stride, q_row_stride, o_batch_stride,
                               o_head_stride, o_row_stride, kv_page_stride, kv_row_stride, block_table_stride, is_causal, q_dtype, kv_dtype,
                               workspace, workspace_bytes, hip_stream);
}

// ---- fa_fwd_mla_decode_sparse: the wide call's rules on q, o, the pool and the workspace (the shared helpers, in its order, with its
// statuses and texts; a token is its (b, i) with Nq = 1, so the row stride it checks is the row itself), and in place of the block table
// and the lengths the rules of the index lists. The split count is the wide call's at B = T, Nq = 1 and a capacity of
// cap = 64 ceil(topk / 64) keys: the call's bits are that call's on the gathered pool.
static long long mla_sparse_cap(int topk) { return ((long long)topk + 63) / 64 * 64; }
int fa_fwd_mla_decode_sparse_supported(int dtype, int Dqk, int Dv, int Hq, int page_size) {
  return mla_decode_shape_ok(dtype, Dqk, Dv, Hq, 1, page_size, 128);
}
long long fa_fwd_mla_decode_sparse_workspace_bytes(int T, int Hq, int Dv, int topk) {
  if (topk < 1 || mla_sparse_cap(topk) > (1 << 30)) return 0;
  return fa_fwd_mla_decode_paged_wide_workspace_bytes(T, Hq, 1, Dv, 64, (int)(mla_sparse_cap(topk) / 64));
}
// The two modes of the one path. MLA_SPARSE_WIDE: f16 / bf16, q and the pool alike (fa_mla_sparse_kernel.hip). MLA_SPARSE_KV8: bf16
// queries on an e4m3 pool (fa_mla_sparse_kv8_kernel.hip), the same split count and workspace; `dtype` is the queries' and kv_dtype the
// pool's (the other mode: both are `dtype`). The dtype-pair rule and the pool's stride multiple are all that differ.
enum { MLA_SPARSE_WIDE = 0, MLA_SPARSE_KV8 = 1 };
static bool mla_sparse_kv8_shape_ok(int q_dtype, int kv_dtype, int Dqk, int Dv, int Hq, int page_size) {
  return mla_kv8_shape_ok(q_dtype, kv_dtype, Dqk, Dv, Hq, 1, page_size);
}
static int mla_decode_sparse_impl(const char *fn, int mode, const void *q, const void *kv_pages, void *o, float *lse, const int *indices,
                                  const int *index_counts, int T, int Hq, int Dqk, int Dv, int topk, int page_size, int num_pages, float scale,
                                  long long q_token_stride, long long q_head_stride, long long o_token_stride, long long o_head_stride,
                                  long long kv_page_stride, long long kv_row_stride, long long indices_stride, int dtype, int kv_dtype,
                                  void *workspace, long long workspace_bytes, void *hip_stream) {
  g_err[0] = 0;
  TRY(nonnull(fn, {q, kv_pages, o, indices, workspace}));
  TRY(positive(fn, {T, Hq, Dqk, Dv, topk, page_size, num_pages}));
  TRY(scale_ok(fn, scale));
  if (mode == MLA_SPARSE_KV8) {
    if (!mla_sparse_kv8_shape_ok(dtype, kv_dtype, Dqk, Dv, Hq, page_size))
      return fail(FA_ERR_UNSUPPORTED, "%s: needs bf16 queries on an e4m3 pool, (Dqk, Dv) = (576, 512), Hq <= 128 heads and a page size of "
                  "16, 32, 64, 128 or 256; got q=%s kv=%s Dqk=%d Dv=%d Hq=%d page_size=%d", fn, fa_dtype_name(dtype), fa_dtype_name(kv_dtype),
                  Dqk, Dv, Hq, page_size);
  } else if (!mla_decode_shape_ok(dtype, Dqk, Dv, Hq, 1, page_size, 128))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 (q and the pool alike), (Dqk, Dv) = (576, 512), Hq <= 128 heads and a page size of "
                "16, 32, 64, 128 or 256; got dtype=%s Dqk=%d Dv=%d Hq=%d page_size=%d", fn, fa_dtype_name(dtype), Dqk, Dv, Hq, page_size);
  if (indices_stride < topk || (indices_stride % 4))
    return fail(FA_ERR_INVALID_ARG, "%s: indices_stride=%lld must be a multiple of 4 and >= topk=%d", fn, indices_stride, topk);
  TRY(mla_strides_ok(fn, "", T, Dqk, q_token_stride, q_head_stride, Dqk));
  TRY(mla_strides_ok(fn, "output ", T, Dv, o_token_stride, o_head_stride, Dv));
  // (an e4m3 pool: strides in elements = bytes, multiples of 16, a page counted in bytes of 1 -- fa_fwd_mla_decode_paged_kv8's rule)
  TRY(page_strides_ok(fn, Dqk, page_size, kv_page_stride, kv_row_stride, kv_row_stride, 0, kv_dtype));
  TRY(aligned16(fn, "tensors and workspace", {q, kv_pages, o, workspace}));
  TRY(aligned16(fn, "indices", {indices}));
  if ((uintptr_t)index_counts & 3) return fail(FA_ERR_INVALID_ARG, "%s: index_counts must be int32-aligned", fn);
  if (mla_sparse_cap(topk) > (1 << 30)) return fail(FA_ERR_INVALID_ARG, "%s: capacity above 2^30 keys", fn);
  if ((long long)num_pages * page_size > (1 << 30))
    return fail(FA_ERR_INVALID_ARG, "%s: num_pages * page_size = %lld slots, above 2^30", fn, (long long)num_pages * page_size);
  const int cap = (int)mla_sparse_cap(topk);
  TRY(workspace_fits(fn, workspace_bytes, fa::mla_decode_sparse_workspace_bytes(T, Hq, cap),
                     mode == MLA_SPARSE_KV8 ? "fa_fwd_mla_decode_sparse_kv8_workspace_bytes" : "fa_fwd_mla_decode_sparse_workspace_bytes"));
  const int rblk = (Hq + 15) / 16;
  if ((long long)T * Hq > 0x7fffffffLL || (long long)T * 256 * rblk > 0x7fffffffLL) return fail(FA_ERR_INVALID_ARG, "%s: grid too large", fn);
  const int nw = fa::mla_wide_waves(Hq);
  fa::MlaSparseParams p;
  p.q = q; p.kv = kv_pages; p.ws = (float *)workspace;
  p.indices = indices; p.counts = index_counts;
  p.T = T; p.Hq = Hq; p.Nq = 1; p.RBLK = rblk; p.scale = scale;
  // the wide call's own rule at (T, 1, cap), in both modes: both kernels run four waves for every head count, and for Hq <= 32 (rblk
  // <= 2) the rule is fed ONE row block under either wave count, ceil(rblk / 2) = ceil(rblk / 4) = 1 -- the same S, the same workspace
  p.S = fa::mla_decode_splits(T, (rblk + nw - 1) / nw, cap);
  p.q_bs = q_token_stride; p.q_hs = q_head_stride; p.q_rs = Dqk;
  p.page_stride = kv_page_stride; p.row_stride = kv_row_stride; p.idx_stride = indices_stride;
  p.topk = topk; p.num_slots = num_pages * page_size;
  p.lp = log2_of(page_size);
  fa::MlaDecodeParams pc = {};  // what the combine kernel reads: the workspace's shape and the output
  pc.o = o; pc.lse = lse; pc.ws = p.ws;
  pc.B = T; pc.Hq = Hq; pc.Nq = 1; pc.S = p.S; pc.RBLK = rblk;
  pc.o_bs = o_token_stride; pc.o_hs = o_head_stride; pc.o_rs = Dv;
  return launched(fn, mode == MLA_SPARSE_KV8 ? fa::launch_mla_decode_sparse_kv8(p, pc, (hipStream_t)hip_stream)
                                             : fa::launch_mla_decode_sparse(p, pc, dtype, (hipStream_t)hip_stream));
}
int fa_fwd_mla_decode_sparse(const void *q, const void *kv_pages, void *o, float *lse, const int *indices, const int *index_counts, int T,
                             int Hq, int Dqk, int Dv, int topk, int page_size, int num_pages, float scale, long long q_token_stride,
                             long long q_head_stride, long long o_token_stride, long long o_head_stride, long long kv_page_stride,
                             long long kv_row_stride, long long indices_stride, int dtype, void *workspace, long long workspace_bytes,
                             void *hip_stream) {
  return mla_decode_sparse_impl("fa_fwd_mla_decode_sparse", MLA_SPARSE_WIDE, q, kv_pages, o, lse, indices, index_counts, T, Hq, Dqk, Dv, topk,
                                page_size, num_pages, scale, q_token_stride, q_head_stride, o_token_stride, o_head_stride, kv_page_stride,
                                kv_row_stride, indices_stride, dtype, dtype, workspace, workspace_bytes, hip_stream);
}

// fa_fwd_mla_decode_sparse_kv8: the sparse call on an e4m3 pool under bf16 queries -- the second mode of the path above
int fa_fwd_mla_decode_sparse_kv8_supported(int q_dtype, int kv_dtype, int Dqk, int Dv, int Hq, int page_size) {
  return mla_sparse_kv8_shape_ok(q_dtype, kv_dtype, Dqk, Dv, Hq, page_size);
}
long long fa_fwd_mla_decode_sparse_kv8_workspace_bytes(int T, int Hq, int Dv, int topk) {
  return fa_fwd_mla_decode_sparse_workspace_bytes(T, Hq, Dv, topk);
}
int fa_fwd_mla_decode_sparse_kv8(const void *q, const void *kv_pages, void *o, float *lse, const int *indices, const int *index_counts, int T,
                                 int Hq, int Dqk, int Dv, int topk, int page_size, int num_pages, float scale, long long q_token_stride,
                                 long long q_head_stride, long long o_token_stride, long long o_head_stride, long long kv_page_stride,
                                 long long kv_row_stride, long long indices_stride, int q_dtype, int kv_dtype, void *workspace,
                                 long long workspace_bytes, void *hip_stream) {
  return mla_decode_sparse_impl("fa_fwd_mla_decode_sparse_kv8", MLA_SPARSE_KV8, q, kv_pages, o, lse, indices, index_counts, T, Hq, Dqk, Dv,
                                topk, page_size, num_pages, scale, q_token_stride, q_head_stride, o_token_stride, o_head_stride,
                                kv_page_stride, kv_row_stride, indices_stride, q_dtype, kv_dtype, workspace, workspace_bytes, hip_stream);
}

int fa_fwd_varlen_paged_supported(int dtype, int D, int page_size) { return fa::mfma_varlen_paged_supported(dtype, D, page_size); }
// the key split's scalars: sizes >= 1, a head_dim and a page size the paged prefill has, a capacity of at most 2^30 keys
static bool ksplit_scalars_ok(int B, int Hq, int max_seqlen_q, int D, int page_size, int max_pages_per_seq) {
  return B >= 1 && Hq >= 1 && max_seqlen_q >= 1 && (D == 64 || D == 128) && fa::page_size_ok(page_size) && max_pages_per_seq >= 1 &&
         (long long)page_size * max_pages_per_seq <= (1 << 30) && (long long)B * Hq <= 0x7fffffffLL / (((long long)max_seqlen_q + 127) / 128);  // (64-bit: any int is a legal argument)
}
int fa_fwd_varlen_paged_num_splits(int B, int Hq, int max_seqlen_q, int D, int page_size, int max_pages_per_seq) {
  if (!ksplit_scalars_ok(B, Hq, max_seqlen_q, D, page_size, max_pages_per_seq)) return 0;
  return fa::varlen_paged_ksplit_splits(B, Hq, max_seqlen_q, D, page_size, max_pages_per_seq);
}
long long fa_fwd_varlen_paged_split_workspace_bytes(int B, int Hq, int total_q, int max_seqlen_q, int D, int page_size, int max_pages_per_seq,
                                                    int num_splits) {
  if (!ksplit_scalars_ok(B, Hq, max_seqlen_q, D, page_size, max_pages_per_seq) || total_q < max_seqlen_q || num_splits < 0 ||
      num_splits > FA_VARLEN_PAGED_MAX_SPLITS)
    return 0;
  const int S = num_splits ? num_splits : fa::varlen_paged_ksplit_splits(B, Hq, max_seqlen_q, D, page_size, max_pages_per_seq);
  if (S < 2) return 0;
  const long long rows = (long long)Hq * total_q, per_row = (long long)S * (D + 1) * 4;  // rows < 2^62, per_row <= 64 * 129 * 4
  if (rows > (0x7fffffffffffffffLL - 15) / per_row) return 0;                             // no such size: invalid, like the other zeros
  return (rows * per_row + 15) / 16 * 16;
}
struct KsplitArgs {
  int num_splits;
  void *workspace;
  long long workspace_bytes;
};
static int varlen_paged_impl(const char *fn, const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                             const int *cu_seqlens_q, const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q,
                             int max_seqlen_q, int D, int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride,
                             long long q_head_stride, long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                             long long block_table_stride, int window_left, int window_right, int dtype, void *hip_stream,
                             const float *const *sinks = nullptr, const int *kv8_dtype = nullptr, const float *softcap = nullptr,
                             const KsplitArgs *ksplit = nullptr) {
  // ksplit (fa_fwd_varlen_paged_split): every rule below first, then the split count's range and -- where it resolves to two or more --
  // the workspace. Routing is the sink calls': always the window family. One split launches that family's kernel and nothing else.
  // kv8_dtype (fa_fwd_varlen_paged_kv8): `dtype` is q's and *kv8_dtype the pools'. Every rule below is the one path of both families;
  // what differs is the support table with its text, the pools' stride multiple and bytes per element (page_pool_ok under the pools'
  // type), and the routing: that call always runs its own kernel family, with or without sinks.
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k_pages, v_pages, o, cu_seqlens_q, block_table, seqlens_k}));
  if (sinks) TRY(sinks_ok(fn, *sinks));
  if (softcap) TRY(softcap_ok(fn, *softcap));
  TRY(positive(fn, {B, Hq, Hkv, total_q, max_seqlen_q, D, page_size, num_pages, max_pages_per_seq}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(scale_ok(fn, scale));
  const int kv_dtype = kv8_dtype ? *kv8_dtype : dtype;
  if (kv8_dtype && !fa_fwd_varlen_paged_kv8_supported(dtype, kv_dtype, D, page_size))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs bf16 queries on an fp8_e4m3 pool, D = 64 | 128 and a page size of 16, 32, 64, 128 or 256; "
                "got q=%s kv=%s D=%d page_size=%d (q and the pool of one 16-bit type: fa_fwd_varlen_paged)", fn, fa_dtype_name(dtype),
                fa_dtype_name(kv_dtype), D, page_size);
  if (!kv8_dtype && !fa_fwd_varlen_paged_supported(dtype, D, page_size))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 (q and the pool alike), D = 64 | 128 and a page size of 16, 32, 64, 128 or 256; "
                "got dtype=%s D=%d page_size=%d (an e4m3 pool: fa_fwd_decode_paged)", fn, fa_dtype_name(dtype), D, page_size);
  if (max_seqlen_q > total_q)
    return fail(FA_ERR_INVALID_ARG, "%s: max_seqlen_q=%d exceeds the token count %d", fn, max_seqlen_q, total_q);
  TRY(varlen_strides_ok(fn, "", D, q_row_stride, q_head_stride, stride_mult(dtype)));
  TRY(page_pool_ok(fn, D, page_size, max_pages_per_seq, kv_page_stride, kv_head_stride, kv_row_stride, block_table_stride, kv_dtype, block_table, seqlens_k));
  TRY(aligned16(fn, "tensors", {q, k_pages, v_pages, o}));
  if ((uintptr_t)cu_seqlens_q & 3) return fail(FA_ERR_INVALID_ARG, "%s: cu_seqlens_q must be int32-aligned", fn);
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)q_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  int S = 1;
  if (ksplit) {  // (in front of the grid rule, the last one: a call that is right up to there has been through these)
    if (ksplit->num_splits < 0 || ksplit->num_splits > FA_VARLEN_PAGED_MAX_SPLITS)
      return fail(FA_ERR_INVALID_ARG, "%s: num_splits=%d must be 0 (the heuristic) .. %d", fn, ksplit->num_splits, FA_VARLEN_PAGED_MAX_SPLITS);
    S = ksplit->num_splits ? ksplit->num_splits : fa::varlen_paged_ksplit_splits(B, Hq, max_seqlen_q, D, page_size, max_pages_per_seq);
    if (S >= 2) {
      if (!ksplit->workspace) return fail(FA_ERR_INVALID_ARG, "%s: null pointer", fn);
      TRY(aligned16(fn, "workspace", {ksplit->workspace}));
      TRY(workspace_fits(fn, ksplit->workspace_bytes,
                         fa_fwd_varlen_paged_split_workspace_bytes(B, Hq, total_q, max_seqlen_q, D, page_size, max_pages_per_seq, S),
                         "fa_fwd_varlen_paged_split_workspace_bytes"));
    }
  }
  TRY(grid_fits(fn, (long long)B * Hq, max_seqlen_q));
  const int route = (sinks || kv8_dtype || softcap || ksplit) ? WIN_KERNEL : window_route(window_left, window_right);
  fa::VarlenPagedSinkParams p;
  p.q = q; p.k = k_pages; p.v = v_pages; p.o = o; p.lse = lse;
  p.B = B; p.H = Hq; p.Hkv = Hkv; p.N = max_seqlen_q; p.Nk = page_size * max_pages_per_seq; p.D = D; p.scale = scale;
  p.batch_stride = 0; p.head_stride = q_head_stride; p.kv_batch_stride = 0; p.kv_head_stride = kv_head_stride;
  p.is_causal = route != WIN_FULL;
  p.cu_q = cu_seqlens_q; p.cu_k = nullptr;
  p.total_q = total_q; p.total_k = 0;
  p.q_rs = q_row_stride; p.kv_rs = kv_row_stride;
  p.block_table = block_table; p.seqlens = seqlens_k;
  p.page_stride = kv_page_stride;
  p.bt_stride = (int)block_table_stride; p.num_pages = num_pages; p.max_pages = max_pages_per_seq;
  p.lp = log2_of(page_size);
  if (route != WIN_KERNEL) return launched(fn, fa::launch_mfma_varlen_paged(p, dtype, (hipStream_t)hip_stream));
  p.wl = window_clamp(window_left, p.Nk);
  p.wr = window_clamp(window_right, max_seqlen_q);
  p.sinks = sinks ? *sinks : nullptr;
  if (softcap) {
    fa::VarlenPagedSoftcapParams pc;
    static_cast<fa::VarlenPagedWindowParams &>(pc) = p;
    pc.softcap = *softcap;
    return launched(fn, fa::launch_mfma_varlen_paged_softcap(pc, dtype, (hipStream_t)hip_stream));
  }
  if (kv8_dtype) return launched(fn, fa::launch_mfma_varlen_paged_kv8(p, sinks != nullptr, (hipStream_t)hip_stream));
  if (S >= 2) {
    fa::VarlenPagedKsplitParams pk;
    static_cast<fa::VarlenPagedWindowParams &>(pk) = p;
    pk.sinks = p.sinks; pk.ws = (float *)ksplit->workspace; pk.S = S;
    return launched(fn, fa::launch_mfma_varlen_paged_ksplit(pk, dtype, (hipStream_t)hip_stream));
  }
  if (!sinks) return launched(fn, fa::launch_mfma_varlen_paged_window(p, dtype, (hipStream_t)hip_stream));
  return launched(fn, fa::launch_mfma_varlen_paged_sink(p, dtype, (hipStream_t)hip_stream));
}
int fa_fwd_varlen_paged(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *cu_seqlens_q,
                        const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                        int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride, long long q_head_stride,
                        long long kv_page_stride, long long kv_head_stride, long long kv_row_stride, long long block_table_stride,
                        int is_causal, int dtype, void *hip_stream) {
  return varlen_paged_impl("fa_fwd_varlen_paged", q, k_pages, v_pages, o, lse, cu_seqlens_q, block_table, seqlens_k, B, Hq, Hkv, total_q,
                           max_seqlen_q, D, page_size, num_pages, max_pages_per_seq, scale, q_row_stride, q_head_stride, kv_page_stride,
                           kv_head_stride, kv_row_stride, block_table_stride, -1, is_causal ? 0 : -1, dtype, hip_stream);
}
int fa_fwd_varlen_paged_window(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *cu_seqlens_q,
                               const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                               int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride,
                               long long q_head_stride, long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                               long long block_table_stride, int window_left, int window_right, int dtype, void *hip_stream) {
  return varlen_paged_impl("fa_fwd_varlen_paged_window", q, k_pages, v_pages, o, lse, cu_seqlens_q, block_table, seqlens_k, B, Hq, Hkv, total_q,
                           max_seqlen_q, D, page_size, num_pages, max_pages_per_seq, scale, q_row_stride, q_head_stride, kv_page_stride,
                           kv_head_stride, kv_row_stride, block_table_stride, window_left, window_right, dtype, hip_stream);
}
int fa_fwd_varlen_paged_sink(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *cu_seqlens_q,
                             const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                             int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride,
                             long long q_head_stride, long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                             long long block_table_stride, int window_left, int window_right, const float *sinks, int dtype,
                             void *hip_stream) {
  return varlen_paged_impl("fa_fwd_varlen_paged_sink", q, k_pages, v_pages, o, lse, cu_seqlens_q, block_table, seqlens_k, B, Hq, Hkv, total_q,
                           max_seqlen_q, D, page_size, num_pages, max_pages_per_seq, scale, q_row_stride, q_head_stride, kv_page_stride,
                           kv_head_stride, kv_row_stride, block_table_stride, window_left, window_right, dtype, hip_stream, &sinks);
}
int fa_fwd_varlen_paged_softcap(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *cu_seqlens_q,
                                const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride,
                                long long q_head_stride, long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                                long long block_table_stride, int window_left, int window_right, float softcap, int dtype,
                                void *hip_stream) {
  return varlen_paged_impl("fa_fwd_varlen_paged_softcap", q, k_pages, v_pages, o, lse, cu_seqlens_q, block_table, seqlens_k, B, Hq, Hkv,
                           total_q, max_seqlen_q, D, page_size, num_pages, max_pages_per_seq, scale, q_row_stride, q_head_stride,
                           kv_page_stride, kv_head_stride, kv_row_stride, block_table_stride, window_left, window_right, dtype, hip_stream,
                           nullptr, nullptr, &softcap);
}
int fa_fwd_varlen_paged_split(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *cu_seqlens_q,
                              const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                              int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride,
                              long long q_head_stride, long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                              long long block_table_stride, int window_left, int window_right, const float *sinks, int dtype,
                              int num_splits, void *workspace, long long workspace_bytes, void *hip_stream) {
  // sinks may be NULL, as in fa_fwd_varlen_paged_kv8
  const KsplitArgs ks = {num_splits, workspace, workspace_bytes};
  return varlen_paged_impl("fa_fwd_varlen_paged_split", q, k_pages, v_pages, o, lse, cu_seqlens_q, block_table, seqlens_k, B, Hq, Hkv, total_q,
                           max_seqlen_q, D, page_size, num_pages, max_pages_per_seq, scale, q_row_stride, q_head_stride, kv_page_stride,
                           kv_head_stride, kv_row_stride, block_table_stride, window_left, window_right, dtype, hip_stream,
                           sinks ? &sinks : nullptr, nullptr, nullptr, &ks);
}
int fa_fwd_varlen_paged_kv8_supported(int q_dtype, int kv_dtype, int D, int page_size) {
  return fa::mfma_varlen_paged_kv8_supported(q_dtype, kv_dtype, D, page_size);
}
int fa_fwd_varlen_paged_kv8(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse, const int *cu_seqlens_q,
                            const int *block_table, const int *seqlens_k, int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                            int page_size, int num_pages, int max_pages_per_seq, float scale, long long q_row_stride,
                            long long q_head_stride, long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                            long long block_table_stride, int window_left, int window_right, const float *sinks, int q_dtype, int kv_dtype,
                            void *hip_stream) {
  // sinks may be NULL here: the call without a sink term (a non-NULL pointer is held to sinks_ok)
  return varlen_paged_impl("fa_fwd_varlen_paged_kv8", q, k_pages, v_pages, o, lse, cu_seqlens_q, block_table, seqlens_k, B, Hq, Hkv, total_q,
                           max_seqlen_q, D, page_size, num_pages, max_pages_per_seq, scale, q_row_stride, q_head_stride, kv_page_stride,
                           kv_head_stride, kv_row_stride, block_table_stride, window_left, window_right, q_dtype, hip_stream,
                           sinks ? &sinks : nullptr, &kv_dtype);
}

// fa_kv_append_paged and fa_kv_append_paged_quant: one path. quant: `dtype` is the new rows' (f16 / bf16), the pools are e4m3
static int kv_append_impl(const char *fn, const void *k_new, const void *v_new, void *k_pages, void *v_pages, const int *cu_seqlens_new,
                          const int *block_table, const int *seqlens_k, int B, int Hkv, int total_new, int max_seqlen_new, int D,
                          int page_size, int num_pages, int max_pages_per_seq, long long new_row_stride, long long new_head_stride,
                          long long kv_page_stride, long long kv_head_stride, long long kv_row_stride, long long block_table_stride,
                          int dtype, bool quant, float k_mul, float v_mul, void *hip_stream);

int fa_kv_append_paged(const void *k_new, const void *v_new, void *k_pages, void *v_pages, const int *cu_seqlens_new, const int *block_table,
                       const int *seqlens_k, int B, int Hkv, int total_new, int max_seqlen_new, int D, int page_size, int num_pages,
                       int max_pages_per_seq, long long new_row_stride, long long new_head_stride, long long kv_page_stride,
                       long long kv_head_stride, long long kv_row_stride, long long block_table_stride, int dtype, void *hip_stream) {
  return kv_append_impl("fa_kv_append_paged", k_new, v_new, k_pages, v_pages, cu_seqlens_new, block_table, seqlens_k, B, Hkv, total_new,
                        max_seqlen_new, D, page_size, num_pages, max_pages_per_seq, new_row_stride, new_head_stride, kv_page_stride,
                        kv_head_stride, kv_row_stride, block_table_stride, dtype, false, 1.0f, 1.0f, hip_stream);
}
int fa_kv_append_paged_quant(const void *k_new, const void *v_new, void *k_pages, void *v_pages, const int *cu_seqlens_new,
                             const int *block_table, const int *seqlens_k, int B, int Hkv, int total_new, int max_seqlen_new, int D,
                             int page_size, int num_pages, int max_pages_per_seq, long long new_row_stride, long long new_head_stride,
                             long long kv_page_stride, long long kv_head_stride, long long kv_row_stride, long long block_table_stride,
                             int new_dtype, float k_mul, float v_mul, void *hip_stream) {
  return kv_append_impl("fa_kv_append_paged_quant", k_new, v_new, k_pages, v_pages, cu_seqlens_new, block_table, seqlens_k, B, Hkv, total_new,
                        max_seqlen_new, D, page_size, num_pages, max_pages_per_seq, new_row_stride, new_head_stride, kv_page_stride,
                        kv_head_stride, kv_row_stride, block_table_stride, new_dtype, true, k_mul, v_mul, hip_stream);
}
static int kv_append_impl(const char *fn, const void *k_new, const void *v_new, void *k_pages, void *v_pages, const int *cu_seqlens_new,
                          const int *block_table, const int *seqlens_k, int B, int Hkv, int total_new, int max_seqlen_new, int D,
                          int page_size, int num_pages, int max_pages_per_seq, long long new_row_stride, long long new_head_stride,
                          long long kv_page_stride, long long kv_head_stride, long long kv_row_stride, long long block_table_stride,
                          int dtype, bool quant, float k_mul, float v_mul, void *hip_stream) {
  g_err[0] = 0;
  TRY(nonnull(fn, {k_new, v_new, k_pages, v_pages, cu_seqlens_new, block_table, seqlens_k}));
  TRY(positive(fn, {B, Hkv, total_new, max_seqlen_new, D, page_size, num_pages, max_pages_per_seq}));
  const int pool_dtype = quant ? FA_DTYPE_FP8_E4M3 : dtype;
  const int bytes = fa_dtype_in_bytes(pool_dtype);
  if (quant) {
    if ((dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16) || D % 16 || !fa::page_size_ok(page_size))
      return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 new rows (the pools are fp8_e4m3), rows of whole 16-byte chunks and a page size of "
                  "16, 32, 64, 128 or 256; got new_dtype=%s D=%d page_size=%d", fn, fa_dtype_name(dtype), D, page_size);
    // (the negated form refuses NaN as well)
    if (!(k_mul > 0.0f && k_mul <= 3.4028234663852886e38f) || !(v_mul > 0.0f && v_mul <= 3.4028234663852886e38f))
      return fail(FA_ERR_INVALID_ARG, "%s: k_mul=%g and v_mul=%g must be > 0 and finite", fn, (double)k_mul, (double)v_mul);
  } else if ((dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16 && dtype != FA_DTYPE_FP8_E4M3) || ((long long)D * bytes) % 16 || !fa::page_size_ok(page_size))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 / fp8_e4m3, rows of whole 16-byte chunks and a page size of 16, 32, 64, 128 "
                "or 256; got dtype=%s D=%d page_size=%d", fn, fa_dtype_name(dtype), D, page_size);
  if (max_seqlen_new > total_new)
    return fail(FA_ERR_INVALID_ARG, "%s: max_seqlen_new=%d exceeds the token count %d", fn, max_seqlen_new, total_new);
  TRY(varlen_strides_ok(fn, "new key/value ", D, new_row_stride, new_head_stride, stride_mult(dtype)));
  TRY(page_pool_ok(fn, D, page_size, max_pages_per_seq, kv_page_stride, kv_head_stride, kv_row_stride, block_table_stride, pool_dtype, block_table, seqlens_k));
  TRY(aligned16(fn, "tensors", {k_new, v_new, k_pages, v_pages}));
  if ((uintptr_t)cu_seqlens_new & 3) return fail(FA_ERR_INVALID_ARG, "%s: cu_seqlens_new must be int32-aligned", fn);
  const long long nblk = (max_seqlen_new + fa::APPEND_ROWS - 1) / fa::APPEND_ROWS;
  if (Hkv > 65535 || (long long)B * nblk > 0x7fffffffLL) return fail(FA_ERR_INVALID_ARG, "%s: grid too large", fn);
  fa::AppendPagedParams p;
  p.k_new = k_new; p.v_new = v_new; p.k_pages = k_pages; p.v_pages = v_pages;
  p.cu_new = cu_seqlens_new; p.block_table = block_table; p.seqlens = seqlens_k;
  p.B = B; p.Hkv = Hkv; p.total_new = total_new; p.max_new = max_seqlen_new; p.D = D;
  p.new_rs = new_row_stride; p.new_hs = new_head_stride;
  p.page_stride = kv_page_stride; p.head_stride = kv_head_stride; p.row_stride = kv_row_stride;
  p.bt_stride = (int)block_table_stride; p.num_pages = num_pages; p.max_pages = max_pages_per_seq;
  p.lp = log2_of(page_size);
  if (quant) return launched(fn, fa::launch_kv_append_paged_quant(p, dtype, k_mul, v_mul, (hipStream_t)hip_stream));
  return launched(fn, fa::launch_kv_append_paged(p, bytes, (hipStream_t)hip_stream));
}

long long fa_bwd_workspace_bytes(int B, int H, int N) { return (long long)B * H * N * 4; }
// elements from the first to one past the last of a [B,H,N,D] tensor under (batch, head) strides, rounded up to 16
static long long extent16(int B, int H, int N, int D, long long bs, long long hs) {
  const long long e = (long long)(B - 1) * bs + (long long)(H - 1) * hs + (long long)N * D;
  return (e + 15) / 16 * 16;
}
static long long align256(long long x) { return (x + 255) / 256 * 256; }
long long fa_bwd_workspace_bytes_ex(int dtype, int B, int Hq, int Hkv, int Nq, int Nk, int D, long long q_batch_stride,
                                    long long q_head_stride, long long kv_batch_stride, long long kv_head_stride) {
  long long bytes = align256((long long)B * Hq * Nq * 4);
  if (dtype == FA_DTYPE_FP8_E4M3)  // bf16 copies of Q, K, V under their own strides
    bytes += align256(2 * extent16(B, Hq, Nq, D, q_batch_stride, q_head_stride)) +
             2 * align256(2 * extent16(B, Hkv, Nk, D, kv_batch_stride, kv_head_stride));
  return bytes;
}
int fa_bwd_supported(int dtype, int D) { return fa::bwd_supported(dtype, D); }
double fa_bwd_algorithmic_flops(int B, int H, int N, int D, int is_causal) {
  return 2.5 * fa_algorithmic_flops(B, H, N, D, is_causal);
}

static int bwd_impl(const char *fn, const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                    float *dq, float *dk, float *dv, void *workspace, int B, int H, int Hkv, int N, int Nk, int D, float scale,
                    long long bs, long long hs, long long kbs, long long khs, int is_causal, int dtype, void *hip_stream) {
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k, v, o, d_o, lse, dq, dk, dv, workspace}));
  TRY(positive(fn, {B, H, N, Nk, D}));
  TRY(causal_fits(fn, is_causal, N, Nk));
  TRY(grouped(fn, H, Hkv));
  TRY(scale_ok(fn, scale));
  TRY(strides_ok(fn, "", N, D, bs, hs, stride_mult(dtype), H > 1));
  TRY(strides_ok(fn, "key/value ", Nk, D, kbs, khs, stride_mult(dtype), Hkv > 1));
  TRY(aligned16(fn, "tensors", {q, k, v, o, d_o, dq, dk, dv}));
  if (!fa::bwd_supported(dtype, D))
    return fail(FA_ERR_UNSUPPORTED, "%s: no kernel for dtype=%s D=%d (f16 / bf16: D a multiple of 8 up to 128, or 256; fp8_e4m3: D a multiple of 16 up to 128)", fn, fa_dtype_name(dtype), D);
  const int rows = std::max(N, Nk);
  TRY(head_fits(fn, (double)rows * D * 2, 4, ""));
  // head dims other than 64 / 128 run on zero-padded rows whose padding is fetched from offset 2^31 + ... (fa_bwd_kernels.hip, PAD)
  if (D != 64 && D != 128 && D != 256)  // (+128: rows past the end are addressed too)
    TRY(head_fits(fn, (double)(rows + 128) * D * 2, 2, " (head dims other than 64 / 128)"));
  TRY(grid_fits(fn, (long long)B * H, rows));
  if (dtype == FA_DTYPE_FP8_E4M3) {
    TRY(aligned16(fn, "workspace", {workspace}));
    // e4m3 Q, K, V (O and dO are bf16, as fa_fwd writes O for this dtype): widen them into the workspace behind delta
    // (layout of fa_bwd_workspace_bytes_ex) and run the bf16 kernels on the copies
    char *w = (char *)workspace + align256((long long)B * H * N * 4);
    const long long eq = extent16(B, H, N, D, bs, hs), ek = extent16(B, Hkv, Nk, D, kbs, khs);
    void *q16 = w, *k16 = w + align256(2 * eq), *v16 = w + align256(2 * eq) + align256(2 * ek);
    hipError_t ec = fa::launch_widen_e4m3(q, q16, eq, (hipStream_t)hip_stream);
    if (ec == hipSuccess) ec = fa::launch_widen_e4m3(k, k16, ek, (hipStream_t)hip_stream);
    if (ec == hipSuccess) ec = fa::launch_widen_e4m3(v, v16, ek, (hipStream_t)hip_stream);
    TRY(launched(fn, ec));
    q = q16; k = k16; v = v16;
    dtype = FA_DTYPE_BF16;
  }
  return launched(fn, fa::launch_bwd(q, k, v, o, d_o, lse, dq, dk, dv, (float *)workspace, B, H, Hkv, N, Nk, D, scale, bs, hs, kbs, khs,
                                     is_causal ? 1 : 0, dtype, (hipStream_t)hip_stream));
}

int fa_bwd(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
           float *dk, float *dv, void *workspace, int B, int H, int N, int D, float scale, long long batch_stride,
           long long head_stride, int is_causal, int dtype, void *hip_stream) {
  return bwd_impl("fa_bwd", q, k, v, o, d_o, lse, dq, dk, dv, workspace, B, H, H, N, N, D, scale, batch_stride, head_stride,
                  batch_stride, head_stride, is_causal, dtype, hip_stream);
}

int fa_bwd_ex(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
              float *dk, float *dv, void *workspace, int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale,
              long long q_batch_stride, long long q_head_stride, long long kv_batch_stride, long long kv_head_stride,
              int is_causal, int dtype, void *hip_stream) {
  return bwd_impl("fa_bwd_ex", q, k, v, o, d_o, lse, dq, dk, dv, workspace, B, Hq, Hkv, Nq, Nk, D, scale, q_batch_stride,
                  q_head_stride, kv_batch_stride, kv_head_stride, is_causal, dtype, hip_stream);
}

long long fa_bwd_varlen_workspace_bytes(int Hq, int total_q) { return Hq < 1 || total_q < 1 ? 0 : (long long)Hq * total_q * 4; }
int fa_bwd_varlen_supported(int dtype, int D) { return fa::bwd_varlen_supported(dtype, D); }
// fa_bwd_varlen (window_left = -1, window_right = is_causal ? 0 : -1), fa_bwd_varlen_window and fa_bwd_varlen_sink (`sinks`: its own
// argument, null for the other two; dsinks may be null): one set of rules, one launch path. The sinks need nothing of the dQ and dK/dV
// kernels -- the forward's LSE contains them -- so those launch exactly as for fa_bwd_varlen_window; the dsink reduction follows them.
static int bwd_varlen_impl(const char *fn, const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                           float *dq, float *dk, float *dv, void *workspace, const int *cu_seqlens_q, const int *cu_seqlens_k, int B, int Hq,
                           int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale, long long q_row_stride,
                           long long q_head_stride, long long kv_row_stride, long long kv_head_stride, int window_left, int window_right,
                           int dtype, void *hip_stream, const float *const *sinks = nullptr, float *dsinks = nullptr,
                           const float *softcap = nullptr) {
  // softcap (fa_bwd_varlen_softcap): always the windowed kernels, in their softcap mode
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k, v, o, d_o, lse, dq, dk, dv, workspace, cu_seqlens_q, cu_seqlens_k}));
  if (sinks) {
    TRY(sinks_ok(fn, *sinks));
    if ((uintptr_t)dsinks & 3) return fail(FA_ERR_INVALID_ARG, "%s: dsinks must be fp32-aligned", fn);
  }
  if (softcap) TRY(softcap_ok(fn, *softcap));
  TRY(positive(fn, {B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, D}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(scale_ok(fn, scale));
  if (!fa_bwd_varlen_supported(dtype, D))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 and D = 64 | 128, got dtype=%s D=%d", fn, fa_dtype_name(dtype), D);
  if (max_seqlen_q > total_q || max_seqlen_k > total_k)
    return fail(FA_ERR_INVALID_ARG, "%s: max_seqlen (%d, %d) exceeds the token count (%d, %d)", fn, max_seqlen_q, max_seqlen_k, total_q, total_k);
  TRY(varlen_strides_ok(fn, "", D, q_row_stride, q_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "key/value ", D, kv_row_stride, kv_head_stride, stride_mult(dtype)));
  TRY(aligned16(fn, "tensors", {q, k, v, o, d_o, dq, dk, dv}));
  if (((uintptr_t)cu_seqlens_q | (uintptr_t)cu_seqlens_k) & 3) return fail(FA_ERR_INVALID_ARG, "%s: cu_seqlens_q / cu_seqlens_k must be int32-aligned", fn);
  if (((uintptr_t)lse | (uintptr_t)workspace) & 3) return fail(FA_ERR_INVALID_ARG, "%s: lse / workspace must be fp32-aligned", fn);
  // as fa_fwd_varlen: 32-bit byte offsets inside ONE sequence of one head of the 16-bit tensors (the gradients are stored through 64-bit
  // addresses), and the staging may address up to two 64-row tiles past its end
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)q_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_k + 128) * (double)kv_row_stride * 2, 4, " (one sequence of max_seqlen_k rows)"));
  TRY(grid_fits(fn, (long long)B * Hq, max_seqlen_q));   // the dQ kernel's
  TRY(grid_fits(fn, (long long)B * Hkv, max_seqlen_k));  // the dK/dV kernel's
  const int route = window_route(window_left, window_right);
  hipError_t e;
  if (softcap)
    e = fa::launch_bwd_varlen_softcap(q, k, v, o, d_o, lse, dq, dk, dv, (float *)workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q,
                                      total_k, max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride,
                                      kv_head_stride, window_clamp(window_left, max_seqlen_k), window_clamp(window_right, max_seqlen_q),
                                      *softcap, dtype, (hipStream_t)hip_stream);
  else if (route != WIN_KERNEL)
    e = fa::launch_bwd_varlen(q, k, v, o, d_o, lse, dq, dk, dv, (float *)workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q, total_k,
                              max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride,
                              route == WIN_CAUSAL ? 1 : 0, dtype, (hipStream_t)hip_stream);
  else
    e = fa::launch_bwd_varlen_window(q, k, v, o, d_o, lse, dq, dk, dv, (float *)workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q,
                                     total_k, max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride,
                                     kv_head_stride, window_clamp(window_left, max_seqlen_k), window_clamp(window_right, max_seqlen_q),
                                     dtype, (hipStream_t)hip_stream);
  if (e == hipSuccess && sinks && dsinks)
    e = fa::launch_dsink(*sinks, lse, (const float *)workspace, dsinks, cu_seqlens_q, B, Hq, total_q, max_seqlen_q, (hipStream_t)hip_stream);
  return launched(fn, e);
}
int fa_bwd_varlen(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq, float *dk,
                  float *dv, void *workspace, const int *cu_seqlens_q, const int *cu_seqlens_k, int B, int Hq, int Hkv, int total_q,
                  int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale, long long q_row_stride, long long q_head_stride,
                  long long kv_row_stride, long long kv_head_stride, int is_causal, int dtype, void *hip_stream) {
  return bwd_varlen_impl("fa_bwd_varlen", q, k, v, o, d_o, lse, dq, dk, dv, workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q, total_k,
                         max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride, -1,
                         is_causal ? 0 : -1, dtype, hip_stream);
}
int fa_bwd_varlen_window(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq, float *dk,
                         float *dv, void *workspace, const int *cu_seqlens_q, const int *cu_seqlens_k, int B, int Hq, int Hkv, int total_q,
                         int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale, long long q_row_stride,
                         long long q_head_stride, long long kv_row_stride, long long kv_head_stride, int window_left, int window_right,
                         int dtype, void *hip_stream) {
  return bwd_varlen_impl("fa_bwd_varlen_window", q, k, v, o, d_o, lse, dq, dk, dv, workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q,
                         total_k, max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride,
                         window_left, window_right, dtype, hip_stream);
}
int fa_bwd_varlen_sink(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq, float *dk,
                       float *dv, void *workspace, const int *cu_seqlens_q, const int *cu_seqlens_k, int B, int Hq, int Hkv, int total_q,
                       int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale, long long q_row_stride, long long q_head_stride,
                       long long kv_row_stride, long long kv_head_stride, int window_left, int window_right, const float *sinks,
                       float *dsinks, int dtype, void *hip_stream) {
  return bwd_varlen_impl("fa_bwd_varlen_sink", q, k, v, o, d_o, lse, dq, dk, dv, workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q,
                         total_k, max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride,
                         window_left, window_right, dtype, hip_stream, &sinks, dsinks);
}
int fa_bwd_varlen_softcap(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq, float *dk,
                          float *dv, void *workspace, const int *cu_seqlens_q, const int *cu_seqlens_k, int B, int Hq, int Hkv, int total_q,
                          int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale, long long q_row_stride,
                          long long q_head_stride, long long kv_row_stride, long long kv_head_stride, int window_left, int window_right,
                          float softcap, int dtype, void *hip_stream) {
  return bwd_varlen_impl("fa_bwd_varlen_softcap", q, k, v, o, d_o, lse, dq, dk, dv, workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv, total_q,
                         total_k, max_seqlen_q, max_seqlen_k, D, scale, q_row_stride, q_head_stride, kv_row_stride, kv_head_stride,
                         window_left, window_right, dtype, hip_stream, nullptr, nullptr, &softcap);
}
// fa_bwd_varlen_mla: fa_bwd_varlen's rules in its order, with the stride, alignment and 4 GiB rules once per tensor as fa_fwd_varlen_mla
// has them (q, k, v, o; d_o under o's strides, the gradients under those of q, k, v)
int fa_bwd_varlen_mla_supported(int dtype, int Dqk, int Dv) { return fa::bwd_varlen_mla_supported(dtype, Dqk, Dv); }
int fa_bwd_varlen_mla(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq, float *dk,
                      float *dv, void *workspace, const int *cu_seqlens_q, const int *cu_seqlens_k, int B, int Hq, int Hkv, int total_q,
                      int total_k, int max_seqlen_q, int max_seqlen_k, int Dqk, int Dv, float scale, long long q_row_stride,
                      long long q_head_stride, long long k_row_stride, long long k_head_stride, long long v_row_stride,
                      long long v_head_stride, long long o_row_stride, long long o_head_stride, int is_causal, int dtype, void *hip_stream) {
  const char *fn = "fa_bwd_varlen_mla";
  g_err[0] = 0;
  TRY(nonnull(fn, {q, k, v, o, d_o, lse, dq, dk, dv, workspace, cu_seqlens_q, cu_seqlens_k}));
  TRY(positive(fn, {B, Hq, Hkv, total_q, total_k, max_seqlen_q, max_seqlen_k, Dqk, Dv}));
  TRY(grouped(fn, Hq, Hkv));
  TRY(scale_ok(fn, scale));
  if (!fa_bwd_varlen_mla_supported(dtype, Dqk, Dv))
    return fail(FA_ERR_UNSUPPORTED, "%s: needs f16 / bf16 and (Dqk, Dv) = (192, 128), got dtype=%s Dqk=%d Dv=%d", fn, fa_dtype_name(dtype), Dqk, Dv);
  if (max_seqlen_q > total_q || max_seqlen_k > total_k)
    return fail(FA_ERR_INVALID_ARG, "%s: max_seqlen (%d, %d) exceeds the token count (%d, %d)", fn, max_seqlen_q, max_seqlen_k, total_q, total_k);
  TRY(varlen_strides_ok(fn, "", Dqk, q_row_stride, q_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "key ", Dqk, k_row_stride, k_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "value ", Dv, v_row_stride, v_head_stride, stride_mult(dtype)));
  TRY(varlen_strides_ok(fn, "output ", Dv, o_row_stride, o_head_stride, stride_mult(dtype)));
  TRY(aligned16(fn, "tensors", {q, k, v, o, d_o, dq, dk, dv}));
  if (((uintptr_t)cu_seqlens_q | (uintptr_t)cu_seqlens_k) & 3) return fail(FA_ERR_INVALID_ARG, "%s: cu_seqlens_q / cu_seqlens_k must be int32-aligned", fn);
  if (((uintptr_t)lse | (uintptr_t)workspace) & 3) return fail(FA_ERR_INVALID_ARG, "%s: lse / workspace must be fp32-aligned", fn);
  // 32-bit byte offsets inside ONE sequence of one head of the 16-bit tensors, per tensor (the gradients are stored through 64-bit addresses)
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)q_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_q + 128) * (double)o_row_stride * 2, 4, " (one sequence of max_seqlen_q rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_k + 128) * (double)k_row_stride * 2, 4, " (one sequence of max_seqlen_k rows)"));
  TRY(head_fits(fn, (double)(max_seqlen_k + 128) * (double)v_row_stride * 2, 4, " (one sequence of max_seqlen_k rows)"));
  TRY(grid_fits(fn, (long long)B * Hq, max_seqlen_q));   // the dQ kernel's
  TRY(grid_fits(fn, (long long)B * Hkv, max_seqlen_k));  // the dK/dV kernel's
  return launched(fn, fa::launch_bwd_varlen_mla(q, k, v, o, d_o, lse, dq, dk, dv, (float *)workspace, cu_seqlens_q, cu_seqlens_k, B, Hq, Hkv,
                                                total_q, total_k, max_seqlen_q, max_seqlen_k, scale, q_row_stride, q_head_stride, k_row_stride,
                                                k_head_stride, v_row_stride, v_head_stride, o_row_stride, o_head_stride, is_causal ? 1 : 0,
                                                dtype, (hipStream_t)hip_stream));
}
int fa_window_query_range(int Lq, int Lk, int window_left, int window_right, int key_first, int key_last, int *row_lo, int *row_hi) {
  g_err[0] = 0;
  if (!row_lo || !row_hi) return fail(FA_ERR_INVALID_ARG, "fa_window_query_range: null pointer");
  if (Lq < 0 || Lk < 0) return fail(FA_ERR_INVALID_ARG, "fa_window_query_range: lengths must be >= 0");
  fa::window_query_range(Lq, Lk, window_left, window_right, key_first, key_last, *row_lo, *row_hi);
  return FA_OK;
}

}  // extern "C"
