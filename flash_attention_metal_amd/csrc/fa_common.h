// fa_common.h -- internal declarations shared by the gfx950 kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <set>
#include <utility>

#include "../../include/fa_mi355.h"

namespace fa {

// One launch of the operator (mirror of the binding table kernels.metal:600-613).
// Exact unsigned division by a run-time constant (Granlund-Montgomery): q = (t + ((n - t) >> sh1)) >> sh2 with
// t = mulhi(mul, n). The kernels map a block id to (batch, head, q block) with five divisions by launch constants; as
// generic divisions they cost ~30 instructions each and sat in front of the first global load of every workgroup.
struct FastDiv {
  unsigned mul = 1, sh1 = 0, sh2 = 0;  // default: divide by 1
};
inline FastDiv make_fastdiv(unsigned d) {  // d >= 1
  unsigned l = 0;
  while ((1ull << l) < d) ++l;  // ceil(log2 d)
  FastDiv f;
  f.mul = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  f.sh1 = l < 1 ? l : 1u;
  f.sh2 = l > 1 ? l - 1 : 0u;
  return f;
}

struct Params {
  const void *q, *k, *v;
  void *o;
  float *lse;  // nullable
  int B, H, N, D;
  float scale;
  long long batch_stride, head_stride;  // elements
  int is_causal;
  // generalised operator (fa_fwd_ex; fa_fwd sets Nk = N, Hkv = H, kv strides = q strides):
  int Nk = 0, Hkv = 0;                          // keys per head; key/value heads (H % Hkv == 0)
  long long kv_batch_stride = 0, kv_head_stride = 0;
  int exact = 0;       // 128-row kernel: 1 = no pre-scaled query operand (variant mfma_exact)
  int head_group = 0;  // internal: causal blocks are issued heaviest-first within groups of this many heads (0 = all)
  // internal, filled by the matrix-core launchers (set_block_divisors): divisors of the block id -> (batch, head, q block) map
  int nq = 0, hg = 0;  // q blocks per head for this kernel's block height; effective head group (a divisor of B*H)
  FastDiv fd_h, fd_gq, fd_nq, fd_hg, fd_per;  // by H, H/Hkv, nq, hg, hg*nq
};

// one fa_fwd_varlen call (the varlen mode of csrc/fa_mfma_kernel.hip): q / o are [total_q, H, D] and k / v [total_k, Hkv, D] under a row
// (token) stride and the head strides of Params; B counts sequences, N / Nk hold max_seqlen_q / max_seqlen_k (the grid and the issue
// order depend on nothing else), batch strides are unused. Sequence b owns tokens cu_q[b] .. cu_q[b+1) and keys cu_k[b] .. cu_k[b+1):
// both tables are device memory read by the kernels only.
struct VarlenParams : Params {
  const int *cu_q, *cu_k;     // int32 [B + 1]
  int total_q, total_k;       // tokens in q / o and in k / v: every table entry is clamped to [0, total]
  long long q_rs, kv_rs;      // row strides, elements
};

// one fa_fwd_varlen_mla call (the MLA mode of the varlen mode, csrc/fa_mfma_kernel.hip): q / k rows of 192 elements, v / o rows of 128, and
// a (row, head) stride pair per tensor -- q: q_rs / head_stride, k: kv_rs / kv_head_stride, v and o: the four below. D holds 192.
struct VarlenMlaParams : VarlenParams {
  long long v_rs, v_head_stride, o_rs, o_head_stride;  // elements
};

// one fa_fwd_varlen_paged call (the varlen paged mode of csrc/fa_mfma_kernel.hip): the query side of VarlenParams (cu_k / total_k unused);
// k / v are the page pools, kv_head_stride their head stride, kv_rs their row stride, Nk the capacity max_pages * page size. Key j of
// sequence b is slot j % P of page block_table[b * bt_stride + j / P]; both tables are device memory read by the kernels.
struct VarlenPagedParams : VarlenParams {
  const int *block_table, *seqlens;
  long long page_stride;  // elements
  int bt_stride, num_pages, max_pages;
  int lp;  // log2 of the page size (16 .. 256)
};

// The sliding window of the *_window entry points (include/fa_mi355.h, "Sliding window"): key j is visible to query i iff
// i + coff - wl <= j <= i + coff + wr and 0 <= j < Lk, with coff = Lk - Lq; a negative wl / wr leaves that side unbounded. The half-open
// key range [lo, hi) that rows row_first .. row_last (clamped to the sequence's rows) see together; empty iff lo >= hi. 64-bit
// arithmetic: any int is a legal argument. fa_window_key_range is this function; the windowed kernels take their first and last tile
// from it.
__host__ __device__ inline void window_key_range(int Lq, int Lk, int wl, int wr, int row_first, int row_last, int &lo, int &hi) {
  const long long coff = (long long)Lk - Lq;
  const long long r0 = row_first > 0 ? row_first : 0, r1 = row_last < Lq - 1 ? row_last : (long long)Lq - 1;
  lo = hi = 0;
  if (r0 > r1 || Lk <= 0) return;
  const long long a = wl < 0 ? 0 : r0 + coff - wl, b = wr < 0 ? (long long)Lk : r1 + coff + wr + 1;
  lo = (int)(a < 0 ? 0 : a > Lk ? Lk : a);
  hi = (int)(b < 0 ? 0 : b > Lk ? Lk : b);
}

// The inverse: the half-open query range [lo, hi) of the rows that see at least one of the keys key_first .. key_last (clamped to the
// sequence's keys) -- key j is seen by rows j - coff - wr <= i <= j - coff + wl, 0 <= i < Lq; empty iff lo >= hi. 64-bit arithmetic:
// any int is a legal argument. fa_window_query_range is this function; the windowed dK/dV kernel takes its first and last query tile
// from it.
__host__ __device__ inline void window_query_range(int Lq, int Lk, int wl, int wr, int key_first, int key_last, int &lo, int &hi) {
  const long long coff = (long long)Lk - Lq;
  const long long k0 = key_first > 0 ? key_first : 0, k1 = key_last < Lk - 1 ? key_last : (long long)Lk - 1;
  lo = hi = 0;
  if (k0 > k1 || Lq <= 0) return;
  const long long a = wr < 0 ? 0 : k0 - coff - wr, b = wl < 0 ? (long long)Lq : k1 - coff + wl + 1;
  lo = (int)(a < 0 ? 0 : a > Lq ? Lq : a);
  hi = (int)(b < 0 ? 0 : b > Lq ? Lq : b);
}

// the windowed modes of csrc/fa_mfma_kernel.hip (fa_fwd_varlen_window, fa_fwd_varlen_paged_window): the un-windowed call's parameters
// plus both bounds, which the host has made non-negative (an unbounded or oversized side is the smallest value that can never bind: wl
// <= max keys, wr <= max_seqlen_q -- so that coff - wl and row + coff + wr stay inside an int)
struct VarlenWindowParams : VarlenParams {
  int wl, wr;
};
struct VarlenPagedWindowParams : VarlenPagedParams {
  int wl, wr;
};

// the sink modes of the windowed modes (fa_fwd_varlen_sink, fa_fwd_varlen_paged_sink; include/fa_mi355.h, "Attention sinks"): the windowed
// call's parameters plus one fp32 logit per QUERY head (natural-log units, the softmax scale is not applied to it), device memory read
// by the kernels only. It enters the row's denominator once, in the epilogue.
struct VarlenSinkParams : VarlenWindowParams {
  const float *sinks;  // [H]
};
struct VarlenPagedSinkParams : VarlenPagedWindowParams {
  const float *sinks;  // [H]
};

// the KV8 modes of the paged window / sink modes (fa_fwd_varlen_paged_kv8; include/fa_mi355.h, "e4m3 pools in the prefill"): the same
// parameters over pools of OCP e4m3 bytes -- page_stride, kv_head_stride and kv_rs count elements of ONE byte. Types of their own, because
// the kernel body picks the register staging with the widening by the parameter type.
struct VarlenPagedKv8Params : VarlenPagedWindowParams {};
struct VarlenPagedKv8SinkParams : VarlenPagedSinkParams {};

// the key-split mode of the paged window mode (fa_fwd_varlen_paged_split; include/fa_mi355.h, "Key split in the paged prefill"): the
// windowed call's parameters plus the split count S >= 2 and the caller's workspace. Split s (= blockIdx.y of the partial grid) of a
// block walks the tiles ksplit_tiles gives it and leaves, per owned row, the normalised state (o_s = acc / l in fp32, lse2_s = m + log2 l)
// in the workspace: [S][H * total_q][D] floats of o_s, then [S][H * total_q] floats of lse2_s, row index hq * total_q + token as in LSE.
// The combine kernel takes the same parameters (o, lse, cu_q, sinks).
struct VarlenPagedKsplitParams : VarlenPagedWindowParams {
  const float *sinks;  // [H] or nullptr: read by the combine kernel only
  float *ws;
  int S;
};
// tiles [t0, t1) of split s of S over a block whose tile range is [tb, nT): the decode's rule per block, n = nT - tb <= 2^24, S <= 64
__host__ __device__ inline void ksplit_tiles(int tb, int nT, int s, int S, int &t0, int &t1) {
  const unsigned n = (unsigned)(nT - tb);
  t0 = tb + (int)((unsigned)s * n / (unsigned)S);
  t1 = tb + (int)((unsigned)(s + 1) * n / (unsigned)S);
}

// the softcap modes of the windowed modes (fa_fwd_varlen_softcap, fa_fwd_varlen_paged_softcap; include/fa_mi355.h, "Logit soft-capping"):
// the windowed call's parameters plus the cap, a finite positive host scalar. Every score becomes softcap * tanh(scale * s / softcap)
// before the mask; the kernels pre-scale the query operand by 2 log2(e) scale / softcap instead of scale log2(e).
struct VarlenSoftcapParams : VarlenWindowParams {
  float softcap;
};
struct VarlenPagedSoftcapParams : VarlenPagedWindowParams {
  float softcap;
};

// tanh as the softcap kernels of all three families evaluate it, from y = 2 x log2(e) (what the matrix core delivers under the pre-scaled
// operand): 1 - 2 / (1 + 2^y), one v_exp_f32 and one v_rcp_f32. Finite at both ends: 2^y = inf gives 1, 2^y = 0 gives -1.
__device__ __forceinline__ float tanh_from_exp2_arg(float y) {
  return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y)), 1.0f);
}

// one fa_fwd_decode call (csrc/fa_decode_kernel.hip)
struct DecodeParams {
  const void *q, *k, *v;
  void *o;
  float *lse;  // nullable
  float *ws;   // workspace: per item [16 QT rows][D] partial O (unnormalised), then [16 QT rows][2] (m, l)
  int B, Hq, Hkv, Nq, Nk;
  float scale;
  long long q_bs, q_hs, kv_bs, kv_hs;  // elements
  int is_causal;
  int S;  // key splits per (batch, key head)
  int q8 = 0;  // e4m3 K / V: the queries are e4m3 too (else 16-bit)
};

// one fa_fwd_decode_paged call: k / v are the page pools, kv_hs their head stride, Nk the capacity max_pages * page size (kv_bs unused).
// Key j of sequence b is slot j % P of page block_table[b * bt_stride + j / P]; both tables are device memory read by the kernels.
struct DecodePagedParams : DecodeParams {
  const int *block_table, *seqlens;
  long long page_stride, row_stride;  // elements
  int bt_stride, num_pages, max_pages;
  int lp;  // log2 of the page size (16 .. 256)
};

// one fa_fwd_decode_paged_window call: the paged decode's parameters plus both bounds, made non-negative by the host (wl <= capacity,
// wr <= Nq: see VarlenWindowParams)
struct DecodeWindowParams : DecodePagedParams {
  int wl, wr;
};

// the combine step of fa_fwd_decode_paged_sink: what the combine kernel reads of a decode call, plus the sinks ([Hq] fp32, natural-log
// units). The partial kernels of the windowed call run unchanged; the sink is folded once per row behind the splits' reduction.
struct CombineSinkParams : DecodeParams {
  const float *sinks;
};

// one fa_fwd_decode_paged_softcap call: the windowed paged decode's parameters plus the cap (see VarlenSoftcapParams). The combine kernels
// run unchanged: they see only (acc, m, l).
struct DecodeSoftcapParams : DecodePagedParams {
  int wl, wr;
  float softcap;
};

// one fa_fwd_mla_decode_paged call (csrc/fa_mla_kernel.hip): kv is the one latent pool ([num_pages, P, 576]: no head stride), q and o
// carry (batch, head, row) element strides of their own. Rows r = h * Nq + iq are packed into RBLK blocks of 16.
struct MlaDecodeParams {
  const void *q, *kv;
  void *o;
  float *lse;  // nullable
  float *ws;   // workspace: per (b, split, row block) [16][512] partial O (unnormalised), then [16][2] (m, l)
  const int *block_table, *seqlens;
  int B, Hq, Nq;
  int S;     // key splits per sequence
  int RBLK;  // 16-row blocks: ceil(Hq * Nq / 16), 1 or 2 (fa_fwd_mla_decode_paged_wide: up to 8)
  float scale;
  long long q_bs, q_hs, q_rs, o_bs, o_hs, o_rs, page_stride, row_stride;  // elements
  int bt_stride, num_pages, max_pages;
  int lp;  // log2 of the page size (16 .. 256)
  int is_causal;
};

// one fa_fwd_mla_decode_sparse call (csrc/fa_mla_sparse_kernel.hip): the partial kernel's view. A token is what the dense calls name
// (b, i): fa_mla_body.h reads q, q_bs (the token stride), q_hs, q_rs, Nq (= 1), Hq, scale, ws and RBLK under these names. Keys are SLOTS
// x = page * P + row of the pool, named by indices[t][0 .. n_t - 1]. The combine kernel gets a MlaDecodeParams with B = T, Nq = 1.
struct MlaSparseParams {
  const void *q, *kv;
  float *ws;  // workspace: the dense calls' format, per (token, split, row block)
  const int *indices, *counts;  // [T, idx_stride]; [T] or null (every list holds topk entries)
  int T, Hq, Nq;
  int S;     // key splits per token
  int RBLK;  // 16-row blocks: ceil(Hq / 16)
  float scale;
  long long q_bs, q_hs, q_rs, page_stride, row_stride, idx_stride;  // elements
  int topk, num_slots;  // entries per list; num_pages * P
  int lp;               // log2 of the page size (16 .. 256)
};

// dtype tags
struct F32 {};
struct F16 {};
struct BF16 {};
struct FP8 {};

// launchers: return hipError_t of the launch
hipError_t launch_naive(const Params &p, int dtype, hipStream_t s);
hipError_t launch_tiled(const Params &p, int dtype, hipStream_t s);
hipError_t launch_tiled_v2(const Params &p, int dtype, hipStream_t s);
hipError_t launch_mfma(const Params &p, int dtype, hipStream_t s);
hipError_t launch_mfma_varlen(const VarlenParams &p, int dtype, hipStream_t s);
bool mfma_varlen_supported(int dtype, int D);
// fa_fwd_varlen_mla: (Dqk, Dv) = (192, 128), f16 / bf16
hipError_t launch_mfma_varlen_mla(const VarlenMlaParams &p, int dtype, hipStream_t s);
bool mfma_varlen_mla_supported(int dtype, int Dqk, int Dv);
hipError_t launch_mfma_varlen_paged(const VarlenPagedParams &p, int dtype, hipStream_t s);
bool mfma_varlen_paged_supported(int dtype, int D, int page_size);
// page sizes of the paged entry points: 16, 32, 64, 128 or 256 rows
inline bool page_size_ok(int page_size) { return page_size >= 16 && page_size <= 256 && (page_size & (page_size - 1)) == 0; }
hipError_t launch_mfma_varlen_window(const VarlenWindowParams &p, int dtype, hipStream_t s);
hipError_t launch_mfma_varlen_paged_window(const VarlenPagedWindowParams &p, int dtype, hipStream_t s);
hipError_t launch_mfma_varlen_sink(const VarlenSinkParams &p, int dtype, hipStream_t s);
hipError_t launch_mfma_varlen_paged_sink(const VarlenPagedSinkParams &p, int dtype, hipStream_t s);
hipError_t launch_mfma_varlen_softcap(const VarlenSoftcapParams &p, int dtype, hipStream_t s);
hipError_t launch_mfma_varlen_paged_softcap(const VarlenPagedSoftcapParams &p, int dtype, hipStream_t s);
// fa_fwd_varlen_paged_kv8: bf16 queries on e4m3 pools, always the KV8 window-mode kernels (with_sink: p.sinks is read, their sink mode)
hipError_t launch_mfma_varlen_paged_kv8(const VarlenPagedSinkParams &p, bool with_sink, hipStream_t s);
bool mfma_varlen_paged_kv8_supported(int q_dtype, int kv_dtype, int D, int page_size);
// fa_fwd_varlen_paged_split with S >= 2: the key-split partial kernel on the block map times S, then the combine kernel on the block map
hipError_t launch_mfma_varlen_paged_ksplit(const VarlenPagedKsplitParams &p, int dtype, hipStream_t s);
// the split count fa_fwd_varlen_paged_num_splits answers (host scalars only; arguments already validated)
int varlen_paged_ksplit_splits(int B, int Hq, int max_seqlen_q, int D, int page_size, int max_pages_per_seq);
// fa_kv_append_paged (csrc/fa_decode_kernel.hip): a byte copy of new K / V rows into their slots of the page pools
struct AppendPagedParams {
  const void *k_new, *v_new;
  void *k_pages, *v_pages;
  const int *cu_new, *block_table, *seqlens;
  int B, Hkv, total_new, max_new, D;
  long long new_rs, new_hs, page_stride, head_stride, row_stride;  // elements
  int bt_stride, num_pages, max_pages;
  int lp;  // log2 of the page size
};
constexpr int APPEND_ROWS = 16;  // new rows per workgroup of the append kernel
hipError_t launch_kv_append_paged(const AppendPagedParams &p, int elem_bytes, hipStream_t s);
// fa_kv_append_paged_quant: the same placement with 16-bit new rows (new_dtype f16 / bf16) quantised into e4m3 pools,
// byte = e4m3_rne(clamp(fp32(x) * mul, -448, 448))
hipError_t launch_kv_append_paged_quant(const AppendPagedParams &p, int new_dtype, float k_mul, float v_mul, hipStream_t s);
hipError_t launch_mfma_split2(const Params &p, int dtype, hipStream_t s);
bool mfma_split2_supported(int dtype, int D);
hipError_t launch_mfma_h64s2(const Params &p, int dtype, hipStream_t s);
bool mfma_h64s2_supported(int dtype, int D);
hipError_t launch_mfma16(const Params &p, int dtype, hipStream_t s);
bool mfma16_supported(int dtype, int D);
int mfma16_waves(int D, int BH, int N, int Nk, int is_causal);  // 4 or 8 waves (128 / 256 query rows) per workgroup
hipError_t launch_fp8pv(const Params &p, int dtype, hipStream_t s);
bool fp8pv_supported(int dtype, int D);
hipError_t launch_splitkv(const Params &p, int dtype, hipStream_t s);

hipError_t launch_decode(const DecodeParams &p, int D, int dtype, int kv8, hipStream_t s);
bool decode_supported(int dtype, int D);
int decode_splits(int B, int Hkv, int Nk, int D, int kv8);  // kv8: e4m3 inputs (one LDS image per item: twice the items per CU)
long long decode_workspace_bytes(int B, int Hq, int Hkv, int Nq, int Nk, int D);
hipError_t launch_decode_paged(const DecodePagedParams &p, int D, int dtype, int kv8, hipStream_t s);
hipError_t launch_decode_paged_window(const DecodeWindowParams &p, int D, int dtype, int kv8, hipStream_t s);
// fa_fwd_decode_paged_sink: the windowed partial kernels, then the combine kernel that folds sinks[hq] into every row
hipError_t launch_decode_paged_sink(const DecodeWindowParams &p, const float *sinks, int D, int dtype, int kv8, hipStream_t s);
// fa_fwd_decode_paged_softcap: the windowed partial kernels in their softcap mode, then the unchanged paged combine
hipError_t launch_decode_paged_softcap(const DecodeSoftcapParams &p, int D, int dtype, int kv8, hipStream_t s);
// fa_fwd_mla_decode_paged (csrc/fa_mla_kernel.hip): (Dqk, Dv) = (576, 512), f16 / bf16; the split rule at the capacity Nk
hipError_t launch_mla_decode_paged(const MlaDecodeParams &p, int dtype, hipStream_t s);
bool mla_decode_supported(int dtype, int Dqk, int Dv);
int mla_decode_splits(int B, int rblk, int Nk);
long long mla_decode_workspace_bytes(int B, int Hq, int Nq, int Nk);
// fa_fwd_mla_decode_paged_wide (csrc/fa_mla_wide_kernel.hip): up to 128 packed rows in workgroups of NW waves x 16 rows over one shared
// tile image; the split rule is fed the ceil(rows / (16 NW)) workgroup row blocks; the workspace format and the combine kernel are the
// one-wave call's
inline int mla_wide_waves(int rows) { return rows <= 32 ? 2 : 4; }
hipError_t launch_mla_decode_paged_wide(const MlaDecodeParams &p, int dtype, hipStream_t s);
hipError_t launch_mla_combine(const MlaDecodeParams &p, int dtype, hipStream_t s);
long long mla_decode_wide_workspace_bytes(int B, int Hq, int Nq, int Nk);
// fa_fwd_mla_decode_paged_kv8 (csrc/fa_mla_kv8_kernel.hip): bf16 queries on an e4m3 latent pool, always four waves, the tile staged through
// registers and widened into the wide call's image; the wide call's split count, workspace and combine kernel
hipError_t launch_mla_decode_paged_kv8(const MlaDecodeParams &p, hipStream_t s);
long long mla_decode_kv8_workspace_bytes(int B, int Hq, int Nq, int Nk);
// fa_fwd_mla_decode_sparse (csrc/fa_mla_sparse_kernel.hip): the wide call's workgroup over tiles gathered from a per-token list of slots,
// always four waves; the wide call's split count and workspace at B = T, Nq = 1 and the capacity cap = 64 ceil(topk / 64), its combine
// kernel on pc
hipError_t launch_mla_decode_sparse(const MlaSparseParams &p, const MlaDecodeParams &pc, int dtype, hipStream_t s);
long long mla_decode_sparse_workspace_bytes(int T, int Hq, int cap);
// fa_fwd_mla_decode_sparse_kv8 (csrc/fa_mla_sparse_kv8_kernel.hip): the sparse call over an e4m3 pool (p's pool strides count bytes), bf16
// queries, the tile staged through registers and widened as fa_fwd_mla_decode_paged_kv8 does; the sparse call's split count, workspace
// and (bf16) combine kernel
hipError_t launch_mla_decode_sparse_kv8(const MlaSparseParams &p, const MlaDecodeParams &pc, hipStream_t s);
bool naive_supported(int dtype, int D);
bool tiled_supported(int dtype, int D);
bool tiled_v2_supported(int dtype, int D);
bool mfma_supported(int dtype, int D);
bool splitkv_supported(int dtype, int D);
int splitkv_waves(int D, int Nk);
bool bwd_supported(int dtype, int D);
hipError_t launch_widen_e4m3(const void *in, void *out, long long n, hipStream_t s);  // e4m3 -> bf16, n % 16 == 0
hipError_t launch_bwd(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                      float *dq, float *dk, float *dv, float *ws, int B, int H, int Hkv, int N, int Nk, int D, float scale,
                      long long bs, long long hs, long long kv_bs, long long kv_hs, int causal, int dtype, hipStream_t s);
// fa_bwd_varlen (csrc/fa_bwd_varlen_kernels.hip): max_q / max_k size the grids, the cu tables are device memory
bool bwd_varlen_supported(int dtype, int D);
hipError_t launch_bwd_varlen(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                             float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                             int total_k, int max_q, int max_k, int D, float scale, long long q_rs, long long q_hs, long long kv_rs,
                             long long kv_hs, int causal, int dtype, hipStream_t s);
// fa_bwd_varlen_window (csrc/fa_bwd_window_kernels.hip): the same under a window whose bounds the caller has made non-negative
hipError_t launch_bwd_varlen_window(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                                    float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                                    int total_k, int max_q, int max_k, int D, float scale, long long q_rs, long long q_hs, long long kv_rs,
                                    long long kv_hs, int wl, int wr, int dtype, hipStream_t s);
// fa_bwd_varlen_softcap (csrc/fa_bwd_softcap_kernels.hip): fa_bwd_varlen_window under a logit cap (finite, > 0)
hipError_t launch_bwd_varlen_softcap(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                                     float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                                     int total_k, int max_q, int max_k, int D, float scale, long long q_rs, long long q_hs, long long kv_rs,
                                     long long kv_hs, int wl, int wr, float softcap, int dtype, hipStream_t s);
// fa_bwd_varlen_mla (csrc/fa_bwd_mla_kernels.hip): the backward of the MLA prefill, head dims (192, 128), a stride pair per tensor
bool bwd_varlen_mla_supported(int dtype, int Dqk, int Dv);
hipError_t launch_bwd_varlen_mla(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse, float *dq,
                                 float *dk, float *dv, float *ws, const int *cu_q, const int *cu_k, int B, int H, int Hkv, int total_q,
                                 int total_k, int max_q, int max_k, float scale, long long q_rs, long long q_hs, long long k_rs,
                                 long long k_hs, long long v_rs, long long v_hs, long long o_rs, long long o_hs, int causal, int dtype,
                                 hipStream_t s);
// the sinks' gradient of fa_bwd_varlen_sink (csrc/fa_sink_kernels.hip): dsinks[h] = -sum_i exp(sinks[h] - lse[h, i]) * delta[h, i] over the
// query tokens a sequence owns, one workgroup per head, launched behind the dQ kernel that wrote delta
hipError_t launch_dsink(const float *sinks, const float *lse, const float *delta, float *dsinks, const int *cu_q, int B, int H, int total_q,
                        int max_q, hipStream_t s);

// ---- host-side launch helper shared by every kernel file that needs more than 48 KiB of dynamic LDS
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device) instead of on every launch.
inline hipError_t set_dyn_lds_once(const void *fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void *, int>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.insert({fn, dev});
  return e;
}

// ---- element load/store helpers for the scalar kernels -------------------
__device__ __forceinline__ float ld_elem(const float *p, long long i) { return p[i]; }
__device__ __forceinline__ float ld_elem(const _Float16 *p, long long i) { return (float)p[i]; }
__device__ __forceinline__ float ld_elem(const __bf16 *p, long long i) { return (float)p[i]; }
__device__ __forceinline__ void st_elem(float *p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void st_elem(_Float16 *p, long long i, float v) { p[i] = (_Float16)v; }
__device__ __forceinline__ void st_elem(__bf16 *p, long long i, float v) { p[i] = (__bf16)v; }

}  // namespace fa
