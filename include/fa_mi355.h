/*
 * fa_mi355.h -- C-ABI of the MI355X (gfx950) attention-forward kernel library.
 *
 * This is the drop-in boundary for the reference's one operator,
 *     (Q, K, V, is_causal) -> O (+ LSE)
 * The reference has no FFI: its operator interface is the Metal binding table
 * of flash_attention_v4_half_kernel (/root/reference/kernels.metal:600-613) as
 * bound by the host at /root/reference/main.mm:821-852. fa_fwd() replaces that
 * table one argument for one slot:
 *
 *   buffer 0-2  Q,K,V  kernels.metal:601-603 / main.mm:822-824  -> q, k, v
 *   buffer 3    O      kernels.metal:604     / main.mm:825      -> o
 *   bytes  4    N      kernels.metal:605     / main.mm:826      -> N
 *   bytes  5    D      kernels.metal:606     / main.mm:827      -> D
 *   bytes  6    scale  kernels.metal:607     / main.mm:828      -> scale
 *   bytes  7,8  batch_stride, head_stride (elements)
 *                      kernels.metal:608-609 / main.mm:835-839  -> batch_stride, head_stride
 *   buffer 9    L_out  kernels.metal:611     / main.mm:840      -> lse  ([B,H,N] fp32)
 *   bytes  10   is_causal kernels.metal:612  / main.mm:842-843  -> is_causal
 *   grid (ceil(N/16), H, B) main.mm:846-852                     -> B, H (grid is the library's business)
 *
 * The other kernels the reference host dispatches by name
 * (naive_attention_kernel kernels.metal:12, flash_attention_kernel :72,
 * flash_attention_v2_kernel :462, flash_attention_simd_kernel :177;
 * looked up at main.mm:69-95) are selected with `variant`.
 *
 * Conventions (mirroring main.mm): the caller owns every buffer, all pointers
 * are DEVICE pointers, the library allocates nothing and keeps no state, the
 * launch is asynchronous on `hip_stream` (hipStream_t, may be NULL = default
 * stream) and re-entrant across devices/streams. Errors are returned, never
 * exit()ed (main.mm:16-22 exits; a library must not).
 */
#ifndef FA_MI355_H
#define FA_MI355_H

#ifdef __cplusplus
extern "C" {
#endif

#define FA_MI355_VERSION 400 /* major*10000 + minor*100 + patch */

/* element type of Q, K, V and O */
enum fa_dtype {
  FA_DTYPE_F32 = 0,      /* naive / v1 / v2 variants (kernels.metal:12,72,462) */
  FA_DTYPE_F16 = 1,      /* the reference operator's type (kernels.metal:601) */
  FA_DTYPE_BF16 = 2,     /* BASELINE.json configs 3,4 */
  FA_DTYPE_FP8_E4M3 = 3  /* Q,K,V OCP e4m3fn, O bf16, fp32 accumulate (BASELINE.json config 5); MFMA variant only */
};

/* which kernel computes the operator */
enum fa_variant {
  FA_VARIANT_AUTO = 0,   /* fastest kernel that supports (dtype, D) */
  FA_VARIANT_NAIVE = 1,  /* one thread per query row, two passes   (kernels.metal:12-64)   */
  FA_VARIANT_TILED = 2,  /* LDS-tiled scalar "V1"                  (kernels.metal:72-171)  */
  FA_VARIANT_TILED_V2 = 3, /* 128-bit loads, double-buffered K/V "V2" (kernels.metal:462-596) */
  FA_VARIANT_MFMA = 4,   /* matrix-core kernel "V3/V4"             (kernels.metal:177,600): 128 query rows per workgroup */
  FA_VARIANT_MFMA_PP = 5, /* RETIRED in library version 400 (reserved: fa_supported() answers 0, fa_fwd FA_ERR_UNSUPPORTED). Rounds 2-3:
                            the paired-block pipeline (256 query rows per workgroup, one wave per SIMD, asm-owned accumulators); the
                            128-row kernels beat it on every shape since they stage by LDS-DMA. Source: tools/experiments/ */
  FA_VARIANT_MFMA_SPLITKV = 6, /* same operator for small grids: one 32-row query block per workgroup, its keys split over
                            2-8 waves and merged in LDS through the row LSE (short sequences / few heads) */
  FA_VARIANT_MFMA_SPLIT2 = 7, /* same operator for grids that fill part of the chip: the 128-row workgroup of MFMA with eight
                            waves, waves 0-3 / 4-7 taking the even / odd KV tiles and merging once (halves the sequential
                            tile count of a block; head_dim 64, 128) */
  FA_VARIANT_MFMA_EXACT = 8, /* FA_VARIANT_MFMA without the pre-scaled query operand: every score is scaled in fp32 (one more
                            FMA per score, 6-8 % slower at head_dim 64). For logits far larger than a trained model
                            produces; see "LSE accuracy" below. Identical to FA_VARIANT_MFMA for fp8 inputs and D = 256 */
  FA_VARIANT_MFMA_H64S2 = 9, /* same operator, 64 query rows per workgroup: four waves, the two wave pairs take the even / odd
                            KV tiles and merge once (twice the workgroups, half the sequential tiles of a block): grids
                            whose critical path is the heaviest causal block (f16 / bf16, head_dim 64) */
  FA_VARIANT_MFMA16 = 10, /* FA_VARIANT_MFMA's workgroup (128 query rows, pre-scaled query operand) with every product on
                            v_mfma_f32_16x16x32 instead of 32x32x16: the chip holds a higher clock on that shape under
                            power-limited loops (f16 / bf16, head_dim 64) */
  FA_VARIANT_MFMA_FP8PV = 11 /* fp8 inputs, head_dim 64 or 128: BOTH products on the scaled fp8 MFMA -- the probabilities are rounded to e4m3
                            for the PV product (FA_VARIANT_MFMA / _EXACT keep them in bf16); see "fp8 probabilities" below */
};

/* status codes (0 = success, negative = error; text via fa_last_error()) */
enum fa_status {
  FA_OK = 0,
  FA_ERR_INVALID_ARG = -1,   /* null pointer, non-positive size, bad enum, misaligned */
  FA_ERR_UNSUPPORTED = -2,   /* (dtype, variant, D) combination has no kernel */
  FA_ERR_LAUNCH = -3,        /* HIP runtime reported an error at launch */
  FA_ERR_NO_DEVICE = -4      /* main.mm:42-45: no device */
};

/*
 * The operator. O[b,h,i,:] = sum_j softmax_j(scale * Q[b,h,i,:].K[b,h,j,:]) V[b,h,j,:]
 * with key j visible to query i iff (!is_causal || j <= i)   (kernels.metal:748);
 * lse[b,h,i] = max_j(scale*s_ij) + ln(sum_j exp(scale*s_ij - max))  (kernels.metal:862-864),
 * natural exp/log. Accumulation is fp32 for every dtype.
 *
 *  q,k,v,o       device pointers; element (b,h,i,d) at b*batch_stride + h*head_stride + i*D + d
 *                (rows contiguous, row pitch D); 16-byte aligned, strides multiples of 8 elements (16 for fp8)
 *  lse           device pointer to B*H*N floats, contiguous [B,H,N]; may be NULL
 *  N             sequence length (queries == keys); any N >= 1
 *  D             head dim: 32, 64, 96, 128 or 256 for FA_VARIANT_MFMA (fp8 inputs: 64, 128, 256); any multiple of 8 up to 128 for
 *                FA_VARIANT_MFMA16 (f16 / bf16: 64 and 128 natively, the others on zero-padded rows of the next larger one -- what
 *                FA_VARIANT_AUTO takes for head dims such as 40, 72, 80, 112; a head must then stay below 2 GiB); 64 or 128 for
 *                FA_VARIANT_MFMA_SPLIT2 / _FP8PV, 64 for _H64S2 / _SPLITKV, <= 128 (multiple of 4) for the scalar variants
 *  scale         softmax scale (> 0); the reference passes 1/sqrt(D) (main.mm:13)
 *  dtype/variant enums above
 *  hip_stream    hipStream_t on the current device, or NULL
 * Inputs are expected to be finite: the matrix-core kernels are compiled without NaN handling (their
 * own -inf mask values never meet anything that could produce one), so NaN/Inf in Q, K or V give
 * unspecified output values (never a fault).
 *
 * LSE accuracy. The reference never checks L_out (main.mm:1083 only feeds it to its backward) and forms its scores in
 * half precision (kernels.metal:709-712). Here every sum is fp32. The kernels with a PRE-SCALED query operand -- FA_VARIANT_MFMA,
 * FA_VARIANT_MFMA_SPLIT2, FA_VARIANT_MFMA_H64S2 and FA_VARIANT_MFMA16 with f16 / bf16 inputs and D <= 128 (what FA_VARIANT_AUTO
 * picks for BASELINE configs 3 and 4, and the 128-row route of fa_fwd_ex) -- multiply the query operand by scale*log2(e) and round
 * it to the input type ONCE per block of query rows, so that the matrix core delivers the exponent of every probability directly
 * (replaces the per-score scale-and-subtract of kernels.metal:763-771): the result is the exact operator applied to a
 * Q' that differs from Q by one rounding per element: at most half an ulp of the input type, which is eps = 2^-9 (bf16) / 2^-12 (f16)
 * relative for an element just below a power of two and up to 2 eps = 2^-8 / 2^-11 just above one, so |Q' - Q| <= 2 eps |Q| holds
 * element-wise; over a row the roundings are independent and |Q' - Q|_2 is typically below eps |Q|_2 (rms 0.6-1.2 eps per element; the bound below uses norms, and the tests hold it as stated). Consequently
 *     |lse - exact| <= 1e-4 + eps * scale * |q_i|_2 * max_j |k_j|_2        (row i),
 * i.e. relative to the score magnitude (measured on BASELINE config 3, U(-1,1) inputs: max 1.0e-3, rms 4e-5 for
 * bf16; 1.3e-4 / 5e-6 for f16), while O keeps the tolerance of the other kernels (max|O - exact| 3.1e-3 vs 2.9e-3
 * without the pre-scaling on config 3). FA_VARIANT_MFMA16 additionally takes its row sums from the matrix core, i.e. it adds the
 * probabilities AFTER their rounding to the input type (the very values the PV product multiplies: O's weights then add up to
 * exactly 1): ln(l) carries that rounding, at most 2^-8 (bf16) / 2^-11 (f16) on top of the bound above and far less on average
 * (measured: 4e-4 at N = 128, below 1e-4 from N = 1024 on, bf16). With f16 inputs FA_VARIANT_MFMA16 rounds a probability with all 11
 * bits while it is at least 2^-11 of the largest one its row had seen when the row's reference was last set (2^-14 of the row sum of the
 * first 64 keys, until a score rises 4 log2 units above them), with one bit less per factor of 2 below that, and drops it below 2^-22
 * (2^-25): n such keys move lse by at most n * 2^-22 (n * 2^-25), all roundings in one direction. Where the scores sit does not
 * matter: the first tile is started over from its true row maxima whenever its probabilities against the assumed maximum of 0 add up
 * to less than 1. With bf16 inputs at D = 64 (and the smaller head dims that run padded on that kernel) FA_VARIANT_MFMA16 renews a
 * row's reference LAZILY: probabilities keep their 8 bits at any scale, the row sums are looked at while the NEXT 64-key tile is
 * multiplied, and a row whose sum has reached 2^20 then takes an exact power of two out of O, its sum and its reference behind that tile --
 * a rise is answered two tiles after it began, and nothing is rounded on the way. The bounds above hold for any scores; what the
 * lag costs is time only: a row that rises more than about 44 log2 units (e^30) within TWO consecutive tiles (its sum going from below
 * 2^20 past 2^64 before the answer) sends its workgroup of 128 or 256 query rows through a second pass on true row maxima. inf / NaN
 * inputs give inf / NaN rows, as everywhere. Every other kernel / dtype (FA_VARIANT_MFMA_EXACT, the split-KV and paired-block kernels, fp8 inputs):
 * |lse - exact| <= 1e-4 for |lse| <= ~10.
 *
 * fp8 probabilities. FA_VARIANT_MFMA_FP8PV (e4m3 inputs, D = 64 or 128; FA_VARIANT_AUTO's choice for grids that fill the chip) runs BOTH
 * products on the fp8 matrix pipe: the probabilities are rounded to e4m3 (3 mantissa bits) on their way into the PV product, as the
 * inputs themselves were. Every softmax weight moves by a factor within 1 +- 2^-4, so
 *     |O - exact| <= 2^-4 * max_j |v_j|     (plus the bf16 rounding of O),
 * reached only by rows with one or two visible keys; the roundings of a row's weights are independent, so rows with many comparable
 * keys see a small fraction of it (measured on BASELINE config 5, U(-1,1) inputs: max 2.3e-2 over the first rows of the causal mask,
 * below the other kernels' 6e-3 on every row with more than 1024 keys). Weights below 2^-13 of the row's reference are flushed to
 * zero (e4m3's range). The row sum comes out of the matrix core as well (a block of ones against the e4m3 probabilities): l adds the
 * ROUNDED weights -- O's weights add up to exactly 1 -- and
 *     |lse - exact| <= ln(1 + 2^-4) < 2^-4,
 * again reached only by rows with two or three comparable keys (measured on config 5: at most 4.1e-3 over rows with more than 64
 * keys, 1e-3 typical). Callers that need the 1e-4 LSE with fp8 inputs name FA_VARIANT_MFMA / FA_VARIANT_MFMA_EXACT, which keep the
 * probabilities in bf16 and add them in fp32 (the score product alone on the fp8 pipe).
 */
int fa_fwd(const void *q, const void *k, const void *v, void *o, float *lse,
           int B, int H, int N, int D, float scale,
           long long batch_stride, long long head_stride,
           int is_causal, int dtype, int variant, void *hip_stream);

/*
 * Generalised forward (scope row f3; not in the reference, whose operator is square and multi-head):
 * grouped-query / multi-query heads and a key length different from the query length.
 *   q, o  [B, Hq, Nq, D] with q_batch_stride / q_head_stride;  k, v  [B, Hkv, Nk, D] with kv strides
 *   query head h attends to key/value head h / (Hq / Hkv)   (Hq % Hkv == 0)
 *   causal is bottom-right aligned: key j is visible to query i iff j <= i + (Nk - Nq); needs Nk >= Nq
 *   lse [B, Hq, Nq]. Matrix-core kernels only (f16 / bf16: D a multiple of 8 up to 128, or 256; fp8 inputs: D = 64, 128, 256).
 *   FA_VARIANT_AUTO here has a rule of its own, which differs from fa_fwd's: the split-KV kernel for at most 64 blocks of 128 query
 *   rows against more than 64 keys (e.g. decode steps; D = 64); else the 16x16x32 kernel (FA_VARIANT_MFMA16) for the f16 / bf16 head
 *   dims up to 128 other than 32, 64, 96 and 128 (zero-padded rows), and for f16 / bf16 on more than 512 blocks of 128 query rows
 *   from Nk = 1024 on (causal: from 1536 at D = 64, from 2048 otherwise); else the 128-row kernel (FA_VARIANT_MFMA).
 * With Hkv = Hq, Nk = Nq and equal strides this is fa_fwd with the variant this rule picks.
 */
int fa_fwd_ex(const void *q, const void *k, const void *v, void *o, float *lse,
              int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale,
              long long q_batch_stride, long long q_head_stride,
              long long kv_batch_stride, long long kv_head_stride,
              int is_causal, int dtype, void *hip_stream);
/* fa_fwd_ex with the kernel named by the caller: FA_VARIANT_AUTO (= fa_fwd_ex), FA_VARIANT_MFMA, FA_VARIANT_MFMA_EXACT (no pre-scaled
 * query operand), FA_VARIANT_MFMA16 (f16 / bf16, D = 64, 128) or FA_VARIANT_MFMA_SPLITKV (D = 64); any other variant: FA_ERR_UNSUPPORTED. */
int fa_fwd_exv(const void *q, const void *k, const void *v, void *o, float *lse,
               int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale,
               long long q_batch_stride, long long q_head_stride,
               long long kv_batch_stride, long long kv_head_stride,
               int is_causal, int dtype, int variant, void *hip_stream);

/*
 * The forward over PACKED variable-length sequences ("varlen"; the prefill of a first prompt, whose K / V are not in a cache yet -- fa_fwd_varlen_paged below reads a paged cache; not in the reference):
 * B sequences lie back to back in q / o [total_q tokens] and k / v [total_k tokens]. Token t, head h, element d of q and o sits at
 * t * q_row_stride + h * q_head_stride + d, of k and v (one stride set for both) at t * kv_row_stride + h * kv_head_stride + d: both
 * [total, H, D] (strides H*D, D) and [H, total, D] (strides D, total*D) work, and so do three views of one packed [total, Hq + 2*Hkv, D]
 * QKV projection (row stride (Hq + 2*Hkv)*D, head stride D). Strides are multiples of 8 elements and at least D, bases 16-byte aligned,
 * the element stride is 1; lse is [Hq, total_q] fp32 contiguous, or NULL. The tensors may exceed 4 GiB: a sequence's base is a 64-bit
 * address, and only (max_seqlen + 128) * row_stride * 2 bytes must stay below 4 GiB, for q and for k / v (loads and stores above 4 GiB
 * and in-sequence offsets of 2 - 4 GiB are run by tests/test_gpu_far_addresses.py, cases A and C).
 * cu_seqlens_q / cu_seqlens_k (int32, [B + 1]) are DEVICE memory read by the kernels -- the host never reads them and the launch
 * geometry depends on the host scalars alone (B * Hq * ceil(max_seqlen_q / 128) workgroups), so one captured graph serves any set of
 * lengths under the same B, total_* and max_seqlen_*. Sequence b owns query tokens cu_seqlens_q[b] .. cu_seqlens_q[b+1) and keys
 * cu_seqlens_k[b] .. cu_seqlens_k[b+1). Every table entry is clamped to [0, total], a non-increasing pair gives length 0, and the
 * lengths Lq_b / Lk_b are clamped to max_seqlen_q / max_seqlen_k: rows of a sequence beyond that clamp and tokens at or past
 * cu_seqlens_q[B] are not written, and a corrupt table touches nothing outside tokens [0, total) of any tensor.
 * Per sequence the operator is exactly fa_fwd_ex on that sequence: query head h reads key/value head h / (Hq / Hkv); causal is
 * bottom-right aligned PER SEQUENCE (key j visible to query i iff j <= i + Lk_b - Lq_b). Unlike fa_fwd_ex, Lk_b < Lq_b and Lk_b = 0 are
 * legal (the host cannot see the lengths): a row with no visible key gets O = 0 exactly and LSE = -inf, as in fa_fwd_decode_paged.
 * f16 / bf16, D = 64 | 128, the pre-scaled query operand of FA_VARIANT_MFMA: anything else FA_ERR_UNSUPPORTED. Tolerances are
 * FA_VARIANT_MFMA's and "LSE accuracy" above applies unchanged; more than that, for every sequence with Lk_b >= Lq_b >= 1 (without the
 * mask: any Lk_b >= 1, Lq_b >= 1) O and LSE are BIT-IDENTICAL to fa_fwd_exv(..., FA_VARIANT_MFMA) run on that sequence alone, whatever
 * the strides, the other sequences or max_seqlen_* are. Null pointers (lse may be NULL), sizes < 1, Hq % Hkv != 0, scale <= 0, bad
 * strides or alignment, max_seqlen_* > total_*, a sequence above the 4 GiB bound or a grid that does not fit an int: FA_ERR_INVALID_ARG
 * before any launch.
 */
int fa_fwd_varlen(const void *q, const void *k, const void *v, void *o, float *lse,
                  const int *cu_seqlens_q, const int *cu_seqlens_k,
                  int B, int Hq, int Hkv, int total_q, int total_k,
                  int max_seqlen_q, int max_seqlen_k, int D, float scale,
                  long long q_row_stride, long long q_head_stride,
                  long long kv_row_stride, long long kv_head_stride,
                  int is_causal, int dtype, void *hip_stream);
int fa_fwd_varlen_supported(int dtype, int D);

/*
 * Few query rows against a long key sequence (decode steps, short chunks; scope row f3, not in the reference): the same operator as
 * fa_fwd_ex for (Hq / Hkv) * Nq <= 32, f16 / bf16 / e4m3, D = 64 | 128, laid out for the HBM roofline instead of the matrix cores -- the query
 * heads of a key/value head are packed into one row block (K and V are read once per key head), the keys are split over several
 * work items per (batch, key head), and the partial results (unnormalised O, m, l per item) meet in `workspace`, caller-owned device
 * memory of fa_fwd_decode_workspace_bytes() bytes, 16-byte aligned, contents irrelevant before and after the call; a second launch
 * on the same stream combines them. Pre-scaled query operand as FA_VARIANT_MFMA ("LSE accuracy" above). Asynchronous, allocates nothing.
 * dtype FA_DTYPE_FP8_E4M3 (an e4m3 KV cache: Q, K, V e4m3 under strides that are multiples of 16, O bf16 as in fa_fwd): half the bytes of
 * the stream; the tiles are widened EXACTLY to bf16 on their way into LDS, so the arithmetic and the tolerances are the bf16 path's (the
 * probabilities stay bf16 here). The workspace size does not depend on the dtype.
 */
int fa_fwd_decode(const void *q, const void *k, const void *v, void *o, float *lse,
                  int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale,
                  long long q_batch_stride, long long q_head_stride,
                  long long kv_batch_stride, long long kv_head_stride,
                  int is_causal, int dtype, void *workspace, long long workspace_bytes, void *hip_stream);
/* The same step on an e4m3 KV cache under 16-bit queries, the usual serving layout: k, v e4m3 (kv strides in elements, multiples of 16),
 * q and o bf16 (q_dtype FA_DTYPE_BF16; FA_DTYPE_FP8_E4M3 makes this fa_fwd_decode with dtype e4m3). K and V are widened exactly to bf16
 * on their way into LDS: the arithmetic and tolerances are those of the bf16 path on the widened cache. Same workspace. */
int fa_fwd_decode_kv8(const void *q, const void *k, const void *v, void *o, float *lse,
                      int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale,
                      long long q_batch_stride, long long q_head_stride,
                      long long kv_batch_stride, long long kv_head_stride,
                      int is_causal, int q_dtype, void *workspace, long long workspace_bytes, void *hip_stream);
long long fa_fwd_decode_workspace_bytes(int B, int Hq, int Hkv, int Nq, int Nk, int D);
int fa_fwd_decode_supported(int dtype, int D, int Hq, int Hkv, int Nq);
/*
 * The same decode step against a PAGED KV cache with a length per sequence (the block-table layout of serving engines; not in the
 * reference). k_pages / v_pages are page pools of num_pages pages of page_size (P) key slots each, sharing one set of element strides:
 * element d of slot r of key head h in page p sits at p * kv_page_stride + h * kv_head_stride + r * kv_row_stride + d. Both usual layouts
 * work: HND [num_pages, Hkv, P, D] (strides Hkv*P*D, P*D, D) and NHD [num_pages, P, Hkv, D] (strides P*Hkv*D, D, Hkv*D); strides are
 * multiples of 8 elements (16 for e4m3), bases 16-byte aligned; the pool may exceed 4 GiB. block_table (int32, [B, block_table_stride],
 * block_table_stride >= max_pages_per_seq) and seqlens_k (int32, [B]) are DEVICE memory read by the kernels -- the host never reads
 * them, so one captured graph serves every step: key j < L_b = seqlens_k[b] of sequence b is slot j % P of page block_table[b][j / P].
 * Lengths are clamped to [0, max_pages_per_seq * P]. q, o, lse as in fa_fwd_decode; causal is bottom-right aligned PER SEQUENCE (key j
 * visible to query i iff j <= i + L_b - Nq). A row with no visible key (L_b = 0, or causal with i + L_b < Nq) gets O = 0 exactly and
 * LSE = -inf. Results depend neither on slots >= L_b of a sequence's last page (NaN there is harmless: they read as zeros), nor on table
 * entries past ceil(L_b / P), nor on the workspace's prior contents, and are bitwise reproducible; a page index outside
 * [0, num_pages) reads as zeros and touches nothing outside the pool. With every L_b at the capacity max_pages_per_seq * P the results
 * are bit-identical to fa_fwd_decode / fa_fwd_decode_kv8 on the gathered dense cache (same key splits, same workspace size).
 * (q_dtype, kv_dtype): (f16, f16), (bf16, bf16), (e4m3, e4m3) and (bf16, e4m3), the last two with bf16 O; D = 64 | 128;
 * (Hq / Hkv) * Nq <= 32; P in {16, 32, 64, 128, 256}: anything else FA_ERR_UNSUPPORTED. Tolerances are those of fa_fwd_decode.
 * Bad pointers, sizes or strides, a short workspace or block_table_stride < max_pages_per_seq: FA_ERR_INVALID_ARG before any launch.
 */
int fa_fwd_decode_paged(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                        const int *block_table, const int *seqlens_k,
                        int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages, int max_pages_per_seq,
                        float scale, long long q_batch_stride, long long q_head_stride,
                        long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                        long long block_table_stride, int is_causal, int q_dtype, int kv_dtype,
                        void *workspace, long long workspace_bytes, void *hip_stream);
/* = fa_fwd_decode_workspace_bytes(B, Hq, Hkv, Nq, page_size * max_pages_per_seq, D): depends on the capacity only (0 if invalid) */
long long fa_fwd_decode_paged_workspace_bytes(int B, int Hq, int Hkv, int Nq, int D, int page_size, int max_pages_per_seq);
int fa_fwd_decode_paged_supported(int q_dtype, int kv_dtype, int D, int Hq, int Hkv, int Nq, int page_size);

/*
 * PACKED queries against a PAGED KV cache (chunked prefill, prefix caching, speculative verification of many tokens; not in the
 * reference): the query side of fa_fwd_varlen over the key side of fa_fwd_decode_paged, in the 128-row kernel.
 * q, o, lse, cu_seqlens_q, total_q, max_seqlen_q and the q strides behave exactly as in fa_fwd_varlen: q and o are packed
 * [total_q, Hq, D] under row / head element strides (multiples of 8, at least D), lse is [Hq, total_q] fp32 or NULL; table entries are
 * clamped to [0, total_q], a non-increasing pair gives length 0, Lq_b is clamped to max_seqlen_q, and tokens owned by nobody (at or
 * past cu_seqlens_q[B], rows of a sequence beyond max_seqlen_q) are not written.
 * k_pages, v_pages, block_table, seqlens_k, page_size (P), num_pages, max_pages_per_seq, the three kv strides and block_table_stride
 * behave exactly as in fa_fwd_decode_paged: HND or NHD pools under one set of strides, L_b = seqlens_k[b] clamped to
 * [0, max_pages_per_seq * P], key j < L_b is slot j % P of page block_table[b][j / P]; a page index outside [0, num_pages) reads as
 * zeros and touches nothing; slots >= L_b of a last page and table entries past ceil(L_b / P) have no influence (NaN there is harmless).
 * The pool may exceed 4 GiB, one page of one head stays below 2 GiB, the capacity is at most 2^30 keys (pools whose used pages lie past
 * ELEMENT offset 2^32, bf16 and e4m3, are run by tests/test_gpu_far_addresses.py, cases D - F).
 * Per sequence the operator is fa_fwd_ex: query head h reads key head h / (Hq / Hkv); causal is bottom-right aligned per sequence (key
 * j visible to query i iff j <= i + L_b - Lq_b), where L_b is the cache length WITH the chunk already appended (fa_kv_append_paged
 * below) -- that makes a causal call a chunked-prefill step. L_b < Lq_b and L_b = 0 are legal: a row with no visible key gets O = 0
 * exactly and LSE = -inf. The host reads neither table nor the lengths; the grid is B * Hq * ceil(max_seqlen_q / 128) workgroups, so
 * one captured graph serves every step under the same scalars. No workspace and no key split; asynchronous, allocates nothing.
 * f16 / bf16 with q and the pool of the same type, D = 64 | 128, P in {16, 32, 64, 128, 256}: anything else FA_ERR_UNSUPPORTED. An
 * e4m3 pool is out of scope here: the 128-row kernel's varlen mode has no widening stage (fa_fwd_varlen_paged_kv8 below and
 * fa_fwd_decode_paged take such pools).
 * Null pointers (lse may be NULL), sizes < 1, Hq % Hkv != 0, scale <= 0, bad strides or alignment, max_seqlen_q > total_q,
 * block_table_stride < max_pages_per_seq, a capacity above 2^30, a page of one head at or above 2 GiB,
 * (max_seqlen_q + 128) * q_row_stride * 2 >= 4 GiB or a grid that does not fit an int: FA_ERR_INVALID_ARG before any launch.
 * Tolerances are FA_VARIANT_MFMA's and "LSE accuracy" above applies; more than that, for every sequence with L_b >= Lq_b >= 1 (without
 * the mask: both >= 1) O and LSE are BIT-IDENTICAL to fa_fwd_varlen on the gathered dense cache of that sequence, whatever the page
 * size, layout, page order, strides or other sequences are. Results are bitwise reproducible.
 */
int fa_fwd_varlen_paged(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                        const int *cu_seqlens_q, const int *block_table, const int *seqlens_k,
                        int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                        int page_size, int num_pages, int max_pages_per_seq, float scale,
                        long long q_row_stride, long long q_head_stride,
                        long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                        long long block_table_stride, int is_causal, int dtype, void *hip_stream);
int fa_fwd_varlen_paged_supported(int dtype, int D, int page_size);
/*
 * Sliding window: fa_fwd_varlen_window, fa_fwd_varlen_paged_window and fa_fwd_decode_paged_window are fa_fwd_varlen,
 * fa_fwd_varlen_paged and fa_fwd_decode_paged with `is_causal` replaced by two ints, window_left (wl) and window_right (wr). With
 * coff = Lk_b - Lq_b (paged: L_b - Lq_b; decode: L_b - Nq), key j is visible to query i of its sequence iff
 *     i + coff - wl <= j <= i + coff + wr   and   0 <= j < Lk_b.
 * A negative value leaves that side unbounded: (-1, -1) is the full operator, (-1, 0) bottom-right causal, (W - 1, 0) a causal window
 * of W keys, (W, W) a symmetric band. Every non-negative int up to INT_MAX is legal: the host replaces an unbounded side, and any
 * width that can never bind (wl above the most keys a sequence of the call can hold -- max_seqlen_k or the capacity --, wr above
 * max_seqlen_q / Nq), by that smallest never-binding width, so the kernels' 32-bit index arithmetic cannot wrap (CLAMPED ON THE HOST;
 * fa_window_key_range itself computes in 64 bits). A row with no visible key (i + coff + wr < 0, or Lk_b = 0) gets O = 0 exactly and
 * LSE = -inf. Everything else -- layouts, strides, tables and their clamping, what is written, every argument rule and its status code,
 * the support tables (fa_fwd_varlen_supported, fa_fwd_varlen_paged_supported, fa_fwd_decode_paged_supported), the decode workspace
 * (fa_fwd_decode_paged_workspace_bytes), tolerances and "LSE accuracy" -- is the un-windowed entry point's.
 * ROUTING IS BY SIGN ONLY: (wl < 0, wr < 0) and (wl < 0, wr == 0) launch the kernels of the un-windowed call without / with the mask
 * and are bit-identical to it; every other pair launches the windowed kernels, however large its values. Through those, (INT_MAX, 0)
 * is bit-identical to the causal call and (INT_MAX, INT_MAX) to the full one on every sequence with Lk_b >= Lq_b >= 1.
 * The 128-row kernels walk the 64-key tiles [lo / 64, ceil(hi / 64)) of each 128-row block, [lo, hi) being fa_window_key_range of the
 * block's rows. The decode divides tiles [t_lo, nT) over its S key splits, t_lo = max(0, L_b - Nq - wl) / 64 and nT =
 * ceil(min(L_b, L_b + wr) / 64): split s takes tiles t_lo + floor(s n / S) .. t_lo + floor((s + 1) n / S), n = nT - t_lo (the
 * un-windowed rule at t_lo = 0). Keys outside [lo, hi) of every block of a sequence are never read.
 */
int fa_fwd_varlen_window(const void *q, const void *k, const void *v, void *o, float *lse,
                         const int *cu_seqlens_q, const int *cu_seqlens_k,
                         int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                         int D, float scale, long long q_row_stride, long long q_head_stride,
                         long long kv_row_stride, long long kv_head_stride,
                         int window_left, int window_right, int dtype, void *hip_stream);
int fa_fwd_varlen_paged_window(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                               const int *cu_seqlens_q, const int *block_table, const int *seqlens_k,
                               int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                               int page_size, int num_pages, int max_pages_per_seq, float scale,
                               long long q_row_stride, long long q_head_stride,
                               long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                               long long block_table_stride, int window_left, int window_right, int dtype, void *hip_stream);
int fa_fwd_decode_paged_window(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                               const int *block_table, const int *seqlens_k,
                               int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages, int max_pages_per_seq,
                               float scale, long long q_batch_stride, long long q_head_stride,
                               long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                               long long block_table_stride, int window_left, int window_right, int q_dtype, int kv_dtype,
                               void *workspace, long long workspace_bytes, void *hip_stream);
/*
 * The half-open key range [*key_lo, *key_hi) that rows row_first .. row_last (clamped to 0 .. Lq - 1) of a sequence of Lq queries and Lk
 * keys see together under (window_left, window_right); empty iff *key_lo >= *key_hi. Host only, no device needed; any int is a legal
 * window or row (64-bit arithmetic). FA_OK, or FA_ERR_INVALID_ARG for a null pointer or a negative length. The kernels take their
 * first and last tile from the same inline function (csrc/fa_common.h, window_key_range).
 */
int fa_window_key_range(int Lq, int Lk, int window_left, int window_right, int row_first, int row_last, int *key_lo, int *key_hi);
/*
 * Write new K / V rows into the page pools ("append"; the step in front of fa_fwd_varlen_paged or fa_fwd_decode_paged): k_new / v_new
 * are packed [total_new, Hkv, D] views under one (row, head) stride pair; sequence b owns tokens cu_seqlens_new[b] ..
 * cu_seqlens_new[b+1) (entries clamped to [0, total_new], a non-increasing pair is length 0, n_b clamped to max_seqlen_new). Token i
 * of sequence b goes to key position seqlens_k[b] - n_b + i of that sequence: seqlens_k is the length AFTER the append, the same table
 * the attention call then reads. A position below 0, at or above the capacity max_pages_per_seq * P, or on a table entry outside
 * [0, num_pages) is skipped; nothing else in the pools is written -- no other slot, and no bytes between heads or rows under wide
 * strides. A pure byte copy: f16 / bf16 / e4m3 (element size fa_dtype_in_bytes(dtype)), D * bytes a multiple of 16, strides multiples
 * of 8 elements (16 for e4m3) and at least D, bases 16-byte aligned, P in {16, 32, 64, 128, 256}. The tables are DEVICE memory; the grid
 * (B * ceil(max_seqlen_new / 16) x Hkv workgroups) depends on host scalars only: asynchronous, allocates nothing, graph-capturable.
 * Bad pointers, sizes, strides or alignment, max_seqlen_new > total_new, block_table_stride < max_pages_per_seq, a capacity above
 * 2^30, a page of one head at or above 2 GiB, Hkv > 65535 or a grid that does not fit an int: FA_ERR_INVALID_ARG before any launch.
 */
int fa_kv_append_paged(const void *k_new, const void *v_new, void *k_pages, void *v_pages,
                       const int *cu_seqlens_new, const int *block_table, const int *seqlens_k,
                       int B, int Hkv, int total_new, int max_seqlen_new, int D,
                       int page_size, int num_pages, int max_pages_per_seq,
                       long long new_row_stride, long long new_head_stride,
                       long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                       long long block_table_stride, int dtype, void *hip_stream);

/*
 * Backward of the operator (row f1 of the scope table): the reference binds it as
 * flash_attention_backward_kernel, /root/reference/kernels.metal:905-921, host side
 * /root/reference/main.mm:1015-1058:
 *   buffer 0-5  Q,K,V,O,dO (16-bit), L (fp32 [B,H,N], the forward's lse)   -> q,k,v,o,d_o,lse
 *   buffer 6-8  dQ,dK,dV  fp32 (the reference accumulates into them with atomics and the host
 *               zero-fills them first, main.mm:1018-1021)                  -> dq,dk,dv
 *   bytes 9-14  N, D, scale, batch_stride, head_stride, is_causal          -> same names
 * Here dq/dk/dv are WRITTEN (no zero-fill needed, no atomics, bitwise reproducible), laid out
 * like the inputs (element (b,h,i,d) at b*batch_stride + h*head_stride + i*D + d, fp32).
 * `workspace` is caller-owned scratch of fa_bwd_workspace_bytes(B,H,N) bytes (device memory).
 * dtype F16 or BF16 (FP8_E4M3: see fa_bwd_workspace_bytes_ex); D = 64 (the reference's, kernels.metal:905-1265) or 128 natively, any other multiple of 8 up to 128 (32, 96, ...)
 * through the next larger kernel on zero-padded rows (same results per real column; a head must then stay below 2 GiB). D = 256: its own
 * instantiation (one workgroup per CU, f16 / bf16 only).
 *
 * Backward accuracy. Sums are fp32; what is rounded to the 16-bit input type (unit roundoff u = 2^-8 bf16 / 2^-11 f16: half an ulp
 * is up to u relative just above a power of two) is the operand pre-scaled by scale*log2(e) (Q in the dQ kernel, K in the dK/dV
 * kernel: score (i,j) moves by at most d_ij = u * scale * sum_d |q_id k_jd|), and P and dS = P o (dP - delta) on their way into the
 * second products; delta is formed from the O the caller passes. Element by element, with the exact P and dS,
 *     |dQ_id - exact| <= scale * sum_j E_ij |k_jd|,   |dK_jd - exact| <= scale * sum_i E_ij |q_id|,
 *     |dV_jd - exact| <= sum_i (P_ij (u + expm1(d_ij)) + t) |dO_id|,
 *     E_ij = |dS_ij| (u + expm1(d_ij)) + P_ij exp(d_ij) (u sum_d |dO_id O_id| + fp32 terms) + t
 * (plus 2^-24 * N relative for the fp32 sums; over the query heads of a group the bounds add; tests/backward_bound.py spells out
 * every term, tests/test_gpu_backward_rows.py holds every element of the three gradients to it: measured worst error / bound 0.87).
 * That is about 2-5e-2 (bf16) / 3-6e-3 (f16) of a row's own largest gradient. t = 2^-25 for f16 and 0 for bf16: f16 values below
 * 2^-14 are subnormal and rounded absolutely, to a multiple of 2^-24. They are KEPT -- the conversions and the matrix cores honour
 * subnormal f16 operands, nothing is flushed to zero -- so a d_o of order 2^-8 and less (f16 training without loss scaling), where
 * every dS is subnormal, still gives dQ / dK within the bound above (test_rows_small_d_o), at the absolute resolution 2^-25 per
 * (query, key) pair instead of 11 bits; below about 2^-24 / P_ij a dS is rounded to zero, as f16 itself would. e4m3 inputs: u = 2^-8.
 * On the forward's own O and LSE -- what training and torch.ops.fa_mi355 feed it -- the bound above reads "the exact O rounded to the
 * type, the exact LSE" as two substitutions. With lse_err_i >= |lse_i - exact| and o_err_id >= |O_id - exact| of the forward route that
 * wrote them: d_ij becomes d_ij + lse_err_i (every P of row i moves by exp(-+lse_err_i)), and u sum_d |dO_id O_id| becomes
 * sum_d |dO_id| o_err_id (delta moves by sum_d dO_id (O_id - exact)). The forward terms, per route ("LSE accuracy" / "fp8 probabilities"
 * above): lse_err_i = 1e-4, + eps * scale * |q_i|_2 * max_j |k_j|_2 for the pre-scaled kernels, + 2^-8 (bf16) / 2^-11 (f16) for
 * FA_VARIANT_MFMA16 (+ n * 2^-22 for n low probabilities of an f16 row), + ln(1 + 2^-4) for FA_VARIANT_MFMA_FP8PV;
 *     o_err_id = u_out |O_id| + (u_p + u_l + expm1(2 max_j d_ij) + 2^-24 (visible keys + tiles)) * sum_j P_ij |v_jd|
 * with u_p the rounding of a probability into the PV product (u; 2^-4 for FA_VARIANT_MFMA_FP8PV), u_l = u_p where the row sum adds the
 * rounded probabilities (FA_VARIANT_MFMA16, _FP8PV) and 0 otherwise, the d_ij term for the pre-scaled kernels only, and
 * 2 (S + 3) 2^-24 sum_j P_ij |v_jd| more where S key splits are merged. Judged as a function of the six tensors it is handed, whatever
 * wrote them, the backward is within the bound above with P^_ij = exp(scale s_ij - lse_i) and dS^ = P^ o (dP - sum_d dO o) for P and dS
 * and without the u sum_d |dO_id O_id| term. tests/chain_bound.py spells out the forward terms, tests/test_chain_bound_model.py checks
 * them on a model of the kernels' arithmetic, tests/test_gpu_chain.py holds every element of dQ, dK, dV to both bounds on the chains
 * fa_fwd -> fa_bwd, fa_fwd_exv -> fa_bwd_ex, the torch op under autograd and e4m3 inputs.
 */
int fa_bwd(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
           float *dq, float *dk, float *dv, void *workspace,
           int B, int H, int N, int D, float scale,
           long long batch_stride, long long head_stride,
           int is_causal, int dtype, void *hip_stream);
/* Generalised backward, the counterpart of fa_fwd_ex (scope row f3 applied to f1; the reference's operator is square and has one
 * head count, kernels.metal:906-920): q, o, d_o, dq are [B,Hq,Nq,D] under the q strides, k, v, dk, dv are [B,Hkv,Nk,D] under the
 * kv strides, Hq % Hkv == 0, query head h reads key/value head h / (Hq / Hkv); causal is bottom-right aligned (key j visible to
 * query i iff j <= i + Nk - Nq; needs Nk >= Nq) exactly as in fa_fwd_ex. dK / dV of a key head are the sums over its Hq / Hkv
 * query heads, formed in registers by the one workgroup that owns the key block (no atomics, bitwise reproducible). lse is
 * [B,Hq,Nq]; workspace is fa_bwd_workspace_bytes(B,Hq,Nq). With Hkv = Hq, Nk = Nq and equal strides this is exactly fa_bwd. */
int fa_bwd_ex(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
              float *dq, float *dk, float *dv, void *workspace,
              int B, int Hq, int Hkv, int Nq, int Nk, int D, float scale,
              long long q_batch_stride, long long q_head_stride, long long kv_batch_stride, long long kv_head_stride,
              int is_causal, int dtype, void *hip_stream);
long long fa_bwd_workspace_bytes(int B, int H, int N);
/* the same for any dtype and for fa_bwd_ex's shapes (fa_bwd: Hq = Hkv, Nq = Nk, one stride pair). dtype FA_DTYPE_FP8_E4M3 (Q, K, V
 * e4m3 under their element strides, multiples of 16; O and d_o bf16 -- what fa_fwd writes for e4m3 inputs -- under the same element
 * strides; D a multiple of 16): the backward first widens Q, K, V to bf16 -- exactly -- into this workspace, which is why it grows by two
 * bytes per element of their extents, and then runs the bf16 kernels. For f16 / bf16 it returns fa_bwd_workspace_bytes(B,Hq,Nq) rounded up. */
long long fa_bwd_workspace_bytes_ex(int dtype, int B, int Hq, int Hkv, int Nq, int Nk, int D, long long q_batch_stride,
                                    long long q_head_stride, long long kv_batch_stride, long long kv_head_stride);
int fa_bwd_supported(int dtype, int D);
/* algorithmic FLOPs of one fa_bwd call: 2.5x the forward (five N x N x D products) */
double fa_bwd_algorithmic_flops(int B, int H, int N, int D, int is_causal);

/*
 * The backward over PACKED variable-length sequences: the counterpart of fa_fwd_varlen, per sequence exactly fa_bwd_ex (not in the
 * reference). Layout, tables and clamping are fa_fwd_varlen's: q, o, d_o (16-bit) and dq (fp32) share the q ELEMENT strides -- token t,
 * head h, element d at t * q_row_stride + h * q_head_stride + d --, k, v (16-bit) and dk, dv (fp32) the kv element strides, so the
 * fp32 gradient of three views of one packed [total, Hq + 2*Hkv, D] QKV projection is three views of one fp32 buffer of that shape.
 * lse is the forward's [Hq, total_q] fp32. Strides are multiples of 8 elements and at least D, bases 16-byte aligned. The tensors may
 * exceed 4 GiB (gradients are stored through 64-bit addresses); only (max_seqlen + 128) * row_stride * 2 bytes must stay below 4 GiB,
 * for q and for k / v (fp32 stores past byte 2^33 are run by tests/test_gpu_far_addresses.py, cases B and C). `workspace`: caller-owned device memory of fa_bwd_varlen_workspace_bytes(Hq, total_q) bytes (delta, [Hq, total_q]
 * fp32; 0 for invalid sizes), contents irrelevant before the call. The size cannot be seen from the pointer: the caller answers for it.
 * cu_seqlens_q / cu_seqlens_k (int32, [B + 1]) are DEVICE memory read by the kernels -- the host never reads them; the grids are
 * B * Hq * ceil(max_seqlen_q / 128) workgroups for dQ and B * Hkv * ceil(max_seqlen_k / 128) for dK / dV, so one captured graph serves
 * any set of lengths under the same scalars. Table entries and lengths are clamped exactly as in fa_fwd_varlen, and a corrupt table
 * touches nothing outside tokens [0, total) of any tensor.
 * What is written: the dQ row of every query token owned by a sequence and the dK and dV rows of every key token owned by a sequence
 * (zeros when no query sees the key, e.g. Lq_b = 0). Tokens owned by nobody -- at or past cu_seqlens[B], or beyond the max_seqlen clamp
 * of their sequence -- are not written, and neither are bytes between heads or rows under wide strides.
 * A query row without a visible key (Lk_b = 0, or causal with i + Lk_b - Lq_b < 0; the forward gave it O = 0 and LSE = -inf) gets
 * dQ = 0 exactly and contributes exactly nothing to dK / dV; it is recognised by the forward's integer test, never by its LSE.
 * Results do not depend on the workspace's prior contents and are bitwise reproducible. For every sequence with Lk_b >= Lq_b >= 1
 * (without the mask: any Lq_b, Lk_b >= 1) dQ, dK, dV are BIT-IDENTICAL to fa_bwd_ex run on that sequence alone, whatever the strides,
 * the other sequences or max_seqlen_* are; "Backward accuracy" above applies per sequence.
 * f16 / bf16, D = 64 | 128: anything else FA_ERR_UNSUPPORTED. Null pointers, sizes < 1, Hq % Hkv != 0, scale <= 0, bad strides or
 * alignment, max_seqlen_* > total_*, a sequence above the 4 GiB bound or a grid that does not fit an int: FA_ERR_INVALID_ARG before any
 * launch.
 */
int fa_bwd_varlen(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                  float *dq, float *dk, float *dv, void *workspace,
                  const int *cu_seqlens_q, const int *cu_seqlens_k,
                  int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                  long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                  int is_causal, int dtype, void *hip_stream);
long long fa_bwd_varlen_workspace_bytes(int Hq, int total_q);
int fa_bwd_varlen_supported(int dtype, int D);

/*
 * The backward of fa_fwd_varlen_window: fa_bwd_varlen with is_causal replaced by (window_left, window_right); the visibility rule is that
 * of "Sliding window" above (key j visible to query i iff i + coff - window_left <= j <= i + coff + window_right and 0 <= j < Lk_b,
 * coff = Lk_b - Lq_b, a negative side unbounded). Every argument rule, status and the workspace (fa_bwd_varlen_workspace_bytes,
 * fa_bwd_varlen_supported) are fa_bwd_varlen's. Routing is by sign only: (< 0, < 0) and (< 0, 0) launch fa_bwd_varlen's kernels without
 * and with the mask and are bit-identical to it; every other pair launches the windowed kernels, an unbounded or oversized side clamped
 * to max_seqlen_k (left) / max_seqlen_q (right), which can never bind.
 * What is written: as fa_bwd_varlen -- the dQ row of every owned query token and the dK and dV rows of every owned key token; a key no
 * query sees gets dK = dV = 0. Dead rows: a query row without a visible key (Lk_b = 0 or i + coff + window_right < 0, the forward's
 * integer test; O = 0 and LSE = -inf there) gets dQ = 0 exactly and contributes exactly nothing to dK / dV; its delta is still written.
 * Through the windowed kernels (INT_MAX, 0) is bit-identical to the causal call and (INT_MAX, INT_MAX) to the full call on every
 * sequence with Lk_b >= Lq_b >= 1. "Backward accuracy" above applies per sequence under the window's visibility.
 * Inputs must be finite: the mask discards a hidden score, not its operands -- a NaN in a key that no query sees still reaches that
 * key's own dK / dV.
 * The dQ kernel walks the key tiles [lo / 64, ceil(hi / 64)) of fa_window_key_range of each 128-row block; the dK/dV kernel the query
 * tiles [lo / 64, ceil(hi / 64)) of fa_window_query_range of each 128-key block, for every query head of the group.
 */
int fa_bwd_varlen_window(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                         float *dq, float *dk, float *dv, void *workspace,
                         const int *cu_seqlens_q, const int *cu_seqlens_k,
                         int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                         long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                         int window_left, int window_right, int dtype, void *hip_stream);
/* The inverse of fa_window_key_range (host only, any int is legal, 64-bit arithmetic): the half-open range [*row_lo, *row_hi) of the
 * query rows that see at least one of the keys key_first .. key_last (clamped to the sequence's keys); empty iff *row_lo >= *row_hi.
 * FA_ERR_INVALID_ARG for a null pointer or a negative length. */
int fa_window_query_range(int Lq, int Lk, int window_left, int window_right, int key_first, int key_last, int *row_lo, int *row_hi);

/*
 * Attention sinks: fa_fwd_varlen_sink, fa_fwd_varlen_paged_sink, fa_fwd_decode_paged_sink and fa_bwd_varlen_sink are the four *_window
 * entry points with one learnt logit per QUERY head in every softmax (the layers of models that alternate sliding-window and full causal
 * attention): a term in the denominator that carries no value,
 *     P_ij  = exp(scale s_ij) / (sum_{j' visible} exp(scale s_ij') + exp(sinks[h]))
 *     O_i   = sum_j P_ij v_j
 *     LSE_i = ln(sum_{j visible} exp(scale s_ij) + exp(sinks[h])).
 * `sinks` is a DEVICE pointer to Hq fp32 values, read by the kernels only (the host never reads them: the calls stay graph-capturable and
 * the values may change between replays). Units are natural-log logits: the softmax scale is NOT applied to them. They must be finite.
 * Visibility is the rule of "Sliding window" above under (window_left, window_right), unchanged. A row with no visible key (that section's
 * integer test) has the sink alone in its softmax: O = 0 exactly and LSE = sinks[h], the fp32 value bit for bit -- not -inf.
 * Each forward takes the matching *_window signature with `const float *sinks` added behind the window, and shares that call's validation,
 * status codes, error texts, support tables and decode workspace; sinks == NULL (or not fp32-aligned) is FA_ERR_INVALID_ARG.
 * ROUTING: the three forwards ALWAYS run the window-mode kernels, in their sink mode -- (-1, 0) with sinks is the causal layer, (127, 0) the
 * windowed one, (-1, -1) the full one, through one kernel family (eight 128-row kernels; the decode reuses the windowed partial kernels and
 * folds the sink in its combine step). An unbounded or oversized side is clamped on the host to the never-binding width, as in
 * "Sliding window". Never-binding bounds were measured at 0.2-6 % over the un-windowed kernels (README, round 14; round 18: 0.9-5.2 %, in one
 * session 10 % on the paged head_dim-64 prefill); that price is accepted here instead of sixteen more kernels.
 * The sink enters once per row, where the row is normalised; the tile loops do not know of it. With the row's reference m and sum l
 * (log2 units, as the kernels keep them) and s2 = sinks[h] * log2(e):
 *     mm = max(m, s2),   l' = l * 2^(m - mm) + 2^(s2 - mm),   O = acc * 2^(m - mm) / l',   LSE = (mm + log2 l') * ln 2.
 * Neither exponent is positive, so the merge overflows in neither direction: a sink far above every score gives finite, tiny O and
 * LSE ~ sink; a sink whose 2^(s2 - m) underflows to 0 in fp32 (e.g. sinks[h] = -1e4) leaves mm = m, a factor of exactly 1
 * and l' = l + 0: O and LSE are then BIT-IDENTICAL to the *_window call. The paged prefill with sinks is bit-identical to the packed call
 * with sinks on every sequence with L_b >= Lq_b >= 1, as without.
 * Accuracy. By the identity O' = O * exp(lse - lse'), lse' = ln(exp(lse) + exp(sink)), with (O, lse) the results without the sink:
 * d lse' / d lse = exp(lse - lse') <= 1, so the route's own LSE error ("LSE accuracy") enters with a weight of at most 1, and the fold
 * costs a handful of fp32 roundings -- sinks[h] * log2(e) (felt through the sink's share 1 - exp(lse - lse') of the sum), the two exp2, the
 * sum, log and the product by ln 2:
 *     |LSE' - exact| <= lse_tol + 2^-22 * ((1 - exp(lse - lse')) * |sinks[h]| + |lse'| + 4) =: lse_tol'
 *     |O'_d - exact| <= o_tol + |O'_d| * lse_tol'
 * (the factor exp(lse - lse') on O carries the error of both logarithms; o_tol itself shrinks with it and is kept as it is).
 *
 * fa_bwd_varlen_sink: fa_bwd_varlen_window plus `const float *sinks, float *dsinks`. lse is the forward's, which contains the sink, so
 * P = exp(scale s - lse) and delta = rowsum(dO o O) are exactly what the dQ and dK/dV kernels compute already: they run UNCHANGED, routed by
 * sign as in fa_bwd_varlen_window, and dQ, dK, dV are BIT-IDENTICAL to fa_bwd_varlen_window on the same six tensors. "Backward accuracy"
 * applies with the sink-including LSE and lse_tol' / the O bound above as its forward terms. dsinks is [Hq] fp32, WRITTEN, not accumulated;
 * it may be NULL, then the reduction is skipped. One more launch on the same stream, behind the pair:
 *     dsinks[h] = - sum_i exp(sinks[h] - lse[h, i]) * delta[h, i]
 * over the query tokens i a sequence OWNS (cu_seqlens_q walked with the dQ kernel's clamps; tokens owned by nobody and rows past the
 * max_seqlen_q clamp hold stale workspace and are never read). One workgroup per head, thread t adds rows t, t + 1024, ... of every
 * sequence in order, then a fixed binary tree: no atomics, bitwise reproducible; the grid is Hq, host scalars only. A dead row adds
 * exp(0) * 0 = 0. Against the fp64 formula on the lse and delta it was given, with x_i = sinks[h] - lse_i, t_i = exp(x_i) delta_i and
 * c = sum_b ceil(Lq_b / 1024) + 10 additions on the longest path:
 *     |dsinks[h] - exact| <= 2^-24 * sum_i |t_i| * (|x_i| + 3 + c)
 * (the subtraction moves exp by a factor within 2^-24 |x_i|, expf and the product add 2.5 ulp, the sum c per term). Against the true
 * gradient the chain adds sum_i p_i exp(lse_err_i) (|delta_i| lse_err_i + delta_err_i), delta_err_i = sum_d |dO_id| o_err_id (p moves by a
 * factor within exp(+-lse_err), delta by delta_err). tests/sink.py spells the bars out, tests/test_sink_cases.py holds an fp32 model of the
 * epilogues and of the reduction to them, tests/test_gpu_sink.py and test_gpu_sink_bwd.py the kernels.
 */
int fa_fwd_varlen_sink(const void *q, const void *k, const void *v, void *o, float *lse,
                       const int *cu_seqlens_q, const int *cu_seqlens_k,
                       int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                       int D, float scale, long long q_row_stride, long long q_head_stride,
                       long long kv_row_stride, long long kv_head_stride,
                       int window_left, int window_right, const float *sinks, int dtype, void *hip_stream);
int fa_fwd_varlen_paged_sink(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                             const int *cu_seqlens_q, const int *block_table, const int *seqlens_k,
                             int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                             int page_size, int num_pages, int max_pages_per_seq, float scale,
                             long long q_row_stride, long long q_head_stride,
                             long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                             long long block_table_stride, int window_left, int window_right, const float *sinks, int dtype,
                             void *hip_stream);
int fa_fwd_decode_paged_sink(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                             const int *block_table, const int *seqlens_k,
                             int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages, int max_pages_per_seq,
                             float scale, long long q_batch_stride, long long q_head_stride,
                             long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                             long long block_table_stride, int window_left, int window_right, const float *sinks,
                             int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes, void *hip_stream);
int fa_bwd_varlen_sink(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                       float *dq, float *dk, float *dv, void *workspace,
                       const int *cu_seqlens_q, const int *cu_seqlens_k,
                       int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                       long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                       int window_left, int window_right, const float *sinks, float *dsinks, int dtype, void *hip_stream);

/*
 * e4m3 pools in the prefill: fa_fwd_varlen_paged_kv8 is fa_fwd_varlen_paged_sink with `int dtype` replaced by `int q_dtype, int kv_dtype`,
 * for bf16 queries on page pools of OCP e4m3 (e4m3fn) bytes -- the serving layout fa_fwd_decode_paged takes at decode time, here for chunked
 * prefill, a prompt behind a cached prefix and the verification of many speculated tokens. fa_fwd_varlen_paged_kv8_supported answers 1
 * for (FA_DTYPE_BF16, FA_DTYPE_FP8_E4M3), D = 64 | 128, P in {16, 32, 64, 128, 256} and 0 for everything else -- (f16, e4m3) and (e4m3,
 * e4m3) included --, and the call answers FA_ERR_UNSUPPORTED there. fa_fwd_varlen_paged_supported(FA_DTYPE_FP8_E4M3, ...) stays 0 and the
 * fa_fwd_varlen_paged* calls are untouched.
 * q and o are bf16 under the q strides and lse is [Hq, total_q] fp32 or NULL, as in fa_fwd_varlen_paged; k_pages / v_pages are e4m3, HND or
 * NHD; the three kv strides count ELEMENTS (= bytes), are multiples of 16 and at least D (fa_fwd_decode_paged's rule for e4m3 pools); a
 * page of one head stays below 2 GiB, counted in bytes of 1. `sinks` may be NULL: NULL runs without a sink term, non-NULL has the
 * semantics of "Attention sinks". (window_left, window_right) follows "Sliding window": (-1, 0) is causal, (-1, -1) full. ROUTING is not by
 * sign: as the sink forwards do, the call always runs ONE kernel family (the paged window / sink kernels in their KV8 mode, four kernels),
 * with never-binding bounds clamped on the host. Validation is fa_fwd_varlen_paged_sink's path: every rule the two calls share carries the
 * same status and the same error text; only the dtype pair and the 16-element stride rule differ.
 * NO SCALES, as in fa_fwd_decode_kv8: the bytes are read as plain e4m3 values. A caller with a per-tensor K scale folds it into `scale`,
 * and a V scale into whatever consumes O (fa_kv_append_paged_quant's k_mul / v_mul are their reciprocals).
 * The result is the bf16 call on the exactly widened pool: for every owned query token O and LSE are BIT-IDENTICAL to the bf16 call on a
 * bf16 pool that holds the same values widened (same page order and strides in elements, the same slots unused, the same entries out of
 * range) -- with sinks == NULL fa_fwd_varlen_paged_window routed through the window kernels ((INT_MAX, 0) / (INT_MAX, INT_MAX) where
 * the sign routing would pick the un-windowed ones), with sinks fa_fwd_varlen_paged_sink. The kernels load e4m3 chunks into registers
 * through per-page range-checked descriptors, widen them exactly and write the bf16 LDS images of the bf16 kernels; everything from LDS
 * onwards is the same code. Tolerances, "LSE accuracy", dead rows (O = 0; LSE = -inf, or sinks[h] bit for bit), the clamping of the tables
 * and graph capturability are inherited unchanged. Slots >= L_b, spare pages and table entries outside [0, num_pages) read as zeros and
 * touch nothing: the e4m3 NaN bytes 0x7F / 0xFF there are harmless.
 */
int fa_fwd_varlen_paged_kv8(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                            const int *cu_seqlens_q, const int *block_table, const int *seqlens_k,
                            int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                            int page_size, int num_pages, int max_pages_per_seq, float scale,
                            long long q_row_stride, long long q_head_stride,
                            long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                            long long block_table_stride, int window_left, int window_right, const float *sinks,
                            int q_dtype, int kv_dtype, void *hip_stream);
int fa_fwd_varlen_paged_kv8_supported(int q_dtype, int kv_dtype, int D, int page_size);
/*
 * The quantising append: fa_kv_append_paged's argument list with `int dtype` replaced by `int new_dtype` (FA_DTYPE_F16 | FA_DTYPE_BF16, the
 * type of k_new / v_new; the pools are e4m3) and two host scalars k_mul, v_mul (> 0 and finite, else FA_ERR_INVALID_ARG). Every element
 * is stored as the byte
 *     e4m3_rne(clamp(fp32(x) * mul, -448, 448))
 * -- ONE fp32 multiply; the clamp FIRST (the hardware conversion gives NaN above 448 instead of saturating); round to nearest even,
 * subnormals included; -0 keeps its sign; inputs must be finite. Placement, skipping, clamping, footprint and grid are
 * fa_kv_append_paged's, word for word: token i goes to seqlens_k[b] - n_b + i, positions out of capacity or on bad table entries are
 * skipped, nothing else in the pools is written. New-row strides are multiples of 8 elements, pool strides multiples of 16, D a multiple
 * of 16; every other rule, status and text is fa_kv_append_paged's. No scales are stored: a caller that quantises with k_mul = 1 / s_k
 * passes scale * s_k to the attention calls.
 */
int fa_kv_append_paged_quant(const void *k_new, const void *v_new, void *k_pages, void *v_pages,
                             const int *cu_seqlens_new, const int *block_table, const int *seqlens_k,
                             int B, int Hkv, int total_new, int max_seqlen_new, int D,
                             int page_size, int num_pages, int max_pages_per_seq,
                             long long new_row_stride, long long new_head_stride,
                             long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                             long long block_table_stride, int new_dtype, float k_mul, float v_mul, void *hip_stream);

/*
 * Key split in the paged prefill: fa_fwd_varlen_paged_split is fa_fwd_varlen_paged_sink with `int num_splits, void *workspace, long long
 * workspace_bytes` added behind `int dtype`, for calls whose B * Hq * ceil(max_seqlen_q / 128) blocks of 128 rows cannot fill the chip: a
 * chunk of a few hundred queries, or the verification of a few speculated tokens, on one or a few long sequences. The keys of every
 * 128-row block are dealt to S workgroups, which leave per-row partial states in the caller's workspace, and a second launch on the same
 * stream combines them. Semantics are fa_fwd_varlen_paged_sink's: layouts, strides, tables and their clamping, owned tokens, the window
 * rule, dead rows, f16 / bf16 with q and the pools of one type, D = 64 | 128, P in {16 .. 256}; fa_fwd_varlen_paged_supported applies as
 * it stands. `sinks` may be NULL, as in fa_fwd_varlen_paged_kv8: then there is no sink term and a dead row gets LSE = -inf. Validation is
 * the one paged-prefill path: every rule the call shares with fa_fwd_varlen_paged_sink carries the same status and the same error text.
 * num_splits: 0 .. FA_VARLEN_PAGED_MAX_SPLITS, else FA_ERR_INVALID_ARG; 0 stands for what fa_fwd_varlen_paged_num_splits answers for the
 * call's scalars. With S >= 2 splits `workspace` must be non-NULL, 16-byte aligned device memory of at least
 * fa_fwd_varlen_paged_split_workspace_bytes(..., S) bytes, else FA_ERR_INVALID_ARG; what it holds before and after the call is irrelevant.
 * S = 1: the call launches the kernel of the window family it would have launched without the split (the paged window kernel, or the
 * paged sink kernel when sinks != NULL; never-binding bounds clamped on the host as in the sink calls) and nothing else; the workspace may
 * be NULL; the result is that call's, bit for bit.
 * THE SPLIT RULE (per block, as fa_fwd_decode's is per call): a block's tile range is what the window kernel walks, tiles [tb, nT) of 64
 * keys from fa_window_key_range of the block's rows, n = nT - tb. Split s of S takes tiles
 *     tb + floor(s * n / S) .. tb + floor((s + 1) * n / S) - 1
 * so every causal block balances its own length, the capacity plays no part, and a split is empty when n < S.
 * What a split leaves per owned row, normalised: o_s = acc / l in fp32 (formed as the un-split epilogue forms it before rounding to the
 * type: acc * (1 / l), the fp32 product for bf16; for f16, whose epilogue rounds the exact product to f16 once, that product rounded to
 * odd in fp32, so that one rounding to f16 in the combine lands on the same bits) and lse2_s = m + log2 l in log2 units; -inf for an empty split and for a row without a visible key in the split. The combine
 * runs on the partial kernel's own (sequence, head, 128-row block) map with the same cu_seqlens_q lookup and clamps, per row
 *     M = max_s lse2_s;  w_s = 2^(lse2_s - M);  W = sum_s w_s;  O = (sum_s w_s o_s) / W;  LSE = (M + log2 W) ln 2
 * over s in order: no atomics, bitwise reproducible. A split with lse2_s = -inf is skipped, never multiplied. M = -inf: O = 0 exactly and
 * LSE = -inf. A sink is folded once, behind the reduction, with fa_fwd_decode_paged_sink's overflow-safe merge: a dead row gets LSE =
 * sinks[h] bit for bit, a sink whose term underflows leaves the bits of the call with sinks == NULL.
 * Without sinks, O of every row of a block with n = 1 is BIT-IDENTICAL to the S = 1 call under any S >= 2: the one non-empty split weighs
 * exactly 1, W = 1, and O is rounded to the type once. (Its LSE is (m + log2 l) ln 2 where the un-split kernel forms m ln 2 + ln l: equal
 * within the roundings below, not bit for bit.)
 * Accuracy: the un-split call's bounds ("LSE accuracy"; with sinks lse_tol' / the O bound of "Attention sinks") plus the merge term of
 * merged key splits, 2 (S + 3) 2^-24 sum_j P_ij |v_jd| on O -- and, because a split's state is ONE fp32 number
 * lse2_s whose resolution is that of its magnitude, 6 2^-24 |LSE| sum_j P_ij |v_jd| more (nothing at |LSE| of a few units) --, and on LSE 2^-22 (2 |LSE| + S + 6) (the splits' own log2 and sum, the differences,
 * the exponentials and W's S additions, log2 W, the sum and the product by ln 2). tests/ksplit.py spells both out.
 * Graph capture: the host reads no device memory and both grids depend on host scalars only (the block map x S, then the block map).
 * fa_fwd_varlen_paged_num_splits (host only): with blocks = B * Hq * ceil(max_seqlen_q / 128) and slots = 512 (256 CUs x 2, at both head dims: measured) the
 * smallest S with blocks * S >= slots, capped so that a split of a block spanning the capacity max_pages_per_seq * page_size keeps at
 * least 4 tiles, capped by FA_VARLEN_PAGED_MAX_SPLITS, at least 1; 0 for invalid arguments. The workspace holds S * Hq * total_q * (D + 1)
 * floats, rounded up to 16 bytes; the size function resolves num_splits = 0 like the call and answers 0 for invalid sizes and for S = 1.
 * Not offered with softcap, on e4m3 pools, or on the packed and dense calls.
 */
#define FA_VARLEN_PAGED_MAX_SPLITS 64
int fa_fwd_varlen_paged_split(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                              const int *cu_seqlens_q, const int *block_table, const int *seqlens_k,
                              int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                              int page_size, int num_pages, int max_pages_per_seq, float scale,
                              long long q_row_stride, long long q_head_stride,
                              long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                              long long block_table_stride, int window_left, int window_right, const float *sinks, int dtype,
                              int num_splits, void *workspace, long long workspace_bytes, void *hip_stream);
int fa_fwd_varlen_paged_num_splits(int B, int Hq, int max_seqlen_q, int D, int page_size, int max_pages_per_seq);
long long fa_fwd_varlen_paged_split_workspace_bytes(int B, int Hq, int total_q, int max_seqlen_q, int D,
                                                    int page_size, int max_pages_per_seq, int num_splits);

/*
 * Logit soft-capping: fa_fwd_varlen_softcap, fa_fwd_varlen_paged_softcap, fa_fwd_decode_paged_softcap and fa_bwd_varlen_softcap are the
 * four *_window entry points with `float softcap` added directly behind window_right (where the sink calls take `sinks`), for models that
 * cap their attention logits (Gemma-2: head_dim 128, grouped heads, a window of 4096 alternating with full causal layers, a cap of 50).
 * With x_ij = scale * s_ij / softcap and t_ij = tanh(x_ij) the capped score
 *     s'_ij = softcap * t_ij
 * takes the place of scale * s_ij everywhere: P_ij = exp(s'_ij) / sum_{j' visible} exp(s'_ij'), O_i = sum_j P_ij v_j, and LSE is that of the
 * capped scores. `softcap` is a HOST scalar and must be finite and greater than 0, else FA_ERR_INVALID_ARG ("softcap must be finite and
 * > 0"). Visibility is the rule of "Sliding window", unchanged, and it is applied AFTER the cap: tanh(-inf) is -1, not -inf, so a key
 * masked before the cap would enter the softmax with weight exp(-softcap). A row without a visible key (that section's integer test) gets
 * O = 0 and LSE = -inf, as there.
 * Each call goes through its *_window sibling's one validation and launch path: every shared rule keeps its status code and its error
 * text; support tables, the decode workspace and the backward workspace are the siblings' (the decode takes all four dtype pairs of
 * fa_fwd_decode_paged; the prefill calls and the backward take f16 / bf16 with D = 64 | 128).
 * ROUTING follows the sink forwards: the softcap forwards ALWAYS run one kernel family, the window-mode kernels in a softcap mode (eight
 * 128-row kernels, twelve decode partial kernels; the decode's combine kernels run unchanged, they see only (acc, m, l)), and the backward
 * always runs its windowed kernels in their softcap mode (eight kernels). An unbounded or never-binding side is clamped on the host, so
 * (-1, 0) is the capped causal layer and (4095, 0) the capped window layer. Not combined with sinks, and not offered on e4m3 pools in the
 * prefill (fa_fwd_varlen_paged_kv8), on the dense fa_fwd / fa_fwd_ex / fa_fwd_decode / fa_bwd, or at head_dim 256.
 * How the kernels form it: the operand held in registers (Q~; K~ in the dK/dV kernel) is pre-scaled once per block by
 * 2 * log2(e) * scale / softcap instead of scale * log2(e), so the matrix core delivers y with 2^y = e^(2x), the argument of the one
 * exponential tanh needs, and the score chain starts from zero instead of from the row's reference. Per score
 *     t = 1 - 2 / (1 + 2^y)          (one v_exp_f32, one v_rcp_f32; finite at both ends: 2^y = inf gives 1, 2^y = 0 gives -1)
 * then the mask, then P = exp2(fma(t, C, -m)) with C = softcap * log2(e) and m the row's reference in log2 units of the capped scores
 * (backward: -lse * log2(e) in m's place). Everything from P onwards is the window mode's code. The paged prefill is BIT-IDENTICAL to the
 * packed softcap call on every sequence with L_b >= Lq_b >= 1, as without a cap.
 * Backward: with the forward's LSE, P = exp(softcap * t - lse) and delta = rowsum(dO o O) is unchanged; the gradient with respect to the raw
 * score is dS_ij = P_ij * (dP_ij - delta_i) * (1 - t_ij^2), dQ = scale * dS K and dK = scale * dS^T Q are the existing final multiplies,
 * dV = P^T dO. The cap gets no gradient. delta and the write rules are fa_bwd_varlen_window's: owned tokens only, a key no query sees gets
 * dK = dV = 0, a dead row dQ = 0.
 * Accuracy. |d(softcap * tanh(x)) / d(scale * s)| = 1 - t^2 <= 1: the one rounding of the pre-scaled operand moves a capped score by no more
 * than it moved the raw one, so "LSE accuracy" (lse_tol, o_tol) and "Backward accuracy" stay valid upper bounds with their pre-scale terms
 * as they are. New is the evaluation of tanh in four fp32 steps (the exponential, 1 + e, the reciprocal, the fma): with u = 2^-24 and the
 * two hardware instructions within eps = 3 u (half an ulp plus the one ulp they may be off by),
 *     tanh_err = eps / 2 + 2 eps + 3 u = 10.5 * 2^-24 = 6.3e-7          (correctly rounded steps: 5.5 * 2^-24; measured in numpy: 1.9e-7)
 *     |LSE - exact| <= lse_tol + softcap * tanh_err          |O_d - exact| <= o_tol + |O_d| * softcap * tanh_err
 * and in the backward the per-element bound E_ij of "Backward accuracy", formed on g_ij = P_ij (dP_ij - delta_i), becomes
 *     E'_ij = E_ij * (1 - t_ij^2) + |g_ij| * (2 |t_ij| tanh_err + 2^-23)
 * (the factor 1 - t^2 scales what was there; t off by tanh_err moves the factor by 2 |t| tanh_err, and forming and applying it rounds
 * twice). tests/softcap.py spells every term out, tests/test_softcap_cases.py holds an fp32 model of the kernels' arithmetic to the bars
 * and shows eight planted mistakes to break them, tests/test_gpu_softcap.py and test_gpu_softcap_bwd.py hold the kernels.
 */
int fa_fwd_varlen_softcap(const void *q, const void *k, const void *v, void *o, float *lse,
                          const int *cu_seqlens_q, const int *cu_seqlens_k,
                          int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                          int D, float scale, long long q_row_stride, long long q_head_stride,
                          long long kv_row_stride, long long kv_head_stride,
                          int window_left, int window_right, float softcap, int dtype, void *hip_stream);
int fa_fwd_varlen_paged_softcap(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                                const int *cu_seqlens_q, const int *block_table, const int *seqlens_k,
                                int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                int page_size, int num_pages, int max_pages_per_seq, float scale,
                                long long q_row_stride, long long q_head_stride,
                                long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                                long long block_table_stride, int window_left, int window_right, float softcap, int dtype,
                                void *hip_stream);
int fa_fwd_decode_paged_softcap(const void *q, const void *k_pages, const void *v_pages, void *o, float *lse,
                                const int *block_table, const int *seqlens_k,
                                int B, int Hq, int Hkv, int Nq, int D, int page_size, int num_pages, int max_pages_per_seq,
                                float scale, long long q_batch_stride, long long q_head_stride,
                                long long kv_page_stride, long long kv_head_stride, long long kv_row_stride,
                                long long block_table_stride, int window_left, int window_right, float softcap,
                                int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes, void *hip_stream);
int fa_bwd_varlen_softcap(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                          float *dq, float *dk, float *dv, void *workspace,
                          const int *cu_seqlens_q, const int *cu_seqlens_k,
                          int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k, int D, float scale,
                          long long q_row_stride, long long q_head_stride, long long kv_row_stride, long long kv_head_stride,
                          int window_left, int window_right, float softcap, int dtype, void *hip_stream);

/*
 * Multi-head latent attention (decode): fa_fwd_mla_decode_paged is the "absorbed" decode step of MLA (DeepSeek-V2 / V3 / R1, Kimi-K2)
 * over a paged LATENT cache. Every query head reads ONE shared latent row per key, Dqk = 576 elements: 512 of compressed KV followed by 64
 * of rotary key. All 576 take part in the score, the first Dv = 512 are the value. Per sequence b, with L_b = seqlens_k[b] clamped to
 * [0, max_pages_per_seq * P]:
 *     s_ij = q[b,h,i,0:Dqk] . kv_j[0:Dqk]      P = softmax_j(scale * s_ij) over visible keys      O[b,h,i,0:Dv] = sum_j P_ij * kv_j[0:Dv]
 * LSE is in natural log, [B, Hq, Nq] fp32, or NULL. `scale` is the caller's: there is no default, the model's head dim is not 576.
 * The pool: key j of sequence b is slot j % P of page block_table[b][j / P] of ONE pool (K and V are the same bytes); element d of slot r
 * of page p sits at p * kv_page_stride + r * kv_row_stride + d. The natural layout is [num_pages, P, 576]: one latent head, no head
 * stride (the layout of vLLM's and FlashMLA's latent cache). The pool may exceed 4 GiB; one page stays below 2 GiB, the capacity
 * max_pages_per_seq * P is at most 2^30 keys.
 * q and o: element (b, h, i, d) sits at b * q_batch_stride + h * q_head_stride + i * q_row_stride + d, and of o likewise under the o_*
 * strides, so [B, Hq, Nq, D] and token-major [B, Nq, Hq, D] both work. Strides are multiples of 8 elements, each at least Dqk (Dv for
 * o; the batch stride may be anything >= 0 when B = 1); bases are 16-byte aligned. O rows of 512 elements are written, never 576.
 * Causal is bottom-right aligned per sequence, as in fa_fwd_decode_paged: key j is visible to query i iff j <= i + L_b - Nq.
 * Supported: f16 / bf16 (q and the pool of one type), (Dqk, Dv) = (576, 512), Hq * Nq <= 32 packed rows r = h * Nq + i (16 heads under
 * tensor parallelism of 8 with one or two tokens per step), P in {16, 32, 64, 128, 256}; anything else FA_ERR_UNSUPPORTED with a message
 * that names what was given.
 * As fa_fwd_decode_paged, in its words:
 *  - block_table (int32, [B, block_table_stride], block_table_stride >= max_pages_per_seq) and seqlens_k (int32, [B]) are DEVICE memory
 *    read by the kernels -- the host never reads them, and both grids depend on host scalars only, so one captured graph serves every step;
 *  - a row with no visible key (L_b = 0, or causal with i + L_b < Nq) gets O = 0 exactly and LSE = -inf;
 *  - results depend neither on slots >= L_b of a sequence's last page (NaN there is harmless: they read as zeros), nor on table entries
 *    past ceil(L_b / P), nor on the workspace's prior contents, and are bitwise reproducible; a page index outside [0, num_pages) reads
 *    as zeros and touches nothing outside the pool;
 *  - `workspace` is caller-owned device memory of fa_fwd_mla_decode_paged_workspace_bytes() bytes, 16-byte aligned, contents irrelevant
 *    before and after the call; the call is asynchronous and allocates nothing;
 *  - bad pointers, sizes or strides, a short workspace or block_table_stride < max_pages_per_seq: FA_ERR_INVALID_ARG before any launch.
 *    Every rule the two calls share carries the same status and the same text after the function name.
 * How it runs (csrc/fa_mla_kernel.hip): the keys of a sequence are split over S one-wave items per 16-row block,
 * S by fa_fwd_decode_paged's rule evaluated at the capacity; an item streams 64-key tiles (72 KiB: a [64][512] latent part and a [64][64]
 * rotary part in one LDS image that serves both products) and writes its partial (O * l, m, l) to the workspace, B * S * rows16 *
 * (Dv + 2) floats with rows16 = 16 * ceil(Hq * Nq / 16); a second launch combines them by their maxima. Rows 17..32 are a second
 * 16-row item over the same keys. Pre-scaled query operand as FA_VARIANT_MFMA ("LSE accuracy" above): the tolerances are
 * fa_fwd_decode's, formed on the 576-wide rows.
 * The append needs no entry point of its own: fa_kv_append_paged with Hkv = 1, D = 576, k_new == v_new and k_pages == v_pages (a row is
 * 72 whole 16-byte chunks; both copies write the same bytes).
 * Not here: more than 32 packed rows (fa_fwd_mla_decode_paged_wide, below: up to 128), e4m3 latent pools (fa_fwd_mla_decode_paged_kv8, below),
 * window / sink / softcap, the MLA prefill
 * (192 / 128 head dims: fa_fwd_varlen_mla, below), a backward.
 */
int fa_fwd_mla_decode_paged(const void *q, const void *kv_pages, void *o, float *lse,
                            const int *block_table, const int *seqlens_k,
                            int B, int Hq, int Nq, int Dqk, int Dv,
                            int page_size, int num_pages, int max_pages_per_seq, float scale,
                            long long q_batch_stride, long long q_head_stride, long long q_row_stride,
                            long long o_batch_stride, long long o_head_stride, long long o_row_stride,
                            long long kv_page_stride, long long kv_row_stride, long long block_table_stride,
                            int is_causal, int dtype, void *workspace, long long workspace_bytes, void *hip_stream);
/* depends on host scalars only (the split rule at the capacity); 0 if a size is invalid or unsupported */
long long fa_fwd_mla_decode_paged_workspace_bytes(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq);
int fa_fwd_mla_decode_paged_supported(int dtype, int Dqk, int Dv, int Hq, int Nq, int page_size);

/*
 * Multi-head latent attention (decode, wide): fa_fwd_mla_decode_paged_wide is fa_fwd_mla_decode_paged for up to 128 packed query rows:
 * all 128 heads on one GPU under data-parallel attention, or k-token verification at 16 heads (16 x 3 = 48 rows, 16 x 8 = 128). The
 * argument list is identical, and so is the contract, in the same words: packed rows r = h * Nq + i; three strides each for q and o;
 * the one pool [num_pages, P, 576]; device-side tables read by the kernels only (graph-capturable); causal bottom-right aligned; a row
 * with no visible key gets O = 0 exactly and LSE = -inf; slots >= L_b and pages outside the pool read as zeros; no dependence on the
 * workspace's prior contents; bitwise reproducible; asynchronous, allocates nothing; O rows of 512 elements are written, never 576.
 * Supported: f16 / bf16, (Dqk, Dv) = (576, 512), 1 <= Hq * Nq <= 128, P in {16, 32, 64, 128, 256}; anything else FA_ERR_UNSUPPORTED with
 * a message that names what was given. Both calls validate on one path: every rule they share carries the same status and the same
 * text after the function name.
 * How it runs (csrc/fa_mla_wide_kernel.hip): a WORKGROUP of NW waves shares one tile image in LDS, NW = 2 for
 * Hq * Nq <= 32 and NW = 4 above. Row-to-wave map: wave w of row block wb holds packed rows 16 * (wb * NW + w) .. + 15 and does with
 * them exactly what a one-wave item of fa_fwd_mla_decode_paged does (the same source text: over the same key split its bits are that
 * call's); wave w stages rows (64 / NW) * w .. of every 64-key tile, so each latent row is streamed once for 16 * NW query rows. Grid
 * (B * S, WB) with WB = ceil(Hq * Nq / (16 * NW)) row blocks, 64 * NW threads, 144 KiB of LDS. Split rule: S is
 * fa_fwd_mla_decode_paged's rule fed WB in place of the number of 16-row blocks, evaluated at the capacity (host scalars only, S <= 256).
 * The workspace has that call's format, B * S * rows16 * (Dv + 2) floats with rows16 = 16 * ceil(Hq * Nq / 16) (wave w of block wb
 * writes 16-row slot wb * NW + w; a wave whose 16 rows are all padding has no slot and writes nothing), and its combine kernel runs
 * unchanged. For Hq * Nq <= 32 both calls are legal; they differ in S, hence in the last bits, and in cost (README.md, round 26).
 * Not here: more than 128 packed rows, window / sink / softcap (e4m3 latent pools: fa_fwd_mla_decode_paged_kv8, below).
 */
int fa_fwd_mla_decode_paged_wide(const void *q, const void *kv_pages, void *o, float *lse,
                                 const int *block_table, const int *seqlens_k,
                                 int B, int Hq, int Nq, int Dqk, int Dv,
                                 int page_size, int num_pages, int max_pages_per_seq, float scale,
                                 long long q_batch_stride, long long q_head_stride, long long q_row_stride,
                                 long long o_batch_stride, long long o_head_stride, long long o_row_stride,
                                 long long kv_page_stride, long long kv_row_stride, long long block_table_stride,
                                 int is_causal, int dtype, void *workspace, long long workspace_bytes, void *hip_stream);
/* depends on host scalars only (the split rule at the capacity); 0 if a size is invalid or unsupported */
long long fa_fwd_mla_decode_paged_wide_workspace_bytes(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq);
int fa_fwd_mla_decode_paged_wide_supported(int dtype, int Dqk, int Dv, int Hq, int Nq, int page_size);

/*
 * Multi-head latent attention (decode, e4m3 pool): fa_fwd_mla_decode_paged_kv8 is fa_fwd_mla_decode_paged_wide under bf16 queries on a latent
 * pool of OCP e4m3 (e4m3fn) bytes: 576 bytes per key in place of 1152, twice the context or the batch in the same memory. The argument
 * list is the wide call's with `int dtype` replaced by `int q_dtype, int kv_dtype`.
 * Supported: (q_dtype, kv_dtype) = (FA_DTYPE_BF16, FA_DTYPE_FP8_E4M3) only, O is bf16; (Dqk, Dv) = (576, 512), 1 <= Hq * Nq <= 128,
 * P in {16, 32, 64, 128, 256}; anything else -- (f16, e4m3), (e4m3, e4m3) and (bf16, bf16) included -- FA_ERR_UNSUPPORTED with a message
 * that names what was given. fa_fwd_mla_decode_paged_supported / _wide_supported keep answering 0 for e4m3: those calls are untouched.
 * The pool is [num_pages, P, 576] bytes; kv_page_stride and kv_row_stride count elements (= bytes), are multiples of 16 and at least 576,
 * the base is 16-byte aligned (fa_fwd_decode_paged's rule for e4m3 pools, with its status and text); one page stays below 2 GiB. q and o
 * keep the wide call's rules: three strides each, multiples of 8, bf16.
 * NO SCALES, in the words of fa_fwd_decode_kv8: the bytes are read as plain e4m3 values. K and V are the same bytes here, so there is one
 * per-tensor scale s: a caller that appended with k_mul = v_mul = 1 / s passes scale * s to this call and multiplies O by s (or folds s
 * into the projection behind it).
 * THE CONTRACT: the result is the wide call on the exactly widened pool. O and LSE are BIT-IDENTICAL to
 * fa_fwd_mla_decode_paged_wide(..., FA_DTYPE_BF16) on a bf16 pool that holds the same values widened (every e4m3 value is a bf16 value) --
 * the same page order, the same strides in elements, the same slots unused, the same table entries out of range -- for every legal
 * Hq * Nq. The split count S and the workspace size are the wide call's: fa_fwd_mla_decode_paged_kv8_workspace_bytes equals
 * fa_fwd_mla_decode_paged_wide_workspace_bytes on every legal input and is 0 where that is 0. Everything else is inherited in the same
 * words: the tolerances and "LSE accuracy"; a row with no visible key gets O = 0 exactly and LSE = -inf; clamped lengths; slots >= L_b
 * and pages outside [0, num_pages) read as zeros (the e4m3 NaN bytes 0x7F / 0xFF there are harmless); no dependence on the workspace's
 * prior contents; bitwise reproducible; device-side tables read by the kernels only (graph-capturable); asynchronous, allocates nothing.
 * Validation runs on the path of the other two calls: every rule shared with the wide call carries the same status and the same text
 * after the function name; only the dtype pair and the 16-element stride rule differ.
 * The quantising append needs no entry point of its own: fa_kv_append_paged_quant with Hkv = 1, D = 576, k_pages == v_pages, k_new ==
 * v_new and k_mul == v_mul (a row is 36 whole 16-byte chunks; both copies write the same bytes).
 * How it runs (csrc/fa_mla_kv8_kernel.hip): the wide call's four-wave workgroup for EVERY row count (for
 * Hq * Nq <= 32 the split rule is still fed one row block, so S is the wide call's). LDS-DMA cannot widen, so wave w stages rows
 * 16 * w .. + 15 of a tile through registers: nine 16-byte loads per lane under one range-checked descriptor, widened and written into
 * the wide call's tile image with its swizzles, one tile ahead of the arithmetic. From LDS onwards the source text is the wide call's.
 * Not here: f16 or e4m3 queries, scales inside the kernel, block or per-token scales, a bf16 rotary part behind an e4m3 latent part,
 * more than 128 rows, window / sink / softcap.
 */
int fa_fwd_mla_decode_paged_kv8(const void *q, const void *kv_pages, void *o, float *lse,
                                const int *block_table, const int *seqlens_k,
                                int B, int Hq, int Nq, int Dqk, int Dv,
                                int page_size, int num_pages, int max_pages_per_seq, float scale,
                                long long q_batch_stride, long long q_head_stride, long long q_row_stride,
                                long long o_batch_stride, long long o_head_stride, long long o_row_stride,
                                long long kv_page_stride, long long kv_row_stride, long long block_table_stride,
                                int is_causal, int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes, void *hip_stream);
/* the wide call's size on every legal input; 0 if a size is invalid or unsupported */
long long fa_fwd_mla_decode_paged_kv8_workspace_bytes(int B, int Hq, int Nq, int Dv, int page_size, int max_pages_per_seq);
int fa_fwd_mla_decode_paged_kv8_supported(int q_dtype, int kv_dtype, int Dqk, int Dv, int Hq, int Nq, int page_size);

/*
 * Multi-head latent attention (decode, sparse): fa_fwd_mla_decode_sparse is the absorbed MLA step over a LIST of keys per query token, as
 * the models with an indexer in front of attention run it (DeepSeek-V3.2 and its successors: at most topk = 2048 keys per token), in
 * decode and in prefill alike. The rows named by the list are read in place: no gather into a second pool.
 * Queries are packed TOKENS: q is [T, Hq, 576] and o is [T, Hq, 512], each under its own (token, head) element strides -- the wide call's
 * rules for q and o: multiples of 8, at least 576 / 512, bases 16-byte aligned, the token stride free when T = 1. lse is [T, Hq] fp32
 * contiguous, or NULL. O rows of 512 elements are written, never 576. A token is what the dense calls name (b, i): a decode step with
 * Nq tokens per sequence passes T = B * Nq, a prefill chunk its packed tokens.
 * The pool is the family's [num_pages, P, 576] under kv_page_stride / kv_row_stride, with the wide call's rules, statuses and texts: the
 * pool may exceed 4 GiB, one page stays below 2 GiB. A key is named by its SLOT x = page * P + row, 0 <= x < num_pages * P; its address
 * is (x >> log2 P) * kv_page_stride + (x & (P - 1)) * kv_row_stride. (Slots, not positions: a serving engine turns the indexer's output
 * into slots once per step for all layers, and packed prefill tokens then need no block table.)
 * indices is int32 DEVICE memory, [T, indices_stride] with indices_stride >= topk a multiple of 4 and a 16-byte aligned base.
 * index_counts is int32 [T] DEVICE memory or NULL: n_t = clamp(index_counts[t], 0, topk), and n_t = topk under NULL. The kernels read
 * both; the host never does, and both grids depend on host scalars alone: one captured graph serves every step.
 * For token t and head h, with x_j = indices[t][j] for j < n_t: s_j = q[t,h,0:576] . row(x_j)[0:576], P = softmax_j(scale * s_j),
 * O[t,h,0:512] = sum_j P_j row(x_j)[0:512]; LSE in natural log. The list is a list, not a set: a slot named twice enters twice. There is
 * no mask and no is_causal: visibility is the list. n_t = 0 gives O = 0 exactly and LSE = -inf. An entry among the first n_t outside
 * [0, num_pages * P) reads as a row of zeros (a key of score 0 and value 0) and touches nothing outside the pool -- the family's rule for
 * a page outside the pool. That is a safety rule, not a way to mask: valid entries stand in front and index_counts says how many.
 * Entries at j >= n_t have no influence, whatever they hold, and are never read; nor are positions j >= topk of a row. Pool rows that
 * no list names have no influence: NaN there is harmless.
 * Supported: f16 / bf16 (q and the pool of one type), (Dqk, Dv) = (576, 512), 1 <= Hq <= 128, topk >= 1, T >= 1, P in {16, 32, 64, 128,
 * 256}; anything else FA_ERR_UNSUPPORTED with a message that names what was given. Every rule shared with
 * fa_fwd_mla_decode_paged_wide carries that call's status and text after the function name. Rules of this call's own, each
 * FA_ERR_INVALID_ARG before any launch: null indices; topk < 1; indices_stride < topk or not a multiple of 4; misaligned indices (16
 * bytes) or index_counts (4); 64 * ceil(topk / 64) or num_pages * P above 2^30; a grid that does not fit an int.
 * THE CONTRACT: with cap = 64 * ceil(topk / 64), O and LSE are BIT-IDENTICAL to fa_fwd_mla_decode_paged_wide(B = T, Nq = 1,
 * page_size = 64, max_pages_per_seq = cap / 64, is_causal = 0, seqlens_k = n) on a pool into which every token's listed rows were
 * copied in list order (row j of token t in slot j % 64 of page block_table[t][j / 64]; out-of-range entries as zero rows). The split
 * count is that call's own rule there, S = splits(T, ceil(Hq / (16 * NW(Hq))), cap), and fa_fwd_mla_decode_sparse_workspace_bytes equals
 * fa_fwd_mla_decode_paged_wide_workspace_bytes(T, Hq, 1, 512, 64, cap / 64) on every legal input and is 0 elsewhere. Everything else is
 * inherited in the wide call's words: the tolerances and "LSE accuracy" on the 576-wide rows; no dependence on the workspace's prior
 * contents; bitwise reproducible; asynchronous, allocates nothing.
 * How it runs (csrc/fa_mla_sparse_kernel.hip): the wide call's four-wave workgroup for every head count, over
 * the item (token, split). Only the staging of a tile is new: each of a tile's 64 latent rows moves by LDS-DMA under a descriptor of its
 * OWN, built on the row's 64-bit address (num_records = 1152, or 0 for an entry behind n_t or outside the pool); the rotary 128 bytes
 * of a row go through registers, two predicated 16-byte loads per lane and tile, written into the image behind the tile's arithmetic.
 * From LDS onwards the source text is the wide call's.
 * Not here: e4m3 pools and the 656-byte rows with per-tile scales; a mask inside the list; more than 128 heads; sinks; the indexer
 * itself; a sparse backward. No dense call is rerouted.
 */
int fa_fwd_mla_decode_sparse(const void *q, const void *kv_pages, void *o, float *lse,
                             const int *indices, const int *index_counts,
                             int T, int Hq, int Dqk, int Dv, int topk,
                             int page_size, int num_pages, float scale,
                             long long q_token_stride, long long q_head_stride,
                             long long o_token_stride, long long o_head_stride,
                             long long kv_page_stride, long long kv_row_stride, long long indices_stride,
                             int dtype, void *workspace, long long workspace_bytes, void *hip_stream);
/* the wide call's size at (T, Hq, 1, 512, 64, ceil(topk / 64)) on every legal input; 0 if a size is invalid or unsupported */
long long fa_fwd_mla_decode_sparse_workspace_bytes(int T, int Hq, int Dv, int topk);
int fa_fwd_mla_decode_sparse_supported(int dtype, int Dqk, int Dv, int Hq, int page_size);

/*
 * Multi-head latent attention (decode, sparse, e4m3 pool): fa_fwd_mla_decode_sparse_kv8 is fa_fwd_mla_decode_sparse under bf16 queries on a
 * latent pool of OCP e4m3 (e4m3fn) bytes, 576 bytes per key: what a sparse-attention model served with an fp8 KV cache calls at every
 * layer and step. The listed rows are read in place; no gather into a second e4m3 pool. The argument list is the sparse call's with
 * `int dtype` replaced by `int q_dtype, int kv_dtype`.
 * Supported: (q_dtype, kv_dtype) = (FA_DTYPE_BF16, FA_DTYPE_FP8_E4M3) only, O is bf16; (Dqk, Dv) = (576, 512), 1 <= Hq <= 128, topk >= 1,
 * T >= 1, P in {16, 32, 64, 128, 256}; anything else -- (f16, e4m3), (e4m3, e4m3) and (bf16, bf16) included -- FA_ERR_UNSUPPORTED with a
 * message that names what was given. fa_fwd_mla_decode_sparse_supported keeps answering 0 for e4m3 and that call keeps refusing such pools.
 * The pool is [num_pages, P, 576] BYTES; kv_page_stride and kv_row_stride count elements (= bytes), are multiples of 16 and at least 576,
 * the base is 16-byte aligned (fa_fwd_mla_decode_paged_kv8's rule, with its statuses and texts). The pool may exceed 4 GiB, one page stays
 * below 2 GiB. A key is the SLOT x = page * P + row; its byte address is (x >> log2 P) * kv_page_stride + (x & (P - 1)) * kv_row_stride.
 * Lists, counts, q and o follow fa_fwd_mla_decode_sparse exactly, in its words: indices is int32 [T, indices_stride], the stride at
 * least topk and a multiple of 4, the base 16-byte aligned; index_counts is int32 [T] or NULL; a slot named twice enters twice; an entry
 * among the first n_t outside [0, num_pages * P) is a key of zeros and no address is formed from it; nothing at j >= n_t or j >= topk
 * is ever read; n_t = 0 gives O = 0 exactly and LSE = -inf; pool bytes that no list names have no influence (the e4m3 NaN codes 0x7F /
 * 0xFF there are harmless); the host reads neither table and both grids depend on host scalars alone (graph-capturable).
 * NO SCALES, in the words of fa_fwd_mla_decode_paged_kv8: the bytes are read as plain e4m3 values. The cache's one per-tensor scale s goes
 * into scale * s and behind O (a caller that appended with k_mul = v_mul = 1 / s multiplies O by s or folds s into the projection).
 * THE CONTRACT: with cap = 64 * ceil(topk / 64), O and LSE are BIT-IDENTICAL to both of
 *   1. fa_fwd_mla_decode_sparse(..., FA_DTYPE_BF16) on a bf16 pool that holds the same values widened (every e4m3 value is a bf16 value),
 *      under the same lists and counts, the same strides in elements and the same page size;
 *   2. fa_fwd_mla_decode_paged_kv8(B = T, Nq = 1, page_size = 64, max_pages_per_seq = cap / 64, is_causal = 0, seqlens_k = n) on an e4m3
 *      pool into which every token's listed rows were copied in list order, out-of-range entries as zero rows.
 * The split count S is what fa_fwd_mla_decode_sparse computes (for Hq <= 32 the split rule is fed one row block under either wave
 * count), and fa_fwd_mla_decode_sparse_kv8_workspace_bytes equals fa_fwd_mla_decode_sparse_workspace_bytes(T, Hq, Dv, topk) on every legal
 * input and is 0 elsewhere. Everything else is inherited in the same words: the tolerances and "LSE accuracy"; no dependence on the
 * workspace's prior contents; bitwise reproducible; asynchronous, allocates nothing.
 * Validation runs on the sparse call's path: every rule the two calls share carries the same status and the same text after the
 * function name; only the dtype-pair rule and the 16-element stride rule differ.
 * The quantising append is fa_kv_append_paged_quant on the aliased pool (Hkv = 1, D = 576, k_pages == v_pages, k_mul == v_mul).
 * How it runs (csrc/fa_mla_sparse_kv8_kernel.hip): fa_fwd_mla_decode_paged_kv8's four-wave workgroup over the item
 * (token, split). Wave w stages rows 16 * w .. + 15 of a tile through registers under that kernel's lane maps; only the nine raw loads
 * per lane differ: each lane takes its row's entry from the wave's entry register, forms the row's 64-bit byte address and issues one
 * predicated 16-byte load (an invalid entry: zeros, no load). Widening, the tile image and everything from LDS onwards are the twins'.
 * Not here: f16 or e4m3 queries; scales inside the kernel, block or per-token scales; the 656-byte rows (e4m3 latent + fp32 tile scales
 * + bf16 rotary); a mask inside the list; more than 128 heads; sinks, window and softcap; the indexer itself; a sparse backward. No
 * dense call is rerouted.
 */
int fa_fwd_mla_decode_sparse_kv8(const void *q, const void *kv_pages, void *o, float *lse,
                                 const int *indices, const int *index_counts,
                                 int T, int Hq, int Dqk, int Dv, int topk,
                                 int page_size, int num_pages, float scale,
                                 long long q_token_stride, long long q_head_stride,
                                 long long o_token_stride, long long o_head_stride,
                                 long long kv_page_stride, long long kv_row_stride, long long indices_stride,
                                 int q_dtype, int kv_dtype, void *workspace, long long workspace_bytes, void *hip_stream);
/* the sparse call's size on every legal input; 0 if a size is invalid or unsupported */
long long fa_fwd_mla_decode_sparse_kv8_workspace_bytes(int T, int Hq, int Dv, int topk);
int fa_fwd_mla_decode_sparse_kv8_supported(int q_dtype, int kv_dtype, int Dqk, int Dv, int Hq, int page_size);

/*
 * Multi-head latent attention (prefill): fa_fwd_varlen_mla is the NON-absorbed form of the same layer, as serving engines run its
 * prefill: the latent rows are up-projected to per-head keys and values, and ordinary multi-head attention runs over packed sequences
 * with a query / key head dim of Dqk = 192 (128 "nope" + 64 rotary) and a value head dim of Dv = 128. Per sequence the operator is
 * fa_fwd_varlen's with two head dims:
 *     s_ij = q_i[0:192] . k_j[0:192]      P = softmax_j(scale * s_ij) over visible keys      O_i[0:128] = sum_j P_ij * v_j[0:128]
 * LSE is in natural log, [Hq, total_q] fp32 contiguous, or NULL. `scale` is the caller's (DeepSeek: 192^-0.5 times its mscale); nothing
 * is derived from Dv.
 * Everything fa_fwd_varlen promises holds, in its words: cu_seqlens_q / cu_seqlens_k (int32, [B + 1]) are DEVICE memory read by the
 * kernels -- the host never reads them and the launch geometry depends on the host scalars alone (B * Hq * ceil(max_seqlen_q / 128)
 * workgroups), so one captured graph serves any set of lengths under the same B, total_* and max_seqlen_*. Every table entry is clamped
 * to [0, total], a non-increasing pair gives length 0, and the lengths Lq_b / Lk_b are clamped to max_seqlen_q / max_seqlen_k: rows of a
 * sequence beyond that clamp and tokens at or past cu_seqlens_q[B] are not written, neither are bytes between heads or rows under wide
 * strides, and a corrupt table touches nothing outside tokens [0, total) of any tensor. Lk_b < Lq_b and Lk_b = 0 are legal: a row with
 * no visible key gets O = 0 exactly and LSE = -inf. Causal is bottom-right aligned PER SEQUENCE (key j visible to query i iff
 * j <= i + Lk_b - Lq_b); query head h reads key/value head h / (Hq / Hkv). Results are bitwise reproducible, nothing is allocated, the
 * call is asynchronous on hip_stream.
 * What differs: q, k, v and o EACH have their own (row, head) element strides -- token t, head h, element d of tensor x sits at
 * t * x_row_stride + h * x_head_stride + d -- multiples of 8, at least 192 / 192 / 128 / 128, bases 16-byte aligned, element stride 1;
 * (max_seqlen + 128) * row_stride * 2 bytes stay below 4 GiB for each of the four (max_seqlen_q for q and o, max_seqlen_k for k and v).
 * So v may be a view of the [total_k, H, 256] output of the kv up-projection (head stride 256, offset 128: k's nope part is the other
 * half), and o a slice of a wider buffer. O rows of 128 elements are written, never 192.
 * f16 / bf16, (Dqk, Dv) = (192, 128): anything else FA_ERR_UNSUPPORTED with a message that names what was given. Null pointers (lse may
 * be NULL), sizes < 1, Hq % Hkv != 0, scale <= 0, bad strides or alignment, max_seqlen_* > total_*, a sequence above the 4 GiB bound or
 * a grid that does not fit an int: FA_ERR_INVALID_ARG before any launch; every rule shared with fa_fwd_varlen carries its status and
 * its text after the function name.
 * How it runs (csrc/fa_mfma_kernel.hip, MLA mode): the head_dim-128 varlen kernel from the scores onwards
 * (pre-scaled query operand: tolerances are FA_VARIANT_MFMA's formed on the 192-wide rows, "LSE accuracy" above), over a two-part K
 * image in LDS -- the head_dim-128 image of the nope columns, behind it the head_dim-64 image of the rotary columns. A score chain runs
 * the eight nope k-steps, then the four rotary ones: with columns 128..191 of q and k zero, O and LSE are BIT-IDENTICAL to
 * fa_fwd_varlen at D = 128 on the first 128 columns under the same scale.
 * Chunked context ("Latent-attention layers: prefill"): one un-masked call per chunk of cached context, one causal
 * call on the new tokens, merged by the caller through the LSEs.
 * Not here: the rotary key as a separate broadcast tensor, a paged or e4m3 key side, window / sink / softcap, a key split, other
 * head-dim pairs, an in-library merge. (The backward: fa_bwd_varlen_mla, below.)
 */
int fa_fwd_varlen_mla(const void *q, const void *k, const void *v, void *o, float *lse,
                      const int *cu_seqlens_q, const int *cu_seqlens_k,
                      int B, int Hq, int Hkv, int total_q, int total_k,
                      int max_seqlen_q, int max_seqlen_k, int Dqk, int Dv, float scale,
                      long long q_row_stride, long long q_head_stride,
                      long long k_row_stride, long long k_head_stride,
                      long long v_row_stride, long long v_head_stride,
                      long long o_row_stride, long long o_head_stride,
                      int is_causal, int dtype, void *hip_stream);
int fa_fwd_varlen_mla_supported(int dtype, int Dqk, int Dv);   /* f16 | bf16, (192, 128) */

/*
 * Multi-head latent attention (prefill, backward): fa_bwd_varlen_mla is the backward of fa_fwd_varlen_mla -- the form in which these
 * layers are trained. Per sequence it is fa_bwd_ex's operator with two head dims, on the forward's operator:
 *     P = exp(scale * q.k - lse) over 192 columns       delta_i = sum_d dO_id O_id and dP = dO.V^T over 128 columns
 *     dS = P o (dP - delta)       dQ = scale * dS K (192 wide)
 *     dK = scale * dS^T Q (192 wide) and dV = P^T dO (128 wide), both summed over the query heads of a group.
 * Layout: q, k, v and o each keep the forward's own (row, head) ELEMENT stride pair under the forward's rules (multiples of 8, at least
 * 192 / 192 / 128 / 128, bases 16-byte aligned, the 4 GiB rule per tensor). d_o is addressed under o's strides. The fp32 gradients dq,
 * dk, dv are addressed under the element strides of q, k, v respectively -- fa_bwd_varlen's convention applied tensor by tensor: with v
 * the upper half of a [total_k, H, 256] kv up-projection, dv is the upper half of an fp32 buffer of that shape. lse is the forward's
 * [Hq, total_q]. `workspace`: caller-owned device memory of fa_bwd_varlen_workspace_bytes(Hq, total_q) bytes; it holds delta,
 * [Hq, total_q] fp32. There is no size function of its own.
 * What is kept from fa_bwd_varlen, in its words: the cu_seqlens tables are DEVICE memory read by the kernels and clamped as the forward
 * clamps them; both grids depend on host scalars only (B * Hq * ceil(max_seqlen_q / 128) and B * Hkv * ceil(max_seqlen_k / 128)
 * workgroups), so the call can be captured in a graph. Only owned tokens are written -- dq rows of owned query tokens (192 elements),
 * dk / dv rows of owned keys (192 / 128 elements) -- and no bytes between heads or rows under wide strides. dK = dV = 0 for a key no
 * query sees. A dead query row (no visible key) is recognised by the forward's integer test and never by its LSE: it gets dQ = 0 exactly
 * and adds exactly nothing to dK / dV. The result does not depend on the workspace's prior contents. Bitwise reproducible: no atomics,
 * no allocation; asynchronous on hip_stream.
 * f16 / bf16, (Dqk, Dv) = (192, 128): anything else FA_ERR_UNSUPPORTED with a message that names what was given. Every rule shared with
 * fa_fwd_varlen_mla or fa_bwd_varlen carries that call's status and its text after the function name.
 * The bit contract mirrors the forward's. With columns 128..191 of q and k zero, dq[..., :128], dk[..., :128] and dv are BIT-IDENTICAL to
 * fa_bwd_varlen at D = 128 on the first 128 columns under the same scale, per sequence, and columns 128..191 of dq and dk are zero: the
 * eight nope k-steps of a score chain run first in that kernel's order, then the four rotary ones; the dP chain and both second
 * products run in its order (csrc/fa_bwd_mla_kernels.hip).
 * Not here: a paged or e4m3 key side, window / sink / softcap, other head-dim pairs, the rotary key as a separate broadcast tensor, a
 * gradient through LSE, a dense (non-varlen) form.
 */
int fa_bwd_varlen_mla(const void *q, const void *k, const void *v, const void *o, const void *d_o, const float *lse,
                      float *dq, float *dk, float *dv, void *workspace,
                      const int *cu_seqlens_q, const int *cu_seqlens_k,
                      int B, int Hq, int Hkv, int total_q, int total_k, int max_seqlen_q, int max_seqlen_k,
                      int Dqk, int Dv, float scale,
                      long long q_row_stride, long long q_head_stride, long long k_row_stride, long long k_head_stride,
                      long long v_row_stride, long long v_head_stride, long long o_row_stride, long long o_head_stride,
                      int is_causal, int dtype, void *hip_stream);
int fa_bwd_varlen_mla_supported(int dtype, int Dqk, int Dv);   /* f16 | bf16, (192, 128) */

/* 1 if fa_fwd has a kernel for the combination, else 0 (no GPU needed). */
int fa_supported(int dtype, int variant, int D);

/* variant FA_VARIANT_AUTO resolves to for (dtype, D); FA_ERR_UNSUPPORTED if none. */
int fa_resolve_variant(int dtype, int D);

/* variant FA_VARIANT_AUTO resolves to for a whole problem (the choice between the matrix-core kernels depends on
 * the grid the shape gives); FA_ERR_UNSUPPORTED if none. */
int fa_resolve_variant_for(int dtype, int D, int B, int H, int N, int is_causal);

/* name of the device kernel fa_fwd(..., FA_VARIANT_AUTO) launches for the problem, as rocprofv3 prints it
 * (e.g. "fa::fwd_pp_kernel<fa::BF16, 64, true>"); "" if none. Static storage. */
const char *fa_fwd_kernel_name(int dtype, int D, int B, int H, int N, int is_causal);

/* bytes per element of Q/K/V and of O for a dtype (fp8: 1 and 2). 0 if bad enum. */
int fa_dtype_in_bytes(int dtype);
int fa_dtype_out_bytes(int dtype);

/* algorithmic work of one fa_fwd call:
 * flops = 4*B*H*N^2*D (2*.. causal); bytes = (3*in + out)*B*H*N*D + 4*B*H*N */
double fa_algorithmic_flops(int B, int H, int N, int D, int is_causal);
double fa_algorithmic_bytes(int B, int H, int N, int D, int dtype);

/* thread-local text of the last error on this thread ("" if none). */
const char *fa_last_error(void);

int fa_version(void);
const char *fa_variant_name(int variant);
const char *fa_dtype_name(int dtype);

#ifdef __cplusplus
}
#endif
#endif /* FA_MI355_H */
