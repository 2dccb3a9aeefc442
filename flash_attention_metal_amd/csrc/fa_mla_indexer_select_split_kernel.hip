// fa_mla_indexer_select_split_kernel.hip -- fa_mla_indexer_select's contract with ONE TOKEN'S ROW SPLIT OVER SEVERAL WORKGROUPS: entry point
// fa_mla_indexer_select_split. A decode step on a few long sequences leaves fa_mla_indexer_select one workgroup per token, that is a few
// compute units for the whole row; here S workgroups share a token and the radix select becomes a CHAIN OF FIVE PLAIN LAUNCHES.
//
//   * THE SPLIT. The capacity cap = max_pages_per_seq * P is cut into S segments of seg = roundup64(ceil(cap / S)) keys; workgroup
//     (token, s) of 256 threads owns the positions [s * seg, min((s + 1) * seg, v)). The grid, B * max_seqlen_q * S, comes from host
//     scalars alone. A segment that starts at or behind v leaves every launch in front of its first barrier, as a whole workgroup.
//   * NOBODY WAITS FOR ANYBODY. What one workgroup needs from another it reads in the NEXT launch: the stream orders the launches, so
//     there is no flag, no ticket, no grid-wide sync and no global atomic. A workgroup never reads a word written in its own launch
//     by another workgroup.
//   * LAUNCHES H0 .. H3 (mla_indexer_split_hist_kernel<K>): one radix digit of idx_image() each, most significant byte first. The
//     workgroup reads its segment ONCE, counts the keys that match the threshold prefix found so far into a 256-bin LDS histogram (LDS
//     atomics only) and writes the histogram to the workspace at [K][token][s][256].
//   * THE PICK OF ROUND K - 1 is re-derived by every workgroup of launch K (and of the emission launch for round 3) from that round's
//     histograms: thread `bin` sums its bin over the segments that start below v, and keeps a second sum over the segments IN FRONT of
//     its own; idx_block_scan over the bins from the top finds the bin that holds rank `need`. All S workgroups of a token compute the
//     same (T prefix, need); segment 0 stores it in the state slot [K - 1][token] for launch K + 1, which is where the others read it
//     from (one round later, never their own launch's). The second sum gives, in the same scan, the keys of the segments in front that
//     fall into GREATER bins: added up round by round in the slot carry[token][s], which (token, s) alone reads and writes, they are the
//     keys greater than the final threshold in front of the segment.
//   * LAUNCH E (mla_indexer_split_emit_kernel) resolves round 3 the same way: T is a whole image, `need` the equals still to take, G_s
//     = carry + the round's share the keys > T in front of the segment, E_s = the front sum of the picked bin the keys == T in front
//     of it. The segment then runs fa_mla_indexer_select's emission loop over its own keys from ng = G_s, ne = E_s: a taken key lands
//     at (greater in front) + min(equals in front, need). The places are those of the one-workgroup kernel: the lists are bit-identical.
//     A segment with G_s + min(E_s, need) >= topk has nothing to write and leaves.
//   * v <= topk: the H launches leave at once, E writes slot(j) for its own positions and the logits are not read. Segment 0 writes the
//     count, whatever v is.
//   * THE WORKSPACE'S PRIOR CONTENTS have no influence: every word read was written earlier in the same call -- a histogram of a
//     segment that starts below v by that segment in the launch before, a state slot by segment 0 (which always starts below v > topk),
//     the carry by its owner -- and histograms of segments at or behind v are skipped by the readers as by their writers.
//   * BOUNDS. Every address is formed from (token < total_q, s < S, bin < 256) and positions < v; an emitted place is additionally held
//     below topk, which it always is when the state is what this call wrote.
#include "fa_mla_indexer_common.h"  // IdxSeq, idx_seq, idx_visible, idx_image, idx_block_scan

namespace fa {

// the words of the workspace, in ints: histograms [4][total_q][S][256], states [4][total_q][2] (three used), carries [total_q][S]
long long mla_indexer_select_split_workspace_ints(long long total_q, int S) { return 4 * total_q * S * 256 + 4 * total_q * 2 + total_q * S; }
// THE SPLIT RULE, on host scalars alone. Two pulls, as in the logits kernel's chunk rule: few tokens must still fill the chip -- 512
// workgroups, two on each of 256 compute units -- and a segment must not be so short that the S * 256 histogram words a workgroup sums
// per launch weigh against the keys it reads: at least 1024 keys wherever the capacity has them (measured: DESIGN.md 4.7w). Never
// more than 64.
int mla_indexer_select_num_splits(int B, int max_seqlen_q, int page_size, int max_pages_per_seq) {
  const long long tokens = (long long)B * max_seqlen_q, cap = (long long)page_size * max_pages_per_seq;
  const long long want = (512 + tokens - 1) / tokens, most = cap / 1024 > 1 ? cap / 1024 : 1;
  const long long s = want < most ? want : most;
  return (int)(s < 64 ? s : 64);
}
int mla_indexer_select_split_seg(int page_size, int max_pages_per_seq, int S) {
  const long long cap = (long long)page_size * max_pages_per_seq;
  return (int)(((cap + S - 1) / S + 63) / 64 * 64);  // (<= 2^30)
}

struct IdxSplitWs {
  int *hist, *state, *carry;
};
__device__ __forceinline__ IdxSplitWs idx_split_ws(const MlaIndexerSelectSplitParams &q) {
  int *h = q.ws;
  int *st = h + 4LL * q.p.total_q * q.S * 256;
  return {h, st, st + 4LL * q.p.total_q * 2};
}

// the workgroup (token, s) of a launch; `live`: the token is somebody's
struct IdxSplitItem {
  IdxSeq sq;
  int b, i, s, v;
  long long tok;
  bool live;
};
__device__ __forceinline__ IdxSplitItem idx_split_item(const MlaIndexerSelectSplitParams &q) {
  const MlaIndexerSelectParams &p = q.p;
  IdxSplitItem it;
  int x = blockIdx.x;
  it.s = x % q.S;
  x /= q.S;
  it.b = x / p.max_q;
  it.i = x - it.b * p.max_q;
  it.sq = idx_seq(p.cu_q, p.seqlens, it.b, p.total_q, p.max_q, p.max_pages << p.lp);
  it.live = it.i < it.sq.Lq;
  it.v = it.live ? idx_visible(it.sq, it.i) : 0;
  it.tok = it.sq.sq + it.i;
  return it;
}

// The pick of round r for token `tok` as segment s sees it, from the histograms the launch before wrote. In: the rank `need` looked for
// among the keys that match the prefix. Out (workgroup-uniform): the digit, the rank inside its bin, and of the keys in the segments in
// front of s the number in greater bins and the number in the picked bin. Segments [0, nseg) are the ones that start below v.
struct IdxPick {
  int bin, need, gfront, efront;
};
__device__ __forceinline__ IdxPick idx_split_resolve(const int *hist_r, int S, int s, int nseg, int need, int *ws, int *pick) {
  const int tid = threadIdx.x, bin = 255 - tid;  // thread order = bins from the top, as in the one-workgroup kernel
  int n = 0, f = 0, k = 0;
  for (; k + 8 <= nseg; k += 8) {  // eight loads in flight: one at a time, the sum is S memory round trips long
    int h[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) h[u] = hist_r[(k + u) * 256 + bin];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      n += h[u];
      f += k + u < s ? h[u] : 0;
    }
  }
  for (; k < nseg; ++k) {
    const int h = hist_r[k * 256 + bin];
    n += h;
    f += k < s ? h : 0;
  }
  if (tid < 4) pick[tid] = 0;  // (a rank nobody holds cannot happen on this call's own histograms; it must not leave garbage either)
  int total, ftotal;
  const int above = idx_block_scan(n, total, ws);  // (barriers inside: pick is cleared before anybody writes it)
  const int fabove = idx_block_scan(f, ftotal, ws);
  if (above < need && need <= above + n) {  // exactly one thread
    pick[0] = bin;
    pick[1] = need - above;
    pick[2] = fabove;
    pick[3] = f;
  }
  __syncthreads();
  return {pick[0], pick[1], pick[2], pick[3]};  // (one resolve per kernel: pick is not written again)
}

template <int K>
__global__ __launch_bounds__(IDX_SEL_THREADS) void mla_indexer_split_hist_kernel(MlaIndexerSelectSplitParams q) {
  __shared__ int hist[256];
  __shared__ int ws[IDX_SEL_THREADS / 64];
  __shared__ int pick[4];
  const MlaIndexerSelectParams &p = q.p;
  const int tid = threadIdx.x, S = q.S;
  const IdxSplitItem it = idx_split_item(q);
  const int v = it.v, topk = p.topk, s = it.s;
  if (!it.live || v <= topk) return;  // nobody's token, or one whose list is every visible key
  const int j0 = s * q.seg;           // (< cap + 64 S)
  if (j0 >= v) return;                // the segment lies behind the token's keys
  const int j1 = min(j0 + q.seg, v), nseg = min(S, (v + q.seg - 1) / q.seg);
  const IdxSplitWs w = idx_split_ws(q);
  const long long T_ = p.total_q, tok = it.tok;

  unsigned T = 0;
  int need = topk;
  if (K >= 1) {
    if (K >= 2) {  // the state after round K - 2: segment 0 wrote it one launch ago
      T = (unsigned)w.state[((K - 2) * T_ + tok) * 2];
      need = w.state[((K - 2) * T_ + tok) * 2 + 1];
    }
    const IdxPick r = idx_split_resolve(w.hist + ((K - 1) * T_ + tok) * S * 256, S, s, nseg, need, ws, pick);
    T |= (unsigned)r.bin << (24 - 8 * (K - 1));
    need = r.need;
    if (tid == 0) {
      if (s == 0) {
        w.state[((K - 1) * T_ + tok) * 2] = (int)T;
        w.state[((K - 1) * T_ + tok) * 2 + 1] = need;
      }
      int *c = w.carry + tok * S + s;
      *c = (K >= 2 ? *c : 0) + r.gfront;
    }
  }

  constexpr int sh = 24 - 8 * K, ph = K == 0 ? 0 : sh + 8;  // the digit's shift, the prefix's (round 0 has no prefix)
  const float *row = p.logits + tok * p.logits_stride;
  hist[tid] = 0;
  __syncthreads();
  auto count = [&](unsigned u) __attribute__((always_inline)) {
    if (K == 0 || (u >> ph) == (T >> ph)) atomicAdd(&hist[(u >> sh) & 255], 1);
  };
  int j = j0 + tid;
  for (; j + 3 * IDX_SEL_THREADS < j1; j += 4 * IDX_SEL_THREADS) {  // four loads in flight
    const float a0 = row[j], a1 = row[j + IDX_SEL_THREADS], a2 = row[j + 2 * IDX_SEL_THREADS], a3 = row[j + 3 * IDX_SEL_THREADS];
    count(idx_image(a0));
    count(idx_image(a1));
    count(idx_image(a2));
    count(idx_image(a3));
  }
  for (; j < j1; j += IDX_SEL_THREADS) count(idx_image(row[j]));
  __syncthreads();
  w.hist[((K * T_ + tok) * S + s) * 256 + tid] = hist[tid];
}

__global__ __launch_bounds__(IDX_SEL_THREADS) void mla_indexer_split_emit_kernel(MlaIndexerSelectSplitParams q) {
  __shared__ int ws[IDX_SEL_THREADS / 64];
  __shared__ int pick[4];
  const MlaIndexerSelectParams &p = q.p;
  const int tid = threadIdx.x, S = q.S;
  const IdxSplitItem it = idx_split_item(q);
  if (!it.live) return;  // nobody's token
  const int v = it.v, topk = p.topk, s = it.s, b = it.b;
  const int lp = p.lp, PM = (1 << lp) - 1;
  const long long T_ = p.total_q, tok = it.tok;
  if (s == 0 && tid == 0) p.counts[tok] = min(topk, v);
  const int j0 = s * q.seg;
  if (j0 >= v) return;
  const int j1 = min(j0 + q.seg, v), nseg = min(S, (v + q.seg - 1) / q.seg);
  int *out = p.indices + tok * p.idx_stride;
  const int *tbl = p.block_table + (long long)b * p.bt_stride;
  // position j < v <= L_b -> its slot (j >> lp < max_pages), -1 under a table entry outside the pool
  auto slot = [&](int j) __attribute__((always_inline)) {
    const int page = tbl[j >> lp];
    return (unsigned)page < (unsigned)p.num_pages ? (page << lp) + (j & PM) : -1;
  };
  if (v <= topk) {  // everything visible is taken: the logits are not read
    for (int j = j0 + tid; j < j1; j += IDX_SEL_THREADS) out[j] = slot(j);
    return;
  }
  const IdxSplitWs w = idx_split_ws(q);
  unsigned T = (unsigned)w.state[(2 * T_ + tok) * 2];
  int need = w.state[(2 * T_ + tok) * 2 + 1];
  const IdxPick r = idx_split_resolve(w.hist + (3 * T_ + tok) * S * 256, S, s, nseg, need, ws, pick);
  T |= (unsigned)r.bin;
  need = r.need;
  int ng = w.carry[tok * S + s] + r.gfront, ne = r.efront;  // greater / equal keys in front of this round's 256
  if (ng + min(ne, need) >= topk) return;                   // (workgroup-uniform) the list is complete in front of this segment
  const float *row = p.logits + tok * p.logits_stride;
  for (int jb = j0; jb < j1; jb += IDX_SEL_THREADS) {
    const int j = jb + tid;
    int gt = 0, eq = 0;
    if (j < j1) {
      const unsigned u = idx_image(row[j]);
      gt = u > T;
      eq = u == T;
    }
    int total;
    const int ex = idx_block_scan(gt | (eq << 16), total, ws);  // (at most 256 of either: sixteen bits each)
    const int g0 = ng + (ex & 0xffff), e0 = ne + (ex >> 16);
    const int at = g0 + min(e0, need);
    if ((gt || (eq && e0 < need)) && (unsigned)at < (unsigned)topk) out[at] = slot(j);
    ng += total & 0xffff;
    ne += total >> 16;
    if (ng + min(ne, need) >= topk) break;  // (workgroup-uniform) the list is complete
  }
}

// ---- the launch chain: H0 .. H3, then E, on one stream; every grid is B * max_seqlen_q * S
hipError_t launch_mla_indexer_select_split(const MlaIndexerSelectSplitParams &q, hipStream_t s) {
  (void)hipGetLastError();
  const dim3 grid((unsigned)((long long)q.p.B * q.p.max_q * q.S)), block(IDX_SEL_THREADS);
  hipLaunchKernelGGL(mla_indexer_split_hist_kernel<0>, grid, block, 0, s, q);
  hipLaunchKernelGGL(mla_indexer_split_hist_kernel<1>, grid, block, 0, s, q);
  hipLaunchKernelGGL(mla_indexer_split_hist_kernel<2>, grid, block, 0, s, q);
  hipLaunchKernelGGL(mla_indexer_split_hist_kernel<3>, grid, block, 0, s, q);
  hipLaunchKernelGGL(mla_indexer_split_emit_kernel, grid, block, 0, s, q);
  return hipGetLastError();
}

}  // namespace fa
