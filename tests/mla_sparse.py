"""Shared pieces of the tests of fa_fwd_mla_decode_sparse (absorbed MLA decode over a list of keys per query token; include/fa_mi355.h,
"Multi-head latent attention (decode, sparse)"). Pools are the family's layout, the fp64 reference, the fp32 model and the bars are
tests/mla.py's, unchanged: here are the gather that turns a list into the kvs[t] those helpers take (B = T, Nq = 1, not causal), the twin
pool and table on which fa_fwd_mla_decode_paged_wide must return the same bits, the cases the GPU runs, and six mistakes a gather kernel
can make, planted in the gather."""
import functools

import numpy as np

import mla

DQK, DV, SCALE = mla.DQK, mla.DV, mla.SCALE
INT_MAX = 2 ** 31 - 1

# the parity cases: (Hq, topk, P, pool row stride, padded page stride, counts given, list pitch, kind of list)
#   counts given: tokens with the counts {0, 1, 63, 64, 65, topk - 1, topk} that topk allows, in random order; else index_counts = NULL and
#   three tokens with full lists
#   kind: "perm" a random permutation of slots across all pages, "dup" slots drawn with repetition from a few, "run" consecutive slots from
#   a random start, "oob" a permutation with -1, num_pages * P and INT_MAX among every token's first entries
CASES = [(1, 1, 16, 576, False, True, 4, "perm"),         # counts 0 and 1
         (16, 63, 64, 640, True, True, 64, "perm"),      # a list pitch above topk, padded rows and pages
         (17, 64, 256, 576, True, True, 64, "dup"),
         (33, 65, 16, 640, False, True, 72, "perm"),     # a lone row in the third wave; two tiles, the second with one entry
         (64, 320, 64, 576, False, True, 320, "perm"),   # five tiles
         (65, 320, 256, 640, True, False, 384, "run"),
         (128, 320, 16, 576, True, True, 320, "perm"),
         (16, 320, 64, 576, False, True, 320, "run"),
         (16, 65, 64, 640, True, True, 68, "oob")]
POOL_SLOTS = {16: 1024, 64: 2048, 256: 2048}  # slots of a case's pool (at most 8192)


def counts_for(topk):
    return sorted({min(c, topk) for c in (0, 1, 63, 64, 65, topk - 1, topk)})


def row_offset(x, P, page_stride, row_stride):
    """element offset of slot x = page * P + row in the pool's storage"""
    return (x // P) * page_stride + (x % P) * row_stride


MISTAKES = ("pitch_topk", "token0_list", "count_ignored", "row_stride_only", "page_row_swapped", "oob_clamped")


def gather(c, mistake=None):
    """kvs[t] fp32 [n_t, 576] and the lengths n_t: the rows token t's list names, in list order, an entry outside the pool as a row of
    zeros. `mistake` plants one of MISTAKES:
    pitch_topk:       the list read at a pitch of topk instead of indices_stride
    token0_list:      every token reads token 0's list (under its own count)
    count_ignored:    the count ignored: all topk entries used
    row_stride_only:  the slot's address formed as x * kv_row_stride (wrong wherever the page stride is not P row strides)
    page_row_swapped: x >> lp and x & (P - 1) exchanged
    oob_clamped:      an entry outside the pool clamped to the nearest real slot instead of read as zeros"""
    pool, idx, P, topk = c["pool"], c["indices"], c["P"], c["topk"]
    ps, rs = pool.shape[1] * pool.shape[2], pool.shape[2]
    flat, nslots = pool.reshape(-1), pool.shape[0] * P
    flat_idx = idx.reshape(-1)
    kvs, lens = [], []
    for t in range(c["T"]):
        n = topk if (c["counts"] is None or mistake == "count_ignored") else int(np.clip(c["counts"][t], 0, topk))
        rows = np.zeros((n, DQK), np.float32)
        for j in range(n):
            x = int(idx[0, j] if mistake == "token0_list" else flat_idx[t * topk + j] if mistake == "pitch_topk" else idx[t, j])
            if not 0 <= x < nslots:
                if mistake != "oob_clamped":
                    continue
                x = min(max(x, 0), nslots - 1)
            if mistake == "row_stride_only":
                a = x * rs
            elif mistake == "page_row_swapped":
                a = (x % P) * ps + (x // P) * rs
            else:
                a = row_offset(x, P, ps, rs)
            if a + DQK <= flat.size:
                rows[j] = flat[a:a + DQK]
        kvs.append(rows)
        lens.append(n)
    return kvs, lens


def twin(c, rng, spare=2):
    """(pool fp32 [pages, 64, 576], table int32 [T, cap / 64], lens): the pool of 64-row pages on which fa_fwd_mla_decode_paged_wide(B = T,
    Nq = 1, max_pages_per_seq = cap / 64, seqlens_k = n) must return the sparse call's bits: row j of token t in slot j % 64 of page
    table[t][j / 64], entries outside the pool as zero rows, NaN wherever no list entry lives, pages in random order."""
    kvs, lens = gather(c)
    mp = -(-c["topk"] // 64)
    num_pages = c["T"] * mp + spare
    perm = rng.permutation(num_pages)
    pool = np.full((num_pages, 64, DQK), np.nan, np.float32)
    table = perm[:c["T"] * mp].reshape(c["T"], mp).astype(np.int32)
    for t, kv in enumerate(kvs):
        for j0 in range(0, lens[t], 64):
            pool[table[t, j0 // 64], :min(64, lens[t] - j0)] = kv[j0:j0 + 64]
    return pool, table, lens


def make_lists(rng, T, topk, pitch, nslots, kind, tail=None):
    """indices int32 [T, pitch]: the first topk entries of a row by `kind`; behind them whatever `tail` says (default: valid slots)"""
    idx = rng.integers(0, nslots, (T, pitch)).astype(np.int32) if tail is None else np.full((T, pitch), tail, np.int32)
    for t in range(T):
        if kind in ("perm", "oob"):
            row = rng.permutation(nslots)[:topk] if topk <= nslots else rng.integers(0, nslots, topk)
        elif kind == "dup":
            row = rng.choice(rng.permutation(nslots)[:7], topk)  # seven slots, each named about topk / 7 times
        else:
            row = (int(rng.integers(0, nslots)) + np.arange(topk)) % nslots
        idx[t, :topk] = row
        if kind == "oob":
            idx[t, [0, 2, 3]] = [-1, nslots, INT_MAX]
    return idx


def make_pool(oracle, rng, P, nslots, dtype, row_stride=DQK, pad_page=False):
    """pool fp32 [num_pages, P (+ 1 padding row), row_stride]: every slot holds values of the type, padding rows and columns are NaN. The
    device view a test passes is pool[:, :P, :576]."""
    num_pages = nslots // P
    pool = np.full((num_pages, P + (1 if pad_page else 0), row_stride), np.nan, np.float32)
    pool[:, :P, :DQK] = oracle.round_to(rng.uniform(-1.0, 1.0, (num_pages, P, DQK)).astype(np.float32), dtype)
    return pool


@functools.lru_cache(maxsize=None)
def _case(idx, dtype):
    import oracle

    oracle.build()
    Hq, topk, P, row_stride, pad_page, counted, pitch, kind = CASES[idx]
    rng = np.random.default_rng(3000 + idx)
    nslots = POOL_SLOTS[P]
    counts = np.array(rng.permutation(counts_for(topk)), np.int32) if counted else None
    if kind == "oob":
        counts = np.array([5, 20, topk], np.int32)  # the three entries outside the pool stand among the first five
    T = 3 if counts is None else len(counts)
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), dtype)
    pool = make_pool(oracle, rng, P, nslots, dtype, row_stride, pad_page)
    indices = make_lists(rng, T, topk, pitch, nslots, kind)
    c = {"Hq": Hq, "topk": topk, "P": P, "dtype": dtype, "T": T, "q": q, "pool": pool, "indices": indices, "counts": counts, "kind": kind}
    c["kvs"], c["lens"] = gather(c)
    for a in [q, pool, indices] + c["kvs"] + ([] if counts is None else [counts]):
        a.setflags(write=False)  # computed once, shared, left unchanged
    return c


def case(idx, dtype):
    """One parity case (inputs built once per process and shared read-only)."""
    return _case(idx, dtype)


def q4(q):
    """q [T, Hq, 576] as the [B = T, Hq, Nq = 1, 576] the helpers of tests/mla.py take"""
    return q[:, :, None, :]
