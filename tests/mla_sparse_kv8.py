"""Shared pieces of the tests of fa_fwd_mla_decode_sparse_kv8 (absorbed MLA decode over a list of slots per query token of an e4m3 latent
pool; include/fa_mi355.h, "Multi-head latent attention (decode, sparse, e4m3 pool)"). The fp64 reference, the fp32 model and the bars
are tests/mla.py's (bf16, unchanged) on the WIDENED values; the lists, the gather and its six mistakes are tests/mla_sparse.py's; the
codes, their widening and the four staging mistakes are tests/kv8.py's and tests/mla_kv8.py's. Here are the cases the GPU runs -- an
e4m3 pool of bytes and the bf16 pool that holds the same values, every slot, padding row and padding column that nobody may read 0x7F /
0xFF here and NaN there --, the gathered e4m3 twin pool and table on which fa_fwd_mla_decode_paged_kv8 must return the same bits, and a
model of the kernel's staging that rebuilds every case's key values from the pool's BYTES and the lists, with twelve plantable mistakes:
the six of the gather, the four of the widening stage and two of the combination."""
import functools

import numpy as np

import kv8
import mla
import mla_kv8
import mla_sparse

DQK, DV, SCALE = mla.DQK, mla.DV, mla.SCALE
DTYPE = mla_kv8.DTYPE  # the queries' and the output's type, and the bf16 twin pool's

# the parity cases: tests/mla_sparse.py's, structure and pool sizes (at most 2048 slots), over values on the e4m3 grid
CASES = mla_sparse.CASES
POOL_SLOTS = mla_sparse.POOL_SLOTS


def named_slots(indices, counts, topk, nslots):
    """bool [nslots]: the slots some token's counted entries name"""
    named = np.zeros(nslots, bool)
    for t in range(indices.shape[0]):
        n = topk if counts is None else int(np.clip(counts[t], 0, topk))
        x = indices[t, :n].astype(np.int64)
        named[x[(x >= 0) & (x < nslots)]] = True
    return named


def make_pools(rng, P, nslots, indices, counts, topk, row_stride=DQK, pad_page=False, draw=None):
    """(codes uint8 [num_pages, P (+ 1 padding row), row_stride], twin fp32 of the same shape holding the widened values): values drawn on
    the e4m3 grid in the slots the counted entries name; every other slot, every padding row and column unreadable (0x7F / 0xFF in the
    codes, NaN in the twin). The device view a test passes is [:, :P, :576] of either."""
    draw = draw or (lambda *shape: kv8.draw_e4m3(rng, *shape))
    num_pages = nslots // P
    pool = np.full((num_pages, P + (1 if pad_page else 0), row_stride), np.nan, np.float32)
    pool[:, :P, :DQK] = draw(num_pages, P, DQK)
    pool[:, :P][~named_slots(indices, counts, topk, nslots).reshape(num_pages, P)] = np.nan
    codes = mla_kv8.codes_of(pool)
    return codes, kv8.widen(codes)


def _finish(c):
    """kvs / lens from the bf16 twin through tests/mla_sparse.py's gather; everything read-only"""
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    assert not any(np.isnan(kv).any() for kv in c["kvs"]), "a counted entry names an unreadable slot"
    for a in [c["q"], c["codes"], c["pool"], c["indices"]] + c["kvs"] + ([] if c["counts"] is None else [c["counts"]]):
        a.setflags(write=False)  # computed once, shared, left unchanged
    return c


@functools.lru_cache(maxsize=None)
def _case(idx):
    import oracle

    oracle.build()
    Hq, topk, P, row_stride, pad_page, counted, pitch, kind = CASES[idx]
    rng = np.random.default_rng(3100 + idx)
    nslots = POOL_SLOTS[P]
    counts = np.array(rng.permutation(mla_sparse.counts_for(topk)), np.int32) if counted else None
    if kind == "oob":
        counts = np.array([5, 20, topk], np.int32)  # the three entries outside the pool stand among the first five
    T = 3 if counts is None else len(counts)
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)
    indices = mla_sparse.make_lists(rng, T, topk, pitch, nslots, kind)
    codes, twin = make_pools(rng, P, nslots, indices, counts, topk, row_stride, pad_page)
    # "pool" is the bf16 twin: the dict is a case of tests/mla_sparse.py as its gather and its twin() read one
    return _finish({"Hq": Hq, "topk": topk, "P": P, "dtype": DTYPE, "T": T, "q": q, "codes": codes, "pool": twin, "indices": indices,
                    "counts": counts, "kind": kind})


def case(idx):
    """One parity case (inputs built once per process and shared read-only)."""
    return _case(idx)


# a case whose values lie mostly below 2^-6, the smallest normal e4m3 value (tests/mla_kv8.py's small case, under a list)
@functools.lru_cache(maxsize=None)
def small_case():
    import oracle

    oracle.build()
    rng = np.random.default_rng(3199)
    Hq, topk, P, nslots, T = 16, 200, 16, 1024, 3
    counts = np.array([5, 64, 200], np.int32)
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)
    indices = mla_sparse.make_lists(rng, T, topk, topk, nslots, "perm")
    codes, twin = make_pools(rng, P, nslots, indices, counts, topk,
                             draw=lambda *shape: kv8.widen(kv8.to_e4m3_bytes(rng.uniform(-1, 1, shape) / 64.0)))
    return _finish({"Hq": Hq, "topk": topk, "P": P, "dtype": DTYPE, "T": T, "q": q, "codes": codes, "pool": twin, "indices": indices,
                    "counts": counts, "kind": "perm"})


def twin8(c, rng, spare=2):
    """(codes uint8 [pages, 64, 576], table int32 [T, cap / 64], lens): the e4m3 pool of 64-row pages on which
    fa_fwd_mla_decode_paged_kv8(B = T, Nq = 1, max_pages_per_seq = cap / 64, is_causal = 0, seqlens_k = n) must return the sparse call's
    bits -- tests/mla_sparse.py's twin in codes: row j of token t in slot j % 64 of page table[t][j / 64], entries outside the pool as zero
    rows, 0x7F / 0xFF wherever no list entry lives, pages in random order."""
    pool, table, lens = mla_sparse.twin(c, rng, spare)
    return mla_kv8.codes_of(pool), table, lens


# ---- the staging: what the kernel reads for entry j of a token, from the BYTES of the pool and the lists
OWN_MISTAKES = ("offset_doubled", "oob_reads_offset0")
MISTAKES = mla_sparse.MISTAKES + mla_kv8.MISTAKES + OWN_MISTAKES


def staged(c, mistake=None):
    """kvs as the kernel's staging sees them, per token fp32 [n_t, 576], and the lengths n_t. Entry x of the first n_t names the 576 bytes
    at byte (x // P) * page_stride + (x % P) * row_stride of the pool: sixteen-byte chunk e of the 512 latent bytes becomes bf16 chunks
    2e, 2e + 1, the 64 rotary bytes sit at byte 512; an entry outside [0, num_pages * P) is a row of zeros and no address is formed.
    Bytes behind the pool's end read as zeros here (a wrong address must read something). `mistake` plants one of MISTAKES: the six of
    tests/mla_sparse.py's gather (pitch_topk, token0_list, count_ignored, row_stride_only, page_row_swapped, oob_clamped), the four of
    tests/mla_kv8.py's stage (halves_exchanged, rotary_from_1024, stride_in_2_bytes: the row's part of the offset doubled,
    subnormals_flushed), and two of the combination:
    offset_doubled:    the slot's whole byte offset doubled (the bf16 kernel's * 2)
    oob_reads_offset0: an entry outside the pool read as the bytes at offset 0 instead of zeros"""
    assert mistake is None or mistake in MISTAKES
    codes, idx, P, topk = c["codes"], c["indices"], c["P"], c["topk"]
    ps, rs = codes.shape[1] * codes.shape[2], codes.shape[2]
    flat, nslots = codes.reshape(-1), codes.shape[0] * P
    flat_idx = idx.reshape(-1)

    def rd(a, n):
        out = np.zeros(n, np.uint8)
        seg = flat[a:a + n]
        out[:seg.size] = seg
        return out

    kvs, lens = [], []
    for t in range(c["T"]):
        n = topk if (c["counts"] is None or mistake == "count_ignored") else int(np.clip(c["counts"][t], 0, topk))
        rows = np.zeros((n, DQK), np.float32)
        for j in range(n):
            x = int(idx[0, j] if mistake == "token0_list" else flat_idx[t * topk + j] if mistake == "pitch_topk" else idx[t, j])
            if not 0 <= x < nslots:
                if mistake == "oob_clamped":
                    x = min(max(x, 0), nslots - 1)
                elif mistake == "oob_reads_offset0":
                    x = 0
                else:
                    continue
            if mistake == "row_stride_only":
                a = x * rs
            elif mistake == "page_row_swapped":
                a = (x % P) * ps + (x // P) * rs
            elif mistake == "stride_in_2_bytes":
                a = (x // P) * ps + 2 * (x % P) * rs
            else:
                a = mla_sparse.row_offset(x, P, ps, rs)
            if mistake == "offset_doubled":
                a *= 2
            row = np.concatenate([rd(a, DV), rd(a + (2 * DV if mistake == "rotary_from_1024" else DV), DQK - DV)])
            if mistake == "subnormals_flushed":
                row = np.where((row & 0x78) == 0, row & 0x80, row).astype(np.uint8)
            val = kv8.widen(row)
            if mistake == "halves_exchanged":
                val = val.reshape(-1, 2, 8)[:, ::-1].reshape(-1)
            rows[j] = val
        kvs.append(rows)
        lens.append(n)
    return kvs, lens
