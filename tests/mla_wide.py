"""Shared pieces of the tests of fa_fwd_mla_decode_paged_wide (absorbed MLA decode, up to 128 packed rows in workgroups of two or four
waves over one shared tile; include/fa_mi355.h, "Multi-head latent attention (decode, wide)"). Pools, the fp64 reference, the fp32 model
and the bars are tests/mla.py's, unchanged; here are the cases, the configurations of the bit-identity test against the one-wave call,
and three mistakes this kernel can make that the one-wave kernel cannot, planted as row maps around mla.model."""
import functools

import numpy as np

import mla

# the parity cases (Hq, Nq, causal). NW = 2 up to 32 rows, 4 above; a workgroup row block is 16 NW rows
SHAPES = [(33, 1, False),   # NW = 4: one live row in the third wave, a padding wave with no workspace slot
          (17, 1, False),   # NW = 2
          (16, 2, True),    # NW = 2, both waves full
          (16, 3, True),    # 48 rows
          (5, 7, True),     # 35 rows: neither 16 nor the head count divides evenly
          (64, 1, False),   # one full block
          (65, 1, False),   # a second block with one row
          (64, 2, True),    # two full blocks
          (16, 8, True),    # 128 rows, eight tokens
          (128, 1, False)]  # 128 heads
PAGES = mla.PAGES


def waves(rows):
    return 2 if rows <= 32 else 4


@functools.lru_cache(maxsize=None)
def _case(P, dtype, shape_idx):
    import oracle

    oracle.build()
    Hq, Nq, causal = SHAPES[shape_idx]
    row_stride, pad_page, token_major, wide_o = mla.LAYOUTS[shape_idx % len(mla.LAYOUTS)]
    rng = np.random.default_rng(2600 + 10 * P + shape_idx)
    lens = [int(x) for x in rng.permutation(mla.lengths(P))]
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, mla.DQK)).astype(np.float32), dtype)
    pool, table, kvs = mla.make_pool(oracle, rng, P, lens, dtype, row_stride, pad_page)
    for a in [q, pool, table] + kvs:
        a.setflags(write=False)  # computed once, shared, left unchanged
    return {"Hq": Hq, "Nq": Nq, "causal": causal, "P": P, "dtype": dtype, "lens": lens, "q": q, "pool": pool, "table": table, "kvs": kvs,
            "token_major": token_major, "wide_o": wide_o}


def case(P, dtype, shape_idx):
    """One parity case (inputs built once per process and shared read-only)."""
    return _case(P, dtype, shape_idx)


# ---- bit-identity with the one-wave call. Both calls run the same per-wave text on the same tiles, so wherever both split the keys of a
# sequence alike, the wide call's rows must carry the one-wave call's bits. The split count comes from (B, row blocks fed to the rule,
# capacity) alone: the wide call feeds ceil(rows / (16 NW)) workgroup blocks, the one-wave call ceil(rows / 16).
# (Hq, Nq, causal) of the wide call -> heads per one-wave call (its Hq; Nq is shared), so that both feed the rule the same block count
BITID = [((64, 1, False), 16),   # NW = 4, one block           | one-wave call on 16 rows: one block
         ((32, 1, False), 16),   # NW = 2, one block           | 16 rows: one block
         ((16, 2, True), 8),     # NW = 2, one block, causal   | 8 heads x 2 tokens = 16 rows: one block
         ((128, 1, False), 32),  # NW = 4, two blocks          | 32 rows: two blocks
         ((16, 2, True), 16)]    # the same tensors through both calls, at a capacity where both rules give one S (BITID_SAME_*)
BITID_P, BITID_LENS = 64, [4097, 1000, 65, 0, 4160]  # 65 tiles of 64 keys (66 with a ragged end); capacity 66 pages
BITID_MAX_PAGES = 66
BITID_SAME_LENS, BITID_SAME_MAX_PAGES = [1024, 1000, 65, 0, 513], 16  # capacity 1024 keys = 16 tiles: S = min(ceil(256 / (5 blocks)), 16 / 4) = 4


def bitid_capacity(i):
    """(lens, max_pages) of BITID[i]"""
    return (BITID_SAME_LENS, BITID_SAME_MAX_PAGES) if i == len(BITID) - 1 else (BITID_LENS, BITID_MAX_PAGES)


# ---- three mistakes of the multi-wave kernel, as row maps around the model
MISTAKES = ("wave_dropped", "block_base", "iq_in_wave")


def model(oracle, q, kvs, lens, causal, scale, dtype, mistake=None):
    """mla.model, or what a kernel with one of MISTAKES would return: (O fp32 [B,Hq,Nq,512], LSE fp32 [B,Hq,Nq]).
    wave_dropped: the wave index left out of the row, r = 16 NW wb + c: rows 16 .. 16 NW - 1 of a block repeat its rows 0 .. 15.
    block_base:   the block's first row taken as 16 wb instead of 16 NW wb (a row past Hq Nq is a padding row: dead).
    iq_in_wave:   the causal limit from the row inside the wave, iq = c % Nq instead of r % Nq."""
    B, Hq, Nq, _ = q.shape
    R = Hq * Nq
    if mistake is None:
        return mla.model(oracle, q, kvs, lens, causal, scale, dtype)
    nw = waves(R)
    r = np.arange(R)
    if mistake == "iq_in_wave":
        # every packed row as a head of its own with its content at all Nq positions: [b, r, i] is row r under the causal limit of token i
        big = np.repeat(q.reshape(B, R, 1, mla.DQK), Nq, axis=2)
        ob, lb = mla.model(oracle, big, kvs, lens, causal, scale, dtype)
        wrong = (r % 16) % Nq
        return ob[:, r, wrong].reshape(B, Hq, Nq, mla.DV), lb[:, r, wrong].reshape(B, Hq, Nq)
    o, lse = mla.model(oracle, q, kvs, lens, causal, scale, dtype)
    wb, inblk = r // (16 * nw), r % (16 * nw)
    src = 16 * nw * wb + inblk % 16 if mistake == "wave_dropped" else 16 * wb + inblk
    pad = src >= R
    src = np.where(pad, 0, src)
    of, lf = o.reshape(B, R, mla.DV)[:, src].copy(), lse.reshape(B, R)[:, src].copy()
    of[:, pad], lf[:, pad] = 0.0, -np.inf
    return of.reshape(B, Hq, Nq, mla.DV), lf.reshape(B, Hq, Nq)
