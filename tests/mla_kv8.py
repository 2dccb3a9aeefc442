"""Shared pieces of the tests of fa_fwd_mla_decode_paged_kv8 (absorbed MLA decode over an e4m3 latent pool; include/fa_mi355.h,
"Multi-head latent attention (decode, e4m3 pool)"). The fp64 reference, the fp32 model and the bars are tests/mla.py's and
tests/mla_wide.py's, unchanged, applied to the WIDENED values; the codes and their exact widening are tests/kv8.py's. Here are the twin
pools (an e4m3 pool of bytes and the bf16 pool that holds the same values, NaN in every slot nobody may read), the cases the GPU runs,
and a model of the kernel's widening stage -- byte offsets, the range check, the conversion -- with four plantable mistakes."""
import functools

import numpy as np

import kv8
import mla

DQK, DV = mla.DQK, mla.DV
DTYPE = "bf16"  # the queries' and the output's type, and the twin pool's

# the parity cases (Hq, Nq, causal): always four waves; 1, 16, 17, 32, 33, 35, 64, 65 and 128 rows
SHAPES = [(1, 1, False), (16, 1, False), (17, 1, False), (16, 2, True), (33, 1, False), (5, 7, True), (64, 1, False), (65, 1, False),
          (16, 8, True), (128, 1, False)]
PAGES = mla.PAGES


def codes_of(pool):
    """fp32 pool of e4m3 values with NaN where nobody may read -> the codes, the NaN slots alternating 0x7F / 0xFF"""
    codes = kv8.to_e4m3_bytes(pool)
    nan = np.isnan(pool)
    assert np.array_equal(kv8.widen(codes)[~nan], pool[~nan]), "the pool must hold e4m3 values"
    codes[nan & (np.arange(pool.size).reshape(pool.shape) % 2 == 1)] = 0xFF
    return codes


def make_twins(rng, P, lens, row_stride=DQK, pad_page=False, spare=3, max_pages=None, draw=None, integer=False):
    """(codes uint8 [num_pages, P (+ 1 padding row), row_stride], twin fp32 of the same shape holding the widened values, table, kvs):
    mla.make_pool's construction -- pages a random permutation of the pool, unused table entries on a spare page, every slot past L_b,
    every padding column and row unreadable (0x7F / 0xFF there, NaN in the twin) -- over values drawn on the e4m3 grid."""
    draw = draw or (lambda L: kv8.draw_e4m3(rng, L, DQK))
    npb = [(L + P - 1) // P for L in lens]
    mp = max_pages or max(max(npb), 1)
    num_pages = sum(npb) + spare
    perm = rng.permutation(num_pages)
    pool = np.full((num_pages, P + (1 if pad_page else 0), row_stride), np.nan, np.float32)
    table = np.full((len(lens), mp), perm[-1], np.int32)
    kvs, used = [], 0
    for b, L in enumerate(lens):
        pages = perm[used:used + npb[b]]
        used += npb[b]
        table[b, :npb[b]] = pages
        kv = rng.integers(-4, 5, (L, DQK)).astype(np.float32) if integer else draw(L).astype(np.float32)
        for j, pg in enumerate(pages):
            n = min(P, L - j * P)
            pool[pg, :n, :DQK] = kv[j * P:j * P + n]
        kvs.append(kv)
    codes = codes_of(pool)
    return codes, kv8.widen(codes), table, kvs


@functools.lru_cache(maxsize=None)
def _case(P, shape_idx):
    import oracle

    oracle.build()
    Hq, Nq, causal = SHAPES[shape_idx]
    row_stride, pad_page, token_major, wide_o = mla.LAYOUTS[shape_idx % len(mla.LAYOUTS)]
    rng = np.random.default_rng(2700 + 10 * P + shape_idx)
    lens = [int(x) for x in rng.permutation(mla.lengths(P))]
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, DQK)).astype(np.float32), DTYPE)
    codes, twin, table, kvs = make_twins(rng, P, lens, row_stride, pad_page)
    for a in [q, codes, twin, table] + kvs:
        a.setflags(write=False)  # computed once, shared, left unchanged
    return {"Hq": Hq, "Nq": Nq, "causal": causal, "P": P, "dtype": DTYPE, "lens": lens, "q": q, "codes": codes, "twin": twin, "table": table,
            "kvs": kvs, "token_major": token_major, "wide_o": wide_o}


def case(P, shape_idx):
    """One parity case (inputs built once per process and shared read-only)."""
    return _case(P, shape_idx)


# a case whose values lie mostly below 2^-6, the smallest normal e4m3 value: U(-1, 1) / 64 on the grid (subnormal codes 0x01 .. 0x07 and
# their negatives carry the multiples of 2^-9). Scores of such keys are tiny; the VALUES are what a flush to zero loses.
SMALL_LENS, SMALL_P, SMALL_SHAPE = [5, 64, 200], 16, (16, 1, False)


@functools.lru_cache(maxsize=None)
def small_case():
    import oracle

    oracle.build()
    rng = np.random.default_rng(2799)
    Hq, Nq, causal = SMALL_SHAPE
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (len(SMALL_LENS), Hq, Nq, DQK)).astype(np.float32), DTYPE)
    codes, twin, table, kvs = make_twins(rng, SMALL_P, SMALL_LENS, draw=lambda L: kv8.widen(kv8.to_e4m3_bytes(rng.uniform(-1, 1, (L, DQK)) / 64.0)))
    return {"Hq": Hq, "Nq": Nq, "causal": causal, "P": SMALL_P, "dtype": DTYPE, "lens": SMALL_LENS, "q": q, "codes": codes, "twin": twin,
            "table": table, "kvs": kvs, "token_major": False, "wide_o": False}


# ---- the widening stage: what the kernel reads for key j of a sequence, from the BYTES of the pool
MISTAKES = ("halves_exchanged", "rotary_from_1024", "stride_in_2_bytes", "subnormals_flushed")


def staged(codes, table, lens, P, mistake=None):
    """kvs as the kernel's staging sees them: per sequence fp32 [L_b, 576]. Row r of a page is read at byte r * row_stride under a range
    check of (valid rows - 1) * row_stride + 576 bytes from the page's base (bytes past it read as zeros); 16-byte chunk e of the 512
    latent bytes becomes bf16 chunks 2e, 2e + 1, the 64 rotary bytes sit at byte 512. `mistake` plants one of MISTAKES:
    halves_exchanged: the two bf16 chunks of every e4m3 chunk exchanged (2e <-> 2e + 1); rotary_from_1024: the rotary bytes taken at
    byte 1024 of the row (the bf16 pool's offset); stride_in_2_bytes: row r read at byte 2 r row_stride; subnormals_flushed: codes with
    a zero exponent field widened to 0."""
    num_pages, rows, rs = codes.shape
    out = []
    for b, L in enumerate(lens):
        kv = np.zeros((L, DQK), np.float32)
        for j in range(-(-L // P)):
            page = int(table[b, j])
            nv = min(P, L - j * P)
            flat = codes[page].reshape(-1) if 0 <= page < num_pages else np.zeros(0, np.uint8)
            nrec = (nv - 1) * rs + DQK if flat.size else 0
            view = np.zeros(max(nrec, 0) + 4 * P * rs + 2048, np.uint8)  # (zeros behind the range: what the hardware returns there)
            view[:nrec] = flat[:nrec]
            for r in range(nv):
                base = r * rs * (2 if mistake == "stride_in_2_bytes" else 1)
                lat = view[base:base + DV].copy()
                rot0 = base + (2 * DV if mistake == "rotary_from_1024" else DV)
                row = np.concatenate([lat, view[rot0:rot0 + DQK - DV]])
                if mistake == "subnormals_flushed":
                    row = np.where((row & 0x78) == 0, row & 0x80, row).astype(np.uint8)
                val = kv8.widen(row)
                if mistake == "halves_exchanged":
                    val = val.reshape(-1, 2, 8)[:, ::-1].reshape(-1)
                kv[j * P + r] = val
        out.append(kv)
    return out
