"""Shared pieces of the tests of fa_fwd_mla_decode_sparse_kv8_scaled and fa_mla_kv_append_paged_scaled (include/fa_mi355.h, "656-byte
rows"): the row layout in numpy -- pack, the stated dequantisation, the append's quantisation -- and the pools the GPU cases run on: a
pool of BYTES and its dequantised twin [num_pages, P, 576] on which fa_fwd_mla_decode_sparse (bf16) must return the same bits. The lists,
the gather and the fp64 bars are tests/mla_sparse.py's and tests/mla.py's, unchanged."""
import functools

import numpy as np

import kv8
import mla
import mla_sparse

DQK, DV, SCALE, DTYPE = mla.DQK, mla.DV, mla.SCALE, "bf16"
ROW, SC0, ROT0 = 656, 512, 528  # bytes of a row; byte of its first scale / first rotary element

# (Hq, topk, P, row stride, padded page, counts given, list pitch, kind of list, power-of-two scales): tests/mla_sparse.py's columns
CASES = [(1, 1, 16, 656, False, True, 4, "perm", True),
         (16, 63, 256, 720, True, True, 64, "perm", False),
         (17, 64, 16, 656, True, True, 68, "dup", True),
         (64, 65, 256, 720, False, True, 72, "oob", False),
         (128, 130, 16, 656, False, False, 132, "perm", False),   # index_counts = NULL; three tiles, the last with two entries
         (16, 2048, 256, 656, False, True, 2052, "perm", True)]   # eight splits; counts 65 / 2048 / 1000: empty splits
POOL_SLOTS = {16: 1024, 256: 8192}


def bf16_bits(x):
    """fp32 values that are bf16 values -> their 16 bits"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def pack(codes, scales, rotary):
    """codes uint8 [n, 512], scales fp32 [n, 4], rotary fp32 [n, 64] holding bf16 values -> rows uint8 [n, 656]"""
    rows = np.empty((codes.shape[0], ROW), np.uint8)
    rows[:, :SC0] = codes
    rows[:, SC0:ROT0] = np.ascontiguousarray(scales, "<f4").view(np.uint8).reshape(-1, 16)
    rows[:, ROT0:] = bf16_bits(rotary).astype("<u2").view(np.uint8).reshape(-1, 128)
    return rows


def dequant(oracle, rows):
    """rows uint8 [n, 656] -> the keys' values fp32 [n, 576] by the stated rule: latent element d is bf16_rne(fp32(code d) * s[d // 128]),
    ONE fp32 multiply, then one rounding; the rotary elements are their bits"""
    s = np.ascontiguousarray(rows[:, SC0:ROT0]).view("<f4")  # [n, 4]
    with np.errstate(invalid="ignore"):
        lat = oracle.round_to(kv8.widen(rows[:, :SC0]) * np.repeat(s, 128, axis=1), "bf16")
    rot = (np.ascontiguousarray(rows[:, ROT0:]).view("<u2").astype(np.uint32) << 16).view(np.float32)
    return np.concatenate([lat, rot], axis=1)


def quantise(x):
    """fa_mla_kv_append_paged_scaled in numpy: x fp32 [n, 576] holding finite bf16 values -> rows uint8 [n, 656]. Per group of 128 latent
    elements e = the smallest integer in [-32, 32] with amax <= 448 * 2^e (frexp: amax = m * 2^k, 0.5 <= m < 1, and 448 = 0.875 * 2^9),
    s = 2^e, code = e4m3_rne(clamp(x * 2^-e, -448, 448)); every step is exact in fp32"""
    g = np.abs(x[:, :DV].reshape(-1, 4, 128)).max(-1)
    m, k = np.frexp(g)
    e = np.clip(np.where(g == 0, -32, k - 9 + (m > 0.875)), -32, 32).astype(np.int32)
    y = np.clip(x[:, :DV].astype(np.float32) * np.repeat(np.ldexp(np.float32(1), -e).astype(np.float32), 128, axis=1), -448.0, 448.0)
    return pack(kv8.to_e4m3_bytes(y), np.ldexp(np.float32(1), e).astype(np.float32), x[:, DV:])


def draw_rows(oracle, rng, n, pow2):
    """n rows whose VALUES are about U(-1, 1) while the scales differ by three orders of magnitude between the four groups of a row and
    between rows (2^-8 .. 2^3, powers of two or amax / 448-style): a scale of the wrong group or row shows"""
    exps = rng.permuted(np.tile(np.arange(-8, 4), (n, 1)), axis=1)[:, :4]  # (no two groups of a row alike)
    s = np.ldexp(np.float32(1) if pow2 else rng.uniform(1.0, 2.0, (n, 4)).astype(np.float32), exps).astype(np.float32)
    codes = kv8.to_e4m3_bytes(np.clip(rng.uniform(-1.0, 1.0, (n, DV)).astype(np.float32) / np.repeat(s, 128, axis=1), -448, 448))
    return pack(codes, s, oracle.round_to(rng.uniform(-1.0, 1.0, (n, DQK - DV)).astype(np.float32), "bf16"))


def unread(shape, flip=False):
    """what no list may read: e4m3 NaN codes, NaN scales, NaN rotary elements -- every byte 0xFF; flip: 0x7F codes and the other NaN"""
    a = np.full(shape, 0x7F if flip else 0xFF, np.uint8)
    if flip and shape[-1] >= ROW:
        a[..., SC0:ROT0] = np.tile(np.array([0x01, 0x00, 0xC0, 0x7F], np.uint8), 4)  # fp32 NaN 0x7FC00001
        a[..., ROT0 + 1:ROW:2] = 0x7F
        a[..., ROT0:ROW:2] = 0xC1  # bf16 NaN 0x7FC1
    return a


def make_pool(oracle, rng, P, nslots, indices, counts, topk, row_stride=ROW, pad_page=False, pow2=True):
    """(pool uint8 [num_pages, P (+ 1 padding row), row_stride], named bool [nslots], twin fp32 [num_pages, P, 576]): drawn rows in the
    slots the counted entries name, `unread` bytes everywhere else (NaN in the twin). The device view is pool[:, :P, :656]."""
    import mla_sparse_kv8

    num_pages = nslots // P
    named = mla_sparse_kv8.named_slots(indices, counts, topk, nslots)
    pool = unread((num_pages, P + (1 if pad_page else 0), row_stride))
    rows = draw_rows(oracle, rng, int(named.sum()), pow2)
    pool[:, :P, :ROW][named.reshape(num_pages, P)] = rows
    twin = np.full((nslots, DQK), np.nan, np.float32)
    twin[named] = dequant(oracle, rows)
    return pool, named, twin.reshape(num_pages, P, DQK)


def refill(pool, named, P):
    """the pool with everything no list names -- unnamed slots, padding rows, the bytes between rows -- exchanged for the other fill"""
    other = unread(pool.shape, flip=True)
    keep = named.reshape(pool.shape[0], P)
    other[:, :P, :ROW][keep] = pool[:, :P, :ROW][keep]
    return other


@functools.lru_cache(maxsize=None)
def case(idx):
    """One parity case (built once per process, shared read-only): a case of tests/mla_sparse.py -- "pool" is the dequantised twin, as
    its gather reads one -- with the pool of bytes under "bytes" and the named slots under "named" """
    import oracle

    oracle.build()
    Hq, topk, P, row_stride, pad_page, counted, pitch, kind, pow2 = CASES[idx]
    rng = np.random.default_rng(3400 + idx)
    nslots = POOL_SLOTS[P]
    counts = np.array(rng.permutation(mla_sparse.counts_for(topk)), np.int32) if counted else None
    if kind == "oob":
        counts = np.array([5, 20, topk], np.int32)  # the three entries outside the pool stand among the first five
    if topk == 2048:
        counts = np.array([65, 2048, 1000], np.int32)
    T = 3 if counts is None else len(counts)
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)
    indices = mla_sparse.make_lists(rng, T, topk, pitch, nslots, kind)
    pool, named, twin = make_pool(oracle, rng, P, nslots, indices, counts, topk, row_stride, pad_page, pow2)
    c = {"Hq": Hq, "topk": topk, "P": P, "dtype": DTYPE, "T": T, "q": q, "bytes": pool, "named": named, "pool": twin, "indices": indices,
         "counts": counts, "kind": kind}
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    assert not any(np.isnan(kv).any() for kv in c["kvs"]), "a counted entry names an unreadable slot"
    for a in [q, pool, named, twin, indices] + c["kvs"] + ([] if counts is None else [counts]):
        a.setflags(write=False)
    return c
