"""The cases of tests/varlen_paged.py are what they claim to be (CPU, numpy only): every length sits on the stated side of each edge,
the rows without a visible key and the spare / NaN / out-of-range pages are where the GPU tests expect them, and a numpy gather of a
pool through its table gives back each sequence's K / V."""
import numpy as np
import pytest

import varlen_paged as vp


def _round(x, dtype):  # the cases need representable values only on the GPU; here any fp32 does
    return x


def test_base_batch_sits_on_its_edges():
    b = vp.BASE
    assert len(b) == 9 and b[0] == (1, 1)
    Lq, L = b[1]
    assert Lq == L == 17 and 16 < L < 32 and vp.pages_of(L, 16) == 2 and L % 16 == 1          # one key past the 16-slot page
    Lq, L = b[2]
    assert (Lq, L) == (33, 15) and L < 16 and vp.pages_of(L, 16) == 1                         # a partial first page
    assert vp.dead_rows(Lq, L, True) == 18 and vp.dead_rows(Lq, L, False) == 0                # rows 0-17 see no key under the mask
    assert Lq > vp.WAVE and vp.dead_rows(Lq, L, True) < vp.WAVE                               # the first wave holds dead and live rows
    Lq, L = b[3]
    assert Lq == vp.TILE and L == 200 and L % vp.TILE != 0 and L // vp.TILE == 3              # whole tiles and a ragged fourth
    Lq, L = b[4]
    assert Lq == L == vp.BLOCK + 1                                                            # a second block holding one row
    Lq, L = b[5]
    assert Lq == vp.BLOCK + 2 and L == 401 and L % 16 == 1 and L % vp.TILE == 17              # the last key alone in its page at P = 16
    Lq, L = b[6]
    assert L == 0 and Lq > 0 and vp.dead_rows(Lq, L, False) == Lq == vp.dead_rows(Lq, L, True)
    Lq, L = b[7]
    assert Lq == 0 and L > 0
    Lq, L = b[8]
    assert Lq == vp.BLOCK and L == 16 * vp.TILE                                               # sixteen tiles, four full waves
    assert vp.pages_of(L, 16) == 64 and vp.pages_of(L, 256) == 4
    # which sequences carry the bit-identity claim
    assert [vp.identity_claimed(q, k, True) for q, k in b] == [True, True, False, True, True, True, False, False, True]
    assert [vp.identity_claimed(q, k, False) for q, k in b] == [True, True, True, True, True, True, False, False, True]
    # lengths on both sides of every page size in use
    for P in vp.PAGE_SIZES:
        assert any(0 < k < P for _, k in b) and any(k > P for _, k in b), P
    assert max(q for q, _ in b) > vp.BLOCK and sum(q for q, _ in b) == 507


def test_heads_cover_grouping():
    assert set(vp.HEADS) == {(4, 4), (8, 2), (4, 1)} and all(hq % hkv == 0 for hq, hkv in vp.HEADS)
    assert {hq // hkv for hq, hkv in vp.HEADS} == {1, 4}


@pytest.mark.parametrize("P", vp.PAGE_SIZES)
@pytest.mark.parametrize("order", ["random", "table"])
def test_gather_through_the_table_gives_back_the_sequences(P, order):
    rng = np.random.default_rng(P)
    Hq, Hkv, D = 8, 2, 64
    seqs = vp.draw_seqs(_round, rng, Hq, Hkv, D, "f16", vp.BASE)
    ks, vs = [s[1] for s in seqs], [s[2] for s in seqs]
    pool = vp.build_pool(ks, vs, P, rng=rng if order == "random" else None, spare=3)
    npb = [vp.pages_of(L, P) for _, L in vp.BASE]
    assert pool["num_pages"] == sum(npb) + 3 and pool["table"].shape == (len(vp.BASE), max(npb))
    used = [pg for ids in pool["pages"] for pg in ids]
    assert len(set(used)) == len(used) == sum(npb) and not set(used) & set(pool["spare"])      # every page has one owner
    if order == "table":
        assert used == list(range(sum(npb)))
    else:
        assert used != sorted(used)
    for b, (_, L) in enumerate(vp.BASE):
        assert np.array_equal(vp.gather(pool["k"], pool["table"][b], L, P), ks[b])
        assert np.array_equal(vp.gather(pool["v"], pool["table"][b], L, P), vs[b])
        assert (pool["table"][b, npb[b]:] == pool["spare"][-1]).all()                          # unused entries name a spare page
        if L % P:                                                                              # slots >= L_b of the last page are NaN
            last = pool["pages"][b][-1]
            assert np.isnan(pool["k"][last, :, L % P:]).all() and np.isfinite(pool["k"][last, :, :L % P]).all()
    for pg in pool["spare"]:
        assert np.isnan(pool["k"][pg]).all() and np.isnan(pool["v"][pg]).all()


def test_unused_entries_and_fill_variants():
    rng = np.random.default_rng(1)
    seqs = vp.draw_seqs(_round, rng, 4, 2, 64, "f16", [(3, 20), (5, 100)])
    ks, vs = [s[1] for s in seqs], [s[2] for s in seqs]
    clean = vp.build_pool(ks, vs, 16, fill=0.0, unused="zero", spare=2)
    assert np.isfinite(clean["k"]).all() and (clean["table"][0, 2:] == 0).all()
    for how, val in (("minus1", -1), ("beyond", clean["num_pages"]), ("spare", clean["spare"][-1])):
        p = vp.build_pool(ks, vs, 16, fill=np.nan, unused=how, spare=2)
        assert (p["table"][0, 2:] == val).all() and (p["table"][1] >= 0).all()
        assert np.array_equal(p["table"][:, :2], clean["table"][:, :2])                        # the used entries do not depend on the variant
        assert np.array_equal(np.nan_to_num(p["k"], nan=0.0), clean["k"])                      # the same pool but for what nobody reads
    # an out-of-range entry INSIDE the used range reads as zeros
    p = vp.build_pool(ks, vs, 16, fill=0.0, unused="zero")
    row = p["table"][1].copy()
    row[2] = p["num_pages"]
    g = vp.gather(p["k"], row, 100, 16)
    assert (g[:, 32:48] == 0).all() and np.array_equal(g[:, :32], ks[1][:, :32]) and np.array_equal(g[:, 48:], ks[1][:, 48:])


def test_append_positions_and_chunks():
    assert vp.append_positions(3, 10, 64) == [7, 8, 9]
    assert vp.append_positions(3, 2, 64) == [None, 0, 1]                                      # a position below 0 is skipped
    assert vp.append_positions(4, 66, 64) == [62, 63, None, None]                             # at or above the capacity
    assert vp.append_positions(0, 5, 64) == []
    c = vp.chunks(300, 48)
    assert c[0] == (0, 48) and c[-1] == (288, 12) and sum(n for _, n in c) == 300 and len(c) == 7
    # 48 = three 16-slot pages: every chunk starts on a page edge, most of them inside a 64-key tile; the last one is ragged
    assert not any(s % 16 for s, _ in c) and any(s % vp.TILE for s, _ in c) and c[-1][1] % 16
    qs, cu = vp.pack_rows([np.ones((2, 3, 8), np.float32), np.ones((2, 0, 8), np.float32), np.ones((2, 5, 8), np.float32)], tail=4)
    assert qs.shape == (12, 2, 8) and list(cu) == [0, 3, 3, 8] and (qs[8:] == 0).all()
