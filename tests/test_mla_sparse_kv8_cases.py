"""CPU: the cases tests/test_gpu_mla_decode_sparse_kv8.py runs and the bars they are held to (tests/mla.py's bf16 bars, unchanged, on the
widened values), checked without a GPU. The fp64 reference on the kernel's pre-scaled operand and the fp32 model of the kernel's
arithmetic stay inside every bar on every case, so the bars can be held; the model of the staging (tests/mla_sparse_kv8.py) reproduces
every case's values from the pool's BYTES and the lists; each of its twelve mistakes -- six of the gather, four of the widening stage,
two of their combination -- exceeds a bar on a named case, so the cases can tell them apart; the gathered e4m3 twin holds what the lists
name; and the split-rule identity both bit-identities rely on holds for every head count."""
import numpy as np
import pytest

import kv8
import mla
import mla_sparse
import mla_sparse_kv8 as msk
import mla_wide
import util

DTYPE = msk.DTYPE


@pytest.mark.parametrize("idx", range(len(msk.CASES)))
def test_reference_and_model_stay_inside_the_bars_on_every_gpu_case(oracle_mod, idx):
    c = msk.case(idx)
    Hq, topk, P, row_stride, pad_page = msk.CASES[idx][:5]
    assert (c["Hq"], c["topk"], c["P"]) == (Hq, topk, P) and c["T"] <= 8 and c["codes"].shape[0] * P <= 2048
    assert c["codes"].shape[1:] == (P + (1 if pad_page else 0), row_stride) and c["codes"].dtype == np.uint8
    assert c["indices"].shape[1] >= topk and c["indices"].shape[1] % 4 == 0
    if c["counts"] is not None and c["kind"] != "oob":
        assert sorted(c["lens"]) == mla_sparse.counts_for(topk)
    # the two pools hold the same values; whatever nobody may read is 0x7F / 0xFF here and NaN there: padding and every unnamed slot
    assert np.array_equal(kv8.widen(c["codes"].copy()), c["pool"], equal_nan=True)
    unreadable = np.isin(c["codes"], kv8.NAN_CODES)
    assert np.array_equal(np.isnan(c["pool"]), unreadable)
    named = msk.named_slots(c["indices"], c["counts"], topk, c["codes"].shape[0] * P).reshape(-1, P)
    assert named.any() and not unreadable[:, :P, :msk.DQK][named].any() and unreadable[:, :P][~named].all()
    assert unreadable[:, P:].all() and unreadable[:, :, msk.DQK:].all()
    # what the kernel stages from the bytes and the lists is what the case holds
    st, lens = msk.staged(c)
    assert lens == c["lens"] and all(np.array_equal(a, b) for a, b in zip(st, c["kvs"]))
    q = mla_sparse.q4(c["q"])
    args = (q, c["kvs"], c["lens"], False, DTYPE)
    o64, l64 = mla.reference(util.effective_q(oracle_mod, q, DTYPE, mla.SCALE), c["kvs"], c["lens"], False, util.LN2)
    mla.check(oracle_mod, o64, l64, *args, ("reference", idx))
    o, lse = mla_wide.model(oracle_mod, q, c["kvs"], c["lens"], False, mla.SCALE, DTYPE)
    mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), *args, ("model", idx))


# mistake -> the case (an index into the parity cases, or "small") that shows it, and why that one
NAMED = {
    "pitch_topk": 1,            # topk = 63 under a pitch of 64: from token 1 on every entry is its left neighbour's
    "token0_list": 4,           # seven tokens, seven different permutations
    "count_ignored": 4,         # counts 0 .. 319 of 320: the tail names slots nobody may read
    "row_stride_only": 2,       # pages of 256 rows with a padding row behind them: page p would start p rows early
    "page_row_swapped": 6,      # P = 16 over 64 pages: almost every slot lands elsewhere
    "oob_clamped": 8,           # -1, num_pages * P and INT_MAX among the first five entries of every token
    "halves_exchanged": 4,      # every value column and every score column lands eight elements off
    "rotary_from_1024": 4,      # rows of 576 bytes: byte 1024 of a row is the next slot's latent column 448
    "stride_in_2_bytes": 4,     # pages of 64 rows of 576 bytes: row r of a page answers with row 2 r
    "subnormals_flushed": "small",  # values mostly below 2^-6: the flush zeroes most of V
    "offset_doubled": 4,        # slot x answers with slot 2 x, the upper half of the pool with what lies behind it
    "oob_reads_offset0": 8,     # three of the first five entries of every token become slot 0's bytes instead of zeros
}


@pytest.mark.parametrize("mistake", msk.MISTAKES)
def test_each_planted_mistake_exceeds_a_bar_on_its_named_case(oracle_mod, mistake):
    c = msk.small_case() if NAMED[mistake] == "small" else msk.case(NAMED[mistake])
    q = mla_sparse.q4(c["q"])
    kvs, lens = msk.staged(c, mistake)
    assert not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(kvs, c["kvs"])) or lens != c["lens"], mistake
    kvs = [np.nan_to_num(kv, nan=1e4) for kv in kvs]  # (a NaN byte read where nobody may look: far outside every bar)
    o, lse = mla_wide.model(oracle_mod, q, kvs, lens, False, mla.SCALE, DTYPE)
    live = np.array(c["lens"]) > 0  # (a mistake may revive a dead token: judge the live tokens, what is not finite as far outside)
    o = np.where(live[:, None, None, None], np.nan_to_num(o, nan=1e30, posinf=1e30, neginf=-1e30), 0.0)
    lse = np.where(live[:, None, None], np.nan_to_num(lse, nan=1e30, posinf=1e30, neginf=-1e30), -np.inf)
    e = mla.errors(oracle_mod, o.astype(np.float64), lse.astype(np.float64), q, c["kvs"], c["lens"], False, DTYPE)
    assert any(err >= bar for err, bar in e.values()), (mistake, e)
    # and the stage without the mistake is inside every bar on that case
    right, lens = msk.staged(c)
    o, lse = mla_wide.model(oracle_mod, q, right, lens, False, mla.SCALE, DTYPE)
    mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), q, c["kvs"], c["lens"], False, DTYPE, ("stage", mistake))
    assert set(NAMED) == set(msk.MISTAKES) and len(msk.MISTAKES) == 12


def test_small_case_is_mostly_subnormal():
    c = msk.small_case()
    kk = np.concatenate(c["kvs"])
    assert ((np.abs(kk) < 2.0 ** -6) & (kk != 0)).mean() > 0.8 and np.abs(kk).max() <= 2.0 ** -6


def test_the_gathered_twin_holds_the_listed_rows_in_list_order():
    c = msk.case(8)
    codes, table, lens = msk.twin8(c, np.random.default_rng(1))
    assert codes.dtype == np.uint8 and codes.shape[1:] == (64, msk.DQK)
    assert lens == c["lens"] == [5, 20, 65] and table.shape == (3, 2) and len(set(table.reshape(-1))) == 6
    for t, n in enumerate(lens):
        rows = np.concatenate([codes[p] for p in table[t]])
        assert np.array_equal(kv8.widen(rows[:n]), c["kvs"][t]) and np.isin(rows[n:], kv8.NAN_CODES).all()
        assert (rows[[0, 2, 3]] == 0).all() and (rows[1] != 0).any()  # the entries outside the pool became zero rows


def test_split_rule_identity_both_bit_identities_rely_on():
    """the sparse rule (the split count fa_fwd_mla_decode_sparse computes) equals the e4m3 dense call's at (T, 1, cap) for every head
    count, and the new sizer is the sparse call's: read through the workspace sizes, bytes = T * S * ceil(Hq / 16) slots"""
    import flash_attention_metal_amd as fa

    if not __import__("os").path.exists(fa.lib_path()):
        fa.build_library()
    new, sparse, dense = fa.mla_decode_sparse_kv8_workspace_bytes, fa.mla_decode_sparse_workspace_bytes, fa.mla_decode_paged_kv8_workspace_bytes
    slot = 16 * 514 * 4  # bytes of one 16-row slot
    for Hq in range(1, 129):
        for T in (1, 2, 3, 7, 16, 128, 1024):
            for topk in (1, 64, 65, 320, 2048, 16384):
                assert new(T, Hq, 512, topk) == sparse(T, Hq, 512, topk) == dense(T, Hq, 1, 512, 64, -(-topk // 64)) > 0, (Hq, T, topk)
    assert new(1, 16, 512, 2048) == 8 * slot and new(3, 128, 512, 2048) == 3 * 8 * 8 * slot  # the GPU test's split cases: S = 8
    # up to 64 heads are one workgroup row block, whatever the wave count -- for Hq <= 32 too, where the wide call runs two waves
    for Hq in (1, 16, 17, 32, 33, 64):
        assert new(3, Hq, 512, 2048) // -(-Hq // 16) == new(3, 16, 512, 2048)
