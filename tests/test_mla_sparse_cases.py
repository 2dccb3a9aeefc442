"""CPU: the cases tests/test_gpu_mla_decode_sparse.py runs and the bars they are held to (tests/mla.py's, unchanged), checked without a
GPU. The fp64 reference on the kernel's pre-scaled operand and the fp32 model of the kernel's arithmetic stay inside every bar on every
case, so the bars can be held; each of six mistakes a gather kernel can make (tests/mla_sparse.py) exceeds a bar on a named case in both
dtypes, so the cases can tell them apart; the twin pool holds what the lists name; and the split-rule identity the bit-identity tests rely
on holds, through the two workspace-size functions."""
import numpy as np
import pytest

import mla
import mla_sparse
import util


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("idx", range(len(mla_sparse.CASES)))
def test_reference_and_model_stay_inside_the_bars_on_every_gpu_case(oracle_mod, idx, dtype):
    c = mla_sparse.case(idx, dtype)
    Hq, topk, P = mla_sparse.CASES[idx][:3]
    assert (c["Hq"], c["topk"], c["P"]) == (Hq, topk, P) and c["T"] <= 8 and c["pool"].shape[0] * P <= 8192
    assert c["indices"].shape[1] >= topk and c["indices"].shape[1] % 4 == 0
    if c["counts"] is not None and c["kind"] != "oob":
        assert sorted(c["lens"]) == mla_sparse.counts_for(topk)
    q = mla_sparse.q4(c["q"])
    args = (q, c["kvs"], c["lens"], False, dtype)
    # the exact operator on the operand the kernel multiplies, Q~ = round(scale . log2(e) . Q): what the pre-scaling alone costs against
    # the true Q has to fit the true-Q bars (its strict figures are zero by construction)
    o64, l64 = mla.reference(util.effective_q(oracle_mod, q, dtype, mla.SCALE), c["kvs"], c["lens"], False, util.LN2)
    mla.check(oracle_mod, o64, l64, *args, ("reference", idx, dtype))
    o, lse = mla.model(oracle_mod, q, c["kvs"], c["lens"], False, mla.SCALE, dtype)
    mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), *args, ("model", idx, dtype))


# mistake -> the case (index into mla_sparse.CASES) that shows it, and why that one
NAMED = {
    "pitch_topk": 1,        # topk = 63 under a pitch of 64: from token 1 on every entry is its left neighbour's
    "token0_list": 4,       # seven tokens, seven different permutations
    "count_ignored": 4,     # counts 0 .. 319 of 320: the tail holds valid slots
    "row_stride_only": 2,   # pages of 256 rows with a padding row behind them: page p would start p rows early
    "page_row_swapped": 6,  # P = 16 over 64 pages: almost every slot lands elsewhere
    "oob_clamped": 8,       # -1, num_pages * P and INT_MAX among the first five entries of every token
}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mistake", mla_sparse.MISTAKES)
def test_each_planted_mistake_exceeds_a_bar_on_its_named_case(oracle_mod, mistake, dtype):
    c = mla_sparse.case(NAMED[mistake], dtype)
    q = mla_sparse.q4(c["q"])
    kvs, lens = mla_sparse.gather(c, mistake)
    assert not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(kvs, c["kvs"])) or lens != c["lens"], mistake
    o, lse = mla.model(oracle_mod, q, kvs, lens, False, mla.SCALE, dtype)
    live = np.array(c["lens"]) > 0  # (a mistake may revive a dead token or read NaN padding: judge the live tokens, NaN as far outside)
    o = np.where(live[:, None, None, None], np.nan_to_num(o, nan=1e30, posinf=1e30, neginf=-1e30), 0.0)
    lse = np.where(live[:, None, None], np.nan_to_num(lse, nan=1e30, posinf=1e30, neginf=-1e30), -np.inf)
    e = mla.errors(oracle_mod, o.astype(np.float64), lse.astype(np.float64), q, c["kvs"], c["lens"], False, dtype)
    assert any(err >= bar for err, bar in e.values()), (mistake, dtype, e)
    assert set(NAMED) == set(mla_sparse.MISTAKES)


def test_the_twin_pool_holds_the_listed_rows_in_list_order():
    c = mla_sparse.case(8, "bf16")
    pool, table, lens = mla_sparse.twin(c, np.random.default_rng(1))
    assert lens == c["lens"] == [5, 20, 65] and table.shape == (3, 2) and len(set(table.reshape(-1))) == 6
    for t, n in enumerate(lens):
        rows = np.concatenate([pool[p] for p in table[t]])
        assert np.array_equal(rows[:n], c["kvs"][t]) and np.isnan(rows[n:]).all()
        assert (rows[[0, 2, 3]] == 0).all() and (rows[1] != 0).any()  # the entries outside the pool became zero rows


def test_split_rule_identity_the_bit_identity_tests_rely_on():
    import flash_attention_metal_amd as fa

    if not __import__("os").path.exists(fa.lib_path()):
        fa.build_library()
    sparse, wide = fa.mla_decode_sparse_workspace_bytes, fa.mla_decode_paged_wide_workspace_bytes
    slot = 16 * 514 * 4  # bytes of one 16-row slot
    for Hq, topk, *_ in mla_sparse.CASES:
        for T in range(1, 9):
            assert sparse(T, Hq, 512, topk) == wide(T, Hq, 1, 512, 64, -(-topk // 64)) > 0
    # the split cases of the GPU test: S = bytes / (T * 16-row slots * slot bytes)
    assert sparse(1, 16, 512, 2048) == 8 * slot                # T = 1, Hq = 16, topk = 2048: 32 tiles, four per split: S = 8
    assert sparse(2, 128, 512, 2048) == 2 * 8 * 8 * slot       # T = 2, Hq = 128: two workgroup row blocks, eight 16-row slots, S = 8
    assert sparse(1, 16, 512, 2047) == sparse(1, 16, 512, 1985) == 8 * slot  # the capacity is 64 * ceil(topk / 64)
    assert sparse(1, 16, 512, 1984) == 7 * slot
    # up to 64 heads are one workgroup row block, whatever the waves: the wide call's S (its two-wave form feeds the rule one block too)
    for Hq in (1, 16, 17, 32, 33, 64):
        assert sparse(3, Hq, 512, 2048) // -(-Hq // 16) == sparse(3, 16, 512, 2048)
