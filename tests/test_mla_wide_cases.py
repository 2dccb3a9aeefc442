"""CPU: the cases tests/test_gpu_mla_decode_wide.py runs and the bars they are held to (tests/mla.py's, unchanged), checked without a GPU.
The fp64 reference on the kernel's pre-scaled operand and the fp32 model of the kernel's arithmetic stay inside every bar on every case,
so the bars can be held; each of three mistakes a multi-wave kernel can make (tests/mla_wide.py) exceeds a bar on a named case in both dtypes, so the cases can
tell them apart; and the split-rule identities the bit-identity tests rely on hold, through the two workspace-size functions."""
import numpy as np
import pytest

import mla
import mla_wide
import util


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", mla_wide.PAGES)
def test_reference_and_model_stay_inside_the_bars_on_every_gpu_case(oracle_mod, P, dtype):
    for idx, shape in enumerate(mla_wide.SHAPES):
        c = mla_wide.case(P, dtype, idx)
        assert (c["Hq"], c["Nq"], c["causal"]) == shape and sorted(c["lens"]) == sorted(mla.lengths(P))
        args = (c["q"], c["kvs"], c["lens"], c["causal"], dtype)
        # the exact operator on the operand the kernel multiplies, Q~ = round(scale . log2(e) . Q): what the pre-scaling alone costs against
        # the true Q has to fit the true-Q bars (its strict figures are zero by construction)
        o64, l64 = mla.reference(util.effective_q(oracle_mod, c["q"], dtype, mla.SCALE), c["kvs"], c["lens"], c["causal"], util.LN2)
        mla.check(oracle_mod, o64, l64, *args, ("reference", P, dtype, shape))
        o, lse = mla_wide.model(oracle_mod, c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE, dtype)
        mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), *args, ("model", P, dtype, shape))


# mistake -> the case (index into mla_wide.SHAPES) that shows it, and why that one
NAMED = {
    "wave_dropped": 5,  # (64, 1): heads 16..63 would answer with the queries of heads 0..15
    "block_base": 9,    # (128, 1): the second block would start at row 16 instead of row 64
    "iq_in_wave": 3,    # (16, 3) causal: 16 is no multiple of 3, so c % Nq != r % Nq from row 16 on
}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mistake", mla_wide.MISTAKES)
def test_each_planted_mistake_exceeds_a_bar_on_its_named_case(oracle_mod, mistake, dtype):
    c = mla_wide.case(64, dtype, NAMED[mistake])
    o, lse = mla_wide.model(oracle_mod, c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE, dtype, mistake=mistake)
    live = ~np.isneginf(mla.reference(c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE)[1])
    lse = np.where(live, lse, -np.inf)  # (a mistake in the mask may revive a dead row: judge the live rows)
    o = np.where(live[..., None], o, 0.0)
    with np.errstate(invalid="ignore"):
        lse = np.where(live & ~np.isfinite(lse), 1e30, lse)  # ... or kill a live one: far outside every bar
    e = mla.errors(oracle_mod, o.astype(np.float64), lse.astype(np.float64), c["q"], c["kvs"], c["lens"], c["causal"], dtype)
    assert any(err >= bar for err, bar in e.values()), (mistake, dtype, e)
    assert set(NAMED) == set(mla_wide.MISTAKES)


def test_split_rule_identities_the_bit_identity_tests_rely_on():
    import flash_attention_metal_amd as fa

    if not __import__("os").path.exists(fa.lib_path()):
        fa.build_library()
    wide, old = fa.mla_decode_paged_wide_workspace_bytes, fa.mla_decode_paged_workspace_bytes
    slot = 16 * 514 * 4  # bytes of one 16-row slot
    P = mla_wide.BITID_P
    for i, ((Hq, Nq, _), heads) in enumerate(mla_wide.BITID):
        lens, mp = mla_wide.bitid_capacity(i)
        B = len(lens)
        assert max(lens) <= P * mp
        # S = bytes / (B * 16-row slots * slot bytes): the wide call on all rows and the one-wave call on `heads` heads split alike
        s_wide = wide(B, Hq, Nq, 512, P, mp) // (B * -(-Hq * Nq // 16) * slot)
        s_old = old(B, heads, Nq, 512, P, mp) // (B * -(-heads * Nq // 16) * slot)
        assert s_wide == s_old >= 1 and wide(B, Hq, Nq, 512, P, mp) == B * s_wide * -(-Hq * Nq // 16) * slot, (i, s_wide, s_old)
        if i < len(mla_wide.BITID) - 1:  # both feed the rule the same number of blocks: workgroup blocks of 16 NW rows there, 16-row blocks here
            assert -(-Hq * Nq // (16 * mla_wide.waves(Hq * Nq))) == -(-heads * Nq // 16) and s_wide == 16
        else:  # one block there, two here: the capacity's four tiles per split bind both
            assert s_wide == 4
    # at most 64 rows are one workgroup block, like at most 16 rows of the one-wave call: the same S for any B and capacity
    for B, mp in ((1, 1024), (3, 100), (16, 512), (128, 64), (300, 7)):
        for rows in (33, 48, 64):
            assert wide(B, rows, 1, 512, 64, mp) // (-(-rows // 16)) == old(B, 16, 1, 512, 64, mp) == wide(B, 16, 1, 512, 64, mp), (B, mp, rows)
        assert wide(B, 128, 1, 512, 64, mp) // 8 == old(B, 32, 1, 512, 64, mp) // 2
    # B = 1 at a capacity of 65536 keys: 256 splits for one block of 64 rows (test_many_splits_on_one_sequence)
    assert wide(1, 64, 1, 512, 64, 1024) == 256 * 4 * slot
