"""CPU: the cases tests/test_gpu_mla_decode_kv8.py runs and the bars they are held to (tests/mla.py's bf16 bars, unchanged, on the widened
values), checked without a GPU. The fp32 model of the kernel's arithmetic (tests/mla_wide.py) and the fp64 reference on the kernel's
pre-scaled operand stay inside every bar on every case, so the bars can be held; the model of the widening stage (tests/mla_kv8.py)
reproduces every case's values from the pool's BYTES; each of four mistakes a widening stage can make exceeds a bar on a named case, so
the cases can tell them apart; and the e4m3 pool equals its bf16 twin exactly on all 254 finite codes."""
import numpy as np
import pytest

import kv8
import mla
import mla_kv8
import mla_wide
import util

DTYPE = mla_kv8.DTYPE


@pytest.mark.parametrize("P", mla_kv8.PAGES)
def test_model_on_the_widened_pool_stays_inside_the_bars_on_every_gpu_case(oracle_mod, P):
    for idx, shape in enumerate(mla_kv8.SHAPES):
        c = mla_kv8.case(P, idx)
        assert (c["Hq"], c["Nq"], c["causal"]) == shape and sorted(c["lens"]) == sorted(mla.lengths(P))
        # what the kernel stages from the bytes is what the case holds, and the twin holds the same values
        st = mla_kv8.staged(c["codes"], c["table"], c["lens"], P)
        assert all(np.array_equal(a, b) for a, b in zip(st, c["kvs"]))
        assert np.array_equal(kv8.widen(c["codes"]), c["twin"], equal_nan=True)
        assert np.array_equal(np.isnan(c["twin"]), np.isin(c["codes"], kv8.NAN_CODES)) and np.isnan(c["twin"]).any()
        args = (c["q"], c["kvs"], c["lens"], c["causal"], DTYPE)
        o64, l64 = mla.reference(util.effective_q(oracle_mod, c["q"], DTYPE, mla.SCALE), c["kvs"], c["lens"], c["causal"], util.LN2)
        mla.check(oracle_mod, o64, l64, *args, ("reference", P, shape))
        o, lse = mla_wide.model(oracle_mod, c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE, DTYPE)
        mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), *args, ("model", P, shape))


# mistake -> the case that shows it, and why that one
NAMED = {
    "halves_exchanged": ("parity", 64, 1),     # (16, 1): every value column and every score column lands eight elements off
    "rotary_from_1024": ("parity", 16, 2),     # (17, 1), rows of 576 bytes: byte 1024 is the NEXT key's latent column 448
    "stride_in_2_bytes": ("parity", 256, 6),   # (64, 1), pages of 256 rows: key r answers with key 2 r, the upper half with zeros
    "subnormals_flushed": ("small", None, None),  # values mostly below 2^-6: the flush zeroes most of V
}


@pytest.mark.parametrize("mistake", mla_kv8.MISTAKES)
def test_each_planted_mistake_exceeds_a_bar_on_its_named_case(oracle_mod, mistake):
    kind, P, idx = NAMED[mistake]
    c = mla_kv8.case(P, idx) if kind == "parity" else mla_kv8.small_case()
    if mistake == "stride_in_2_bytes":
        assert c["codes"].shape[2] == 576 and c["codes"].shape[1] == c["P"]  # (no padding: the doubled stride reads other keys, not NaN bytes)
    if mistake == "rotary_from_1024":
        assert c["codes"].shape[2] == 576
    wrong = mla_kv8.staged(c["codes"], c["table"], c["lens"], c["P"], mistake=mistake)
    assert not all(np.array_equal(a, b) for a, b in zip(wrong, c["kvs"]))
    wrong = [np.nan_to_num(kv, nan=1e4) for kv in wrong]  # (a NaN byte read where nobody may look: far outside every bar)
    o, lse = mla_wide.model(oracle_mod, c["q"], wrong, c["lens"], c["causal"], mla.SCALE, DTYPE)
    live = ~np.isneginf(mla.reference(c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE)[1])
    lse = np.where(live, lse, -np.inf)
    o = np.where(live[..., None], o, 0.0)
    with np.errstate(invalid="ignore"):
        lse = np.where(live & ~np.isfinite(lse), 1e30, lse)
        o = np.where(np.isfinite(o), o, 1e30)
    e = mla.errors(oracle_mod, o.astype(np.float64), lse.astype(np.float64), c["q"], c["kvs"], c["lens"], c["causal"], DTYPE)
    assert any(err >= bar for err, bar in e.values()), (mistake, e)
    # and the stage without the mistake is inside every bar on that case
    right = mla_kv8.staged(c["codes"], c["table"], c["lens"], c["P"])
    o, lse = mla_wide.model(oracle_mod, c["q"], right, c["lens"], c["causal"], mla.SCALE, DTYPE)
    mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), c["q"], c["kvs"], c["lens"], c["causal"], DTYPE, ("stage", mistake))
    assert set(NAMED) == set(mla_kv8.MISTAKES)


def test_small_case_is_mostly_subnormal():
    c = mla_kv8.small_case()
    kk = np.concatenate(c["kvs"])
    sub = (np.abs(kk) < 2.0 ** -6) & (kk != 0)  # the subnormal codes; the rest rounded to 0 or to 2^-6 itself
    assert sub.mean() > 0.8 and (np.abs(kk) < 2.0 ** -6).mean() > 0.9 and np.abs(kk).max() <= 2.0 ** -6


def test_widened_pool_equals_its_bf16_twin_on_all_finite_codes(oracle_mod):
    import torch

    codes = kv8.FINITE_CODES
    assert len(codes) == 254
    vals = kv8.widen(codes)
    # every finite code is a bf16 value: rounding to bf16 changes nothing, and the hand-decoded value agrees (subnormals, both zeros)
    assert np.array_equal(oracle_mod.round_to(vals, "bf16"), vals)
    assert np.array_equal(torch.from_numpy(vals).to(torch.bfloat16).to(torch.float32).numpy(), vals)
    assert all(kv8.decode_by_hand(int(c)) == float(v) for c, v in zip(codes, vals))
    assert np.signbit(vals[codes == 0x80]).all() and not np.signbit(vals[codes == 0x00]).any()
    # a twin pool built from them: the codes come back, the values are equal bit for bit
    rows = np.resize(codes, 2 * 576).reshape(2, 576)
    it = iter(range(2))
    c8, twin, table, kvs = mla_kv8.make_twins(np.random.default_rng(1), 16, [1, 1], draw=lambda L: kv8.widen(rows[next(it)])[None])
    for b in range(2):
        assert np.array_equal(c8[table[b, 0], 0], rows[b])
        assert np.array_equal(twin[table[b, 0], 0].view(np.uint32), kv8.widen(rows[b]).view(np.uint32))
        assert np.array_equal(kvs[b][0].view(np.uint32), twin[table[b, 0], 0].view(np.uint32))
