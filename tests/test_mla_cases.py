"""CPU: the cases tests/test_gpu_mla_decode.py runs and the bars they are held to (tests/mla.py), checked without a GPU. An fp32 numpy
model of the kernel's arithmetic (pre-scaled 576-wide operand, fp32 sums, probabilities rounded to the input type) stays inside every
bar on every case; each of six planted mistakes exceeds a bar on a named case in both dtypes -- so the cases can tell them apart."""
import numpy as np
import pytest

import mla


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", mla.PAGES)
def test_model_of_the_kernel_stays_inside_the_bars_on_every_gpu_case(oracle_mod, P, dtype):
    for idx in range(len(mla.SHAPES)):
        c = mla.case(P, dtype, idx)
        o, lse = mla.model(oracle_mod, c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE, dtype)
        mla.check(oracle_mod, o.astype(np.float64), lse.astype(np.float64), c["q"], c["kvs"], c["lens"], c["causal"], dtype,
                  ("model", P, dtype, mla.SHAPES[idx]))


# mistake -> the case (index into mla.SHAPES) that shows it, and why that one
NAMED = {
    "v_all_576": 0,    # (16, 1): sixteen packed rows -- every row but the first lands at the wrong pitch
    "v_from_64": 0,    # any case: the value columns are shifted by 64
    "no_rotary": 0,    # any case: the scores lose 64 of their 576 terms
    "scale_576": 0,    # any case: every score shrinks by sqrt(192 / 576)
    "top_left": 1,     # (16, 2) causal: L_b != Nq moves the diagonal
    "row_packing": 1,  # (16, 2): Hq > 1 and Nq > 1, so the two packings differ
}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mistake", mla.MISTAKES)
def test_each_planted_mistake_exceeds_a_bar_on_its_named_case(oracle_mod, mistake, dtype):
    c = mla.case(64, dtype, NAMED[mistake])
    o, lse = mla.model(oracle_mod, c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE, dtype, mistake=mistake)
    live = ~np.isneginf(mla.reference(c["q"], c["kvs"], c["lens"], c["causal"], mla.SCALE)[1])
    lse = np.where(live, lse, -np.inf)  # (a mistake in the mask may revive a dead row: judge the live rows)
    o = np.where(live[..., None], o, 0.0)
    with np.errstate(invalid="ignore"):
        lse = np.where(live & ~np.isfinite(lse), 1e30, lse)  # ... or kill a live one: far outside every bar
    e = mla.errors(oracle_mod, o.astype(np.float64), lse.astype(np.float64), c["q"], c["kvs"], c["lens"], c["causal"], dtype)
    assert any(err >= bar for err, bar in e.values()), (mistake, dtype, e)
    assert set(NAMED) == set(mla.MISTAKES)
