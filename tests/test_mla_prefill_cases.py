"""CPU: the cases of tests/mla_prefill.py are what the GPU tests (tests/test_gpu_mla_prefill.py) need them to be -- the reference alone
stays inside the bars, an fp32 model of the kernel's arithmetic (pre-scaled Q rounded to the type, P rounded to the type into PV, fp32
sums) stays inside every bar on every parity case, each of six planted mistakes exceeds a bar on its named case in both dtypes, and the
merge of the chunked-context chain is exact in fp64 with a bar that follows from the two calls' bars."""
import numpy as np
import pytest

import mla_prefill as mp
from exact_forward import round_to

PARITY = [("seqs", heads) for heads in mp.HEADS] + [("edges", (8, 2))]


def test_the_catalogue_holds_what_the_issue_names():
    lens = mp.case("seqs", (4, 4), "bf16")["lens"]
    assert len(lens) == 8 and any(lk == 0 for _, lk in lens) and any(lq > lk > 0 for lq, lk in lens) and any(lk == 1000 for _, lk in lens)
    assert any((~mp.visible(lq, lk, True).any(1)).any() for lq, lk in lens if lk)  # dead rows under the mask
    assert {lk for _, lk in mp.EDGES} == {63, 64, 65, 128}
    c = mp.case("seqs", (8, 2), "f16")
    assert c["q"].shape[1:] == (8, 192) and c["k"].shape[1:] == (2, 192) and c["v"].shape[1:] == (2, 128)
    assert np.array_equal(round_to(c["q"], "f16"), c["q"]) and not c["q"].flags.writeable
    assert mp.SCALE == 192 ** -0.5


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
@pytest.mark.parametrize("name,heads", PARITY)
def test_reference_and_model_stay_inside_every_bar(name, heads, dtype, causal):
    c = mp.case(name, heads, dtype)
    so, sl, to, tl = mp.references(c, causal)
    # the reference alone: the exact result rounded to the output type is inside the strict bars, and the two references (on Q~ and on
    # the true Q) lie inside the true-Q bars of one another
    mp.check(round_to(so, dtype).astype(np.float64), sl, c, causal, ("reference", name, heads, dtype, causal))
    # the model of the kernel's arithmetic
    o, lse = mp.per_sequence(c, lambda q, k, v: mp.model(q, k, v, causal, mp.SCALE, dtype))
    e = mp.check(o, lse, c, causal, ("model", name, heads, dtype, causal))
    assert e[0] > 0.0  # (a model that returned the reference itself would show nothing)


@pytest.mark.parametrize("dtype", mp.DTYPES)
@pytest.mark.parametrize("bug", mp.BUGS)
def test_each_planted_mistake_exceeds_a_bar_on_its_case(bug, dtype):
    name, heads, causal = mp.BUG_CASE[bug]
    c = mp.case(name, heads, dtype)
    o, lse = mp.per_sequence(c, lambda q, k, v: mp.model(q, k, v, causal, mp.SCALE, dtype, bug=bug))
    e, b = mp.errors(o, lse, c, causal), mp.bars(c)
    print(bug, dtype, [f"{x:.3e} / {y:.3e}" for x, y in zip(e, b)])
    assert mp.exceeds_a_bar(o, lse, c, causal), (bug, dtype, e, b)
    # and against the TRUE-Q bars alone, the wider pair: the mistake is not a matter of the operand rounding
    assert not (e[2] < b[2] and e[3] < b[3]), (bug, dtype, e, b)


def test_the_model_without_a_mistake_is_the_same_function():
    c = mp.case("edges", (8, 2), "bf16")
    a = mp.per_sequence(c, lambda q, k, v: mp.model(q, k, v, True, mp.SCALE, "bf16"))
    b = mp.per_sequence(c, lambda q, k, v: mp.model(q, k, v, True, mp.SCALE, "bf16", bug=None))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert set(mp.BUG_CASE) == set(mp.BUGS) and len(mp.BUGS) == 6


def test_merge_of_exact_partials_is_the_causal_reference_and_its_bar_follows_from_the_calls():
    rng = np.random.default_rng(5)
    Hq, Hkv = 4, 2
    for Ln, Lc in mp.CHAIN:
        q, k, v = (rng.uniform(-1, 1, s) for s in ((Hq, Ln, 192), (Hkv, Lc + Ln, 192), (Hkv, Lc + Ln, 128)))
        oa, la = mp.reference(q, k[:, :Lc], v[:, :Lc], False, mp.SCALE)
        ob, lb = mp.reference(q, k[:, Lc:], v[:, Lc:], True, mp.SCALE)
        o1, l1 = mp.reference(q, k, v, True, mp.SCALE)
        om, lm = mp.merge(oa.transpose(1, 0, 2), la, ob.transpose(1, 0, 2), lb)
        assert np.abs(om - o1.transpose(1, 0, 2)).max() < 1e-12 and np.abs(lm - l1).max() < 1e-12, (Ln, Lc)
        # perturb both partials by their bars in the worst directions: the merged result stays inside merge_bars
        eO, eL = 6e-3, 9e-3
        for sa, sb in ((1, -1), (-1, 1), (1, 1)):
            pm, plm = mp.merge(oa.transpose(1, 0, 2) + eO, np.where(np.isneginf(la), la, la + sa * eL), ob.transpose(1, 0, 2) + eO, lb + sb * eL)
            bo, bl = mp.merge_bars(eO, eL, eO, eL, 1.0)
            assert np.abs(pm - om).max() <= bo and np.abs(plm - lm).max() <= bl + 1e-15, (Ln, Lc, sa, sb)
    assert any(Lc == 0 for _, Lc in mp.CHAIN)  # a side with LSE = -inf is skipped
