"""CPU: the cases tests/test_gpu_mla_bwd.py holds fa_bwd_varlen_mla to (tests/mla_bwd.py) -- the numpy model of the kernels' roundings
(backward_bound.head_model, two head dims) stays inside the derived bound on every GPU parity case, also under the forward terms of the
chain, and each planted mistake of a two-head-dim backward lies beyond the bound on the case mla_bwd.BUG_CASE names, in both dtypes.
Measured here on five (Lq, Lk) shapes with U(-1, 1) inputs: model error / bound <= 0.27 (bf16 and f16)."""
import numpy as np
import pytest

import mla_bwd as mb
import mla_prefill as mp


def worst(c, causal, bug=None, chain=False):
    per = []
    for b in range(len(c["lens"])):
        sb = mb.seq_bounds(c, b, causal, chain)
        per.append(mb.worst_ratio(sb.model(bug), sb))
    return per


@pytest.mark.parametrize("name,heads,dtype,causal", mb.PARITY)
def test_the_rounding_model_stays_inside_the_bound_on_every_parity_case(name, heads, dtype, causal):
    c = mp.case(name, heads, dtype)
    per = worst(c, causal)
    print(f"mla_bwd model {name} {heads} {dtype} causal={causal}: error / bound per sequence {[round(x, 3) for x in per]}")
    assert max(per) <= 1.0, per
    # what the bound is made of exists on this case: some sequence has live rows, and under the mask some has dead ones
    sbs = [mb.seq_bounds(c, b, causal) for b in range(len(c["lens"]))]
    assert any(sb.R for sb in sbs)
    if causal and name == "seqs":
        assert any(0 < sb.n0 for sb in sbs) and any(sb.n0 >= lq > 0 for sb, (lq, _) in zip(sbs, c["lens"]))


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_the_chain_bound_contains_the_given_input_bound(dtype):
    # the forward terms only widen: lse_err >= 0 takes the place of 0 and o_err >= u |O| that of u |O|
    c = mp.case("seqs", (8, 2), dtype)
    for b in range(len(c["lens"])):
        plain, chain = mb.seq_bounds(c, b, True), mb.seq_bounds(c, b, True, chain=True)
        assert all((y >= x).all() for x, y in zip(plain.bound, chain.bound))
    assert max(worst(c, True, chain=True)) <= 1.0


@pytest.mark.parametrize("dtype", mp.DTYPES)
@pytest.mark.parametrize("bug", mb.BUGS)
def test_each_planted_mistake_lies_beyond_the_bound_on_its_named_case(bug, dtype):
    name, heads, causal = mb.BUG_CASE[bug]
    c = mp.case(name, heads, dtype)
    per = worst(c, causal, bug)
    print(f"mla_bwd bug {bug} {dtype}: error / bound per sequence {[round(x, 2) for x in per]}")
    assert max(per) > 1.0, (bug, dtype, per)


def test_the_reference_of_a_sequence_is_the_autograd_formula():
    # one small sequence against a plain restatement: dQ, dK, dV of sum(O * dO) through softmax(scale q k^T) v, grouped heads
    c = mp.case("edges", (8, 2), "bf16")
    b = 4  # (5, 63)
    q, k, v, do = (np.asarray(x, np.float64) for x in mb.sequence(c, b))
    sb = mb.seq_bounds(c, b, False)
    G = q.shape[0] // k.shape[0]
    dq, dk, dv = np.zeros(q.shape), np.zeros(k.shape), np.zeros(v.shape)
    for h in range(q.shape[0]):
        s = mb.SCALE * q[h] @ k[h // G].T
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        dp = do[h] @ v[h // G].T
        ds = p * (dp - (dp * p).sum(-1, keepdims=True))
        dq[h] = mb.SCALE * ds @ k[h // G]
        dk[h // G] += mb.SCALE * ds.T @ q[h]
        dv[h // G] += p.T @ do[h]
    for x, y in zip((dq, dk, dv), sb.ref):
        assert np.allclose(x, y, rtol=1e-10, atol=1e-12)
    assert sb.ref[0].shape[-1] == 192 and sb.ref[1].shape[-1] == 192 and sb.ref[2].shape[-1] == 128
