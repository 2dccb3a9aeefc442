"""The catalogue of the varlen backward's GPU tests, judged on the CPU (numpy only): on every case backward_bound.head_model -- the
kernels' roundings -- applied per sequence stays inside the per-sequence bound (tests/varlen_backward.py), and each of a list of
structural mistakes a varlen kernel can make exceeds the bound on at least one case, in both dtypes. A catalogue on which a mistake
does not show is no evidence that the kernels do not make it."""
import numpy as np
import pytest

import backward_bound as bb
from varlen_backward import CASES, SeqBounds, draw_seq, worst_ratio


def build(ci, dtype, D, causal, scale=None):
    Hq, Hkv, _, lens = CASES[ci]
    rng = np.random.default_rng(77 * ci + D + (3 if causal else 0))
    seqs = [draw_seq(rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in lens]
    return [SeqBounds(*s, causal, scale, dtype) for s in seqs]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_rounding_model_stays_inside_the_bound_on_every_case(dtype, D, causal):
    worst = 0.0
    for ci in range(len(CASES)):
        for b, sb in enumerate(build(ci, dtype, D, causal)):
            r = worst_ratio(sb.model(), sb)
            assert r <= 1.0, (ci, b, r)
            worst = max(worst, r)
            n0 = sb.n0  # rows without a visible key: zero gradient, zero bound
            assert not sb.ref[0][:, :n0].any() and not sb.bound[0][:, :n0].any()
    print(f"worst model error / bound {dtype} D={D} causal={causal}: {worst:.3f}")
    assert worst > 0.01  # the bound is not vacuous


# ---- structural mistakes: each returns the three gradients of sequence b as the mistaken kernel would form them, or None where the
# mistake cannot show (first sequence, no mask, ...)
def _with(R, **kw):
    R2 = dict(R)
    R2.update(kw)
    return R2


def leak_neighbour_key(sbs, b, max_q, max_k):
    """the descriptor ends one row late at the front: the previous sequence's last key is read as this sequence's first"""
    sb, prev = sbs[b], sbs[b - 1] if b else None
    if prev is None or prev.k.shape[1] == 0 or not sb.R:
        return None

    def fn(h, q, k, v, do, R):
        hk = h // sb.G
        k2, v2 = np.concatenate([prev.k[hk, -1:], k]), np.concatenate([prev.v[hk, -1:], v])
        mask = None if R["mask"] is None else np.concatenate([np.ones((q.shape[0], 1), bool), R["mask"]], 1)
        g = bb.head_model(q, k2, v2, do, sb.causal, sb.scale, sb.dtype, _with(R, mask=mask))
        return g[0], g[1][1:], g[2][1:]
    return sb.model(fn)


def _masked(sbs, b, shift):
    sb = sbs[b]
    if not sb.causal or not sb.R:
        return None
    Lq, Lk = sb.q.shape[1], sb.k.shape[1]
    if shift == Lk - Lq:
        return None
    mask = np.arange(Lk)[None, :] <= np.arange(sb.n0, Lq)[:, None] + shift
    return sb.model(lambda h, q, k, v, do, R: bb.head_model(q, k, v, do, True, sb.scale, sb.dtype, _with(R, mask=mask)))


def coff_from_max_seqlen(sbs, b, max_q, max_k):
    """the mask's offset taken from max_seqlen_k - max_seqlen_q instead of Lk_b - Lq_b"""
    return _masked(sbs, b, max_k - max_q)


def top_left_mask(sbs, b, max_q, max_k):
    """key j visible to query i iff j <= i"""
    return _masked(sbs, b, 0)


def lse_without_cu(sbs, b, max_q, max_k):
    """lse (and delta) rows indexed by i instead of cu_q[b] + i: sequence b reads the rows of the start of the batch"""
    sb = sbs[b]
    if b == 0 or not sb.R:
        return None
    packed = np.concatenate([s.lse for s in sbs], axis=1)  # [Hq, total_q]
    Lq = sb.q.shape[1]
    with np.errstate(all="ignore"):
        return sb.model(lambda h, q, k, v, do, R: bb.head_model(q, k, v, do, sb.causal, sb.scale, sb.dtype, _with(R, lse=packed[h, sb.n0:Lq])))


def empty_rows_lse_used(sbs, b, max_q, max_k):
    """a row without a visible key starts its score chain from -lse = +inf, and the mask's -inf meets it"""
    sb = sbs[b]
    if sb.n0 == 0 or sb.k.shape[1] == 0:
        return None
    g = sb.model()
    with np.errstate(all="ignore"):
        s = -sb.lse[:, :sb.n0] + -np.inf  # +inf + -inf
    g[0][:, :sb.n0] = (np.exp2(s) * 0.0)[:, :, None]
    g[1][:] += np.exp2(s).sum() * 0.0
    return g


MISTAKES = [leak_neighbour_key, coff_from_max_seqlen, top_left_mask, lse_without_cu, empty_rows_lse_used]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("mistake", MISTAKES, ids=lambda f: f.__name__)
def test_each_structural_mistake_exceeds_the_bound_somewhere(mistake, dtype):
    caught = []
    for causal in (False, True):
        for ci, (_, _, _, lens) in enumerate(CASES):
            sbs = build(ci, dtype, 64, causal)
            max_q, max_k = max(l[0] for l in lens), max(l[1] for l in lens)
            for b in range(len(sbs)):
                g = mistake(sbs, b, max_q, max_k)
                if g is not None and not worst_ratio(g, sbs[b]) <= 1.0:
                    caught.append((causal, ci, b))
    print(mistake.__name__, dtype, "caught on", len(caught), "sequences, e.g.", caught[:4])
    assert caught, mistake.__doc__
