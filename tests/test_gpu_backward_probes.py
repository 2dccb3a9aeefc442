"""Exact index logic of the backward: the counterpart of test_mask_index_probe_exact / test_head_batch_addressing_bit_exact.

Uniform-softmax probes. With Q = 0 (probe V) or K = 0 (probe K) every score is 0, so P_ij = 1 / vis(i) on the vis(i) visible keys of
row i, LSE_i = ln(vis(i)) and O_i is the mean of the visible V rows: exact inputs, fed to the backward. dO is one row: dO[i] = delta(i, t) w.
  probe V: dV[j] = P_tj w for the keys row t sees and EXACTLY 0 for the others; dK exactly 0 everywhere (Q = 0); dQ[i] exactly 0 for
           i != t (dO_i = 0, so delta_i = 0 and dS_ij = P_ij * 0); dQ[t] within the bound of tests/backward_bound.py. The nonzero dV
           rows are round(1 / vis(t)) * w: one rounding of P to the 16-bit type (the bars of the forward probe: 1e-3 f16, 8e-3 bf16, relative).
  probe K: dK[j] = scale * dS_tj * q_t, exactly 0 for the keys row t does not see, within the bound for the others; dQ exactly 0.
A masked (query, key) pair contributing anything at all, a key block's first / last tile or a wave's 32-row half taking the wrong
limit, shows as a nonzero where a zero belongs or as a missing step.
Measured on the MI355X, worst err / bound of the entries held to the bound: probe V 0.70 (f16) / 0.76 (bf16), probe K 0.72 / 0.88 --
a gradient row is a single product here, so one rounding that lands just above a power of two nearly attains the bound (the numpy
model of the roundings reads 0.88 on the same probes).
"""
import numpy as np
import pytest

import backward_bound as bb
from util import to_dev

pytestmark = pytest.mark.gpu
ULP_BAR = {"f16": 1e-3, "bf16": 8e-3}
T_LIST = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257)
MASKS = {"causal": (True, 0), "causal+70": (True, 70), "full": (False, 0)}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available()
    fa.load_library()
    return fa


def rand(oracle, shape, dtype, seed):
    return oracle.round_to(np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32), dtype)


def visible(Nq, Nk, causal):
    if not causal:
        return np.ones((Nq, Nk), bool)
    return np.arange(Nk)[None, :] <= np.arange(Nq)[:, None] + (Nk - Nq)


def backward(fa, oracle, q, k, v, do, X, dtype, causal):
    """fa's backward on the exact O (rounded to the type) and LSE of the probe, as numpy arrays."""
    import torch

    o = oracle.round_to(X.o.astype(np.float32), dtype)
    lse = torch.from_numpy(X.lse.astype(np.float32)).cuda()
    g = fa.flash_attention_backward(*(to_dev(x, dtype) for x in (q, k, v, o, do)), lse, is_causal=causal)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in g]


def zeros_exactly(a):
    return np.array_equal(a, np.zeros_like(a))


@pytest.mark.parametrize("N", [320, 333])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("D", [64, 128, 256, 40])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_probe_v(fa, oracle_mod, dtype, D, mask, N):
    causal, coff = MASKS[mask]
    G, Nk = 2, N + coff
    vis = visible(N, Nk, causal)
    k, v = rand(oracle_mod, (1, 1, Nk, D), dtype, 1), rand(oracle_mod, (1, 1, Nk, D), dtype, 2)
    q = np.zeros((1, G, N, D), np.float32)
    w = rand(oracle_mod, (G, D), dtype, 3)
    w[np.abs(w) < 2.0 ** -6] = 0.5  # keep w / vis(t) in the normal range of f16
    worst = 0.0
    ts = T_LIST + (N - 1,)
    for n, t in enumerate(ts):
        tt = (t, ts[(n + 5) % len(ts)])  # the two query heads of the key head carry different rows
        do = np.zeros((1, G, N, D), np.float32)
        for h in range(G):
            do[0, h, tt[h]] = w[h]
        X = bb.Bounds(q, k, v, do, causal, None, dtype)
        for h in range(G):  # the probe's forward is what the docstring says it is
            assert np.abs(X.lse[0, h] - np.log(vis.sum(1))).max() < 1e-12
        dq, dk, dv = backward(fa, oracle_mod, q, k, v, do, X, dtype, causal)
        assert zeros_exactly(dk), (t, np.abs(dk).max())
        want = sum(vis[tt[h]][:, None] * (w[h].astype(np.float64) / vis[tt[h]].sum()) for h in range(G))
        scale_ = sum(vis[tt[h]][:, None] * (np.abs(w[h]).astype(np.float64) / vis[tt[h]].sum()) for h in range(G))
        seen = vis[tt[0]] | vis[tt[1]]
        assert zeros_exactly(dv[0, 0, ~seen]), (tt, np.flatnonzero(np.abs(dv[0, 0]).max(-1) * ~seen))
        assert (np.abs(dv[0, 0] - want) <= ULP_BAR[dtype] * scale_).all(), (tt, np.abs(dv[0, 0] - want).max())
        assert (np.abs(dv[0, 0, seen]).max(-1) > 0).all()  # the step is there for every key the rows see
        for h in range(G):
            rows = np.arange(N) != tt[h]
            assert zeros_exactly(dq[0, h, rows]), (tt, h)
        r = bb.ratios([dq, dv], [X.ref[0], X.ref[2]], [X.bound[0], X.bound[2]])
        assert max(r) <= 1.0, (tt, r)
        worst = max(worst, *r)
    print(f"PROBE V {dtype} D{D} {mask} N{N}: worst err/bound (dq[t], dv) {worst:.3f}")


@pytest.mark.parametrize("N", [320, 333])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("D", [64, 128, 256, 40])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_probe_k(fa, oracle_mod, dtype, D, mask, N):
    causal, coff = MASKS[mask]
    G, Nk = 2, N + coff
    vis = visible(N, Nk, causal)
    q, v = rand(oracle_mod, (1, G, N, D), dtype, 4), rand(oracle_mod, (1, 1, Nk, D), dtype, 5)
    k = np.zeros((1, 1, Nk, D), np.float32)
    w = rand(oracle_mod, (G, D), dtype, 6)
    worst = 0.0
    ts = T_LIST + (N - 1,)
    for n, t in enumerate(ts):
        tt = (t, ts[(n + 5) % len(ts)])
        do = np.zeros((1, G, N, D), np.float32)
        for h in range(G):
            do[0, h, tt[h]] = w[h]
        X = bb.Bounds(q, k, v, do, causal, None, dtype)
        dq, dk, dv = backward(fa, oracle_mod, q, k, v, do, X, dtype, causal)
        assert zeros_exactly(dq), (tt, np.abs(dq).max())
        seen = vis[tt[0]] | vis[tt[1]]
        assert zeros_exactly(dk[0, 0, ~seen]) and zeros_exactly(dv[0, 0, ~seen]), (tt, np.flatnonzero(np.abs(dk[0, 0]).max(-1) * ~seen))
        r = bb.ratios([dk, dv], X.ref[1:], X.bound[1:])
        assert max(r) <= 1.0, (tt, r)
        worst = max(worst, *r)
        if vis[tt[0]].sum() > 1 and vis[tt[1]].sum() > 1:  # (a single visible key: dS = 0 exactly) the step is there, and it is dS q_t
            assert (np.abs(X.ref[1][0, 0, seen]).max(-1) > 4 * X.bound[1][0, 0, seen].max(-1)).mean() > 0.9
    print(f"PROBE K {dtype} D{D} {mask} N{N}: worst err/bound (dk, dv) {worst:.3f}")


def _problem(oracle, dtype, B, Hq, Hkv, Nq, Nk, D):
    q = rand(oracle, (B, Hq, Nq, D), dtype, 11)
    k, v = rand(oracle, (B, Hkv, Nk, D), dtype, 12), rand(oracle, (B, Hkv, Nk, D), dtype, 13)
    do = rand(oracle, (B, Hq, Nq, D), dtype, 14)
    return q, k, v, do


@pytest.mark.parametrize("D", [64, 128, 256, 40, 96])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_head_batch_addressing_bit_exact(fa, oracle_mod, dtype, causal, D):
    """A (batch, key head) slice run alone gives the bits it has inside the batch; permuting the key heads (with their groups)
    permutes the outputs; padded strides give the bits of the contiguous call; two runs are identical."""
    import torch

    B, Hq, Hkv, Nq, Nk = 2, 6, 3, 200, 270
    G = Hq // Hkv
    q, k, v, do = _problem(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D)
    o64, lse64 = oracle_mod.attn_fwd_ex_f64(q, k, v, causal)
    o, lse = oracle_mod.round_to(o64.astype(np.float32), dtype), lse64.astype(np.float32)

    def run(q_, k_, v_, o_, do_, lse_, pad=False):
        if pad:
            def wrap(x, er, eh):
                b, h, n, d = x.shape
                buf = torch.full((b, h + eh, n + er, d), float("nan"), dtype=to_dev(x[:1, :1, :1], dtype).dtype, device="cuda")
                view = buf[:, :h, :n]
                view.copy_(to_dev(x, dtype))
                return view
            dev = [wrap(q_, 8, 1), wrap(k_, 16, 2), wrap(v_, 16, 2), wrap(o_, 8, 1), wrap(do_, 8, 1)]
        else:
            dev = [to_dev(x, dtype) for x in (q_, k_, v_, o_, do_)]
        g = fa.flash_attention_backward(*dev, torch.from_numpy(np.ascontiguousarray(lse_)).cuda(), is_causal=causal)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in g]

    full = run(q, k, v, o, do, lse)
    again = run(q, k, v, o, do, lse)
    for a, b in zip(full, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(full, run(q, k, v, o, do, lse, pad=True)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for b in range(B):
        for hk in range(Hkv):
            hs = slice(hk * G, hk * G + G)
            c = np.ascontiguousarray
            alone = run(c(q[b:b + 1, hs]), c(k[b:b + 1, hk:hk + 1]), c(v[b:b + 1, hk:hk + 1]), c(o[b:b + 1, hs]), c(do[b:b + 1, hs]), c(lse[b:b + 1, hs]))
            assert np.array_equal(alone[0].view(np.uint32), full[0][b:b + 1, hs].view(np.uint32)), ("dq", b, hk)
            assert np.array_equal(alone[1].view(np.uint32), full[1][b:b + 1, hk:hk + 1].view(np.uint32)), ("dk", b, hk)
            assert np.array_equal(alone[2].view(np.uint32), full[2][b:b + 1, hk:hk + 1].view(np.uint32)), ("dv", b, hk)
    perm = np.array([2, 0, 1])
    qperm = (perm[:, None] * G + np.arange(G)[None, :]).reshape(-1)
    c = np.ascontiguousarray
    shuffled = run(c(q[:, qperm]), c(k[:, perm]), c(v[:, perm]), c(o[:, qperm]), c(do[:, qperm]), c(lse[:, qperm]))
    assert np.array_equal(shuffled[0].view(np.uint32), full[0][:, qperm].view(np.uint32))
    assert np.array_equal(shuffled[1].view(np.uint32), full[1][:, perm].view(np.uint32))
    assert np.array_equal(shuffled[2].view(np.uint32), full[2][:, perm].view(np.uint32))
    bflip = run(c(q[::-1]), c(k[::-1]), c(v[::-1]), c(o[::-1]), c(do[::-1]), c(lse[::-1]))
    for a, b_ in zip(bflip, full):
        assert np.array_equal(a.view(np.uint32), b_[::-1].view(np.uint32))
