"""GPU parity of the decode entry points (fa_fwd_decode, fa_fwd_decode_kv8, fa_fwd_decode_paged) where the combine merges more than 64
key splits and where the scores sit far from zero.

flash_attention_metal_amd/csrc/fa_decode_kernel.hip: lane l of the combine takes splits l, l + 64, l + 128, l + 192 of at most 256; S = min(ceil(256 * per_cu / (B * Hkv)),
nT / 4, 256). The other decode tests reach S <= 64 on U(-1,1) data, where any row reference works. Here: S = 65, 78, 129, 193 and 256
(asserted per case against the library's own workspace size: a change of the heuristic fails the assertion), and the families of
tests/decode_range.py -- (L) ordinary data at every one of those S, (S) a depth per key split, (T) per tile, (R) per packed row, (U)
per batch entry, (K) spikes at tile, split and mask edges. That the inputs are what they claim, that the kernel's arithmetic holds
the bars below on them and that a wrong one does not: tests/test_decode_range_cases.py (no GPU).

Bars (no new number): against the fp64 oracle on Q~ (util.effective_q, scale ln 2) O below 2 * TOL_O[type] -- the factor the
forward's range tests use -- and LSE, per row, below 2 * TOL_LSE[type] + 4 * 2^-23 |LSE| (EPI_L of tests/exact_forward.py: fp32
cannot hold an LSE near -960 to 1e-4); against the oracle on the true Q, util.o_tol / util.lse_tol on top of those. e4m3 inputs
(modes fp8 and kv8) are widened exactly to bf16: the bf16 bars on the e4m3 values.
Each case prints its worst error / bar per tensor and reference. Not measured on an MI355X yet: no figure is quoted here (on the CPU
model of the same arithmetic the worst ratios are 0.19 for O and 0.12 for LSE: tests/test_decode_range_cases.py prints them).
"""
import numpy as np
import pytest

import decode_range as dr
from test_gpu_decode_paged import _dev, _i32, check, expected, to_layout
from util import LN2, MFMA_VARIANTS, lse_tol, o_tol, to_dev

pytestmark = pytest.mark.gpu

Q_DTYPE = {"f16": "f16", "bf16": "bf16", "fp8": "fp8", "kv8": "bf16"}
KV_DTYPE = {"f16": "f16", "bf16": "bf16", "fp8": "fp8", "kv8": "fp8"}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


_kept = {}


def case_and_reference(oracle, family, i, build):
    """The case on the values of `build` ("f16", "bf16", "fp8") with its two fp64 references, computed once and shared by the modes and
    entry points that run it (the last one is kept)."""
    key = (family, i, build)
    if key not in _kept:
        _kept.clear()
        c = dr.FAMILIES[family][i](oracle.round_to, build)
        lens = [c.k.shape[2]] * c.q.shape[0]
        ks, vs = list(c.k), list(c.v)
        on_qt = expected(oracle, dr.q_tilde(oracle.round_to, c.q, build), ks, vs, lens, c.causal, LN2)
        on_q = expected(oracle, c.q, ks, vs, lens, c.causal)
        _kept[key] = (c, on_qt, on_q)
    return _kept[key]


def ratios(c, mode, on_qt, on_q, o, lse):
    """Worst error / bar of O and of LSE against both references; everything finite."""
    a = dr.ARITH[mode]
    on, ln = o.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    assert np.isfinite(on).all() and np.isfinite(ln).all(), (c.name, mode)
    bar_o, bar_l = dr.bars(mode, on_qt[1])
    r = [np.abs(on - on_qt[0]).max() / bar_o, (np.abs(ln - on_qt[1]) / bar_l).max(),
         np.abs(on - on_q[0]).max() / o_tol(a, 1, c.q, c.k, c.v, None, bar_o), (np.abs(ln - on_q[1]) / lse_tol(a, 1, c.q, c.k, None, bar_l)).max()]
    return [float(x) for x in r]


def paged_pool(c, P, layout, kv_dtype, rng, spare=3):
    """The case's K and V in a shuffled pool as test_gpu_decode_paged.make_cache lays it out: every page nobody references and every
    slot past Nk in a last page holds NaN. Capacity: the whole pages Nk needs."""
    B, Hkv, Nk, D = c.k.shape
    npb = (Nk + P - 1) // P
    num_pages = B * npb + spare
    perm = rng.permutation(num_pages)
    table = perm[:B * npb].reshape(B, npb).astype(np.int32)
    pools = []
    for x in (c.k, c.v):
        pool = np.full((num_pages, Hkv, P, D), np.nan, np.float32)
        pad = np.full((B, Hkv, npb * P, D), np.nan, np.float32)
        pad[:, :, :Nk] = x
        pool[table.reshape(-1)] = pad.reshape(B, Hkv, npb, P, D).transpose(0, 2, 1, 3, 4).reshape(B * npb, Hkv, P, D)
        pools.append(to_layout(pool, kv_dtype, layout))
    return pools[0], pools[1], table


CASES = [(f, i) for f in dr.FAMILIES for i in range(len(dr.FAMILIES[f]))]
PAGED_COMBOS = (((16, "HND"), (256, "NHD")), ((16, "NHD"), (256, "HND")))  # even / odd cases of a family: each sees both sizes and layouts


@pytest.mark.parametrize("mode", dr.MODES)
@pytest.mark.parametrize("family,i", CASES, ids=[f"{f}-{dr.FAMILIES[f][i].label}" for f, i in CASES])
def test_decode_range(fa, oracle_mod, family, i, mode):
    """Every case of every family through flash_attention_decode in the four modes; the families L, S, R and K also through
    flash_attention_decode_paged on a shuffled pool with NaN in every unused slot (page sizes 16 and 256, both layouts)."""
    import torch

    c, on_qt, on_q = case_and_reference(oracle_mod, family, i, dr.BUILD[mode])
    assert (family, c.name) not in dr.E4M3_LEFT_OUT
    B, Hq, Nq, D = c.q.shape
    Hkv, Nk = c.k.shape[1], c.k.shape[2]
    S = dr.splits_of(fa, B, Hq, Hkv, Nq, Nk, D)
    assert S == c.S, (c.name, S, c.S)  # the split count this case was written for
    qd = to_dev(c.q, Q_DTYPE[mode])
    o, lse = fa.flash_attention_decode(qd, to_dev(c.k, KV_DTYPE[mode]), to_dev(c.v, KV_DTYPE[mode]), is_causal=c.causal)
    torch.cuda.synchronize()
    r = ratios(c, mode, on_qt, on_q, o, lse)
    print(f"{family} {c.name} {mode} S={S} dense: O err / bar {r[0]:.3f} LSE err / bar {r[1]:.3f} (true Q: {r[2]:.3f} {r[3]:.3f})")
    assert max(r) < 1.0, (c.name, mode, r)
    if family not in dr.PAGED_FAMILIES:
        return
    rng = np.random.default_rng(1000 + i)
    for P, layout in PAGED_COMBOS[i % 2]:
        kp, vp, table = paged_pool(c, P, layout, KV_DTYPE[mode], rng)
        Sp = dr.paged_splits_of(fa, B, Hq, Hkv, Nq, D, P, table.shape[1])
        assert Sp == min(max(1, dr.tiles(P * table.shape[1]) // 4), 256) and (Sp >= 65 or Nk == 1100), (c.name, P, Sp)
        o, lse = fa.flash_attention_decode_paged(qd, kp, vp, _i32(table), _i32([Nk] * B), is_causal=c.causal, layout=layout)
        torch.cuda.synchronize()
        del kp, vp
        r = ratios(c, mode, on_qt, on_q, o, lse)
        print(f"{family} {c.name} {mode} S={Sp} paged P={P} {layout}: O err / bar {r[0]:.3f} LSE err / bar {r[1]:.3f} (true Q: {r[2]:.3f} {r[3]:.3f})")
        assert max(r) < 1.0, (c.name, mode, P, layout, r)


# ---- a paged cache sized far above what it holds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,mp", [(16, 4096), (256, 256)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", ["f16", "bf16", "kv8"])
def test_paged_capacity_far_above_the_lengths(fa, oracle_mod, mode, D, P, mp):
    """Capacity 65536 keys, lengths 0 ... 65536: S comes from the capacity, the tiles from L_b, so nearly every item of a short sequence
    is empty (t0 == t1: m = -inf, l = 0). The workspace is sized for 256 splits per (batch, key head) at both head dims -- it serves
    every dtype, and e4m3 caches run 256 items; 16-bit caches at head dim 128 run min(ceil(512 / 4), 256) = 128 of them (decode_splits()
    of fa_decode_kernel.hip), a count the workspace size does not show."""
    import torch

    from test_gpu_decode_paged import make_cache

    B, Hq, Hkv, Nq = 2, 8, 2, 4
    assert dr.paged_splits_of(fa, B, Hq, Hkv, Nq, D, P, mp) == 256
    rng = np.random.default_rng(P + D)
    qdt, kvdt = Q_DTYPE[mode], KV_DTYPE[mode]
    ws = torch.empty(fa.decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp), dtype=torch.uint8, device="cuda")
    for lens in ([0, 37], [1, 1000], [64, 65536], [65, 20000]):
        q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, D)).astype(np.float32), qdt)
        kp, vp, table, ks, vs = make_cache(oracle_mod, rng, Hkv, D, P, lens, kvdt, max_pages=mp)  # unused entries name a NaN page
        assert table.shape == (B, mp)
        qd, bt, sl = _dev(q, qdt), _i32(table), _i32(lens)
        ws.zero_()
        o, lse = fa.flash_attention_decode_paged(qd, kp, vp, bt, sl, is_causal=True, workspace=ws)
        ws.fill_(0xFF)
        o2, lse2 = fa.flash_attention_decode_paged(qd, kp, vp, bt, sl, is_causal=True, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(lse, lse2), (lens, "the workspace's contents leak")
        ln = lse.cpu().numpy()
        for b, L in enumerate(lens):  # exactly 0 / -inf for rows with no visible key (L = 0; causal: i + L < Nq)
            none = np.arange(Nq) + L < Nq
            assert np.isneginf(ln[b][:, none]).all() and np.isfinite(ln[b][:, ~none]).all(), (lens, b)
            assert o[b][:, torch.from_numpy(none)].float().abs().sum().item() == 0.0, (lens, b)
        dt = "fp8" if mode == "kv8" else mode
        check(oracle_mod, o, lse, q, ks, vs, lens, True, dt, (mode, D, P, lens), tol_o=2 * 6e-3 if mode == "kv8" else None, strict=mode != "kv8")


# ---- lse == NULL ----------------------------------------------------------------------------------------------------------------------------------
SCALAR_VARIANTS = ["naive", "tiled", "tiled_v2"]


def _same_without_lse(call, what):
    import torch

    o1, l1 = call(True)
    o2, l2 = call(False)
    torch.cuda.synchronize()
    assert l1 is not None and l2 is None, what
    assert o1.data_ptr() != o2.data_ptr() and torch.equal(o1.view(torch.uint8), o2.view(torch.uint8)), what


def _fwd_dtypes(fa, variant):
    return [d for d in ("bf16", "f16", "fp8", "f32") if fa.supported({"fp8": "fp8_e4m3"}.get(d, d), variant, 64)]


@pytest.mark.parametrize("variant", MFMA_VARIANTS + ["auto"] + SCALAR_VARIANTS)
def test_forward_without_lse_gives_the_same_output(fa, oracle_mod, variant):
    """lse == NULL (return_lse=False): every kernel guards the store; O is the bits of the call that writes the LSE."""
    assert variant in fa.VARIANTS, variant
    dtypes = _fwd_dtypes(fa, variant)
    assert dtypes, variant
    rng = np.random.default_rng(31)
    for dtype in dtypes[-1:] if variant in SCALAR_VARIANTS else dtypes:  # the scalar kernels on one type each supports (f32)
        amp = 2.0 if dtype == "fp8" else 1.0
        q, k, v = (to_dev(oracle_mod.round_to(amp * rng.uniform(-1, 1, (2, 3, 200, 64)).astype(np.float32), dtype), dtype) for _ in range(3))
        for causal in (False, True):
            _same_without_lse(lambda w: fa.flash_attention_forward(q, k, v, is_causal=causal, variant=variant, return_lse=w), (variant, dtype, causal))


@pytest.mark.parametrize("variant", ["mfma", "mfma_splitkv", "mfma_exact", "mfma16", "auto"])
def test_generalised_forward_without_lse_gives_the_same_output(fa, oracle_mod, variant):
    """Grouped heads and a rectangle (fa_fwd_exv): 8 query heads on 2 key heads, 130 queries on 300 keys."""
    rng = np.random.default_rng(32)
    for dtype in ("bf16", "f16"):
        q = to_dev(oracle_mod.round_to(rng.uniform(-1, 1, (2, 8, 130, 64)).astype(np.float32), dtype), dtype)
        k, v = (to_dev(oracle_mod.round_to(rng.uniform(-1, 1, (2, 2, 300, 64)).astype(np.float32), dtype), dtype) for _ in range(2))
        _same_without_lse(lambda w: fa.flash_attention_forward(q, k, v, is_causal=True, variant=variant, return_lse=w), (variant, dtype))


def test_varlen_without_lse_gives_the_same_output(fa, oracle_mod):
    import torch

    rng = np.random.default_rng(33)
    lens_q, lens_k = [5, 130, 1, 64], [70, 130, 300, 64]
    cq = torch.tensor(np.concatenate([[0], np.cumsum(lens_q)]), dtype=torch.int32, device="cuda")
    ck = torch.tensor(np.concatenate([[0], np.cumsum(lens_k)]), dtype=torch.int32, device="cuda")
    for dtype in ("bf16", "f16"):
        for D in (64, 128):
            q = to_dev(oracle_mod.round_to(rng.uniform(-1, 1, (sum(lens_q), 8, D)).astype(np.float32), dtype), dtype)
            k, v = (to_dev(oracle_mod.round_to(rng.uniform(-1, 1, (sum(lens_k), 2, D)).astype(np.float32), dtype), dtype) for _ in range(2))
            for causal in (False, True):
                _same_without_lse(lambda w: fa.flash_attention_varlen(q, k, v, cq, ck, max(lens_q), max(lens_k), is_causal=causal, return_lse=w),
                                  (dtype, D, causal))


@pytest.mark.parametrize("mode", dr.MODES)
def test_decode_without_lse_gives_the_same_output(fa, oracle_mod, mode):
    """The three decode entry points, at 4 and at 65 key splits."""
    from test_gpu_decode_paged import make_cache

    rng = np.random.default_rng(34)
    qdt, kvdt = Q_DTYPE[mode], KV_DTYPE[mode]
    for (Hq, Hkv, Nq, Nk, D) in ((8, 2, 4, 1100, 64), (8, 2, 1, 16704, 128)):
        assert dr.splits_of(fa, 1, Hq, Hkv, Nq, Nk, D) == dr.S_OF_NK[Nk]
        q = _dev(oracle_mod.round_to(rng.uniform(-1, 1, (1, Hq, Nq, D)).astype(np.float32), qdt), qdt)
        k, v = (_dev(oracle_mod.round_to(rng.uniform(-1, 1, (1, Hkv, Nk, D)).astype(np.float32), kvdt), kvdt) for _ in range(2))
        _same_without_lse(lambda w: fa.flash_attention_decode(q, k, v, is_causal=True, return_lse=w), (mode, Nk, "dense"))
        kp, vp, table, _, _ = make_cache(oracle_mod, rng, Hkv, D, 16, [Nk], kvdt)
        bt, sl = _i32(table), _i32([Nk])
        _same_without_lse(lambda w: fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True, return_lse=w), (mode, Nk, "paged"))


# ---- K and V beyond 4 GiB -----------------------------------------------------------------------------------------------------------------------
def test_dense_decode_with_k_and_v_beyond_4gib(fa, oracle_mod):
    """k and v are views [:, :, :Nk] of two uninitialised buffers whose batch stride puts batch entry 1 past byte 2^32 (and key head 1
    past 2^31): the same bits as the same data in compact tensors. (tests/test_gpu_decode_paged.py::test_paged_pool_over_4gib for the pool.)"""
    import torch

    B, Hq, Hkv, Nq, Nk, D = 2, 8, 2, 4, 20000, 128
    rows = (1 << 32) // (Hkv * D * 2) + 4096  # rows per head: the batch stride is just over 2^32 bytes
    rng = np.random.default_rng(35)
    q = _dev(oracle_mod.round_to(rng.uniform(-1, 1, (B, Hq, Nq, D)).astype(np.float32), "bf16"), "bf16")
    k, v = (_dev(oracle_mod.round_to(rng.uniform(-1, 1, (B, Hkv, Nk, D)).astype(np.float32), "bf16"), "bf16") for _ in range(2))
    o_lo, l_lo = fa.flash_attention_decode(q, k, v, is_causal=True)
    big_k = torch.empty(B, Hkv, rows, D, dtype=torch.bfloat16, device="cuda")  # allocated, never filled: only the used rows are written
    big_v = torch.empty_like(big_k)
    kv, vv = big_k[:, :, :Nk], big_v[:, :, :Nk]
    assert kv.stride(0) * 2 > 1 << 32 and kv[1].data_ptr() - big_k.data_ptr() > 1 << 32
    kv.copy_(k)
    vv.copy_(v)
    o_hi, l_hi = fa.flash_attention_decode(q, kv, vv, is_causal=True)
    torch.cuda.synchronize()
    assert torch.equal(o_hi, o_lo) and torch.equal(l_hi, l_lo)
    del big_k, big_v, kv, vv
