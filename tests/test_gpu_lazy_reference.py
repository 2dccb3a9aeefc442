"""GPU parity where a row RISES far above the reference the bf16 16x16x32 forward kernel holds for it (variant mfma16, and `auto` where it
routes there; mfma_exact as a control).

That kernel's bf16 hot pass at head_dim 64 (40 runs it on padded rows) has no staleness test (csrc/fa_mfma16_kernel.hip, LAZY; head_dim
128 keeps the per-tile test and runs the same cases): the row sums are looked at one tile later, a sum of
2^20 and more is renormalised by an exact power of two, and a sum that left the trusted range (2^64 and more, inf, NaN) sends the whole
workgroup through a second run in slow mode. Ordinary data reaches neither; these inputs do (tests/lazy_reference.py; that they are what
they claim, and that the scheme itself holds these bars: tests/test_lazy_reference_cases.py, no GPU). Bars: those of
test_gpu_score_range.py -- check(tol_scale=2), strict against the oracle on Q~ and documented against the oracle on Q -- over every row.
(The issue's case 5, bit-identical results with the threshold forced low, needs a second build of the library: not run here.)
"""
import numpy as np
import pytest

import lazy_reference as lz
from util import LN2, TOL_LSE, TOL_O, check, effective_q, is_prescaled, lse_tol, need, o_tol, rowsum_term, to_dev

pytestmark = pytest.mark.gpu
DT = "bf16"
VARIANTS = ["mfma16", "auto", "mfma_exact"]


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()  # raises if the HIP library is missing: no silent fallback
    return fa


_built = {}


def built(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def run_both(fa, oracle, c, variant, what):
    need(fa, DT, variant, c.q.shape[-1])
    for causal in (False, True):
        err_o, err_l = check(fa, oracle, c.q, c.k, c.v, DT, causal, variant, tol_scale=2.0)
        print(f"{what} {c.name} causal={causal} {variant}: max|O err| {err_o:.2e} max|LSE err| {err_l:.2e}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", [64, 128, 40])
@pytest.mark.parametrize("N", [300, 1100])
def test_climb(fa, oracle_mod, N, D, variant):
    """(1) key depth rises by 6 log2 units per stair from -66 to -6 (steps on tile borders in batch entry 0, mid-tile in entry 1; N = 300
    has narrower stairs so that the climb fits); the rows of every wave sit on a ramp of weights 0 ... 1: some renormalise once, some
    several times, at different tiles, some never. Four waves per workgroup (a grid of 12 ... 36 workgroups)."""
    run_both(fa, oracle_mod, built(("climb", N, D), lambda: lz.climb(oracle_mod.round_to, DT, N, D=D)), variant, "climb")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", [64, 128, 40])
@pytest.mark.parametrize("N", [300, 1100])
def test_spike(fa, oracle_mod, N, D, variant):
    """(2) one key 150 log2 units above everything else of ONE row: in a middle tile, in the workgroup's last tile (found by the test
    behind the tile loop), on the row's diagonal tile in the first wave of a workgroup. inf sums, poison, second run: the other rows
    of those workgroups, and the workgroups without a spike (head 1), hold the ordinary bars."""
    run_both(fa, oracle_mod, built(("spike", N, D), lambda: lz.spike(oracle_mod.round_to, DT, N, lz.spike_places(N), D=D)), variant, "spike")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", [64, 128, 40])
@pytest.mark.parametrize("N", [300, 1100])
def test_spike_after_a_deep_first_tile(fa, oracle_mod, N, D, variant):
    """(3) the first 64 keys at -140 (the first tile starts over on the true maxima), then ordinary keys, 130 above that reference."""
    run_both(fa, oracle_mod, built(("deep", N, D), lambda: lz.deep_first_tile(oracle_mod.round_to, DT, N, D=D)), variant, "deep first tile")


@pytest.mark.parametrize("variant", ["mfma16", "mfma_exact"])
def test_spike_grouped_heads_rectangular(fa, oracle_mod, variant):
    # (2) through fa_fwd_ex: 200 queries on 300 keys (bottom-right aligned mask), 8 query heads on 2 key heads; one spike per batch entry
    # (by name only: fa_fwd_ex's auto sends a grid of 32 such blocks to the split-KV kernel)
    import torch

    c = lz.spike(oracle_mod.round_to, DT, 200, [(150, 170), (199, 298)], Hq=8, Hkv=2, Nk=300)
    pre = {"mfma16": 2}.get(variant, 0)
    o, lse = fa.flash_attention_forward(to_dev(c.q, DT), to_dev(c.k, DT), to_dev(c.v, DT), is_causal=True, variant=variant)
    torch.cuda.synchronize()
    o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    o64, l64 = oracle_mod.attn_fwd_ex_f64(c.q, c.k, c.v, True)
    assert np.abs(o - o64).max() < o_tol(DT, pre, c.q, c.k, c.v, None, TOL_O[DT] * 2.0), (variant, np.abs(o - o64).max())
    assert np.abs(lse - l64).max() < lse_tol(DT, pre, c.q, c.k, None, TOL_LSE[DT] * 2.0), (variant, np.abs(lse - l64).max())
    if pre:
        o64, l64 = oracle_mod.attn_fwd_ex_f64(effective_q(oracle_mod, c.q, DT), c.k, c.v, True, LN2)
        assert np.abs(o - o64).max() < TOL_O[DT] * 2.0, (variant, np.abs(o - o64).max(), "vs oracle on Q~")
        assert np.abs(lse - l64).max() < TOL_LSE[DT] * 2.0 + rowsum_term(DT, pre), (variant, np.abs(lse - l64).max(), "vs oracle on Q~")


@pytest.mark.parametrize("B,H,N,causal", [(4, 16, 4100, True), (1, 128, 1000, False)])
def test_eight_wave_workgroups(fa, oracle_mod, B, H, N, causal):
    """The 256-row workgroups (config 3's causal grid, ragged; 512 non-causal workgroups). Head (0, 0): the climb of (1). Head
    (B - 1, H - 1): a spike in a single row of a single wave, the other seven waves of that workgroup ordinary, mid-sequence, plus one in
    the sequence's last tile. Head (0, 1): ordinary. The oracle on rows sampled across wave and workgroup borders and on the spiked rows."""
    import torch

    D = 64
    lib = fa.load_library()
    assert lib.fa_resolve_variant_for(fa.DTYPES[DT], D, B, H, N, int(causal)) == fa.VARIANTS["mfma16"]
    assert lib.fa_fwd_kernel_name(fa.DTYPES[DT], D, B, H, N, int(causal)).decode().endswith(f"64, {'true' if causal else 'false'}, 8, false, 1>")
    rt = oracle_mod.round_to
    rng = np.random.default_rng(21)
    q, k, v = (rt(rng.uniform(-1, 1, (B, H, N, D)).astype(np.float32), DT) for _ in range(3))
    cl = lz.climb(rt, DT, N, H=1)
    q[0, 0], k[0, 0], v[0, 0] = cl.q[0, 0], cl.k[0, 0], cl.v[0, 0]
    spike_rows = [(N // 2 // 256 * 256 + 70, N // 2 // 256 * 256 - 200), (N - 2, N - 3)]
    for row, key in spike_rows:  # one workgroup each
        sp = lz.spike(rt, DT, N, [(row, key)], Hq=1, seed=22 + row)
        q[B - 1, H - 1, row], k[B - 1, H - 1, key] = sp.q[0, 0, row], sp.k[0, 0, key]
    u = lz.unit(D)
    others = np.setdiff1d(np.arange(N), [r for r, _ in spike_rows])
    q[B - 1, H - 1, others] = rt(q[B - 1, H - 1, others] - (q[B - 1, H - 1, others] @ u)[:, None] * u, DT)
    pre = is_prescaled(fa, DT, "auto", B, H, N, D, causal)
    assert pre == 2
    for variant in ("auto", "mfma16"):
        o, lse = fa.flash_attention_forward(to_dev(q, DT), to_dev(k, DT), to_dev(v, DT), is_causal=causal, variant=variant)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()
        for (b, h) in ((0, 0), (B - 1, H - 1), (0, 1)):
            rows = np.unique(np.concatenate([[0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, 223, 224, 255, 256, 257, 287, 288, N - 257, N - 256, N - 33,
                                              N - 32, N - 1], [r + d for r, _ in spike_rows for d in (-33, -1, 0, 1, 31) if r + d < N],
                                             rng.integers(0, N, 40)])).astype(np.int32)
            qh, kh, vh = q[b, h], k[b, h], v[b, h]
            oh, lh = o[b, h].float().cpu().numpy()[rows], lse[b, h].cpu().numpy()[rows]
            o64, l64 = oracle_mod.attn_rows_f64(effective_q(oracle_mod, qh, DT), kh, vh, rows, causal, LN2)
            assert np.abs(oh - o64).max() < TOL_O[DT] * 2.0, (variant, b, h, np.abs(oh - o64).max(), "vs oracle on Q~")
            assert np.abs(lh - l64).max() < TOL_LSE[DT] * 2.0 + rowsum_term(DT, pre), (variant, b, h, np.abs(lh - l64).max(), "vs oracle on Q~")
            o64, l64 = oracle_mod.attn_rows_f64(qh, kh, vh, rows, causal)
            assert np.abs(oh - o64).max() < o_tol(DT, pre, qh, kh, vh, None, TOL_O[DT] * 2.0), (variant, b, h, np.abs(oh - o64).max())
            assert np.abs(lh - l64).max() < lse_tol(DT, pre, qh, kh, None, TOL_LSE[DT] * 2.0), (variant, b, h, np.abs(lh - l64).max())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", [300, 1100])
def test_non_finite_inputs(fa, oracle_mod, N, variant):
    """(4) one +inf and one NaN element in K, each seen by one row only (the last key of a head, under the mask). The call returns, the
    two rows are inf / NaN and every other row holds the bars (the oracle on K with the two elements zeroed: no other row sees them)."""
    import torch

    c, clean = lz.non_finite(oracle_mod.round_to, DT, N)
    o, lse = fa.flash_attention_forward(to_dev(c.q, DT), to_dev(c.k, DT), to_dev(c.v, DT), is_causal=True, variant=variant)
    torch.cuda.synchronize()
    o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
    hit = np.zeros(lse.shape, bool)
    for (b, h, row, _) in c.spikes:
        hit[b, h, row] = True
        assert not np.isfinite(o[b, h, row]).any() and not np.isfinite(lse[b, h, row]), (variant, b, h, o[b, h, row][:4], lse[b, h, row])
    assert np.isfinite(o[~hit]).all() and np.isfinite(lse[~hit]).all()
    pre = is_prescaled(fa, DT, variant, *c.q.shape, True)
    o64, l64 = oracle_mod.attn_fwd_f64(effective_q(oracle_mod, c.q, DT) if pre else c.q, clean, c.v, True, LN2 if pre else None)
    assert np.abs(o - o64)[~hit].max() < TOL_O[DT] * 2.0, (variant, np.abs(o - o64)[~hit].max())
    assert np.abs(lse - l64)[~hit].max() < TOL_LSE[DT] * 2.0 + rowsum_term(DT, pre), (variant, np.abs(lse - l64)[~hit].max())
