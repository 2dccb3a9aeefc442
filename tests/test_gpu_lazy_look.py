"""GPU parity around the POSITION of the look at the row sums in the bf16 16x16x32 forward kernel (variant mfma16, and `auto` where it
routes there; mfma_exact as a control).

The kernel's bf16 hot pass at head_dim 64 (40 runs it on padded rows) looks at the row sums inside the PV product -- the sums of the
tiles before this one -- and repairs behind the product's last MFMA (csrc/fa_mfma16_kernel.hip, FA16_LOOK): a rise in tile t is
repaired behind tile t + 1, a rise in a wave's last tile stays pending into the epilogue, and a sum that leaves the trusted range while
a repair is pending sends the workgroup through the slow run. Inputs: tests/lazy_look.py; that they are what they claim, which rows
repair where, and that the scheme holds these bars: tests/test_lazy_look_cases.py (no GPU). Bars: those of test_gpu_lazy_reference.py
-- check(tol_scale=2), strict against the oracle on Q~ and documented against the oracle on Q -- over every row.
Shapes: 3 ... 5 tiles of 64 keys, four-wave workgroups, B = 2, H = 2 (head 1 is ordinary: the other workgroups hold the ordinary bars).
"""
import numpy as np
import pytest

import lazy_look as ll
from util import LN2, TOL_LSE, TOL_O, check, effective_q, is_prescaled, lse_tol, need, o_tol, rowsum_term, to_dev

pytestmark = pytest.mark.gpu
DT = "bf16"
VARIANTS = ["mfma16", "auto", "mfma_exact"]
NS, DS = (192, 256, 320), (64, 40)


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


def run_both(fa, oracle, c, variant):
    need(fa, DT, variant, c.q.shape[-1])
    for causal in (False, True):
        err_o, err_l = check(fa, oracle, c.q, c.k, c.v, DT, causal, variant, tol_scale=2.0)
        print(f"{c.name} causal={causal} {variant}: max|O err| {err_o:.2e} max|LSE err| {err_l:.2e}")


def cases_t(last_offset):
    """(N, D, t, variant); the control has no kernel for the padded head dim."""
    return [(N, D, t, v) for N in NS for D in DS for t in range(ll.last_tile(N) + 1 - last_offset) for v in VARIANTS if not (v == "mfma_exact" and D == 40)]


@pytest.mark.parametrize("N,D,t,variant", cases_t(0))
def test_one_rise(fa, oracle_mod, N, D, t, variant):
    """(1) a rise of +24 (a sum of 2^24: repaired, far below 2^64) at tile t, every t from 0 to the last tile -- the last one leaves the
    repair pending when the tile loop ends. Batch entry 0: one row of a wave; entry 1: all 32 rows of a wave on wave_ramp weights."""
    run_both(fa, oracle_mod, built(("one", N, D, t), lambda: ll.one_rise(oracle_mod.round_to, DT, N, D, t)), variant)


@pytest.mark.parametrize("N,D,t,variant", cases_t(1))
def test_rise_then_out_of_range(fa, oracle_mod, N, D, t, variant):
    """(2) the rise at tile t, then at tile t + 1 (the last tile included) a key 150 units higher in the same row: the sum leaves the
    trusted range while a repair is pending, the workgroup takes the slow run; its other rows and the other workgroups hold the bars."""
    run_both(fa, oracle_mod, built(("out", N, D, t), lambda: ll.rise_then_out(oracle_mod.round_to, DT, N, D, t)), variant)


@pytest.mark.parametrize("N,D,t,variant", cases_t(1))
def test_two_rises_in_consecutive_tiles(fa, oracle_mod, N, D, t, variant):
    """(3) +30 at tile t and +30 more at tile t + 1: two repairs of 2^-30 or one of 2^-60, legal with either lag -- the result is tested."""
    run_both(fa, oracle_mod, built(("two", N, D, t), lambda: ll.two_rises(oracle_mod.round_to, DT, N, D, t)), variant)


@pytest.mark.parametrize("N,D,variant", [(N, D, v) for N in (256, 320) for D in DS for v in VARIANTS if not (v == "mfma_exact" and D == 40)])
def test_rise_on_the_diagonal_tile_and_in_a_skipped_tile(fa, oracle_mod, N, D, variant):
    """(4) the rise on the wave's own diagonal tile under the mask, and in a tile the lower waves of the workgroup skip."""
    run_both(fa, oracle_mod, built(("diag", N, D), lambda: ll.diagonal_and_skipped(oracle_mod.round_to, DT, N, D)), variant)


@pytest.mark.parametrize("B,H,N,causal", [(1, 128, 1024, False), (4, 16, 4096, True)])
def test_eight_wave_workgroups(fa, oracle_mod, B, H, N, causal):
    """(5) the 256-row workgroups. Head (0, 0): case (1) in the middle of the sequence, one row and a ramp over another wave. Head
    (B - 1, H - 1): case (2). Head (0, 1): ordinary. The oracle on sampled rows (workgroup and wave borders, the events' rows)."""
    import torch

    D = 64
    lib = fa.load_library()
    assert lib.fa_resolve_variant_for(fa.DTYPES[DT], D, B, H, N, int(causal)) == fa.VARIANTS["mfma16"]
    assert lib.fa_fwd_kernel_name(fa.DTYPES[DT], D, B, H, N, int(causal)).decode().endswith(f"64, {'true' if causal else 'false'}, 8, false, 1>")
    top = N - 256  # the last workgroup: its waves see every tile under the mask
    t = (N // 2) // 64
    ev = [(0, 0, [top + 70], [1.0], 64 * t + 3, ll.RISE), (0, 0, np.arange(top + 160, top + 192), ll.wave_ramp(32), 64 * t + 3, ll.RISE),
          (B - 1, H - 1, [top + 70], [1.0], 64 * t + 3, ll.RISE), (B - 1, H - 1, [top + 70], [1.0], 64 * (t + 1) + 5, ll.RISE + ll.OUT)]
    c = ll.build(oracle_mod.round_to, DT, (B, H, N, D), ev, seed=32)
    pre = is_prescaled(fa, DT, "auto", B, H, N, D, causal)
    assert pre == 2
    rng = np.random.default_rng(33)
    for variant in ("auto", "mfma16"):
        o, lse = fa.flash_attention_forward(to_dev(c.q, DT), to_dev(c.k, DT), to_dev(c.v, DT), is_causal=causal, variant=variant)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()
        for (b, h) in ((0, 0), (B - 1, H - 1), (0, 1)):
            rows = np.unique(np.concatenate([[0, 31, 32, 255, 256, top - 1, top, top + 31, top + 32, top + 69, top + 70, top + 71, top + 127, top + 128,
                                              top + 255], np.arange(top + 160, top + 192), rng.integers(0, N, 24)])).astype(np.int32)
            qh, kh, vh = c.q[b, h], c.k[b, h], c.v[b, h]
            oh, lh = o[b, h].float().cpu().numpy()[rows], lse[b, h].cpu().numpy()[rows]
            o64, l64 = oracle_mod.attn_rows_f64(effective_q(oracle_mod, qh, DT), kh, vh, rows, causal, LN2)
            assert np.abs(oh - o64).max() < TOL_O[DT] * 2.0, (variant, b, h, np.abs(oh - o64).max(), "vs oracle on Q~")
            assert np.abs(lh - l64).max() < TOL_LSE[DT] * 2.0 + rowsum_term(DT, pre), (variant, b, h, np.abs(lh - l64).max(), "vs oracle on Q~")
            o64, l64 = oracle_mod.attn_rows_f64(qh, kh, vh, rows, causal)
            assert np.abs(oh - o64).max() < o_tol(DT, pre, qh, kh, vh, None, TOL_O[DT] * 2.0), (variant, b, h, np.abs(oh - o64).max())
            assert np.abs(lh - l64).max() < lse_tol(DT, pre, qh, kh, None, TOL_LSE[DT] * 2.0), (variant, b, h, np.abs(lh - l64).max())
