"""GPU parity where the scores of a row sit far below zero (log2 units on Q~ = round(scale*log2(e)*Q), "depth").

The 16x16x32 forward kernel (variant mfma16, and `auto` where it routes there) forms its FIRST tile's probabilities against an assumed
row maximum of 0: P' = 2^(s - BIAS). In f16 (BIAS 3) P' is subnormal below 2^-14 and zero below 2^-25, so a row whose scores lie
between about -11 and -22 would be summed from probabilities of 0 ... 10 mantissa bits unless the tile starts over from the true
maxima (FIRST_SUM_FLOOR in csrc/fa_mfma16_kernel.hip; DESIGN.md, "first tile"). test_strongly_negative_scores_from_the_first_tile_on
jumps from ordinary scores to -43 and below, where every P' is zero; these cases fill the range in between, mix depths inside one
32-row wave (the kernel's test is a wave-wide ballot: one flushed row used to rescue the 31 beside it) and pin bf16's own edge at
2^-64. Inputs: tests/score_range.py; that they are what they claim, and that the f16 cases miss the bar on the arithmetic of the
former guard: tests/test_score_range_cases.py (no GPU). Every kernel runs every case, at the bars of test_gpu_parity.py (check(),
tol_scale 2 as in the neighbouring range tests there).
"""
import hashlib

import numpy as np
import pytest

import score_range as sr
from util import LN2, MFMA_VARIANTS, TOL_LSE, TOL_O, check, effective_q, is_prescaled, lse_tol, need, o_tol, rowsum_term, to_dev

pytestmark = pytest.mark.gpu
VARIANTS = MFMA_VARIANTS + ["auto"]


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()  # raises if the HIP library is missing: no silent fallback
    return fa


class Memo:
    """The oracle module with attn_fwd_f64 remembered per input: the eight variants of one case share its two fp64 evaluations."""

    def __init__(self, oracle):
        self._oracle, self._kept = oracle, {}

    def __getattr__(self, name):
        return getattr(self._oracle, name)

    def attn_fwd_f64(self, q, k, v, is_causal, scale=None):
        key = (hashlib.blake2b(b"".join(x.tobytes() for x in (q, k, v)), digest_size=16).digest(), q.shape, bool(is_causal), scale)
        if key not in self._kept:
            if len(self._kept) >= 24:  # one (kind, dtype) worth of cases
                self._kept.clear()
            self._kept[key] = self._oracle.attn_fwd_f64(q, k, v, is_causal, scale)
        return self._kept[key]


@pytest.fixture(scope="module")
def memo(oracle_mod):
    return Memo(oracle_mod)


_built = {}


def cases_of(oracle, kind, dtype):
    if (kind, dtype) not in _built:
        _built.clear()
        _built[(kind, dtype)] = sr.KINDS[kind][0](oracle.round_to, dtype)
    return _built[(kind, dtype)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", list(sr.KINDS))
def test_score_range(fa, memo, kind, dtype, variant):
    """(a) uniform depths -6 ... -30; (b1) / (b2) a ramp 0 ... -20 / -30 inside every wave; (c) one row at a depth among ordinary ones;
    (d) identical keys; (e) causal rows with 1 ... 4 visible keys; (f) the first 64 keys at a depth, the later ones ordinary / climbing
    by 2 per tile without ever renewing the reference / 10 lower; (f-iv) the first 64 keys shallow (-2 ... -10: a first tile that is kept)
    and a thousand keys 8 lower; (g) head dims 128, 40, 104; (h) depths -55 ... -75 (bf16's floor)."""
    cases = cases_of(memo, kind, dtype)
    need(fa, dtype, variant, cases[0].q.shape[-1])
    for c in cases:
        for causal in sr.KINDS[kind][1]:
            err_o, err_l = check(fa, memo, c.q, c.k, c.v, dtype, causal, variant, tol_scale=2.0)
            print(f"{kind} {c.name} {dtype} causal={causal} {variant}: max|O err| {err_o:.2e} max|LSE err| {err_l:.2e}")


@pytest.mark.parametrize("variant", ["mfma16", "mfma", "mfma_exact", "auto"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_few_visible_keys_grouped_heads_rectangular(fa, oracle_mod, dtype, variant):
    # (e) through fa_fwd_ex: 200 queries on 300 keys (bottom-right aligned mask), 8 query heads on 2 key heads; rows 0 ... 3 of the
    # sequence and of the second 128-row block at depths -12 ... -21 among ordinary rows
    import torch

    c = sr.E_EX(oracle_mod.round_to, dtype)
    B, Hq, Nq, D = c.q.shape
    # fa_fwd_ex's AUTO (include/fa_mi355.h): at most 64 blocks of 128 query rows against more than 64 keys at head_dim 64 -> split-KV
    assert B * Hq * ((Nq + 127) // 128) <= 64
    name = "mfma_splitkv" if variant == "auto" else variant
    pre = {"mfma": 1, "mfma16": 2}.get(name, 0)
    o, lse = fa.flash_attention_forward(to_dev(c.q, dtype), to_dev(c.k, dtype), to_dev(c.v, dtype), is_causal=True, variant=variant)
    torch.cuda.synchronize()
    o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    o64, l64 = oracle_mod.attn_fwd_ex_f64(c.q, c.k, c.v, True)
    assert np.abs(o - o64).max() < o_tol(dtype, pre, c.q, c.k, c.v, None, TOL_O[dtype] * 2.0), (variant, np.abs(o - o64).max())
    assert np.abs(lse - l64).max() < lse_tol(dtype, pre, c.q, c.k, None, TOL_LSE[dtype] * 2.0), (variant, np.abs(lse - l64).max())
    if pre:  # strict vs the oracle on the operand the kernel really multiplies
        o64, l64 = oracle_mod.attn_fwd_ex_f64(effective_q(oracle_mod, c.q, dtype), c.k, c.v, True, LN2)
        assert np.abs(o - o64).max() < TOL_O[dtype] * 2.0, (variant, np.abs(o - o64).max(), "vs oracle on Q~")
        assert np.abs(lse - l64).max() < TOL_LSE[dtype] * 2.0 + rowsum_term(dtype, pre), (variant, np.abs(lse - l64).max(), "vs oracle on Q~")


@pytest.mark.parametrize("B,H,N,causal", [(4, 16, 4100, True), (1, 128, 1000, False)])
def test_eight_wave_workgroups_with_a_ramp_inside_every_wave(fa, oracle_mod, B, H, N, causal):
    # (g) the 256-row workgroups of the 16x16x32 kernel (config 3's causal grid, ragged; 512 non-causal workgroups), f16, inputs of kind
    # (b1); oracle on rows sampled across block and wave borders
    import torch

    dtype, D = "f16", 64
    lib = fa.load_library()
    assert lib.fa_resolve_variant_for(fa.DTYPES[dtype], D, B, H, N, int(causal)) == fa.VARIANTS["mfma16"]
    assert lib.fa_fwd_kernel_name(fa.DTYPES[dtype], D, B, H, N, int(causal)).decode().endswith(f"64, {'true' if causal else 'false'}, 8, false, 1>")
    c = sr.ramp(oracle_mod.round_to, dtype, N, -20.0, B=B, H=H)
    pre = is_prescaled(fa, dtype, "auto", B, H, N, D, causal)
    assert pre == 2
    rng = np.random.default_rng(9)
    for variant in ("auto", "mfma16"):
        o, lse = fa.flash_attention_forward(to_dev(c.q, dtype), to_dev(c.k, dtype), to_dev(c.v, dtype), is_causal=causal, variant=variant)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()
        for (b, h) in ((0, 0), (B - 1, H - 1)):
            rows = np.unique(np.concatenate([[0, 1, 15, 16, 31, 32, 33, 63, 64, 127, 128, 223, 224, 255, 256, 257, 287, 288, N - 257, N - 256, N - 33,
                                              N - 32, N - 1], rng.integers(0, N, 40)])).astype(np.int32)
            qh, kh, vh = c.q[b, h], c.k[b, h], c.v[b, h]
            oh, lh = o[b, h].float().cpu().numpy()[rows], lse[b, h].cpu().numpy()[rows]
            o64, l64 = oracle_mod.attn_rows_f64(effective_q(oracle_mod, qh, dtype), kh, vh, rows, causal, LN2)
            assert np.abs(oh - o64).max() < TOL_O[dtype] * 2.0, (variant, b, h, np.abs(oh - o64).max(), "vs oracle on Q~")
            assert np.abs(lh - l64).max() < TOL_LSE[dtype] * 2.0 + rowsum_term(dtype, pre), (variant, b, h, np.abs(lh - l64).max(), "vs oracle on Q~")
            o64, l64 = oracle_mod.attn_rows_f64(qh, kh, vh, rows, causal)
            assert np.abs(oh - o64).max() < o_tol(dtype, pre, qh, kh, vh, None, TOL_O[dtype] * 2.0), (variant, b, h, np.abs(oh - o64).max())
            assert np.abs(lh - l64).max() < lse_tol(dtype, pre, qh, kh, None, TOL_LSE[dtype] * 2.0), (variant, b, h, np.abs(lh - l64).max())


def test_backward_on_the_forward_lse_of_a_ramp(fa, oracle_mod):
    """(i) What the LSE feeds: the backward multiplies every probability by exp(-LSE). f16, D = 64, inputs of kind (b1), N = 300; the
    forward through `auto` and `mfma16`, flash_attention_backward on that forward's own O and LSE, against the fp64 backward with rel()
    of test_gpu_backward.py (error relative to the largest reference gradient).
    The yardstick is the same backward fed with the ORACLE's O and LSE (rounded to f16 / fp32), never the forward under test. Measured
    on MI355X, that run holds TOL (4e-3) on dK (9.3e-4 / 8.5e-4 non-causal / causal) and dV (1.1e-3 / 2.3e-4) but not on dQ: 3.85e-2 /
    2.57e-2 -- the rows of these inputs are nearly uniform over keys that are nearly alike, so dS = P (dP - delta) is a small difference
    of f16-rounded terms. Per the rule "TOL where the yardstick holds it, else twice the yardstick": dK, dV at TOL, dQ at 7.7e-2 /
    5.14e-2. (With the forward's O and LSE: dQ 4.5e-2 / 3.0e-2 through mfma16, 3.9e-2 / 1.9e-2 through auto.)"""
    import torch

    from test_gpu_backward import TOL, rel

    dtype = "f16"
    c = sr.ramp(oracle_mod.round_to, dtype, 300, -20.0)
    do = oracle_mod.round_to(np.random.default_rng(10).uniform(-1, 1, c.q.shape).astype(np.float32), dtype)
    qd, kd, vd, dod = (to_dev(x, dtype) for x in (c.q, c.k, c.v, do))
    YARDSTICK_DQ = {False: 3.85e-2, True: 2.57e-2}  # the backward on the oracle's O and LSE, measured (docstring)
    missed = []
    for causal in (False, True):
        ref = oracle_mod.attn_bwd_f64(c.q, c.k, c.v, do, causal)
        o64, l64 = oracle_mod.attn_fwd_f64(c.q, c.k, c.v, causal)
        fed = [("oracle", to_dev(o64.astype(np.float32), dtype), torch.from_numpy(l64.astype(np.float32)).cuda())]
        fed += [(variant,) + tuple(fa.flash_attention_forward(qd, kd, vd, is_causal=causal, variant=variant)) for variant in ("auto", "mfma16")]
        for source, o, lse in fed:
            grads = fa.flash_attention_backward(qd, kd, vd, o, dod, lse, is_causal=causal)
            torch.cuda.synchronize()
            for name, g, r in zip(("dq", "dk", "dv"), grads, ref):
                g = g.cpu().numpy()
                assert np.isfinite(g).all(), (source, name, causal)
                print(f"backward on the O, LSE of {source}, causal={causal}: rel {name} {rel(g, r):.3e}")
                if rel(g, r) >= (2.0 * YARDSTICK_DQ[causal] if name == "dq" else TOL[dtype]):
                    missed.append((source, name, causal, rel(g, r)))
    assert not missed, missed
