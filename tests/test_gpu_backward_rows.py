"""The backward against the fp64 oracle, ELEMENT BY ELEMENT: |g - ref| <= bound for every entry of dQ, dK, dV, with the componentwise
bound of tests/backward_bound.py (derived from the roundings csrc/fa_bwd_kernels.hip documents; no fitted factor; shown on the CPU
by tests/test_backward_bound_model.py to hold for a model of those roundings and to catch a list of sabotages that the whole-tensor
measure of tests/test_gpu_backward.py lets through).

The backward is judged alone: O (rounded to the type) and LSE (fp32) are the ORACLE's, as in test_backward_any_multiple_of_eight.
ref: oracle.attn_bwd_f64 (square, ungrouped) or util.rect_reference (fp64 numpy). Every case prints its worst err / bound per tensor.

Measured on the MI355X (worst err / bound over all cases of this file, per tensor; profiles/r07/gpu_suite_smoke_bench.log):
              dQ     dK     dV
    bf16    0.381  0.607  0.588     (dK: N = 1100, D = 8, causal; the numpy model of the roundings: 0.59)
    f16     0.355  0.738  0.868     (dK, dV: scale 1.0 at D = 256 -- scores of +-10, a softmax with one visible weight: a gradient row
    e4m3    0.206  0.242  0.312      is ONE product there, and a single rounding of P or dS just above a power of two attains u)
  by family (max over dQ, dK, dV; bf16 / f16): square 0.61 / 0.55, scales 0.57 / 0.87, grouped 0.31 / 0.30, Nq != Nk 0.42 / 0.46,
  inputs x3 0.29 / 0.53, dO x 2^-8 0.27 / 0.44 (f16: every dS subnormal -- kept, not flushed), padded views 0.35 / 0.32.
The bound leaves out what is fp32 on the way to P: the fp32 rounding of the LSE input and of LSE*log2(e) (2^-23 |lse| on the exponent),
v_exp_f32 (1 ulp) and the fp32 accumulation of the score chain -- together below 1e-5 relative on P against u >= 4.9e-4.
"""
import numpy as np
import pytest

import backward_bound as bb
from util import make_qkv, rect_reference, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available()
    fa.load_library()
    return fa


def inputs(oracle, dtype, B, Hq, Hkv, Nq, Nk, D, amp=1.0, do_mul=1.0):
    """The suite's generator (seeds 42 / 43 / 44, dO 45), rounded to the type; amp scales Q and K (e4m3: V too, the suite's e4m3 family)."""
    q, _, _ = make_qkv(oracle, B, Hq, Nq, D, dtype, amp=amp)
    _, k, v = make_qkv(oracle, B, Hkv, Nk, D, dtype, amp=amp)
    if amp != 1.0 and dtype != "fp8":
        v = make_qkv(oracle, B, Hkv, Nk, D, dtype)[2]
    do_t = "bf16" if dtype == "fp8" else dtype
    do = oracle.round_to(oracle.init_random(B * Hq * Nq * D, 45).reshape(B, Hq, Nq, D) * np.float32(do_mul), do_t)
    return q, k, v, do


def padded(x, dtype, extra_rows, extra_heads):
    """x as a view into a larger buffer of NaNs (head stride > N*D, batch stride > H * head stride)."""
    import torch

    from util import TORCH_DTYPE

    b, h, n, d = x.shape
    tdt = getattr(torch, TORCH_DTYPE[dtype])
    buf = torch.full((b, h + extra_heads, n + extra_rows, d), float("nan"), dtype=torch.float32, device="cuda").to(tdt)
    assert torch.isnan(buf.float()).all()
    view = buf[:, :h, :n]
    view.copy_(to_dev(x, dtype))
    return view


def run_case(fa, oracle, dtype, B, Hq, Hkv, Nq, Nk, D, causal, scale=None, amp=1.0, do_mul=1.0, pad=False, tag=""):
    import torch

    q, k, v, do = inputs(oracle, dtype, B, Hq, Hkv, Nq, Nk, D, amp, do_mul)
    X = bb.Bounds(q, k, v, do, causal, scale, dtype)
    odt = "bf16" if dtype == "fp8" else dtype
    o = oracle.round_to(X.o.astype(np.float32), odt)
    lsed = torch.from_numpy(X.lse.astype(np.float32)).cuda()
    if pad:  # Q / O / dO under one stride pair, K / V under another
        qd, od, dod = padded(q, dtype, 8, 1), padded(o, odt, 8, 1), padded(do, odt, 8, 1)
        kd, vd = padded(k, dtype, 24, 2), padded(v, dtype, 24, 2)
        assert qd.stride() == od.stride() == dod.stride() and kd.stride() == vd.stride() and not qd.is_contiguous()
    else:
        qd, kd, vd, od, dod = to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype), to_dev(o, odt), to_dev(do, odt)
    dq, dk, dv = fa.flash_attention_backward(qd, kd, vd, od, dod, lsed, is_causal=causal, scale=scale)
    torch.cuda.synchronize()
    assert dq.shape == qd.shape and dk.shape == kd.shape and dv.shape == kd.shape and dq.dtype == torch.float32
    g = [t.cpu().numpy() for t in (dq, dk, dv)]
    if Nq == Nk and Hq == Hkv:
        ref = oracle.attn_bwd_f64(q, k, v, do, causal, scale)
    else:
        ref = rect_reference(q, k, v, do, causal, bb.default_scale(D) if scale is None else scale)
    for a, b in zip(ref, X.ref):  # (the bound's own fp64 gradients agree with the reference: the oracle takes the scale as an fp32)
        assert np.abs(a - b).max() <= 1e-6 * max(np.abs(b).max(), 1e-30)
    r = bb.ratios(g, ref, X.bound)
    print(f"BWDROWS {dtype} {tag} B{B} Hq{Hq} Hkv{Hkv} Nq{Nq} Nk{Nk} D{D} causal={int(causal)} scale={scale} amp={amp} do_mul={do_mul} pad={int(pad)}"
          f" | err/bound dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
    for name, x, gg in zip(("dq", "dk", "dv"), r, g):
        assert np.isfinite(gg).all(), (name, tag)
        assert x <= 1.0, (name, dtype, tag, (B, Hq, Hkv, Nq, Nk, D), causal, scale, x)
    return r


LONG = 1100  # nine 128-blocks with a ragged tail: the causal block order (map_block_div), t_begin, first / last tiles of many blocks


@pytest.mark.parametrize("D", [64, 128, 256, 32, 96, 8, 40, 120])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_rows_within_bound(fa, oracle_mod, dtype, causal, D):
    for (B, H, N) in ((1, 1, 1), (1, 2, 63), (1, 2, 65), (2, 2, 129), (2, 3, 200), (1, 2, 520), (1, 1 if D == 256 else 2, LONG)):
        run_case(fa, oracle_mod, dtype, B, H, H, N, N, D, causal, tag="square")


@pytest.mark.parametrize("scale", [None, 0.05, 0.3, 1.0])
@pytest.mark.parametrize("D", [64, 128, 40, 256, 96])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_custom_scale(fa, oracle_mod, dtype, D, scale):
    """The kernels use the scale twice (operand pre-scaling by scale*log2e, then * scale on the finished dQ / dK)."""
    for causal in (False, True):
        run_case(fa, oracle_mod, dtype, 1, 2, 2, 203, 203, D, causal, scale=scale, tag="scale")
    run_case(fa, oracle_mod, dtype, 1, 4, 2, 130, 200, D, True, scale=scale, tag="scale-gqa-rect")


@pytest.mark.parametrize("D", [64, 128, 256, 40, 96])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_rows_grouped_heads_and_rectangular(fa, oracle_mod, dtype, causal, D):
    """Grouped heads G = 2, 4, 8 (Hkv = 1) and Nq != Nk with coff = Nk - Nq of 1, 63, 64, 160 and > 256; more queries than keys without mask."""
    for (B, Hq, Hkv, N) in ((1, 4, 2, 200), (2, 4, 1, 129), (1, 8, 1, 130)):
        run_case(fa, oracle_mod, dtype, B, Hq, Hkv, N, N, D, causal, tag="gqa")
    for (B, Hq, Hkv, Nq, Nk) in ((1, 2, 2, 130, 131), (1, 2, 1, 66, 129), (2, 4, 2, 64, 128), (1, 2, 2, 100, 260), (1, 2, 1, 200, 500), (1, 1, 1, 1, 300)):
        run_case(fa, oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D, causal, tag="rect")
    if not causal:
        for (B, Hq, Hkv, Nq, Nk) in ((1, 2, 2, 260, 100), (1, 4, 1, 200, 1), (1, 2, 1, 300, 129)):
            run_case(fa, oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D, False, tag="rect-nq>nk")


@pytest.mark.parametrize("D", [64, 128, 256, 40])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_larger_logits(fa, oracle_mod, dtype, D):
    """Q and K three times the suite's (scores up to about +-20): expm1(d_ij) is no longer small."""
    for causal in (False, True):
        run_case(fa, oracle_mod, dtype, 1, 2, 2, 300, 300, D, causal, amp=3.0, tag="x3")
    run_case(fa, oracle_mod, dtype, 1, 4, 2, 200, 330, D, True, amp=3.0, tag="x3-gqa-rect")


@pytest.mark.parametrize("D", [64, 128, 256, 40])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_small_d_o(fa, oracle_mod, dtype, D):
    """dO = the suite's times 2^-8: in f16 every dS is subnormal (absolute rounding: the bound's t term). A kernel that flushed
    subnormal f16 values to zero would miss the bound by up to 2^11 -- the regime of f16 training without loss scaling."""
    for causal in (False, True):
        run_case(fa, oracle_mod, dtype, 1, 2, 2, 300, 300, D, causal, do_mul=2.0 ** -8, tag="small-dO")


@pytest.mark.parametrize("D", [64, 128, 32, 96])
@pytest.mark.parametrize("causal", [False, True])
def test_rows_e4m3_inputs_padded_strides(fa, oracle_mod, causal, D):
    """e4m3 Q, K, V (bf16 arithmetic on the exactly widened copies: u = 2^-8) as views into NaN-filled padded buffers -- the workspace
    layout of the widened copies is computed from the strides --, and on contiguous tensors."""
    for pad in (True, False):
        for (B, Hq, Hkv, Nq, Nk) in ((1, 2, 2, 200, 200), (2, 4, 2, 129, 129), (1, 2, 1, 100, 260)):
            run_case(fa, oracle_mod, "fp8", B, Hq, Hkv, Nq, Nk, D, causal, amp=2.0, pad=pad, tag="e4m3")


@pytest.mark.parametrize("D", [64, 128, 256, 40, 96])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_rows_padded_views(fa, oracle_mod, dtype, causal, D):
    """Q / O / dO as views into one kind of padded buffer, K / V into another (NaN in the padding), one shape per instantiation."""
    run_case(fa, oracle_mod, dtype, 2, 4, 2, 200, 200, D, causal, pad=True, tag="padded")
    run_case(fa, oracle_mod, dtype, 2, 2, 2, 130, 333, D, causal, pad=True, tag="padded-rect")
