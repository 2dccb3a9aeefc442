"""Shared helpers for the parity tests (test side only: imports the oracle)."""
import numpy as np
import pytest

TORCH_DTYPE = {"f32": "float32", "f16": "float16", "bf16": "bfloat16", "fp8": "float8_e4m3fn"}


def make_qkv(oracle, B, H, N, D, dtype, seeds=(42, 43, 44), amp=1.0):
    """Independent Q,K,V ~ U(-1,1) (main.mm:24-30 generator, seeds 42/43/44), rounded RNE to dtype.

    Returns fp32 numpy arrays holding exactly-representable values of `dtype`."""
    out = []
    for s in seeds:
        x = oracle.init_random(B * H * N * D, s).reshape(B, H, N, D) * np.float32(amp)
        out.append(oracle.round_to(x, dtype))
    return out


def to_dev(x, dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, TORCH_DTYPE[dtype])).cuda()


def run_op(fa, q, k, v, dtype, causal, variant="auto", scale=None):
    import torch

    o, lse = fa.flash_attention_forward(to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype),
                                        is_causal=causal, variant=variant, scale=scale)
    torch.cuda.synchronize()
    return o.float().cpu().numpy(), lse.cpu().numpy()



# ---- the pre-scaled query operand (csrc/fa_mfma_kernel.hip; include/fa_mi355.h "LSE accuracy") ---------------------
# The 128-row matrix-core kernel and its eight-wave form multiply Q by scale*log2(e) in fp32 and round the product to the
# input type once per block: they compute the EXACT operator on that Q~ (with scale ln 2). The tests therefore hold them
# to the strict tolerances against the oracle evaluated on Q~ (effective_q below reproduces the kernel's two fp32
# multiplications and its RNE rounding bit for bit), and to the documented bound against the oracle on the true Q.
PRESCALE_EPS = {"f16": 2.0 ** -12, "bf16": 2.0 ** -9}  # half an ulp relative to the TOP of a binade (the rounding is off by up to twice
# that, 2^-11 / 2^-8 relative, just above a power of two: tests/backward_bound.py uses those; the bars below apply this eps to row norms)
LN2 = 0.6931471805599453


def is_prescaled(fa, dtype, variant, B, H, N, D, causal=False):
    """Does fa_fwd(variant) run a kernel with the pre-scaled operand for this problem?"""
    if dtype not in PRESCALE_EPS or D > 128:
        return False
    v = fa.VARIANTS[variant]
    if v == 0:
        v = fa.load_library().fa_resolve_variant_for(fa.DTYPES[dtype], D, B, H, N, int(causal))
    if v == fa.VARIANTS["mfma16"]:
        return 2  # pre-scaled operand AND row sums over the ROUNDED probabilities (rowsum_term below)
    return int(v in (fa.VARIANTS["mfma"], fa.VARIANTS["mfma_split2"], fa.VARIANTS["mfma_h64s2"]))


# The 16x16x32 kernel (csrc/fa_mfma16_kernel.hip) takes its row sums from the matrix core: l = sum of the probabilities AFTER their
# rounding to the input type (the same values the PV product multiplies, so O's weights add up to exactly 1), where the other kernels
# add the fp32 probabilities. ln(l) therefore carries the rounding of P: at most half an ulp of the input type, relative (every P moves
# by a factor within 1 +- eps), far less on average (the roundings of a row's many P values are independent). include/fa_mi355.h, "LSE accuracy".
ROWSUM_EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}


# The all-fp8 kernel (csrc/fa_fp8_kernel.hip, variant mfma_fp8pv) rounds every probability to e4m3 (3 mantissa bits) for the PV product:
# each weight moves by a factor within 1 +- 2^-4, so |O - exact| <= 2^-4 * max|V| on top of the other kernels' bar (far less where a
# row has many comparable keys: the roundings are independent).
def fp8pv_term(variant, dtype, v):
    return 2.0 ** -4 * float(np.abs(v).max()) if (variant == "mfma_fp8pv" and dtype == "fp8") else 0.0


# ... and its row sum comes out of the matrix core too (ones x the e4m3 probabilities): l adds the ROUNDED weights, each within a factor
# 1 +- 2^-4 of the exact one, so |LSE - exact| <= ln(1 + 2^-4) < 2^-4 -- reached by rows with two or three comparable keys only; the
# independent roundings of a long row average out (measured on config 5: at most 4.1e-3 over rows with more than 64 keys).
def fp8pv_lse_term(variant, dtype):
    return 2.0 ** -4 if (variant == "mfma_fp8pv" and dtype == "fp8") else 0.0


def rowsum_term(dtype, prescaled):
    return ROWSUM_EPS.get(dtype, 0.0) if prescaled == 2 else 0.0


def effective_q(oracle, q, dtype, scale=None):
    """Q~ as the kernel forms it: fp32(scale) * fp32(log2 e) -> c; fp32(q) * c; RNE to dtype. Use with scale = LN2."""
    sc = np.float32(q.shape[-1] ** -0.5 if scale is None else scale)
    c2 = np.float32(sc * np.float32(1.4426950408889634))
    return oracle.round_to((q.astype(np.float32) * c2).astype(np.float32), dtype)


def prescale_delta(dtype, q, k, scale=None):
    """Largest possible perturbation of a (natural-log) score by the operand rounding: eps * scale * max|q_i| * max|k_j|
    (one rounding of every c*q_d moves q_i.k_j by at most eps*scale*sum_d |q_d k_d| <= eps*scale*|q||k|)."""
    sc = q.shape[-1] ** -0.5 if scale is None else scale
    qn = float(np.sqrt((np.asarray(q, np.float64) ** 2).sum(-1)).max())
    kn = float(np.sqrt((np.asarray(k, np.float64) ** 2).sum(-1)).max())
    return PRESCALE_EPS[dtype] * sc * qn * kn


def lse_tol(dtype, prescaled, q, k, scale=None, base=1e-4):
    """LSE tolerance against the oracle on the TRUE Q: `base` (fp32 accumulation) plus, for the pre-scaled kernels, the bound
    the header states (LSE moves by at most the largest score perturbation)."""
    return base + rowsum_term(dtype, prescaled) + (prescale_delta(dtype, q, k, scale) if prescaled and dtype in PRESCALE_EPS else 0.0)


def o_tol(dtype, prescaled, q, k, v, scale=None, base=0.0):
    """O tolerance against the oracle on the TRUE Q: every probability moves by a factor within e^(+-delta), so
    |dO| <= 2 * (e^delta - 1) * max|v| on top of `base`."""
    if not prescaled or dtype not in PRESCALE_EPS:
        return base
    return base + 2.0 * float(np.expm1(prescale_delta(dtype, q, k, scale))) * float(np.abs(v).max())


# ---- the bars of the parity tests (tests/test_gpu_parity.py states where they come from) and the check against the oracle ----------
TOL_O = {"f32": 2e-5, "f16": 1.5e-3, "bf16": 6e-3}
TOL_LSE = {"f32": 2e-5, "f16": 1e-4, "bf16": 1e-4}
# the matrix-core kernels by name; "auto" picks by grid size
MFMA_VARIANTS = ["mfma", "mfma_splitkv", "mfma_split2", "mfma_exact", "mfma_h64s2", "mfma16", "mfma_fp8pv"]


def need(fa, dtype, variant, D):
    if not fa.supported({"fp8": "fp8_e4m3"}.get(dtype, dtype), variant, D):
        pytest.skip(f"{variant} has no kernel for {dtype} D={D}")


def check(fa, oracle, q, k, v, dtype, causal, variant, tol_scale=1.0, scale=None):
    o, lse = run_op(fa, q, k, v, dtype, causal, variant, scale)
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    pre = is_prescaled(fa, dtype, variant, *q.shape, causal)
    if pre:  # strict: the exact operator on the operand the kernel really multiplies
        o64, lse64 = oracle.attn_fwd_f64(effective_q(oracle, q, dtype, scale), k, v, causal, LN2)
        err_o, err_l = np.abs(o - o64).max(), np.abs(lse - lse64).max()
        assert err_o < TOL_O[dtype] * tol_scale, (variant, dtype, causal, q.shape, err_o, "vs oracle on Q~")
        assert err_l < TOL_LSE[dtype] * tol_scale + rowsum_term(dtype, pre), (variant, dtype, causal, q.shape, err_l, "vs oracle on Q~")
    # against the true Q: the plain tolerances, plus the documented operand-rounding bound where it applies
    o64, lse64 = oracle.attn_fwd_f64(q, k, v, causal, scale)
    err_o = np.abs(o - o64).max()
    err_l = np.abs(lse - lse64).max()
    assert err_o < o_tol(dtype, pre, q, k, v, scale, TOL_O[dtype] * tol_scale), (variant, dtype, causal, q.shape, err_o)
    assert err_l < lse_tol(dtype, pre, q, k, scale, TOL_LSE[dtype] * tol_scale), (variant, dtype, causal, q.shape, err_l)
    return err_o, err_l


def rect_reference(q, k, v, do, causal, scale=None):
    """fp64 gradients of softmax(scale * q k^T [+ bottom-right causal mask]) v for q [B,Hq,Nq,D], k / v [B,Hkv,Nk,D]; scale defaults to
    1/sqrt(D) (plain numpy: the C oracle's backward is square). dS = P o (dP - rowsum(dO o O)), kernels.metal:1160-1169."""
    B, Hq, Nq, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    G = Hq // Hkv
    sc = 1.0 / np.sqrt(D) if scale is None else float(scale)
    q64, do64 = q.astype(np.float64), do.astype(np.float64)
    ke, ve = (np.repeat(x.astype(np.float64), G, axis=1) for x in (k, v))
    s_ = (q64 @ ke.swapaxes(-1, -2)) * sc
    if causal:
        i, j = np.arange(Nq)[:, None], np.arange(Nk)[None, :]
        s_ = np.where(j <= i + (Nk - Nq), s_, -np.inf)
    p_ = np.exp(s_ - s_.max(-1, keepdims=True))
    p_ /= p_.sum(-1, keepdims=True)
    o = p_ @ ve
    dv = p_.swapaxes(-1, -2) @ do64
    dp = do64 @ ve.swapaxes(-1, -2)
    ds = p_ * (dp - (do64 * o).sum(-1, keepdims=True)) * sc
    dq = ds @ ke
    dk = ds.swapaxes(-1, -2) @ q64
    return dq, dk.reshape(B, Hkv, G, Nk, D).sum(2), dv.reshape(B, Hkv, G, Nk, D).sum(2)
