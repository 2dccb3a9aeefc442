"""How far a FORWARD kernel's O and LSE may lie from the exact ones, per row and per element (test side only; pure numpy, fp64).

tests/backward_bound.py bounds the backward's gradients given lse_err [Nq] >= |lse_in - exact| and o_err [Nq, D] >= |o_in - exact O|. This
module supplies the two for the O and LSE a forward route of include/fa_mi355.h writes, from the inputs, the fp64 intermediates and
the NAME of the route -- never from a kernel's output. tests/test_chain_bound_model.py checks the derivation on the CPU against an
fp32 model of the kernels' online softmax; tests/test_gpu_chain.py holds forward -> backward chains on the GPU to the result.

lse_err_i, from the header's "LSE accuracy" / "fp8 probabilities" as stated:
    1e-4                                                       every route
  + eps * scale * |q_i|_2 * max_j |k_j|_2                      the pre-scaled query operand (eps = 2^-9 bf16 / 2^-12 f16): mfma, mfma_split2,
                                                               mfma_h64s2, mfma16 with f16 / bf16 inputs at D <= 128
  + 2^-8 (bf16) / 2^-11 (f16)                                  mfma16: its row sum adds the ROUNDED probabilities
  + n_i * 2^-22                                                f16 mfma16: n_i = visible scores of row i more than 11 log2 units below the
                                                               row maximum (rounded with fewer bits); low_probability_rows(): asserted 0 in the GPU cases that do not say otherwise
  + ln(1 + 2^-4)                                               mfma_fp8pv: e4m3 probabilities in the row sum (flat, as the header states it)
o_err_id. The kernel's O is sum_j P~_ij v_jd / l~_i with P~_ij = P_ij e^(+-d_i) (1 +- u_p) (operand rounding, rounding of P into the PV
product) and l~_i = l_i e^(+-d_i) (1 +- u_l); both sums in fp32 (one addition per key, one rescale per tile), the result rounded to
the output type. With A_id = sum_j P_ij |v_jd| >= |O_id|:
    o_err_id = u_out |O_id| + (u_p + u_l + expm1(2 d_i) + 2^-24 (visible_i + tiles)) * A_id
  u_out  2^-11 f16 / 2^-8 bf16 (e4m3 inputs: bf16 O); an f16 O below 2^-14 is subnormal, rounded absolutely: max(u_out |O|, 2^-25)
  u_p    u of the input type (e4m3 inputs: the probabilities are bf16, 2^-8), 2^-4 for mfma_fp8pv
  u_l    u_p where the row sum adds rounded probabilities (mfma16, mfma_fp8pv), else 0 (the fp32 term covers it)
  d_i    max_j d_ij, d_ij = u * scale * sum_d |q_id||k_jd| as in backward_bound.py, for the pre-scaled routes, else 0
  + 2 (S + 3) 2^-24 A_id for the routes that merge S key splits (tests/exact_forward.py): S = 2 mfma_split2 / mfma_h64s2, 8 mfma_splitkv
  + n_i 2^-22 * (max_j |v_jd| + |O_id|) for the low probabilities of f16 mfma16 above (numerator and row sum)
A route that may run one of several kernels (AUTO of fa_fwd_ex, for which no resolver is exported) takes the largest of each term.
"""
from collections import namedtuple

import numpy as np

import backward_bound as bb

LOG2E = 1.4426950408889634
PRESCALE_EPS = {"f16": 2.0 ** -12, "bf16": 2.0 ** -9}
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp8": 2.0 ** -8}
TILE = 64

# what a forward kernel rounds: pre-scaled operand, row sum over rounded probabilities, e4m3 probabilities, key splits it merges
Kernel = namedtuple("Kernel", "prescaled sum_rounded fp8pv splits")
KERNELS = {
    "mfma": Kernel(True, False, False, 0), "mfma_exact": Kernel(False, False, False, 0), "mfma16": Kernel(True, True, False, 0),
    "mfma_splitkv": Kernel(False, False, False, 8), "mfma_split2": Kernel(True, False, False, 2), "mfma_h64s2": Kernel(True, False, False, 2),
    "mfma_fp8pv": Kernel(False, True, True, 0)}
EX_AUTO = ("mfma_splitkv", "mfma16", "mfma")  # fa_fwd_ex's rule picks among these (mfma16: f16 / bf16 only)


def kernels_of(route, dtype, ex=False):
    """The kernels a named route may run: itself; AUTO of fa_fwd_ex: every kernel of its rule. AUTO of fa_fwd is resolved by the caller
    (fa_resolve_variant_for) and passed by name."""
    if route == "auto":
        assert ex, "resolve fa_fwd's AUTO with fa_resolve_variant_for and pass the kernel's name"
        return [n for n in EX_AUTO if not (n == "mfma16" and dtype == "fp8")]
    return [route]


def _prescaled(kern, dtype, D):
    return kern.prescaled and dtype in PRESCALE_EPS and D <= 128


def log2_scores(q, k, causal, scale):
    """(s [Nq, Nk] in log2 units with -inf on masked pairs, visible [Nq, Nk]) of one head, fp64."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    Nq, Nk = q.shape[0], k.shape[0]
    vis = np.ones((Nq, Nk), bool) if not causal else np.arange(Nk)[None, :] <= np.arange(Nq)[:, None] + (Nk - Nq)
    return np.where(vis, (q @ k.T) * (scale * LOG2E), -np.inf), vis


def _low(s2, vis, below):
    return ((s2 < s2.max(1, keepdims=True) - below) & vis).sum(1)


def head_errors(q, k, v, causal, scale, dtype, kernels, R):
    """(lse_err [Nq], o_err [Nq, D]) of the module docstring for one head: q [Nq, D], k, v [Nk, D], R = bb.head_exact(...) (exact p, o),
    kernels = names (or Kernel tuples) of the kernels the route may run."""
    kerns = [KERNELS[x] if isinstance(x, str) else x for x in kernels]
    aq, ak, av = (np.abs(np.asarray(x, np.float64)) for x in (q, k, v))
    Nq, D = aq.shape
    Nk = ak.shape[0]
    u = bb.U[dtype]
    s2, vis = log2_scores(q, k, causal, scale)
    nvis = vis.sum(1)
    tiles = (Nk + TILE - 1) // TILE
    A = R["p"] @ av
    ao = np.abs(R["o"])
    out_round = U_OUT[dtype] * ao
    if dtype == "f16":
        out_round = np.maximum(out_round, 2.0 ** -25)
    qn, kn = np.sqrt((aq ** 2).sum(-1)), float(np.sqrt((ak ** 2).sum(-1)).max())
    dmax = (u * scale * np.where(vis, aq @ ak.T, 0.0)).max(1)
    vmax = av.max(0)[None, :]
    lse_err, o_err = np.zeros(Nq), np.zeros((Nq, D))
    for kern in kerns:
        pre = _prescaled(kern, dtype, D)
        le = np.full(Nq, 1e-4)
        if pre:
            le += PRESCALE_EPS[dtype] * scale * qn * kn
        u_p = 2.0 ** -4 if kern.fp8pv else u
        u_l = u_p if kern.sum_rounded else 0.0
        low = np.zeros(Nq)
        if kern.fp8pv:
            le += np.log1p(2.0 ** -4)
        elif kern.sum_rounded:
            le += u
            if dtype == "f16":
                low = _low(s2, vis, 11.0) * 2.0 ** -22
        le += low
        d = dmax if pre else 0.0
        rel = u_p + u_l + np.expm1(2.0 * d) + bb.U32 * (nvis + tiles) + (2 * (kern.splits + 3) * bb.U32 if kern.splits else 0.0)
        oe = out_round + rel[:, None] * A + low[:, None] * (vmax + ao)
        lse_err, o_err = np.maximum(lse_err, le), np.maximum(o_err, oe)
    return lse_err, o_err


def low_probability_rows(q, k, causal, scale, below=11.0):
    """Over [B,Hq,Nq,D] / [B,Hkv,Nk,D] inputs: the largest number of visible scores of one row more than `below` log2 units under its
    row maximum (f16 mfma16's documented low-probability term is zero where this is 0)."""
    G = q.shape[1] // k.shape[1]
    worst = 0
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            s2, vis = log2_scores(q[b, h], k[b, h // G], causal, scale)
            worst = max(worst, int(_low(s2, vis, below).max()))
    return worst


def errors(q, k, v, causal, scale, dtype, kernels):
    """lse_err [B,Hq,Nq], o_err [B,Hq,Nq,D] for q [B,Hq,Nq,D], k / v [B,Hkv,Nk,D] (fp32 arrays of values of the type)."""
    scale = bb.default_scale(q.shape[-1]) if scale is None else float(scale)
    G = q.shape[1] // k.shape[1]
    lse_err, o_err = np.zeros(q.shape[:3]), np.zeros(q.shape)
    zero = np.zeros(q.shape[2:])
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            R = bb.head_exact(q[b, h], k[b, h // G], v[b, h // G], zero, causal, scale)
            lse_err[b, h], o_err[b, h] = head_errors(q[b, h], k[b, h // G], v[b, h // G], causal, scale, dtype, kernels, R)
    return lse_err, o_err
