"""A componentwise forward-error bound for the backward's three gradients (test side only; pure numpy, fp64).

tests/test_backward_bound_model.py shows on the CPU that a numpy model of the kernels' roundings stays inside it and that a list
of sabotaged gradients does not; tests/test_gpu_backward_rows.py / test_gpu_backward_probes.py hold the GPU kernels to it, element
by element. The bound is derived from what csrc/fa_bwd_kernels.hip documents that it rounds -- never from its output -- and has
no fitted factor.

What the kernels round (fa_bwd_kernels.hip, header and the two kernels):
  * the operand held in registers is multiplied by scale*log2(e) and rounded to the 16-bit type once: Q~ in the dQ kernel, K~ in
    the dK/dV kernel. With u the unit roundoff of that type (2^-8 bf16, 2^-11 f16: round-to-nearest is off by up to half an ulp,
    which is u relative just above a power of two), score (i, j) moves by at most
        d_ij = u * scale * sum_d |q_id| |k_jd|                    (natural-log units)
    so P_ij moves by a factor within exp(+-d_ij);
  * delta_i = sum_d dO_id O_id is formed from the O the caller passes, which is the exact O rounded to the 16-bit type, and the
    chain dP'_ij = dO_i.v_j - delta_i is accumulated in fp32 over D terms:
        e_ij = u * sum_d |dO_id||O_id| + 2^-24 * D * (sum_d |dO_id||v_jd| + sum_d |dO_id||O_id|);
  * dS_ij = P_ij * dP'_ij is rounded to the 16-bit type before the second products, and so is P_ij for dV:
        E_ij = |dS_ij| * (u + expm1(d_ij)) + P_ij * exp(d_ij) * e_ij + t        (visible pairs; 0 on masked ones)
    t = 2^-25 for f16 (values below 2^-14 are subnormal in f16: their rounding error is absolute, half of 2^-24), 0 for bf16
    (its exponent range is fp32's);
  * the second products accumulate in fp32 over the N (Nk) rows of the reduction:
        bound(dQ_id) = scale * (sum_j E_ij |k_jd| + 2^-24 * Nk * sum_j |dS_ij| |k_jd|)
        bound(dK_jd) = scale * (sum_i E_ij |q_id| + 2^-24 * N  * sum_i |dS_ij| |q_id|)
        bound(dV_jd) = sum_i (P_ij (u + expm1(d_ij)) + t) |dO_id| + 2^-24 * N * sum_i P_ij |dO_id|
    and the bounds of a key head's query heads add up (grouped heads: one workgroup sums them in registers).
P, dS and O above are the exact (fp64) ones. e4m3 inputs are widened exactly to bf16 and run the bf16 kernels: u = 2^-8.

The backward on an O and an LSE that are NOT the oracle's (a forward kernel's: tests/chain_bound.py, tests/test_gpu_chain.py):
  * the given-input reference: head_exact(..., o_in=, lse_in=) evaluates the formula the kernels document on the six tensors they
    were handed, in fp64: P^_ij = exp(scale*s_ij - lse_in_i) on visible pairs (its rows need not add up to 1), delta^_i = sum_d dO_id
    o_in_id, dS^ = P^ (dP - delta^), dQ^ = scale dS^ K, dK^ = scale dS^T Q, dV^ = P^T dO. Its bound is the one above with P^ and dS^ for
    P and dS and WITHOUT u * sum_d |dO||O| -- o_in is a value of the type already --, the fp32 terms stay: head_bounds(R^, o_err = 0).
  * the true gradient: head_bounds(..., lse_err=, o_err=) with lse_err [Nq] >= |lse_in - exact| and o_err [Nq, D] >= |o_in - exact O|.
    P^ = P exp(-eps_i), delta^ - delta = sum_d dO_id w_id, hence
        |dS^_ij - dS_ij| <= |dS_ij| expm1(|eps_i|) + P_ij exp(|eps_i|) sum_d |dO_id| |w_id|:
    d_ij becomes d_ij + lse_err_i and u * sum_d |dO_id||O_id| becomes sum_d |dO_id| o_err_id. lse_err = 0 and o_err = u |O| is the
    bound above (the defaults, which evaluate the very expressions above: bit for bit the former numbers).
"""
import numpy as np

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp8": 2.0 ** -8}
TINY = {"f16": 2.0 ** -25, "bf16": 0.0, "fp8": 0.0}
U32 = 2.0 ** -24
LOG2E32 = np.float32(1.4426950408889634)


def rnd(x, dtype):
    """fp32 -> 16-bit type -> fp32, round to nearest even (numpy only; "fp8" inputs compute in bf16)."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    w = x.view(np.uint32).astype(np.uint64)
    w = ((w + 0x7FFF + ((w >> 16) & 1)) >> 16) << 16
    return w.astype(np.uint32).view(np.float32).reshape(x.shape)


def head_exact(q, k, v, do, causal, scale, o_in=None, lse_in=None):
    """fp64 forward and backward of ONE head: q, do [Nq, D], k, v [Nk, D]; bottom-right aligned causal mask. With o_in [Nq, D] and
    lse_in [Nq] (both or neither): the given-input reference of the module docstring -- p, ds, delta, o, lse, dq, dk, dv are then P^,
    dS^, delta^, o_in, lse_in and the gradients the documented formula gives on them."""
    assert (o_in is None) == (lse_in is None)
    q, k, v, do = (np.asarray(x, np.float64) for x in (q, k, v, do))
    Nq, Nk = q.shape[0], k.shape[0]
    s = (q @ k.T) * scale
    mask = None
    if causal:
        mask = np.arange(Nk)[None, :] <= np.arange(Nq)[:, None] + (Nk - Nq)
        s = np.where(mask, s, -np.inf)
    if o_in is not None:
        o, lse = np.asarray(o_in, np.float64), np.asarray(lse_in, np.float64)
        p = np.exp(s - lse[:, None])  # (masked pairs: exp(-inf) = 0)
        dp = do @ v.T
        delta = (do * o).sum(-1, keepdims=True)
        ds = p * (dp - delta)
        return dict(p=p, ds=ds, dp=dp, delta=delta, o=o, lse=lse, mask=mask, dq=scale * (ds @ k), dk=scale * (ds.T @ q), dv=p.T @ do)
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    p /= l
    o = p @ v
    dp = do @ v.T
    delta = (do * o).sum(-1, keepdims=True)
    ds = p * (dp - delta)
    return dict(p=p, ds=ds, dp=dp, delta=delta, o=o, lse=(m + np.log(l))[:, 0], mask=mask,
                dq=scale * (ds @ k), dk=scale * (ds.T @ q), dv=p.T @ do)


def head_bounds(q, k, v, do, scale, dtype, R, lse_err=None, o_err=None):
    """The bound of the module docstring for one head, from the inputs and the exact intermediates R = head_exact(...). lse_err [Nq]
    and o_err [Nq, D]: how far the LSE and the O handed to the kernels may lie from the exact ones (defaults: 0 and u |O|)."""
    u, t = U[dtype], TINY[dtype]
    aq, ak, av, ado = (np.abs(np.asarray(x, np.float64)) for x in (q, k, v, do))
    Nq, Nk, D = q.shape[0], k.shape[0], q.shape[1]
    p, ads, ao = R["p"], np.abs(R["ds"]), np.abs(R["o"])
    vis = np.ones_like(p) if R["mask"] is None else R["mask"].astype(np.float64)
    d = u * scale * (aq @ ak.T)
    if lse_err is not None:
        d = d + np.asarray(lse_err, np.float64)[:, None]
    doo = (ado * ao).sum(-1, keepdims=True)
    doe = u * doo if o_err is None else (ado * np.asarray(o_err, np.float64)).sum(-1, keepdims=True)
    e = doe + U32 * D * (ado @ av.T + doo)
    E = (ads * (u + np.expm1(d)) + p * np.exp(d) * e + t) * vis
    bq = scale * (E @ ak + U32 * Nk * (ads @ ak))
    bk = scale * (E.T @ aq + U32 * Nq * (ads.T @ aq))
    bv = ((p * (u + np.expm1(d)) + t) * vis).T @ ado + U32 * Nq * (p.T @ ado)
    return bq, bk, bv


def head_model(q, k, v, do, causal, scale, dtype, R, o_in=None, lse_in=None):
    """A numpy model of both kernels' roundings for one head (everything else exact): O rounded to the type, LSE to fp32 and taken
    times log2(e) in fp32, Q~ / K~ = round(fp32(scale*log2e) * operand), P and dS rounded to the type before the second products.
    o_in (values of the type) and lse_in: the O and LSE the kernels are handed, where they are not the exact ones of R."""
    q, k, v, do = (np.asarray(x, np.float32) for x in (q, k, v, do))
    c2 = np.float32(np.float32(scale) * LOG2E32)
    o = rnd(R["o"], dtype).astype(np.float64) if o_in is None else np.asarray(o_in, np.float64)
    lse2 = (np.asarray(R["lse"] if lse_in is None else lse_in).astype(np.float32) * LOG2E32).astype(np.float64)
    q64, k64, v64, do64 = (x.astype(np.float64) for x in (q, k, v, do))
    dpp = do64 @ v64.T - (do64 * o).sum(-1, keepdims=True)

    def prob(s2):
        s2 = s2 - lse2[:, None]
        if causal:
            s2 = np.where(R["mask"], s2, -np.inf)
        return np.exp2(s2)

    p1 = prob(rnd(q * c2, dtype).astype(np.float64) @ k64.T)  # the dQ kernel
    dq = scale * (rnd(p1 * dpp, dtype).astype(np.float64) @ k64)
    p2 = prob(q64 @ rnd(k * c2, dtype).astype(np.float64).T)  # the dK/dV kernel
    dk = scale * (rnd(p2 * dpp, dtype).astype(np.float64).T @ q64)
    dv = rnd(p2, dtype).astype(np.float64).T @ do64
    return dq, dk, dv


def _per_head(q, k, v, do, causal, scale, fn):
    """Apply fn(b, h, hk, q_h, k_h, v_h, do_h) -> (gq, gk, gv) to every query head of [B,Hq,Nq,D] / [B,Hkv,Nk,D] inputs; the key-side
    results of a group are added."""
    B, Hq, Nq, D = q.shape
    Hkv, Nk = k.shape[1], k.shape[2]
    G = Hq // Hkv
    assert Hq == G * Hkv and v.shape == k.shape and do.shape == q.shape
    gq = np.zeros((B, Hq, Nq, D))
    gk, gv = np.zeros((B, Hkv, Nk, D)), np.zeros((B, Hkv, Nk, D))
    for b in range(B):
        for h in range(Hq):
            a, c, e = fn(b, h, h // G, q[b, h], k[b, h // G], v[b, h // G], do[b, h])
            gq[b, h] = a
            gk[b, h // G] += c
            gv[b, h // G] += e
    return gq, gk, gv


def default_scale(D):
    return float(np.float32(1.0) / np.float32(np.sqrt(D)))


class Bounds:
    """Everything the tests need for one problem, all fp64: ref = (dQ, dK, dV), bound = (bQ, bK, bV), o [B,Hq,Nq,D], lse [B,Hq,Nq];
    with model=True also model = the rounding model's (dQ, dK, dV).
    lse_err [B,Hq,Nq] / o_err [B,Hq,Nq,D] go to head_bounds per head (the true-gradient bound on an inexact LSE / O). With o_in
    [B,Hq,Nq,D] and lse_in [B,Hq,Nq] -- the O and LSE the kernels were handed -- also given_ref / given_bound, the given-input
    reference and its bound, and the model runs on them."""

    def __init__(self, q, k, v, do, causal, scale, dtype, model=False, lse_err=None, o_err=None, o_in=None, lse_in=None):
        scale = default_scale(q.shape[-1]) if scale is None else float(scale)
        self.o = np.zeros(q.shape)
        self.lse = np.zeros(q.shape[:3])
        bound = [None] * 3
        mod = [None] * 3
        given = o_in is not None
        assert given == (lse_in is not None)
        gref = [np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape)]
        gbound = [np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape)]

        def ref_fn(b, h, hk, qh, kh, vh, doh):
            R = head_exact(qh, kh, vh, doh, causal, scale)
            self.o[b, h], self.lse[b, h] = R["o"], R["lse"]
            bb = head_bounds(qh, kh, vh, doh, scale, dtype, R, None if lse_err is None else lse_err[b, h], None if o_err is None else o_err[b, h])
            oi, li = (o_in[b, h], lse_in[b, h]) if given else (None, None)
            mm = head_model(qh, kh, vh, doh, causal, scale, dtype, R, oi, li) if model else (0.0, 0.0, 0.0)
            if given:
                G = head_exact(qh, kh, vh, doh, causal, scale, oi, li)
                gb = head_bounds(qh, kh, vh, doh, scale, dtype, G, None, np.zeros(qh.shape))
                for t, (x, y) in enumerate(zip((G["dq"], G["dk"], G["dv"]), gb)):
                    if t == 0:
                        gref[t][b, h], gbound[t][b, h] = x, y
                    else:
                        gref[t][b, hk] += x
                        gbound[t][b, hk] += y
            if bound[0] is None:
                bound[0] = np.zeros(q.shape)
                bound[1], bound[2] = np.zeros(k.shape), np.zeros(k.shape)
                mod[0] = np.zeros(q.shape)
                mod[1], mod[2] = np.zeros(k.shape), np.zeros(k.shape)
            bound[0][b, h] = bb[0]
            bound[1][b, hk] += bb[1]
            bound[2][b, hk] += bb[2]
            mod[0][b, h] = mm[0]
            mod[1][b, hk] += mm[1]
            mod[2][b, hk] += mm[2]
            return R["dq"], R["dk"], R["dv"]

        self.ref = _per_head(q, k, v, do, causal, scale, ref_fn)
        self.bound = tuple(bound)
        self.model = tuple(mod) if model else None
        self.given_ref, self.given_bound = (tuple(gref), tuple(gbound)) if given else (None, None)


def ratios(grads, refs, bounds):
    """Worst |g - ref| / bound per tensor. Where the bound is exactly 0 (no visible pair contributes: a masked key, an all-zero
    operand) the gradient has to be exactly the reference: any difference there counts as infinite."""
    out = []
    for g, r, b in zip(grads, refs, bounds):
        err = np.abs(np.asarray(g, np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
        out.append(float(x.max()) if x.size else 0.0)
    return out
