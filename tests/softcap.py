"""Logit soft-capping (include/fa_mi355.h, "Logit soft-capping"), test side only, pure numpy: the fp64 references of the *_softcap entry
points, the bars, an fp32 model of the kernels' arithmetic with one planted mistake at a time, and the per-sequence backward bound under a
cap. Shared by tests/test_softcap_cases.py (CPU) and tests/test_gpu_softcap*.py (GPU).

With x_ij = scale s_ij / softcap and t_ij = tanh(x_ij) the capped score softcap t_ij takes the place of scale s_ij everywhere; the mask
(window.visible) is applied AFTER the cap. Backward, with the forward's LSE: P = exp(softcap t - lse), g = P (dP - delta) is the gradient
with respect to the capped score and dS = g (1 - t^2) the one with respect to scale s; dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO.

The bars (derived, never fitted).
  * |d(softcap tanh(x)) / d(scale s)| = 1 - t^2 <= 1: the one rounding of the pre-scaled operand moves a capped score by no more than it
    moved the raw one, so util.lse_tol / util.o_tol and the chain and backward bounds stay valid upper bounds, pre-scale terms unchanged.
  * new: the evaluation of tanh. The kernels form t = 1 - 2 / (1 + 2^y), y = 2 x log2(e) straight from the matrix core, in four fp32
    steps: e = 2^y (1 + d1), a = (1 + e)(1 + d2), r = (1 / a)(1 + d3), t = (1 - 2 r)(1 + d4), with |d2|, |d4| <= u = 2^-24 (one rounding
    each) and |d1| <= eps_exp, |d3| <= eps_rcp. To first order r is off by the relative amount d1 E / (1 + E) + d2 + d3 (E = 2^y exact), so
    2 r = 2 / (1 + E) is off by at most eps_exp 2 E / (1 + E)^2 + (u + eps_rcp) 2 / (1 + E) <= eps_exp / 2 + 2 (u + eps_rcp), and the last
    rounding adds |t| u <= u:
        tanh_err = eps_exp / 2 + 2 eps_rcp + 3 u.
    Correctly rounded steps (eps = u): 5.5 u = 3.3e-7 (a numpy model measures 1.9e-7 over |x| <= 12). v_exp_f32 and v_rcp_f32 carry one
    ulp (2 u) more each, eps = 3 u: tanh_err = 10.5 u = 6.3e-7. Both ends are exact: 2^y = inf gives r = 0, t = 1; 2^y = 0 (or flushed
    to 0 below 2^-126: a difference under 2^-125) gives t = -1; y = 0 gives e = 1, a = 2, r = 1/2 and t = 0 exactly.
        LSE: lse_tol + softcap tanh_err            O: o_tol + |O| softcap tanh_err
  * backward: backward_bound's per-element E_ij, formed on g, is scaled by (1 - t_ij^2), and gains |g_ij| (2 |t_ij| tanh_err + 2^-23) for
    the factor itself (t off by tanh_err moves 1 - t^2 by 2 |t| tanh_err; the fma that forms it and the multiply round once each):
        E'_ij = E_ij(g) (1 - t_ij^2) + |g_ij| (2 |t_ij| tanh_err + 2^-23)
    and the fp32 accumulation terms of dQ / dK run over |dS| = |g| (1 - t^2). dV's bound is backward_bound's, unchanged. The forward's
    softcap tanh_err enters through lse_err / o_err as every other forward error does."""
import numpy as np

import backward_bound as bb
import window as wn
import window_backward as wb

U32 = 2.0 ** -24
EPS_EXP = EPS_RCP = 3 * U32              # half an ulp of the rounding plus the one ulp the hardware instruction may be off by
TANH_ERR = EPS_EXP / 2 + 2 * EPS_RCP + 3 * U32
TANH_ERR_ROUNDED = 5.5 * U32             # the same formula with correctly rounded steps: what tanh32() below is held to
LOG2E32, LN2_32 = np.float32(1.4426950408889634), np.float32(0.6931471805599453)
WINDOWS = ((-1, 0), (-1, -1), (63, 0), (127, 5), (200, 0))
BWD_WINDOWS = ((-1, 0), (63, 0), (127, 5))
# (name, softcap, scale of a head dim; None = the default 1 / sqrt(D)): on U(-1, 1) data both put at least a tenth of the visible pairs
# in the saturating range |x| > 1.5 and a tenth in the linear one |x| < 0.25 (teeth() below, asserted by tests/test_softcap_cases.py)
REGIMES = (("cap_quarter", 0.25, None), ("cap_50_scale_150", 50.0, 150.0))
BUGS_FWD = ("mask_before_cap", "scale_after_tanh", "no_multiply_back", "cap_not_log2", "recompute_uncapped")
BUGS_BWD = ("bwd_no_factor", "bwd_factor_of_capped", "bwd_scale_over_cap")


def scale_of(regime_scale, D):
    return bb.default_scale(D) if regime_scale is None else float(np.float32(regime_scale / np.sqrt(D)))


def capped(s, scale, softcap):
    """fp64 capped scores from raw products s."""
    return softcap * np.tanh(np.asarray(s, np.float64) * (scale / softcap))


def reference(q, k, v, wl, wr, softcap, scale=None):
    """fp64 O [Hq, Lq, D] and LSE [Hq, Lq] of one sequence: window.reference over capped scores, the mask after the cap."""
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    sc = D ** -0.5 if scale is None else scale
    o, lse = np.zeros((Hq, Lq, D)), np.full((Hq, Lq), -np.inf)
    if Lq == 0 or Lk == 0:
        return o, lse
    vis = wn.visible(Lq, Lk, wl, wr)
    live = vis.any(1)
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    s = np.where(vis[None], capped(q.astype(np.float64) @ ke.swapaxes(-1, -2), sc, softcap), -np.inf)
    m = np.where(live, s.max(-1), 0.0)
    p = np.exp(s - m[..., None])
    l = p.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(live[None, :, None], (p @ ve) / l[..., None], 0.0)
        lse = np.where(live[None], m + np.log(l), -np.inf)
    return o, lse


def bars(lse_tol, o_tol, o64, softcap):
    """(o_bar [like o64], lse_bar scalar) from the un-capped route's scalar tolerances."""
    return o_tol + np.abs(o64) * softcap * TANH_ERR, lse_tol + softcap * TANH_ERR


def teeth(q, k, wl, wr, softcap, scale):
    """(fraction of visible pairs with |x| > 1.5, fraction with |x| < 0.25) of one sequence."""
    Hq, Lq, _ = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    vis = wn.visible(Lq, Lk, wl, wr) if Lk else np.zeros((Lq, 0), bool)
    if not vis.any():
        return None
    ke = np.repeat(k.astype(np.float64), Hq // Hkv, axis=0)
    x = np.abs(q.astype(np.float64) @ ke.swapaxes(-1, -2)) * (scale / softcap)
    x = x[:, vis]
    return float((x > 1.5).mean()), float((x < 0.25).mean())


# ---- fp32 model of the kernels' arithmetic ------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float32)


def exp2_32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(np.asarray(x, np.float64)).astype(np.float32)


def tanh32(y):
    """tanh_from_exp2_arg of csrc/fa_common.h with correctly rounded steps: 1 - 2 / (1 + 2^y) in fp32."""
    with np.errstate(over="ignore", divide="ignore"):
        e = exp2_32(y)
        a = (np.float32(1.0) + e).astype(np.float32)
        r = (np.float32(1.0) / a).astype(np.float32)
        return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)  # one fma: a single rounding


def operand_factor(scale, softcap):
    """The fp32 factor of the pre-scaled operand, in the kernels' order: 2 (scale log2e) / softcap."""
    return np.float32(np.float32(2.0) * np.float32(np.float32(scale) * LOG2E32) / np.float32(softcap))


def first_tile_keys(Lq, Lk, wl, wr):
    """bool [Lq, Lk]: the keys of each row's wave's first active tile (csrc/fa_mfma_kernel.hip: tfw), where the exact path always runs."""
    wl_ = Lk if (wl < 0 or wl > Lk) else wl
    cl = Lk - Lq - wl_
    rows = np.arange(Lq)
    t0 = np.maximum(0, (rows // wn.WAVE) * wn.WAVE + cl) // wn.TILE
    j = np.arange(Lk)[None, :]
    return (j // wn.TILE) == t0[:, None]


def forward_model(q, k, v, wl, wr, softcap, scale, dtype, bug=None):
    """fp32 (O [Hq, Lq, D], LSE [Hq, Lq]) of one sequence as the softcap kernels form them (one pass over a row's keys; dot products
    exact): Q~ = round(factor q), y = Q~ . k, t = tanh32(y), the mask, C = fp32(softcap log2e), m = max t C, P = exp2(fma(t, C, -m)),
    l = sum P, O = sum round(P) v / l rounded to the type, LSE = m ln2 + ln(l). bug: one of BUGS_FWD."""
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    o, lse = np.zeros((Hq, Lq, D), np.float32), np.full((Hq, Lq), -np.inf, np.float32)
    if Lq == 0 or Lk == 0:
        return o, lse
    vis = wn.visible(Lq, Lk, wl, wr)
    live = vis.any(1)
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    fac = operand_factor(1.0 if bug == "scale_after_tanh" else scale, softcap)
    qt = bb.rnd((f32(q) * fac).astype(np.float32), dtype).astype(np.float64)
    y = (qt @ ke.swapaxes(-1, -2)).astype(np.float32)
    if bug == "mask_before_cap":
        y = np.where(vis[None], y, -np.inf).astype(np.float32)
    t = tanh32(y)
    if bug == "recompute_uncapped":
        t = np.where(first_tile_keys(Lq, Lk, wl, wr)[None], y, t).astype(np.float32)
    C = np.float32(np.float32(softcap) * LOG2E32)
    if bug == "cap_not_log2":
        C = np.float32(softcap)
    if bug == "no_multiply_back":
        C = LOG2E32
    if bug == "scale_after_tanh":
        C = np.float32(C * np.float32(scale))
    if bug != "mask_before_cap":
        t = np.where(vis[None], t, -np.inf).astype(np.float32)
    with np.errstate(invalid="ignore"):
        m = np.where(live[None], (t.max(-1) * C).astype(np.float32), np.float32(0))
        s2 = (t.astype(np.float64) * np.float64(C) - m[..., None].astype(np.float64)).astype(np.float32)  # one fma
    p = exp2_32(s2)
    l = p.astype(np.float64).sum(-1).astype(np.float32)
    acc = (bb.rnd(p, dtype).astype(np.float64) @ ve).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        on = bb.rnd((acc * (np.float32(1.0) / l)[..., None]).astype(np.float32), dtype)
        ln = (m * LN2_32 + np.log(l.astype(np.float64)).astype(np.float32)).astype(np.float32)
    o[:, live], lse[:, live] = on[:, live], ln[:, live]
    return o, lse


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def head_exact(q, k, v, do, mask, scale, softcap):
    """fp64 forward and backward of ONE head under a cap and an arbitrary mask [Nq, Nk] in which every row sees a key. p, o, lse: of the
    capped scores; g = p (dp - delta); t = tanh(x); ds = g (1 - t^2)."""
    q, k, v, do = (np.asarray(x, np.float64) for x in (q, k, v, do))
    t = np.tanh((q @ k.T) * (scale / softcap))
    s = np.where(mask, softcap * t, -np.inf)
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    p /= l
    o = p @ v
    dp = do @ v.T
    delta = (do * o).sum(-1, keepdims=True)
    g = p * (dp - delta)
    ds = g * (1.0 - t * t)
    return dict(p=p, g=g, t=t, ds=ds, dp=dp, delta=delta, o=o, lse=(m + np.log(l))[:, 0], mask=mask, dq=scale * (ds @ k), dk=scale * (ds.T @ q),
                dv=p.T @ do)


def head_bounds(q, k, v, do, scale, dtype, R, lse_err, o_err):
    """backward_bound.head_bounds with the two changes of the module docstring. lse_err [Nq] / o_err [Nq, D]: how far the LSE and the O
    handed to the kernels may lie from the exact ones."""
    u, tiny = bb.U[dtype], bb.TINY[dtype]
    aq, ak, av, ado = (np.abs(np.asarray(x, np.float64)) for x in (q, k, v, do))
    Nq, Nk, D = q.shape[0], k.shape[0], q.shape[1]
    p, ag, at, ao = R["p"], np.abs(R["g"]), np.abs(R["t"]), np.abs(R["o"])
    f = 1.0 - at * at
    vis = R["mask"].astype(np.float64)
    d = u * scale * (aq @ ak.T) + np.asarray(lse_err, np.float64)[:, None]
    doo = (ado * ao).sum(-1, keepdims=True)
    doe = (ado * np.asarray(o_err, np.float64)).sum(-1, keepdims=True)
    e = doe + bb.U32 * D * (ado @ av.T + doo)
    E = ((ag * (u + np.expm1(d)) + p * np.exp(d) * e + tiny) * f + ag * (2.0 * at * TANH_ERR + 2.0 ** -23)) * vis
    ads = ag * f * vis
    bq = scale * (E @ ak + bb.U32 * Nk * (ads @ ak))
    bk = scale * (E.T @ aq + bb.U32 * Nq * (ads.T @ aq))
    bv = ((p * (u + np.expm1(d)) + tiny) * vis).T @ ado + bb.U32 * Nq * (p.T @ ado)
    return bq, bk, bv


def head_model(q, k, v, do, scale, softcap, dtype, R, o_in=None, lse_in=None, bug=None):
    """A numpy model of both softcap backward kernels' roundings for one head: O rounded to the type, LSE to fp32 times log2(e), Q~ / K~ =
    round(factor operand), t = tanh32(y), the exponent fma(t, C, -lse2), 1 - t^2 by one fma, dS = round(P ((dP - delta) (1 - t^2))), P
    rounded for dV. bug: one of BUGS_BWD."""
    q, k, v, do = (np.asarray(x, np.float32) for x in (q, k, v, do))
    fac = operand_factor(scale, softcap)
    C = np.float64(np.float32(np.float32(softcap) * LOG2E32))
    o = bb.rnd(R["o"], dtype).astype(np.float64) if o_in is None else np.asarray(o_in, np.float64)
    lse2 = (np.asarray(R["lse"] if lse_in is None else lse_in).astype(np.float32) * LOG2E32).astype(np.float64)
    q64, k64, v64, do64 = (x.astype(np.float64) for x in (q, k, v, do))
    dpp = (do64 @ v64.T - (do64 * o).sum(-1, keepdims=True)).astype(np.float32)
    last = scale / softcap if bug == "bwd_scale_over_cap" else scale

    def p_and_ds(y):
        t = tanh32(y.astype(np.float32))
        a = (t.astype(np.float64) * C - lse2[:, None]).astype(np.float32)
        p = exp2_32(np.where(R["mask"], a, -np.inf))
        t64 = t.astype(np.float64)
        if bug == "bwd_no_factor":
            f = np.ones_like(t)
        elif bug == "bwd_factor_of_capped":
            f = (1.0 - np.tanh(softcap * t64) ** 2).astype(np.float32)
        else:
            f = (1.0 - t64 * t64).astype(np.float32)
        return p, (p * (dpp * f).astype(np.float32)).astype(np.float32)

    p1, ds1 = p_and_ds(bb.rnd(q * fac, dtype).astype(np.float64) @ k64.T)  # the dQ kernel
    dq = last * (bb.rnd(ds1, dtype).astype(np.float64) @ k64)
    p2, ds2 = p_and_ds(q64 @ bb.rnd(k * fac, dtype).astype(np.float64).T)  # the dK/dV kernel
    dk = last * (bb.rnd(ds2, dtype).astype(np.float64).T @ q64)
    dv = bb.rnd(p2, dtype).astype(np.float64).T @ do64
    return dq, dk, dv


class SeqBounds:
    """window_backward.SeqBounds(chain=True) for one sequence under (wl, wr) and a cap: ref / bound of (dQ, dK, dV), with
    window_backward.forward_errors plus softcap tanh_err as the forward's lse_err / o_err; o, lse = the exact forward (dead rows: 0 and
    -inf). model(bug) assembles head_model like the reference."""

    def __init__(self, q, k, v, do, wl, wr, softcap, scale, dtype):
        self.q, self.k, self.v, self.do = q, k, v, do
        self.scale = bb.default_scale(q.shape[-1]) if scale is None else float(scale)
        self.softcap, self.dtype = float(softcap), dtype
        Hq, Lq, D = q.shape
        Hkv, Lk = k.shape[0], k.shape[1]
        self.G, self.n0 = Hq // Hkv, wb.first_live_row(Lq, Lk, wl, wr)
        self.vis = wn.visible(Lq, Lk, wl, wr)
        self.unseen = ~self.vis.any(0) if Lq else np.ones(Lk, bool)
        self.o, self.lse = np.zeros(q.shape), np.full((Hq, Lq), -np.inf)
        self.ref = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.bound = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.R = {}
        n0 = self.n0
        if n0 >= Lq:
            return
        mask = self.vis[n0:]
        assert mask.any(1).all() and not self.vis[:n0].any()  # the dead rows are exactly the prefix
        for h in range(Hq):
            hk = h // self.G
            R = head_exact(q[h, n0:], k[hk], v[hk], do[h, n0:], mask, self.scale, self.softcap)
            le, oe = wb.forward_errors(q[h, n0:], k[hk], v[hk], mask, self.scale, dtype, R)
            le = le + self.softcap * TANH_ERR
            oe = oe + np.abs(R["o"]) * self.softcap * TANH_ERR
            B = head_bounds(q[h, n0:], k[hk], v[hk], do[h, n0:], self.scale, dtype, R, le, oe)
            self.R[h] = R
            self.o[h, n0:], self.lse[h, n0:] = R["o"], R["lse"]
            self.ref[0][h, n0:] = R["dq"]
            self.ref[1][hk] += R["dk"]
            self.ref[2][hk] += R["dv"]
            self.bound[0][h, n0:] = B[0]
            self.bound[1][hk] += B[1]
            self.bound[2][hk] += B[2]

    def model(self, bug=None):
        q, k, v, do, n0 = self.q, self.k, self.v, self.do, self.n0
        out = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        for h, R in self.R.items():
            hk = h // self.G
            g = head_model(q[h, n0:], k[hk], v[hk], do[h, n0:], self.scale, self.softcap, self.dtype, R, bug=bug)
            out[0][h, n0:] = g[0]
            out[1][hk] += g[1]
            out[2][hk] += g[2]
        return out
