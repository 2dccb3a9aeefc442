"""The MLA prefill cases (pure numpy; shared by tests/test_mla_prefill_cases.py on the CPU and tests/test_gpu_mla_prefill.py on the GPU):
fa_fwd_varlen_mla (include/fa_mi355.h, "Multi-head latent attention (prefill)") is fa_fwd_varlen with two head dims, q / k rows of 192
(128 "nope" + 64 rotary) and v / o rows of 128. Here: the fp64 reference of tests/window.py generalised to two head dims, the bars of
tests/util.py with the scale passed explicitly (nothing fitted), an fp32 model of the kernel's arithmetic with six plantable mistakes, the
catalogue of packed calls, and the bar of the chunked-context merge.

Bars (tests/util.py): strict -- against the exact operator on the operand the kernel really multiplies, effective_q(q) under scale ln 2,
at TOL_O / TOL_LSE; and against the true Q at o_tol / lse_tol, the documented operand-rounding bound formed on the 192-wide rows."""
import numpy as np

import window
from exact_forward import round_to
from util import LN2, TOL_LSE, TOL_O, effective_q, lse_tol, o_tol

DQK, DV, DNOPE = 192, 128, 128
SCALE = DQK ** -0.5          # the caller's; every call of the tests passes it explicitly
SEQS = window.SEQS           # dead rows (200, 130), Lk = 0, Lq > Lk, 1000 keys
EDGES = ((63, 63), (64, 64), (65, 65), (128, 128), (5, 63), (5, 64), (5, 65), (5, 128))  # Lk in {63, 64, 65, 128}: the tile edges
HEADS = window.HEADS         # (4, 4) and (8, 2)
DTYPES = ("bf16", "f16")
BUGS = ("scale_dv", "no_rope", "v_pitch_k", "v_from_k", "top_left", "head_mod")
# the case each planted mistake is caught on: (catalogue, heads, causal)
BUG_CASE = {"scale_dv": ("seqs", (4, 4), False), "no_rope": ("seqs", (4, 4), False), "v_pitch_k": ("seqs", (4, 4), False),
            "v_from_k": ("seqs", (4, 4), True), "top_left": ("seqs", (4, 4), True), "head_mod": ("seqs", (8, 2), False)}


class _Rounder:  # util.effective_q asks its first argument for round_to only
    round_to = staticmethod(round_to)


def visible(Lq, Lk, causal):
    return window.visible(Lq, Lk, -1, 0 if causal else -1)


def reference(q, k, v, causal, scale):
    """fp64 O [Hq, Lq, Dv] and LSE [Hq, Lq] of one sequence: q [Hq, Lq, Dqk], k [Hkv, Lk, Dqk], v [Hkv, Lk, Dv] (window.reference with
    two head dims). Dead rows: O = 0, LSE = -inf."""
    Hq, Lq, _ = q.shape
    Hkv, Lk, Dv = v.shape
    o, lse = np.zeros((Hq, Lq, Dv)), np.full((Hq, Lq), -np.inf)
    if Lq == 0 or Lk == 0:
        return o, lse
    vis = visible(Lq, Lk, causal)
    live = vis.any(1)
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    s = np.where(vis[None], (q.astype(np.float64) @ ke.swapaxes(-1, -2)) * scale, -np.inf)
    m = np.where(live, s.max(-1), 0.0)
    p = np.exp(s - m[..., None])
    l = p.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(live[None, :, None], (p @ ve) / l[..., None], 0.0)
        lse = np.where(live[None], m + np.log(l), -np.inf)
    return o, lse


def model(q, k, v, causal, scale, dtype, bug=None):
    """fp32 model of the kernel's arithmetic on one sequence: Q~ = round(q * scale * log2 e) to the type, scores and the row maximum in
    fp32 (log2 units), P = exp2(s - m) with fp32 row sums over the UNROUNDED P, P rounded to the type into the PV product, fp32 sums,
    O = acc / l rounded to the type. `bug` plants one of BUGS."""
    Hq, Lq, _ = q.shape
    Hkv, Lk, Dv = v.shape
    o, lse = np.zeros((Hq, Lq, Dv), np.float32), np.full((Hq, Lq), -np.inf, np.float32)
    if Lq == 0 or Lk == 0:
        return o.astype(np.float64), lse.astype(np.float64)
    if bug == "scale_dv":
        scale = Dv ** -0.5
    if bug == "v_from_k":
        v = k[:, :, :Dv]
    if bug == "v_pitch_k":  # the value tensor [Lk, Hkv, Dv] walked with the key's row pitch Hkv * Dqk (wrapped into the buffer)
        flat = np.ascontiguousarray(v.transpose(1, 0, 2)).reshape(-1)
        j, h, d = np.meshgrid(np.arange(Lk), np.arange(Hkv), np.arange(Dv), indexing="ij")
        v = flat[(j * Hkv * k.shape[2] + h * Dv + d) % flat.size].transpose(1, 0, 2)
    G = Hq // Hkv
    kvh = np.arange(Hq) % Hkv if bug == "head_mod" else np.arange(Hq) // G
    qt = effective_q(_Rounder, q, dtype, scale)
    ke, ve = k[kvh].astype(np.float32), v[kvh].astype(np.float32)
    if bug == "no_rope":
        qt, ke = qt[..., :DNOPE], ke[..., :DNOPE]
    i, j = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    vis = (j <= i) if (bug == "top_left" and causal) else visible(Lq, Lk, causal)
    live = vis.any(1)
    s = np.where(vis[None], np.matmul(qt, ke.swapaxes(-1, -2), dtype=np.float32), -np.inf).astype(np.float32)
    m = np.where(live[None], s.max(-1), np.float32(0.0)).astype(np.float32)
    p = np.exp2(s - m[..., None]).astype(np.float32)
    l = p.sum(-1, dtype=np.float32)
    acc = np.matmul(round_to(p, dtype), ve, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(live[None, :, None], round_to(acc * (np.float32(1.0) / l)[..., None], dtype), np.float32(0.0))
        lse = np.where(live[None], m * np.float32(LN2) + np.log(l), -np.inf)
    return o.astype(np.float64), lse.astype(np.float64)


# ---- the catalogue: one packed call per (catalogue, heads, dtype); values U(-1, 1) rounded to the type, built once and read-only
_CASES, _REFS = {}, {}


def _ro(x):
    x.setflags(write=False)
    return x


def case(name, heads, dtype):
    """dict: lens, cu_q / cu_k (int32 [B + 1]), q [total_q, Hq, 192], k [total_k, Hkv, 192], v [total_k, Hkv, 128] (fp32 arrays holding
    values of `dtype`), max_q, max_k."""
    key = (name, tuple(heads), dtype)
    if key not in _CASES:
        lens = {"seqs": SEQS, "edges": EDGES}[name]
        Hq, Hkv = heads
        rng = np.random.default_rng(2500 + 10 * Hq + Hkv + (0 if name == "seqs" else 1000))
        tq, tk = sum(a for a, _ in lens), sum(b for _, b in lens)
        q, k, v = (_ro(round_to(rng.uniform(-1.0, 1.0, shape).astype(np.float32), dtype))
                   for shape in ((tq, Hq, DQK), (tk, Hkv, DQK), (tk, Hkv, DV)))
        cu_q = np.concatenate([[0], np.cumsum([a for a, _ in lens])]).astype(np.int32)
        cu_k = np.concatenate([[0], np.cumsum([b for _, b in lens])]).astype(np.int32)
        _CASES[key] = dict(name=name, heads=(Hq, Hkv), dtype=dtype, lens=lens, cu_q=_ro(cu_q), cu_k=_ro(cu_k), q=q, k=k, v=v,
                           max_q=max(a for a, _ in lens), max_k=max(max(b for _, b in lens), 1))
    return _CASES[key]


def per_sequence(c, fn):
    """fn(q [Hq, Lq, 192], k [Hkv, Lk, 192], v [Hkv, Lk, 128]) -> (o [Hq, Lq, 128], lse [Hq, Lq]) per sequence, packed as the call
    returns them: o [total_q, Hq, 128], lse [Hq, total_q]."""
    Hq = c["heads"][0]
    o, lse = np.zeros((len(c["q"]), Hq, DV)), np.full((Hq, len(c["q"])), -np.inf)
    for b in range(len(c["lens"])):
        q0, q1, k0, k1 = c["cu_q"][b], c["cu_q"][b + 1], c["cu_k"][b], c["cu_k"][b + 1]
        ob, lb = fn(c["q"][q0:q1].transpose(1, 0, 2), c["k"][k0:k1].transpose(1, 0, 2), c["v"][k0:k1].transpose(1, 0, 2))
        o[q0:q1], lse[:, q0:q1] = ob.transpose(1, 0, 2), lb
    return o, lse


def references(c, causal, scale=SCALE):
    """(strict O, strict LSE, true O, true LSE), fp64, packed; computed once per (case, causal, scale) and read-only."""
    key = (c["name"], c["heads"], c["dtype"], bool(causal), scale)
    if key not in _REFS:
        strict = per_sequence(c, lambda q, k, v: reference(effective_q(_Rounder, q, c["dtype"], scale), k, v, causal, LN2))
        true = per_sequence(c, lambda q, k, v: reference(q, k, v, causal, scale))
        _REFS[key] = tuple(_ro(x) for x in strict + true)
    return _REFS[key]


def bars(c, scale=SCALE):
    """(strict O, strict LSE, true-Q O, true-Q LSE) bars of a case: util's, on the 192-wide rows, the scale explicit."""
    d = c["dtype"]
    return TOL_O[d], TOL_LSE[d], o_tol(d, 1, c["q"], c["k"], c["v"], scale, TOL_O[d]), lse_tol(d, 1, c["q"], c["k"], scale, TOL_LSE[d])


def _err(x, ref):
    """largest |x - ref| over the finite entries of ref; where ref is -inf (dead rows) x must be -inf too, where ref is 0 by death x is
    compared like any other value (0 exactly is asserted by the caller)"""
    dead = np.isneginf(ref)
    if not np.array_equal(np.isneginf(x), dead):
        return np.inf
    return float(np.abs(np.where(dead, 0.0, x) - np.where(dead, 0.0, ref)).max()) if x.size else 0.0


def errors(o, lse, c, causal, scale=SCALE):
    so, sl, to, tl = references(c, causal, scale)
    return _err(o, so), _err(lse, sl), _err(o, to), _err(lse, tl)


def check(o, lse, c, causal, where, scale=SCALE):
    """Every element of O [total_q, Hq, 128] and LSE [Hq, total_q] (fp64 arrays of what the call returned) against both references;
    dead rows O = 0 exactly and LSE = -inf. Prints every figure before it asserts."""
    e, b = errors(o, lse, c, causal, scale), bars(c, scale)
    print(f"mla_prefill {where}: strict O {e[0]:.3e} / {b[0]:.3e}  strict LSE {e[1]:.3e} / {b[1]:.3e}  true O {e[2]:.3e} / {b[2]:.3e}  "
          f"true LSE {e[3]:.3e} / {b[3]:.3e}")
    tl = references(c, causal, scale)[3]
    assert np.isfinite(o).all() and not np.isnan(lse).any(), where
    assert (o[np.isneginf(tl).T] == 0.0).all(), (where, "dead rows")
    for got, bar, what in zip(e, b, ("strict O", "strict LSE", "true-Q O", "true-Q LSE")):
        assert got < bar, (where, what, got, bar)
    return e


def exceeds_a_bar(o, lse, c, causal, scale=SCALE):
    return any(not got < bar for got, bar in zip(errors(o, lse, c, causal, scale), bars(c, scale)))


# ---- the chunked-context chain ("Latent-attention layers: prefill"): call A un-masked over the Lc cached keys, call B
# causal over the Ln new ones, merged through the LSEs:
#     lse = logaddexp(lse_a, lse_b),  O = O_a w_a + O_b w_b,  w_x = exp(lse_x - lse),  w_a + w_b = 1.
# With |dO_x| <= eO_x and |dlse_x| <= eL_x per call (its bars against the exact operator):
#     dlse = w_a dlse_a + w_b dlse_b                                     =>  |dlse| <= max(eL_a, eL_b)
#     w_a = 1 / (1 + exp(lse_b - lse_a)),  dw_a = w_a w_b (dlse_a - dlse_b), dw_b = -dw_a, w_a w_b <= 1/4 (first order; the e's are < 1e-1)
#     dO = w_a dO_a + w_b dO_b + (O_a - O_b) dw_a                        =>  |dO| <= max(eO_a, eO_b) + 2 max|v| (eL_a + eL_b) / 4
# (|O_x| <= max|v|: a convex combination of value rows). Second-order terms: the factor e^{eL} - 1 <= 1.06 eL for eL <= 0.1 is covered by
# taking exp(eL_a + eL_b) - 1 in place of eL_a + eL_b.
CHAIN = ((70, 130), (129, 64), (33, 0), (1, 1), (64, 257))  # (new tokens Ln, cached context Lc); Lc = 0: LSE_a = -inf, the side is skipped


def merge(o_a, lse_a, o_b, lse_b):
    """fp64 merge of two partial results (o [T, H, Dv], lse [H, T]); a side with lse = -inf is skipped"""
    lse = np.logaddexp(lse_a, lse_b)
    with np.errstate(invalid="ignore"):
        wa = np.where(np.isneginf(lse_a), 0.0, np.exp(lse_a - lse)).T[..., None]
        wb = np.where(np.isneginf(lse_b), 0.0, np.exp(lse_b - lse)).T[..., None]
    return np.where(wa > 0, o_a * wa, 0.0) + np.where(wb > 0, o_b * wb, 0.0), lse


def merge_bars(eO_a, eL_a, eO_b, eL_b, vmax):
    return max(eO_a, eO_b) + 2.0 * vmax * float(np.expm1(eL_a + eL_b)) / 4.0, max(eL_a, eL_b)
