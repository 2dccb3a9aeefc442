"""Shared pieces of the tests of fa_fwd_mla_decode_paged (absorbed MLA decode over a paged latent cache; include/fa_mi355.h, "Multi-head
latent attention (decode)"): an fp64 reference in numpy (the C oracle has one head dim), a pool builder in the manner of make_cache in
tests/test_gpu_decode_paged.py, an fp32 model of the kernel's arithmetic with plantable mistakes, the cases the GPU runs, and the bars.

The bars are the project's: against the true Q, util.lse_tol / util.o_tol with the pre-scaled-operand terms formed on the 576-wide rows
and base TOL_O[dtype]; strict, against the exact operator on util.effective_q (scale LN2), TOL_O[dtype] for O and 1e-4 for LSE. The scale
is passed explicitly everywhere: the helpers' default is D^-0.5 and the model's head dim is not 576."""
import functools

import numpy as np

import util

DQK, DV = 576, 512
SCALE = 192.0 ** -0.5  # (128 + 64)^-0.5: DeepSeek's, without mscale
STRICT_LSE = 1e-4

# the parity cases: (Hq, Nq, causal) and, per case, how the operands are laid out -- (pool row stride, padded page stride, q token-major,
# o under wide strides). (5, 3): 15 rows with a padding row and a head count that is no power of two; (32, 1) and (16, 2): two row blocks.
SHAPES = [(16, 1, False), (16, 2, True), (8, 4, True), (5, 3, True), (32, 1, False), (1, 1, False)]
LAYOUTS = [(576, False, False, False), (640, True, True, True), (576, True, True, False), (640, False, False, True),
           (576, False, False, False), (640, True, True, True)]
PAGES = [16, 64, 256]


def lengths(P):
    return [0, 1, 63, 64, 65, P - 1, P, P + 1, 1000, 4097]


def reference(q, kvs, lens, causal, scale, dv=DV):
    """fp64 (O [B,Hq,Nq,dv], LSE [B,Hq,Nq]) of q [B,Hq,Nq,Dqk] against each sequence's latent rows kvs[b] [L_b, Dqk]: every column enters
    the score, the first dv are the value; causal bottom-right aligned per sequence; rows with no visible key: O = 0, LSE = -inf."""
    B, Hq, Nq, _ = q.shape
    o = np.zeros((B, Hq, Nq, dv), np.float64)
    lse = np.full((B, Hq, Nq), -np.inf)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        kv = kvs[b].astype(np.float64)
        s = (q[b].astype(np.float64) @ kv.T) * float(scale)  # [Hq, Nq, L]
        if causal:
            i, j = np.arange(Nq)[:, None], np.arange(L)[None, :]
            s = np.where(j <= i + (L - Nq), s, -np.inf)
        m = s.max(-1, keepdims=True)
        live = np.isfinite(m[..., 0])
        p = np.exp(s - np.where(np.isfinite(m), m, 0.0))
        l = p.sum(-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            ob = (p @ kv[:, :dv]) / l
            lb = m[..., 0] + np.log(l[..., 0])
        o[b][live], lse[b][live] = ob[live], lb[live]
    return o, lse


def make_pool(oracle, rng, P, lens, dtype, row_stride=DQK, pad_page=False, spare=3, max_pages=None, amp=1.0, integer=False):
    """(pool fp32 [num_pages, P (+ 1 padding row), row_stride], table int32 [B, max_pages], kvs): pages are a random permutation of the
    pool; unused table entries name a NaN-filled spare page; slots past L_b of a last page, padding columns and padding rows are NaN.
    The device view a test passes is pool[:, :P, :576]. integer: small integer-valued rows (exact in every type and in fp32 sums)."""
    npb = [(L + P - 1) // P for L in lens]
    mp = max_pages or max(max(npb), 1)
    num_pages = sum(npb) + spare
    perm = rng.permutation(num_pages)
    pool = np.full((num_pages, P + (1 if pad_page else 0), row_stride), np.nan, np.float32)
    table = np.full((len(lens), mp), perm[-1], np.int32)
    kvs, used = [], 0
    for b, L in enumerate(lens):
        pages = perm[used:used + npb[b]]
        used += npb[b]
        table[b, :npb[b]] = pages
        if integer:
            kv = rng.integers(-4, 5, (L, DQK)).astype(np.float32)
        else:
            kv = oracle.round_to((amp * rng.uniform(-1.0, 1.0, (L, DQK))).astype(np.float32), dtype)
        for j, pg in enumerate(pages):
            n = min(P, L - j * P)
            pool[pg, :n, :DQK] = kv[j * P:j * P + n]
        kvs.append(kv)
    return pool, table, kvs


def bars(dtype, q, kvs, scale):
    """(O, LSE) against the true Q."""
    kk = np.concatenate([kv for kv in kvs if kv.size] or [np.zeros((1, DQK), np.float32)])
    return (util.o_tol(dtype, 1, q, kk, kk[:, :DV], scale, base=util.TOL_O[dtype]), util.lse_tol(dtype, 1, q, kk, scale))


def errors(oracle, o, lse, q, kvs, lens, causal, dtype, scale=SCALE):
    """The four figures a result is held to, each as (worst error, bar): O and LSE against the true Q, O and LSE strict (the exact operator
    on the pre-scaled operand the kernel multiplies). Dead rows must be exactly 0 / -inf: asserted here."""
    o64, l64 = reference(q, kvs, lens, causal, scale)
    dead = np.isneginf(l64)
    assert np.array_equal(o[dead], np.zeros_like(o[dead])) and np.isneginf(lse[dead]).all(), "rows with no visible key: O = 0 exactly, LSE = -inf"
    live = ~dead
    assert np.isfinite(o).all() and np.isfinite(lse[live]).all()
    tol_o, tol_l = bars(dtype, q, kvs, scale)
    o64q, l64q = reference(util.effective_q(oracle, q, dtype, scale), kvs, lens, causal, util.LN2)
    return {"o": (float(np.abs(o - o64).max()), tol_o),
            "lse": (float(np.abs(lse[live] - l64[live]).max(initial=0.0)), tol_l),
            "o_strict": (float(np.abs(o - o64q).max()), util.TOL_O[dtype]),
            "lse_strict": (float(np.abs(lse[live] - l64q[live]).max(initial=0.0)), STRICT_LSE)}


def check(oracle, o, lse, q, kvs, lens, causal, dtype, what, scale=SCALE):
    e = errors(oracle, o, lse, q, kvs, lens, causal, dtype, scale)
    print(what, {k: "%.3g / %.3g" % v for k, v in e.items()})
    for k, (err, bar) in e.items():
        assert err < bar, (what, k, err, bar)
    return e


MISTAKES = ("v_all_576", "v_from_64", "no_rotary", "scale_576", "top_left", "row_packing")


def model(oracle, q, kvs, lens, causal, scale, dtype, mistake=None):
    """The kernel's arithmetic in numpy fp32: Q~ = round(fp32(scale * log2 e) * q) to the input type, fp32 score sums over 576 columns,
    P = 2^(s - m) with l summed over the fp32 values and P ROUNDED to the input type in front of the PV product over 512 columns, fp32
    sums, O = acc / l rounded to the input type. `mistake` plants one of MISTAKES."""
    B, Hq, Nq, _ = q.shape
    R = Hq * Nq
    sc = np.float32(scale if mistake != "scale_576" else 576.0 ** -0.5)
    qt = util.effective_q(oracle, q, dtype, sc).astype(np.float32)
    o = np.zeros((B, Hq, Nq, DV), np.float32)
    lse = np.full((B, Hq, Nq), -np.inf, np.float32)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        kv = kvs[b].astype(np.float32)
        rows = qt[b].reshape(R, DQK)  # r = h * Nq + iq
        iq = np.arange(R) % Nq
        if mistake == "row_packing":  # the block filled as r = iq * Hq + h, read back as r = h * Nq + iq
            rows = qt[b].transpose(1, 0, 2).reshape(R, DQK)
        cols = DV if mistake == "no_rotary" else DQK
        s = (rows[:, :cols] @ kv[:, :cols].T).astype(np.float32)  # log2 units
        if causal:
            lim = iq[:, None] + (0 if mistake == "top_left" else L - Nq)
            s = np.where(np.arange(L)[None, :] <= lim, s, -np.inf).astype(np.float32)
        m = s.max(-1, keepdims=True)
        live = np.isfinite(m[:, 0])
        p = np.exp2(s - np.where(np.isfinite(m), m, np.float32(0.0))).astype(np.float32)
        l = p.sum(-1, dtype=np.float32)
        pr = oracle.round_to(p, dtype).astype(np.float32)
        if mistake == "v_all_576":  # rows of 576 formed and written at a pitch of 576, read back at 512
            acc = (pr @ kv).astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                flat = (acc / l[:, None]).reshape(-1)[:R * DV].reshape(R, DV)
        else:
            v = kv[:, DQK - DV:] if mistake == "v_from_64" else kv[:, :DV]
            with np.errstate(divide="ignore", invalid="ignore"):
                flat = (pr @ v).astype(np.float32) / l[:, None]
        with np.errstate(divide="ignore"):
            lb = ((m[:, 0] + np.log2(l)) * np.float32(util.LN2)).astype(np.float32)
        ob = np.where(live[:, None], flat, np.float32(0.0)).astype(np.float32)
        o[b] = oracle.round_to(ob, dtype).reshape(Hq, Nq, DV)
        lse[b] = np.where(live, lb, -np.inf).reshape(Hq, Nq)
    return o, lse


@functools.lru_cache(maxsize=None)
def _case(P, dtype, shape_idx):
    import oracle

    oracle.build()
    Hq, Nq, causal = SHAPES[shape_idx]
    row_stride, pad_page, token_major, wide_o = LAYOUTS[shape_idx]
    rng = np.random.default_rng(2400 + 10 * P + shape_idx)
    lens = [int(x) for x in rng.permutation(lengths(P))]
    q = oracle.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, DQK)).astype(np.float32), dtype)
    pool, table, kvs = make_pool(oracle, rng, P, lens, dtype, row_stride, pad_page)
    for a in [q, pool, table] + kvs:
        a.setflags(write=False)  # computed once, shared, left unchanged
    return {"Hq": Hq, "Nq": Nq, "causal": causal, "P": P, "dtype": dtype, "lens": lens, "q": q, "pool": pool, "table": table, "kvs": kvs,
            "token_major": token_major, "wide_o": wide_o}


def case(P, dtype, shape_idx):
    """One parity case (inputs built once per process and shared read-only)."""
    return _case(P, dtype, shape_idx)
