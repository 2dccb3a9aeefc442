"""The reference and the bound of fa_bwd_mla_sparse (include/fa_mi355.h, "Multi-head latent attention (sparse, backward)"), test side only:
numpy, fp64. Per (token, head) the operator is tests/backward_bound.py's one-head backward with Nq = 1 on the gathered rows (k = the 576
columns, v = the first 512), so head_exact / head_bounds apply unchanged; dk and dv are scattered by slot into pool-shaped arrays, entries
outside the pool dropped, a slot named twice added twice. The cases are tests/mla_sparse.py's; dO is U(-1, 1) rounded to the type.

Two terms are added to the bound of a dkv element, both derived from what csrc/fa_mla_sparse_bwd_kernel.hip documents, none fitted:
  * the head block. One workgroup sums the HB = 32 heads of its block on the matrix cores in fp32 (where head_model adds heads exactly),
    multiplies the key side by scale and adds the value side: HB - 1 additions, one multiplication and one addition, each off by at most
    2^-24 of a partial result that is at most sum_h (|dk_h| + |dv_h|) to first order:  2^-24 (HB + 2) sum_{h in block} (|dk_h| + |dv_h|).
  * the atomic sum. The m contributions a_i (one per token, head block and naming of the slot) meet in memory in any order, every
    addition off by at most 2^-24 of a partial sum that is at most sum_i (|a_i| + b_i), b_i the bound of a_i:  2^-24 m sum_i (|a_i| + b_i).
chain=True: the bound of the TRUE gradient for a backward fed the O and LSE that fa_fwd_mla_decode_sparse wrote. That forward has the
prefill's two error sources -- a query operand pre-scaled and rounded once, an fp32 row sum over unrounded probabilities, tiles of 64 --
so the terms are tests/mla_bwd.py's forward_errors, handed to head_bounds(lse_err=, o_err=) as that module does."""
import functools

import numpy as np

import backward_bound as bb
import mla_bwd
import mla_sparse

DQK, DV, SCALE, HB = mla_sparse.DQK, mla_sparse.DV, mla_sparse.SCALE, 32


@functools.lru_cache(maxsize=None)
def problem(idx, dtype, chain=False):
    """do, exact o and lse, ref / bound of dq [T,Hq,576] and dkv [slots,576], named (slots some list names); built once, read-only"""
    c = mla_sparse.case(idx, dtype)
    T, Hq, P = c["T"], c["Hq"], c["P"]
    nslots = c["pool"].shape[0] * P
    do = bb.rnd(np.random.default_rng(8800 + idx).uniform(-1.0, 1.0, (T, Hq, DV)).astype(np.float32), dtype)
    r = {"do": do, "o": np.zeros((T, Hq, DV)), "lse": np.full((T, Hq), -np.inf), "dq": np.zeros((T, Hq, DQK)), "dq_bound": np.zeros((T, Hq, DQK)),
         "dkv": np.zeros((nslots, DQK)), "dkv_bound": np.zeros((nslots, DQK)), "named": np.zeros(nslots, bool)}
    mass, count = np.zeros((nslots, DQK)), np.zeros(nslots)
    for t in range(T):
        rows, n = c["kvs"][t], c["lens"][t]
        if n == 0:
            continue
        x = c["indices"][t, :n].astype(np.int64)
        ok = (x >= 0) & (x < nslots)
        for h0 in range(0, Hq, HB):
            a, b, inner = np.zeros((n, DQK)), np.zeros((n, DQK)), np.zeros((n, DQK))
            for h in range(h0, min(h0 + HB, Hq)):
                q1, d1 = c["q"][t, h][None], do[t, h][None]
                R = bb.head_exact(q1, rows, rows[:, :DV], d1, False, SCALE)
                le, oe = mla_bwd.forward_errors(q1, rows, rows[:, :DV], False, SCALE, dtype, R) if chain else (None, None)
                bq, bk, bv = bb.head_bounds(q1, rows, rows[:, :DV], d1, SCALE, dtype, R, le, oe)
                r["o"][t, h], r["lse"][t, h], r["dq"][t, h], r["dq_bound"][t, h] = R["o"][0], R["lse"][0], R["dq"][0], bq[0]
                a += R["dk"]
                a[:, :DV] += R["dv"]
                b += bk
                b[:, :DV] += bv
                inner += np.abs(R["dk"])
                inner[:, :DV] += np.abs(R["dv"])
            b += bb.U32 * (HB + 2) * inner
            np.add.at(r["dkv"], x[ok], a[ok])
            np.add.at(r["dkv_bound"], x[ok], b[ok])
            np.add.at(mass, x[ok], np.abs(a[ok]) + b[ok])
            np.add.at(count, x[ok], 1.0)
        r["named"][x[ok]] = True
    r["dkv_bound"] += bb.U32 * count[:, None] * mass
    for v in r.values():
        v.setflags(write=False)
    return r


def worst(r, dq, dkv, scale=1.0, what=""):
    out = bb.ratios((dq, dkv), (scale * r["dq"], scale * r["dkv"]), (scale * r["dq_bound"], scale * r["dkv_bound"]))
    print(what, "worst error / bound: dq %.3g dkv %.3g" % tuple(out))
    return out
