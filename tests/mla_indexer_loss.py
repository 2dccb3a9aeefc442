"""References and bounds of fa_mla_sparse_head_probs and fa_mla_indexer_loss_sparse (include/fa_mi355.h, "Training the MLA indexer"), test
side only: numpy, fp64, on gathered rows. Every bound is derived from the rounding rules the header states, none is fitted.

CALL 1. probs[t][j] = sum_h P_hj, P_hj = exp(s_hj - lse_h), s = scale q . k. The kernel forms the score in log2 units from Q~ = round(c2 Q)
(c2 = scale log2 e): with A_hj = sum_d |c2 q_d k_d| the score is off by at most E_hj = (U + 578 U32) A_hj + U32 (4 |lse2_h| + |s2_hj|) --
one rounding to the type per element of Q~, the fp32 product and 576 fp32 additions, the product lse . log2 e and the subtraction. P is
then off by P (expm1(ln 2 E) + 4 U32) (exp2 within two ulp), and the fp32 sum over Hq heads by Hq U32 sum_h P:
    bound_j = sum_h P_hj (expm1(ln 2 E_hj) + 4 U32) + Hq U32 sum_h P_hj.
A row's sum differs from Hq by the same terms twice -- the forward's own LSE carries each score's error once more -- plus this module's
fp64 sum of fp32 values: |sum_j probs_j - Hq| <= 2 sum_j bound_j + (n + 64) U32 Hq.

CALL 2. q_idx and k_idx sit on multiples of 1/4 in [-1, 1]: every score is a multiple of 1/16 below 128, exact in fp32, and so is the relu
mask. In fp32: I_j = sum_h w_h relu(s_hj) is off by eI_j = (Hi + 2) U32 sum_h |w_h| relu(s_hj); with eI = max_j eI_j a softmax weight is off
by pi_j epi, epi = expm1(2 eI) + (n + 8) U32 (exponentials within two ulp, n additions, one division), tau_j by tau_j (n + 2) U32;
    loss:  sum_j tau_j (2 eI + (n + 8) U32 (1 + |ln tau_j| + |ln pi_j|)) + n U32 sum_j |term_j|
    g_j:   eg_j = |u| (pi_j epi + tau_j (n + 2) U32) + 2 U32 |g_j|
    G_hj = round(g_j w_h) [s_hj > 0] to the type:  eG_hj = (|w_h| eg_j + (2 U + U32) |g_j w_h|) [s_hj > 0]
           (the kernel rounds its own g_j w_h, the reference the exact one: the two roundings differ by at most U each)
    dw_h:  sum_j eg_j relu(s_hj) + (n + 2) U32 sum_j |g_j| relu(s_hj)
    dq_hd: sum_j eG_hj |k_jd| + (n + 2) U32 sum_j |G_hj k_jd|
    dk contribution of (t, j): a = sum_h G_hj q_hd, b = sum_h eG_hj |q_hd| + (Hi + 2) U32 sum_h |G_hj q_hd|; the m contributions of a slot
    meet in memory in any order (tests/mla_sparse_bwd.py's atomic term): + U32 m sum_i (|a_i| + b_i)."""
import functools

import numpy as np

import backward_bound as bb

U32, LOG2E = bb.U32, 1.4426950408889634
DI = 128


def probs_reference(q, kvs, lens, lse, scale, dtype):
    """q [T,Hq,576], kvs[t] [n_t,576] gathered rows, lse [T,Hq] as the call is given it -> (ref, bound), lists of [n_t] fp64"""
    U, c2 = bb.U[dtype], scale * LOG2E
    refs, bounds = [], []
    for t, rows in enumerate(kvs):
        qt, kt = q[t].astype(np.float64), rows[:lens[t]].astype(np.float64)
        s2, A = c2 * qt @ kt.T, c2 * np.abs(qt) @ np.abs(kt).T  # [Hq, n]
        lse2 = lse[t].astype(np.float64)[:, None] * LOG2E
        P = np.exp2(s2 - lse2)
        E = (U + 578 * U32) * A + U32 * (4 * np.abs(lse2) + np.abs(s2))
        refs.append(P.sum(0))
        bounds.append((P * (np.expm1(np.log(2.0) * E) + 4 * U32)).sum(0) + q.shape[1] * U32 * P.sum(0))
    return refs, bounds


# ---- call 2: (Hi, topk, P, counts of the three tokens or None, token with a zero target row or None)
LOSS_CASES = [(32, 1, 16, (0, 1, 1), None), (64, 1, 64, None, None), (32, 65, 64, (1, 33, 65), None), (64, 65, 16, (65, 0, 64), 0),
              (32, 320, 16, None, None), (64, 320, 64, (320, 129, 1), 1)]
NSLOTS = 1024


@functools.lru_cache(maxsize=None)
def loss_case(idx, dtype):
    """inputs (fp32 numpy, values of the type) and the fp64 reference with its bounds; built once, read-only"""
    Hi, topk, P, counts, zero_row = LOSS_CASES[idx]
    rng, T, U = np.random.default_rng(9100 + idx), 3, bb.U[dtype]
    grid = lambda *shape: (rng.integers(-4, 5, shape) / 4.0).astype(np.float32)
    c = {"Hi": Hi, "topk": topk, "P": P, "T": T, "q": grid(T, Hi, DI), "w": (0.25 * rng.uniform(-1, 1, (T, Hi))).astype(np.float32),
         "pool": grid(NSLOTS, DI), "u": rng.uniform(0.5, 2.0, T).astype(np.float32), "counts": None if counts is None else np.array(counts, np.int32)}
    pitch = (topk + 7) // 4 * 4
    idxs = np.stack([rng.permutation(NSLOTS)[:pitch] for _ in range(T)]).astype(np.int32)
    if topk > 2:
        idxs[:, 1], idxs[:, 2] = idxs[:, 0], NSLOTS + 5  # a slot named twice, an entry outside the pool
    target = (rng.uniform(0, 1, (T, pitch)) * (rng.uniform(0, 1, (T, pitch)) > 0.2)).astype(np.float32)
    if topk == 1:
        target[:] = 0.75
    if zero_row is not None:
        target[zero_row, :topk] = 0.0
    lens = [topk if counts is None else int(counts[t]) for t in range(T)]
    r = {"loss": np.zeros(T), "loss_b": np.zeros(T), "dq": np.zeros((T, Hi, DI)), "dq_b": np.zeros((T, Hi, DI)), "dw": np.zeros((T, Hi)),
         "dw_b": np.zeros((T, Hi)), "dk": np.zeros((NSLOTS, DI)), "dk_b": np.zeros((NSLOTS, DI)), "named": np.zeros(NSLOTS, bool)}
    mass, count = np.zeros((NSLOTS, DI)), np.zeros(NSLOTS)
    for t in range(T):
        n, x = lens[t], idxs[t, :lens[t]].astype(np.int64)
        ok = x < NSLOTS
        r["named"][x[ok]] = True
        tg = target[t, :n].astype(np.float64)
        if n == 0 or tg.sum() == 0:
            continue
        q, w, u = c["q"][t].astype(np.float64), c["w"][t].astype(np.float64), float(c["u"][t])
        k = np.where(ok[:, None], c["pool"][np.minimum(x, NSLOTS - 1)], 0.0).astype(np.float64)
        s = q @ k.T  # [Hi, n]
        relu, mask = np.maximum(s, 0.0), s > 0
        I = w @ relu
        eI = ((Hi + 2) * U32 * (np.abs(w) @ relu)).max()
        lpi = I - I.max() - np.log(np.exp(I - I.max()).sum())
        pi, tau = np.exp(lpi), tg / tg.sum()
        pos = tau > 0
        term = np.where(pos, tau * (np.log(np.where(pos, tau, 1.0)) - lpi), 0.0)
        r["loss"][t] = term.sum()
        r["loss_b"][t] = (tau * (2 * eI + (n + 8) * U32 * (1 + np.abs(np.log(np.where(pos, tau, 1.0))) + np.abs(lpi)))).sum() + n * U32 * np.abs(term).sum()
        g = u * (pi - tau)
        eg = abs(u) * (pi * (np.expm1(2 * eI) + (n + 8) * U32) + tau * (n + 2) * U32) + 2 * U32 * np.abs(g)
        G = bb.rnd((w[:, None] * g[None, :]).astype(np.float32), dtype).astype(np.float64) * mask
        eG = (np.abs(w)[:, None] * eg[None, :] + (2 * U + U32) * np.abs(w[:, None] * g[None, :])) * mask
        r["dw"][t], r["dw_b"][t] = relu @ g, relu @ eg + (n + 2) * U32 * (relu @ np.abs(g))
        r["dq"][t], r["dq_b"][t] = G @ k, eG @ np.abs(k) + (n + 2) * U32 * (np.abs(G) @ np.abs(k))
        a, b = G.T @ q, eG.T @ np.abs(q) + (Hi + 2) * U32 * (np.abs(G).T @ np.abs(q))
        np.add.at(r["dk"], x[ok], a[ok])
        np.add.at(r["dk_b"], x[ok], b[ok])
        np.add.at(mass, x[ok], np.abs(a[ok]) + b[ok])
        np.add.at(count, x[ok], 1.0)
    r["dk_b"] += U32 * count[:, None] * mass
    c.update(indices=idxs, target=target, lens=lens, ref=r)
    for v in list(c.values()) + list(r.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
