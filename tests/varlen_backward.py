"""Per-sequence reference, bound and rounding model for the varlen backward (test side only; numpy, fp64), built from
tests/backward_bound.py: per sequence fa_bwd_varlen is fa_bwd_ex on that sequence, so the bound of that module applies sequence by
sequence. What varlen adds are query rows without a visible key (Lk = 0, or causal with i + Lk - Lq < 0): backward_bound.head_exact
yields NaN on an all-masked row, so those rows are CUT before it is called -- under the bottom-right aligned mask the remaining rows
Lq - Lk .. Lq - 1 against the Lk keys are exactly a causal problem with equal lengths -- and their dQ is 0 with bound 0 (exactly zero
is required), as is their share of dK / dV.

The catalogue the CPU and the GPU tests share is CASES: the shapes of tests/test_gpu_varlen.py (CONFIGS, imported) and one more
configuration with Lk < Lq, Lk = 0 and Lq = 0."""
import numpy as np

import backward_bound as bb
from test_gpu_varlen import CONFIGS

# (Hq, Hkv, layout, [(Lq, Lk), ...]); the last one: a sequence with more queries than keys, one without keys, one without queries
CASES = list(CONFIGS) + [(4, 2, "THD", [(70, 70), (200, 130), (64, 0), (0, 70), (130, 257), (129, 1)])]


def first_live_row(Lq, Lk, causal):
    """Query rows [0, n0) of a sequence see no key."""
    if Lk == 0:
        return Lq
    return max(Lq - Lk, 0) if causal else 0


def draw_seq(rng, Hq, Hkv, Lq, Lk, D, dtype):
    """q, do [Hq, Lq, D], k, v [Hkv, Lk, D]: fp32 arrays holding values of `dtype`."""
    def draw(*shape):
        return bb.rnd(rng.uniform(-1.0, 1.0, shape).astype(np.float32), dtype)
    return draw(Hq, Lq, D), draw(Hkv, Lk, D), draw(Hkv, Lk, D), draw(Hq, Lq, D)


class SeqBounds:
    """One sequence: ref = exact (dQ, dK, dV), bound = their bounds, o [Hq, Lq, D] and lse [Hq, Lq] of the exact forward (0 and -inf on
    rows without a visible key); model(fn) applies a per-head model fn(h, q_h, k_h, v_h, do_h, R) -> (dq, dk, dv) of the LIVE rows (default:
    backward_bound.head_model, the kernels' roundings) and assembles it like the reference."""

    def __init__(self, q, k, v, do, causal, scale, dtype):
        self.q, self.k, self.v, self.do = q, k, v, do
        self.causal, self.dtype = causal, dtype
        self.scale = bb.default_scale(q.shape[-1]) if scale is None else float(scale)
        Hq, Lq, D = q.shape
        Hkv, Lk = k.shape[0], k.shape[1]
        self.G, self.n0 = Hq // Hkv, first_live_row(Lq, Lk, causal)
        self.o, self.lse = np.zeros(q.shape), np.full((Hq, Lq), -np.inf)
        self.ref = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.bound = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.R = {}
        n0 = self.n0
        if n0 >= Lq:
            return
        for h in range(Hq):
            hk = h // self.G
            R = bb.head_exact(q[h, n0:], k[hk], v[hk], do[h, n0:], causal, self.scale)
            B = bb.head_bounds(q[h, n0:], k[hk], v[hk], do[h, n0:], self.scale, dtype, R)
            self.R[h] = R
            self.o[h, n0:], self.lse[h, n0:] = R["o"], R["lse"]
            self.ref[0][h, n0:] = R["dq"]
            self.ref[1][hk] += R["dk"]
            self.ref[2][hk] += R["dv"]
            self.bound[0][h, n0:] = B[0]
            self.bound[1][hk] += B[1]
            self.bound[2][hk] += B[2]

    def model(self, fn=None):
        q, k, v, do, n0 = self.q, self.k, self.v, self.do, self.n0
        out = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        for h, R in self.R.items():
            hk = h // self.G
            if fn is None:
                g = bb.head_model(q[h, n0:], k[hk], v[hk], do[h, n0:], self.causal, self.scale, self.dtype, R)
            else:
                g = fn(h, q[h, n0:], k[hk], v[hk], do[h, n0:], R)
            out[0][h, n0:] = g[0]
            out[1][hk] += g[1]
            out[2][hk] += g[2]
        return out


def worst_ratio(grads, sb):
    """Worst |g - ref| / bound over the three gradients of one sequence; NaN / Inf anywhere counts as infinite."""
    if not all(np.isfinite(np.asarray(g, np.float64)).all() for g in grads):
        return float("inf")
    return max(bb.ratios(grads, sb.ref, sb.bound))
