"""GPU: fa_fwd_varlen (flash_attention_varlen), the forward over packed variable-length sequences.

Per sequence the operator is fa_fwd_ex on that sequence, so every check is made sequence by sequence:
  * against the fp64 oracle on the effective (pre-scaled) Q, at the project's bars (util.TOL_O; LSE through util.lse_tol);
  * bit for bit against fa_fwd_exv(FA_VARIANT_MFMA) on the sequence alone (torch.equal on O and LSE), whatever the layout, the other
    sequences, max_seqlen_* or the order of the sequences;
  * on the exact-arithmetic inputs of tests/exact_forward.py, every element to bars();
  * rows without a visible key: O = 0 exactly, LSE = -inf;
  * the write footprint in canary-filled buffers, also under corrupt tables; a K / V buffer above 4 GiB; one captured graph replayed
    after both tables changed in place."""
import numpy as np
import pytest

import exact_forward as ef
from util import LN2, TOL_O, effective_q, lse_tol, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def seq_data(oracle, rng, Hq, Hkv, Lq, Lk, D, dtype):
    """One sequence: q [Hq, Lq, D], k / v [Hkv, Lk, D], fp32 arrays holding values of `dtype`."""
    def draw(*shape):
        return oracle.round_to(rng.uniform(-1.0, 1.0, shape).astype(np.float32), dtype)
    return draw(Hq, Lq, D), draw(Hkv, Lk, D), draw(Hkv, Lk, D)


def pack(seqs, dtype, layout, tail_q=0, tail_k=0):
    """Sequences back to back as device tensors q [total_q, Hq, D], k / v [total_k, Hkv, D] in one of the layouts the header names, plus
    the cu_seqlens as numpy int32. tail_*: tokens behind the last sequence that belong to nobody."""
    Hq, _, D = seqs[0][0].shape
    Hkv = seqs[0][1].shape[0]
    qn = np.concatenate([s[0].transpose(1, 0, 2) for s in seqs] + [np.zeros((tail_q, Hq, D), np.float32)])
    kn = np.concatenate([s[1].transpose(1, 0, 2) for s in seqs] + [np.zeros((tail_k, Hkv, D), np.float32)])
    vn = np.concatenate([s[2].transpose(1, 0, 2) for s in seqs] + [np.zeros((tail_k, Hkv, D), np.float32)])
    cu_q = np.cumsum([0] + [s[0].shape[1] for s in seqs]).astype(np.int32)
    cu_k = np.cumsum([0] + [s[1].shape[1] for s in seqs]).astype(np.int32)
    if layout == "THD":  # [total, H, D]
        q, k, v = to_dev(qn, dtype), to_dev(kn, dtype), to_dev(vn, dtype)
    elif layout == "HTD":  # [H, total, D] storage
        q, k, v = (to_dev(x.transpose(1, 0, 2), dtype).transpose(0, 1) for x in (qn, kn, vn))
    else:  # "QKV": three views of one packed [total, Hq + 2 Hkv, D] projection
        assert layout == "QKV" and qn.shape[0] == kn.shape[0]
        buf = to_dev(np.concatenate([qn, kn, vn], axis=1), dtype)
        q, k, v = buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]
    return q, k, v, cu_q, cu_k


def cu_dev(cu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(cu, np.int32)).cuda()


def varlen(fa, q, k, v, cu_q, cu_k, max_q, max_k, causal, scale=None, **kw):
    import torch

    o, lse = fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), is_causal=causal, scale=scale, **kw)
    torch.cuda.synchronize()
    return o, lse


def dense_exv(fa, q4, k4, v4, dtype, causal, scale=None):
    """fa_fwd_exv(FA_VARIANT_MFMA) through the C entry point on contiguous [B, H, N, D] numpy inputs: (O, LSE) device tensors."""
    import torch

    lib = fa.load_library()
    qd, kd, vd = to_dev(q4, dtype), to_dev(k4, dtype), to_dev(v4, dtype)
    B, Hq, Nq, D = q4.shape
    Hkv, Nk = k4.shape[1], k4.shape[2]
    o = torch.empty_like(qd)
    lse = torch.empty(B, Hq, Nq, dtype=torch.float32, device="cuda")
    sc = D ** -0.5 if scale is None else float(scale)
    st = lib.fa_fwd_exv(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), lse.data_ptr(), B, Hq, Hkv, Nq, Nk, D, sc, Hq * Nq * D, Nq * D,
                        Hkv * Nk * D, Nk * D, int(causal), fa.DTYPES[dtype], fa.VARIANTS["mfma"], torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    return o, lse


def piece(o, lse, cu_q, b):
    """Sequence b of a packed result as ([Hq, Lq, D], [Hq, Lq])."""
    s, e = int(cu_q[b]), int(cu_q[b + 1])
    return o[s:e].transpose(0, 1), lse[:, s:e]


def assert_bits(o, lse, cu_q, b, dense, what):
    import torch

    ob, lb = piece(o, lse, cu_q, b)
    assert torch.equal(ob, dense[0][0]), (what, b, "O differs from fa_fwd_exv on the sequence alone",
                                          float((ob.float() - dense[0][0].float()).abs().max()))
    assert torch.equal(lb, dense[1][0]), (what, b, "LSE differs from fa_fwd_exv on the sequence alone")


# Hq / Hkv in {1, 4, 8}; 1, 5 and 9 sequences; lengths on both sides of 64, 128 and 256; Lq != Lk; every layout
CONFIGS = [
    (4, 4, "THD", [(129, 300)]),
    (8, 2, "HTD", [(63, 63), (64, 200), (65, 65), (127, 129), (128, 257)]),
    (8, 1, "QKV", [(1, 1), (63, 63), (64, 64), (65, 65), (127, 127), (128, 128), (129, 129), (255, 255), (257, 257)]),
    (4, 1, "THD", [(256, 256), (130, 255), (2, 64)]),
]
_CACHE = {}


def run_config(fa, oracle, dtype, D, causal, ci):
    """One configuration through the varlen call (max_seqlen = the true maxima) and, per sequence, through fa_fwd_exv. Cached (a few MB in
    all): the parity and the bit-identity tests look at the same runs."""
    key = (dtype, D, causal, ci)
    if key not in _CACHE:
        Hq, Hkv, layout, lens = CONFIGS[ci]
        rng = np.random.default_rng(1000 * ci + D + (7 if causal else 0))
        seqs = [seq_data(oracle, rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in lens]
        q, k, v, cu_q, cu_k = pack(seqs, dtype, layout)
        o, lse = varlen(fa, q, k, v, cu_q, cu_k, max(l[0] for l in lens), max(l[1] for l in lens), causal)
        dense = [dense_exv(fa, s[0][None], s[1][None], s[2][None], dtype, causal) for s in seqs]
        _CACHE[key] = (seqs, (q, k, v, cu_q, cu_k), (o, lse), dense)
    return _CACHE[key]


GRID = [(t, d, c) for t in ("f16", "bf16") for d in (64, 128) for c in (False, True)]


# ---- oracle parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", GRID)
def test_oracle_parity_per_sequence(fa, oracle_mod, dtype, D, causal):
    for ci, (Hq, Hkv, layout, lens) in enumerate(CONFIGS):
        seqs, (_, _, _, cu_q, _), (o, lse), _ = run_config(fa, oracle_mod, dtype, D, causal, ci)
        for b, (qb, kb, vb) in enumerate(seqs):
            ob, lb = piece(o, lse, cu_q, b)
            on, ln = ob.float().cpu().numpy(), lb.cpu().numpy()
            assert np.isfinite(on).all() and np.isfinite(ln).all(), (ci, b)
            o64, l64 = oracle_mod.attn_fwd_ex_f64(effective_q(oracle_mod, qb, dtype)[None], kb[None], vb[None], causal, LN2)
            err_o, err_l = np.abs(on - o64[0]).max(), np.abs(ln - l64[0]).max()
            tol_l = lse_tol(dtype, 1, qb, kb)
            print(f"VARLEN parity {dtype} D={D} causal={causal} {layout} Hq/Hkv={Hq}/{Hkv} seq {b} {lens[b]}: O {err_o:.2e} (bar {TOL_O[dtype]:.1e}) "
                  f"LSE {err_l:.2e} (bar {tol_l:.2e})")
            assert err_o < TOL_O[dtype], (dtype, D, causal, ci, b, lens[b], err_o)
            assert err_l < tol_l, (dtype, D, causal, ci, b, lens[b], err_l)


# ---- bit-identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", GRID)
def test_bit_identical_to_the_dense_kernel_per_sequence(fa, oracle_mod, dtype, D, causal):
    for ci, (Hq, Hkv, layout, lens) in enumerate(CONFIGS):
        seqs, (q, k, v, cu_q, cu_k), (o, lse), dense = run_config(fa, oracle_mod, dtype, D, causal, ci)
        for b in range(len(seqs)):
            assert_bits(o, lse, cu_q, b, dense[b], (dtype, D, causal, ci, "max_seqlen = the maxima"))
        # a second, larger max_seqlen_q / max_seqlen_k: more (empty) blocks, another issue order, the same bits
        o2, lse2 = varlen(fa, q, k, v, cu_q, cu_k, int(cu_q[-1]), int(cu_k[-1]), causal)
        for b in range(len(seqs)):
            assert_bits(o2, lse2, cu_q, b, dense[b], (dtype, D, causal, ci, "max_seqlen = the totals"))
        # the sequences in another order (and another layout): every sequence keeps its bits
        if len(seqs) > 1:
            perm = np.random.default_rng(ci).permutation(len(seqs))
            other = {"THD": "HTD", "HTD": "THD", "QKV": "QKV"}[layout]
            qp, kp, vp, cq, ck = pack([seqs[i] for i in perm], dtype, other)
            o3, lse3 = varlen(fa, qp, kp, vp, cq, ck, max(l[0] for l in lens) + 5, max(l[1] for l in lens) + 1, causal)
            for pos, i in enumerate(perm):
                assert_bits(o3, lse3, cq, pos, dense[i], (dtype, D, causal, ci, "permuted"))


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, False), ("bf16", 128, True), ("f16", 64, False)])
def test_equal_lengths_match_one_dense_batched_call(fa, oracle_mod, dtype, D, causal):
    import torch

    B, Hq, Hkv, L = 3, 4, 2, 200
    rng = np.random.default_rng(D + causal)
    seqs = [seq_data(oracle_mod, rng, Hq, Hkv, L, L, D, dtype) for _ in range(B)]
    o4, l4 = dense_exv(fa, np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs]), dtype, causal)
    for layout in ("THD", "HTD", "QKV"):
        q, k, v, cu_q, cu_k = pack(seqs, dtype, layout)
        o, lse = varlen(fa, q, k, v, cu_q, cu_k, L, L, causal)
        assert torch.equal(o.reshape(B, L, Hq, D).permute(0, 2, 1, 3), o4), (layout, "O")
        assert torch.equal(lse.reshape(Hq, B, L).permute(1, 0, 2), l4), (layout, "LSE")


# ---- exact-arithmetic inputs: families A and B per sequence, every element to bars() ------------------------------------------------
EXACT_LENS = {"A": [(1, 1), (63, 63), (64, 130), (129, 129), (200, 257), (65, 1000)], "B": [(129, 129), (130, 257), (255, 576), (300, 1000)]}


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("dtype,D,causal", GRID)
def test_exact_arithmetic_per_sequence(fa, dtype, D, causal, family):
    Hq, Hkv, kexp = 4, 2, (0 if D == 64 else -1)
    cases = [ef.build(family, 1, Hq, Hkv, Lq, Lk, D, dtype, causal, kexp=kexp, span=ef.span_for(dtype, False, Lk) if family == "A" else 3,
                      seed=31 * i + D + (1 if causal else 0)) for i, (Lq, Lk) in enumerate(EXACT_LENS[family])]
    for c in cases:
        assert ef.representable(c.q, dtype) and ef.representable(c.k, dtype) and ef.representable(c.v, dtype)
    seqs = [(c.q[0], c.k[0], c.v[0]) for c in cases]
    worst = dict(o=0.0, lse=0.0)
    for layout in ("THD", "HTD"):
        q, k, v, cu_q, cu_k = pack(seqs, dtype, layout)
        o, lse = varlen(fa, q, k, v, cu_q, cu_k, max(l[0] for l in EXACT_LENS[family]), max(l[1] for l in EXACT_LENS[family]), causal,
                        scale=cases[0].scale)
        for b, case in enumerate(cases):
            ob, lb = piece(o, lse, cu_q, b)
            for h in range(Hq):
                ref = ef.reference_head(case, 0, h)
                r = ef.ratios(case, ref, ob[h].float().cpu().numpy(), lb[h].cpu().numpy(), 0, 0.0)
                assert r["o"] <= 1.0 and r["lse"] <= 1.0, (dtype, D, causal, family, layout, b, h, r)
                assert family == "B" or r["proven"] == 1.0, (b, h, "a family-A row is not proven exact: bar A would not apply")
                worst = dict(o=max(worst["o"], r["o"]), lse=max(worst["lse"], r["lse"]))
    print(f"EXACT fa_fwd_varlen {dtype} {family} D={D} causal={causal}: O {worst['o']:.3f} LSE {worst['lse']:.3f} of bar")


# ---- rows without a visible key -------------------------------------------------------------------------------------------------
def _rows_against_oracle(oracle, ob, lb, qb, kb, vb, dtype, first):
    """Causal with Lk < Lq: rows first .. Lq-1 are the causal square problem of the last Lk queries against all keys."""
    on, ln = ob[:, first:].float().cpu().numpy(), lb[:, first:].cpu().numpy()
    qs = np.ascontiguousarray(qb[:, first:])
    o64, l64 = oracle.attn_fwd_ex_f64(effective_q(oracle, qs, dtype)[None], kb[None], vb[None], True, LN2)
    assert np.abs(on - o64[0]).max() < TOL_O[dtype] and np.abs(ln - l64[0]).max() < lse_tol(dtype, 1, qs, kb)


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 64), ("bf16", 128), ("f16", 128)])
def test_rows_without_a_visible_key(fa, oracle_mod, dtype, D):
    import torch

    Hq, Hkv = 4, 2
    lens = [(100, 100), (200, 70), (64, 0), (0, 50), (300, 10), (150, 151), (33, 1)]
    rng = np.random.default_rng(5 + D)
    seqs = [seq_data(oracle_mod, rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in lens]
    for layout in ("THD", "HTD"):
        q, k, v, cu_q, cu_k = pack(seqs, dtype, layout)
        for causal in (True, False):
            o, lse = varlen(fa, q, k, v, cu_q, cu_k, 300, 151, causal)
            for b, (Lq, Lk) in enumerate(lens):
                if Lq == 0:
                    continue
                ob, lb = piece(o, lse, cu_q, b)
                dead = Lq if Lk == 0 else (max(Lq - Lk, 0) if causal else 0)  # rows 0 .. dead-1 see no key
                assert torch.equal(ob[:, :dead], torch.zeros_like(ob[:, :dead])), (layout, causal, b, "O of rows without a visible key must be 0")
                assert bool(torch.isneginf(lb[:, :dead]).all()), (layout, causal, b, "LSE of rows without a visible key must be -inf")
                if dead == 0:  # Lk >= Lq >= 1 (without the mask: Lk >= 1): the dense kernel's bits
                    assert_bits(o, lse, cu_q, b, dense_exv(fa, seqs[b][0][None], seqs[b][1][None], seqs[b][2][None], dtype, causal), (layout, causal))
                elif dead < Lq:
                    assert bool(torch.isfinite(ob[:, dead:].float()).all()) and bool(torch.isfinite(lb[:, dead:]).all())
                    _rows_against_oracle(oracle_mod, ob, lb, *seqs[b], dtype, dead)


# ---- write footprint ------------------------------------------------------------------------------------------------------------
CANARY16 = {"bf16": 0x7FC1, "f16": 0x7E01}  # NaNs with a payload (positive as int16)
CANARY32 = 0x7FC00001


def _footprint(fa, oracle, dtype, D, causal, cu_q, cu_k, max_q, max_k, total_q, total_k, owners, seed):
    """Run one call on canary-filled, gapped buffers. owners: [(first q token, rows written, first key, keys)] per sequence that must
    be written -- the correct answer under the documented clamps; everything else must keep its canary. Sequences with keys >= rows are
    compared bit for bit with fa_fwd_exv on the owner's slice."""
    import torch

    Hq, Hkv = 4, 2
    rng = np.random.default_rng(seed)
    qn, kn, vn = seq_data(oracle, rng, Hq, Hkv, total_q, total_k, D, dtype)  # [H, total, D]
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16

    def gapped(x, H):  # [total, H, D] view with a spare head per row (row gap) and a head pitch of 2 D (head gap), canaries in the gaps
        buf = torch.full((x.shape[1] + 3, H + 1, 2 * D), CANARY16[dtype], dtype=torch.int16, device="cuda").view(tdt)
        view = buf[:x.shape[1], :H, :D]
        view.copy_(to_dev(x.transpose(1, 0, 2), dtype))
        return buf, view

    _, q = gapped(qn, Hq)
    _, k = gapped(kn, Hkv)
    _, v = gapped(vn, Hkv)
    obuf = torch.full((total_q + 3, Hq + 1, 2 * D), CANARY16[dtype], dtype=torch.int16, device="cuda")
    o = obuf.view(tdt)[:total_q, :Hq, :D]
    lbuf = torch.full((Hq * total_q + 64,), CANARY32, dtype=torch.int32, device="cuda")
    lse = lbuf.view(torch.float32)[32:32 + Hq * total_q].view(Hq, total_q)
    assert o.stride() == q.stride()
    fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), max_q, max_k, is_causal=causal, out=o, lse=lse)
    torch.cuda.synchronize()
    written_o = torch.zeros_like(obuf, dtype=torch.bool)
    written_l = torch.zeros_like(lbuf, dtype=torch.bool)
    for (s, n, ks, nk) in owners:
        written_o[s:s + n, :Hq, :D] = True
        written_l[32:32 + Hq * total_q].view(Hq, total_q)[:, s:s + n] = True
    assert bool((obuf[~written_o] == CANARY16[dtype]).all()), "O was written outside the specified rows"
    assert bool((lbuf[~written_l] == CANARY32).all()), "LSE was written outside the specified rows"
    for (s, n, ks, nk) in owners:
        ob, lb = o[s:s + n].transpose(0, 1), lse[:, s:s + n]
        assert bool(torch.isfinite(ob.float()).all()) and bool(torch.isfinite(lb).all()), (s, n, "a specified row was not written")
        assert nk >= n
        d_o, d_l = dense_exv(fa, qn[None, :, s:s + n], kn[None, :, ks:ks + nk], vn[None, :, ks:ks + nk], dtype, causal)
        assert torch.equal(ob, d_o[0]) and torch.equal(lb, d_l[0]), (s, n, ks, nk)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, True), ("bf16", 128, False), ("f16", 64, False)])
def test_write_footprint_with_unowned_tokens_and_a_clamped_sequence(fa, oracle_mod, dtype, D, causal):
    # 37 tokens behind cu_q[B] belong to nobody; sequence 1 has 300 rows but max_seqlen_q = 200: its rows 200 .. 299 are not written,
    # and its first 200 rows are those of a sequence of 200 queries (the documented clamp)
    _footprint(fa, oracle_mod, dtype, D, causal, [0, 100, 400, 450], [0, 150, 500, 700], 200, 350, 487, 731,
               [(0, 100, 0, 150), (100, 200, 150, 350), (400, 50, 500, 200)], 11)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, False)])
def test_out_of_range_table_entries_are_clamped(fa, oracle_mod, dtype, D, causal):
    # entries below 0 and above total: clamped to [0, total] -- sequence 0 starts at token 0, sequence 2 ends with the last token / key
    _footprint(fa, oracle_mod, dtype, D, causal, [-7, 100, 400, 10000], [-1, 150, 500, 2 ** 31 - 1], 300, 350, 487, 731,
               [(0, 100, 0, 150), (100, 300, 150, 350), (400, 87, 500, 231)], 12)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 128, True), ("f16", 64, False)])
def test_a_decreasing_table_entry_gives_an_empty_sequence(fa, oracle_mod, dtype, D, causal):
    # (200, 100) and (400, 150) decrease: sequence 0 has no rows and writes nothing; the others are untouched by it
    _footprint(fa, oracle_mod, dtype, D, causal, [200, 100, 300, 487], [400, 150, 500, 731], 300, 350, 487, 731,
               [(100, 200, 150, 350), (300, 187, 500, 231)], 13)


# ---- a K / V buffer above 4 GiB ----------------------------------------------------------------------------------------------------
def test_kv_buffer_above_4_gib(fa, oracle_mod):
    import torch

    dtype, D, Hq, Hkv, L = "bf16", 128, 16, 8, 300
    total_k = (1 << 32) // (Hkv * D * 2) + 4096  # [total_k, Hkv, D] bf16: 8 MiB past 4 GiB
    assert total_k * Hkv * D * 2 > (1 << 32)
    rng = np.random.default_rng(3)
    first, last = seq_data(oracle_mod, rng, Hq, Hkv, L, L, D, dtype), seq_data(oracle_mod, rng, Hq, Hkv, 257, L, D, dtype)
    k = torch.empty(total_k, Hkv, D, dtype=torch.bfloat16, device="cuda")
    v = torch.empty(total_k, Hkv, D, dtype=torch.bfloat16, device="cuda")
    for buf, a, z in ((k, first[1], last[1]), (v, first[2], last[2])):  # only what is read: sequence 0 is clamped to its first L keys
        buf[:L].copy_(to_dev(a.transpose(1, 0, 2), dtype))
        buf[total_k - L:].copy_(to_dev(z.transpose(1, 0, 2), dtype))
    q = to_dev(np.concatenate([first[0], last[0]], axis=1).transpose(1, 0, 2), dtype)
    cu_q, cu_k = np.array([0, L, L + 257], np.int32), np.array([0, total_k - L, total_k], np.int32)
    for causal in (True, False):
        o, lse = varlen(fa, q, k, v, cu_q, cu_k, L, L, causal)
        assert_bits(o, lse, cu_q, 1, dense_exv(fa, last[0][None], last[1][None], last[2][None], dtype, causal), ("the sequence at the end", causal))
        assert_bits(o, lse, cu_q, 0, dense_exv(fa, first[0][None], first[1][None], first[2][None], dtype, causal), ("the clamped sequence", causal))
    ob, lb = piece(o, lse, cu_q, 1)
    o64, l64 = oracle_mod.attn_fwd_ex_f64(effective_q(oracle_mod, last[0], dtype)[None], last[1][None], last[2][None], False, LN2)
    assert np.abs(ob.float().cpu().numpy() - o64[0]).max() < TOL_O[dtype] and np.abs(lb.cpu().numpy() - l64[0]).max() < lse_tol(dtype, 1, last[0], last[1])
    del k, v
    torch.cuda.empty_cache()


# ---- one captured graph, replayed after both tables changed in place -----------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_graph_replay_after_the_tables_change(fa, oracle_mod, dtype, D):
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k = 8, 2, 700, 900, 400, 500
    rng = np.random.default_rng(21 + D)
    qn, kn, vn = seq_data(oracle_mod, rng, Hq, Hkv, total_q, total_k, D, dtype)
    q, k, v = (to_dev(x.transpose(1, 0, 2), dtype) for x in (qn, kn, vn))
    splits = [([0, 100, 450, 700], [0, 300, 650, 900]), ([0, 390, 400, 700], [0, 400, 900, 900])]  # (the second: one sequence without keys)
    cu_q, cu_k = cu_dev(splits[0][0]), cu_dev(splits[0][1])
    o = torch.empty_like(q)
    lse = torch.empty(Hq, total_q, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fa.flash_attention_varlen(q, k, v, cu_q, cu_k, max_q, max_k, is_causal=True, out=o, lse=lse)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.flash_attention_varlen(q, k, v, cu_q, cu_k, max_q, max_k, is_causal=True, out=o, lse=lse)
    for sq, sk in (splits[1], splits[0], splits[1]):
        cu_q.copy_(cu_dev(sq))
        cu_k.copy_(cu_dev(sk))
        o.fill_(float("nan"))
        lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for b in range(3):
            s, e, ks, ke = sq[b], sq[b + 1], sk[b], sk[b + 1]
            ob, lb = o[s:e].transpose(0, 1), lse[:, s:e]
            if ke == ks:
                assert bool((ob == 0).all()) and bool(torch.isneginf(lb).all())
                continue
            assert ke - ks >= e - s
            qs, kb, vb = (np.ascontiguousarray(x) for x in (qn[:, s:e], kn[:, ks:ke], vn[:, ks:ke]))
            o64, l64 = oracle_mod.attn_fwd_ex_f64(effective_q(oracle_mod, qs, dtype)[None], kb[None], vb[None], True, LN2)
            assert np.abs(ob.float().cpu().numpy() - o64[0]).max() < TOL_O[dtype], (sq, b)
            assert np.abs(lb.cpu().numpy() - l64[0]).max() < lse_tol(dtype, 1, qs, kb), (sq, b)
