"""GPU: fa_fwd_varlen_paged_split (flash_attention_varlen_paged(num_splits=...)), the key split of the paged prefill. The rule, the model
and the bars live in tests/ksplit.py (held by tests/test_ksplit_cases.py on the CPU). The inputs: window.SEQS as one packed batch with
three trailing tokens nobody owns -- (1,1) (70,70) (129,1) (64,0) (200,130) (130,257) (257,513) (100,1000), the last with 16 tiles --
under sink.WINDOWS and S in {2, 3, 5, 16} (mostly empty splits included), pools of P = 16 HND with shuffled pages and P = 256 NHD, NaN in
every slot nobody may read and a table entry outside the pool behind every sequence's last page.
  1. parity: every element of O and LSE against the fp64 reference at the un-split route's bars plus the merge terms (ksplit.bars), with
     and without sinks; and, as the other half of the parity cases, the same sequences, windows and S on the ramped exact-arithmetic inputs
     of ksplit.ramp_case (16 log2 units per key: the splits' LSEs of every row lie 8 or more apart) at exact_forward.bars(split=S);
  2. bit-identity: O of every row of a block with one tile (n = 1) is the un-split window call's under S = 2 and 16 (every live block of a
     cache inside tile 0 is one, and so are the blocks of narrow windows that do not cross a tile's edge); num_splits = 1 is the sink /
     window call; num_splits = 0 the explicit call with the heuristic's answer; two runs agree;
  3. known answers: K = 0 gives O = mean of the visible V rows and LSE = ln(count); with sinks = k ln 2, ln(n + 2^k) and sum v / (n + 2^k);
  4. sinks: -1e4 leaves the sink-free split call's bits, +-100 stay finite, dead rows get O = 0 and LSE = sinks[h] (NULL: -inf) bit for bit;
  5. footprint: a NaN-filled workspace changes nothing, a canary behind workspace_bytes and the sentinels on unowned tokens stay, lse = None,
     q as a view of a packed QKV projection;
  6. the pair of launches replayed in a captured graph after tables, lengths and sinks changed in place;
  7. the wrapper's errors.

Worst error / bar measured on an MI355X (printed by the parity tests): see README.md, round 22."""
import numpy as np
import pytest

import chain_bound as cb
import exact_forward as ef
import ksplit as ks
import sink as sk
import varlen_paged as vp
import window as wn
from test_gpu_decode_paged import to_layout
from test_gpu_window import bits, data, i32, paged, piece, refs, same_bits
from util import TOL_O, lse_tol, o_tol, to_dev

pytestmark = pytest.mark.gpu
INT_MAX = wn.INT_MAX
MATRIX = [(t, D, heads) for t in ("f16", "bf16") for D, heads in ((64, (4, 4)), (128, (8, 2)))]
POOLS = ((16, "HND"), (256, "NHD"))
SO, SL = -3.0e4, 12345.0


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


_POOLS = {}


def nan_pool(d, P, layout, ks_=None, vs_=None, tag=""):
    """The batch's caches in a pool whose unused slots and spare pages hold NaN; table entries behind a sequence's last page lie outside
    the pool (one more page per row than the longest sequence needs, so every row has such an entry)."""
    key = (id(d), P, layout, tag)
    if key not in _POOLS:
        kk = [s[1] for s in d["seqs"]] if ks_ is None else ks_
        vv = [s[2] for s in d["seqs"]] if vs_ is None else vs_
        longest = max(vp.pages_of(lk, P) for _, lk in d["lens"])
        pool = vp.build_pool(kk, vv, P, rng=np.random.default_rng(P + 22), spare=2, fill=np.nan, unused="beyond", max_pages=longest + 1)
        _POOLS[key] = (to_layout(pool["k"], d["dtype"], layout), to_layout(pool["v"], d["dtype"], layout), pool["table"])
    return _POOLS[key]


def split(fa, d, P, layout, window, S, sinks=None, **kw):
    return paged(fa, d, P, layout, window, pool=kw.pop("pool", None) or nan_pool(d, P, layout), num_splits=S,
                 sinks=None if sinks is None else dev(sinks), **kw)


def unsplit_window(fa, d, P, layout, window, **kw):
    """The un-split call through the window kernels: fa_fwd_varlen_paged_window routes by sign, so an unbounded side becomes INT_MAX."""
    wl, wr = window
    return paged(fa, d, P, layout, (INT_MAX if wl < 0 else wl, INT_MAX if wr < 0 else wr), pool=nan_pool(d, P, layout), **kw)


_ABS = {}


def absums(d, wl, wr):
    key = (id(d), wl, wr)
    if key not in _ABS:
        _ABS[key] = [ks.absum_reference(*s, wl, wr) for s in d["seqs"]]
    return _ABS[key]


def check_parity(d, r, wl, wr, S, sinks, what):
    dtype, worst = d["dtype"], [0.0, 0.0]
    for b, (Lq, Lk) in enumerate(d["lens"]):
        q, k, v = d["seqs"][b]
        on, ln = (x.float().cpu().numpy() for x in piece(r, d["cu_q"], b))
        o64, l64 = refs(d, wl, wr)[b]
        dead = wn.dead_rows(Lq, Lk, wl, wr)
        want = np.full((on.shape[0], int(dead.sum())), -np.inf, np.float32) if sinks is None else np.repeat(sinks[:, None], dead.sum(), 1)
        assert not on[:, dead].any() and np.array_equal(ln[:, dead].view(np.int32), want.view(np.int32)), (what, b, "dead rows")
        live = ~dead
        assert np.isfinite(on).all() and np.isfinite(ln[:, live]).all(), (what, b)
        if Lk == 0 or not live.any():
            continue
        bar_o, bar_l, o_ref, l_ref = ks.bars(S, lse_tol(dtype, 1, q, k), o_tol(dtype, 1, q, k, v, None, TOL_O[dtype]), o64, l64, absums(d, wl, wr)[b], sinks)
        ro = float((np.abs(on - o_ref) / bar_o)[:, live].max())
        rl = float((np.abs(ln[:, live] - l_ref[:, live]) / bar_l[:, live]).max())
        assert ro <= 1.0 and rl <= 1.0, (what, b, (Lq, Lk), "error / bar", ro, rl)
        worst = [max(worst[0], ro), max(worst[1], rl)]
    return worst


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,heads", MATRIX)
def test_parity_with_the_fp64_reference(fa, oracle_mod, dtype, D, heads):
    d = data(oracle_mod, dtype, D, heads)
    worst = [0.0, 0.0]
    for n, (wl, wr) in enumerate(sk.WINDOWS):
        for m, S in enumerate(ks.SPLITS):
            P, layout = POOLS[(n + m) % 2]
            # (with sinks: every window under one S, every S under some window)
            for sinks in (None, sk.sinks_for(heads[0])) if m == n % len(ks.SPLITS) else (None,):
                r = split(fa, d, P, layout, (wl, wr), S, sinks)
                w = check_parity(d, r, wl, wr, S, sinks, (dtype, D, heads, (wl, wr), S, P, layout, sinks is not None))
                worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    print(f"KSPLIT parity {dtype} D={D} heads={heads}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    assert worst[0] > 0.01  # the bars are not vacuous


_RAMP_REFS = {}


def ramp_reference(seq, window, D, heads, h):
    """The fp64 reference of one head of a ramped case, once per process (f16 and bf16 cases hold the same values)."""
    key = (tuple(seq), tuple(window), D, tuple(heads), h)
    if key not in _RAMP_REFS:
        _RAMP_REFS[key] = ef.reference_head(ks.ramp_case(seq, D, heads, "bf16", window), 0, h)
    return _RAMP_REFS[key]


@pytest.mark.parametrize("dtype,D,heads", MATRIX)
def test_parity_on_the_ramped_inputs(fa, dtype, D, heads):
    """The other half of the parity cases: the same sequences, windows and S on ksplit.ramp_case, whose scores fall by 16 log2 units per
    key, so that the splits' LSEs of every row lie at least 8 apart (tests/test_ksplit_cases.py asserts it from the fp64 reference for
    these configurations) and a merge whose weights are wrong cannot pass. Exact-arithmetic inputs: exact_forward.bars(split=S)."""
    import torch

    cases = [ks.ramp_case(seq, D, heads, dtype) for seq in wn.SEQS]
    for c in cases:
        assert ef.representable(c.q, dtype) and ef.representable(c.k, dtype) and ef.representable(c.v, dtype)
    qn, cu_q = vp.pack_rows([c.q[0] for c in cases], tail=3)
    q = to_dev(qn, dtype)
    pools = {}
    for P, layout in POOLS:
        pool = vp.build_pool([c.k[0] for c in cases], [c.v[0] for c in cases], P, rng=np.random.default_rng(P + D), spare=2, fill=np.nan, unused="beyond",
                             max_pages=max(vp.pages_of(lk, P) for _, lk in wn.SEQS) + 1)
        pools[P] = (to_layout(pool["k"], dtype, layout), to_layout(pool["v"], dtype, layout), i32(pool["table"]))
    worst = [0.0, 0.0]
    for n, window in enumerate(sk.WINDOWS):
        for m, S in enumerate(ks.SPLITS):
            P, layout = POOLS[(n + m) % 2]
            o, lse = fa.flash_attention_varlen_paged(q, pools[P][0], pools[P][1], i32(cu_q), pools[P][2], i32([lk for _, lk in wn.SEQS]),
                                                     max(lq for lq, _ in wn.SEQS), layout=layout, window=window, scale=cases[0].scale, num_splits=S)
            torch.cuda.synchronize()
            on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
            for b, seq in enumerate(wn.SEQS):
                case = ks.ramp_case(seq, D, heads, dtype, window)
                s0, e0 = int(cu_q[b]), int(cu_q[b + 1])
                for h in range(heads[0]):
                    r = ef.ratios(case, ramp_reference(seq, window, D, heads, h), on[s0:e0, h], ln[h, s0:e0], S, 0.0)
                    assert r["o"] <= 1.0 and r["lse"] <= 1.0, (dtype, D, heads, window, seq, S, P, layout, h, r)
                    worst = [max(worst[0], r["o"]), max(worst[1], r["lse"])]
    print(f"KSPLIT ramped {dtype} D={D} heads={heads}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")


# ---- 2. bit-identity -------------------------------------------------------------------------------------------------------------------
def one_tile_rows(Lq, Lk, wl, wr):
    """bool [Lq]: rows of blocks whose tile range holds exactly one tile."""
    out = np.zeros(Lq, bool)
    for qb in range((Lq + ks.BLOCK - 1) // ks.BLOCK):
        bt = ks.block_tiles(Lq, Lk, wl, wr, qb)
        if bt is not None and bt[1] - bt[0] == 1:
            out[qb * ks.BLOCK:qb * ks.BLOCK + ks.BLOCK] = True
    return out


@pytest.mark.parametrize("dtype,D,heads", MATRIX)
def test_rows_of_one_tile_blocks_are_the_unsplit_calls_bits(fa, oracle_mod, dtype, D, heads):
    import torch

    d = data(oracle_mod, dtype, D, heads)
    seen = 0
    for n, (wl, wr) in enumerate(sk.WINDOWS):
        P, layout = POOLS[n % 2]
        base = unsplit_window(fa, d, P, layout, (wl, wr))
        for S in (2, 16):
            r = split(fa, d, P, layout, (wl, wr), S)
            for b, (Lq, Lk) in enumerate(d["lens"]):
                rows = torch.from_numpy(one_tile_rows(Lq, Lk, wl, wr)).cuda()
                if 1 <= Lk <= ks.TILE:  # a cache inside tile 0: every live block has one tile, under every window
                    assert bool(rows[~torch.from_numpy(wn.dead_rows(Lq, Lk, wl, wr)).cuda()].all()), ((wl, wr), (Lq, Lk))
                (oa, la), (ob, lb) = piece(r, d["cu_q"], b), piece(base, d["cu_q"], b)
                assert torch.equal(bits(oa[:, rows].contiguous()), bits(ob[:, rows].contiguous())), ((wl, wr), S, b, "O of one-tile blocks")
                # LSE: (m + log2 l) ln 2 against m ln 2 + ln l, equal within the merge term's roundings
                dl = (la[:, rows] - lb[:, rows]).abs()
                live = torch.isfinite(lb[:, rows])
                assert torch.equal(torch.isfinite(la[:, rows]), live)
                if bool(live.any()):
                    assert float(dl[live].max()) <= float(ks.merge_lse_term(S, lb[:, rows][live].cpu().numpy().astype(np.float64)).max()), ((wl, wr), S, b)
                seen += int(rows.sum())
    assert seen > 500


@pytest.mark.parametrize("dtype,D,heads", [MATRIX[1], MATRIX[2]])
def test_one_split_the_heuristic_and_two_runs(fa, oracle_mod, dtype, D, heads):
    d = data(oracle_mod, dtype, D, heads)
    sinks = sk.sinks_for(heads[0])
    B, max_q = len(d["lens"]), max(lq for lq, _ in d["lens"])
    for n, (wl, wr) in enumerate(sk.WINDOWS):
        P, layout = POOLS[n % 2]
        pool = nan_pool(d, P, layout)
        # num_splits = 1: the window call (routed through the window kernels), with sinks the sink call
        assert same_bits(split(fa, d, P, layout, (wl, wr), 1), unsplit_window(fa, d, P, layout, (wl, wr))), (wl, wr)
        assert same_bits(split(fa, d, P, layout, (wl, wr), 1, sinks), paged(fa, d, P, layout, (wl, wr), pool=pool, sinks=dev(sinks))), (wl, wr)
        S0 = fa.varlen_paged_num_splits(B, heads[0], max_q, D, P, pool[2].shape[1])
        assert S0 == ks.num_splits(B, heads[0], max_q, D, P, pool[2].shape[1]) and S0 >= 1
        for s in (None, sinks):
            assert same_bits(split(fa, d, P, layout, (wl, wr), 0, s), split(fa, d, P, layout, (wl, wr), S0, s)), ((wl, wr), S0)
            assert same_bits(split(fa, d, P, layout, (wl, wr), 5, s), split(fa, d, P, layout, (wl, wr), 5, s)), (wl, wr)


# ---- 3. known answers ------------------------------------------------------------------------------------------------------------------
KNOWN_SEQS = ((130, 257), (200, 130), (100, 1000))
KNOWN_WINDOWS = ((-1, 0), (-1, -1), (15, 0), (64, 64), (127, 5), (200, 0))


@pytest.mark.parametrize("dtype,D", [("f16", 64), ("bf16", 128)])
def test_known_answers_with_zero_keys(fa, oracle_mod, dtype, D):
    Hq, Hkv = 8, 2
    d = data(oracle_mod, dtype, D, (Hq, Hkv), lens=KNOWN_SEQS, seed=22)
    pool = nan_pool(d, 16, "NHD", ks_=[np.zeros_like(s[1]) for s in d["seqs"]], tag="k0")
    kk = np.arange(Hq) - 2  # 2^k = 1/4 .. 32
    with_sinks = (kk * np.float32(np.log(2.0))).astype(np.float32)
    for wl, wr in KNOWN_WINDOWS:
        for S in (3, 16):
            for sinks in (None, with_sinks):
                r = split(fa, d, 16, "NHD", (wl, wr), S, sinks, pool=pool)
                for b, (Lq, Lk) in enumerate(KNOWN_SEQS):
                    on, ln = (x.float().cpu().numpy() for x in piece(r, d["cu_q"], b))
                    vis = wn.visible(Lq, Lk, wl, wr)
                    n = vis.sum(1).astype(np.float64)
                    dead = n == 0
                    v = np.repeat(d["seqs"][b][2].astype(np.float64), Hq // Hkv, axis=0)
                    extra = np.zeros((Hq, 1)) if sinks is None else 2.0 ** kk[:, None]
                    den = n[None, :] + extra
                    with np.errstate(divide="ignore", invalid="ignore"):
                        o2 = np.where(dead[None, :, None], 0.0, np.einsum("ij,hjd->hid", vis.astype(np.float64), v) / den[..., None])
                        A = np.where(dead[None, :, None], 0.0, np.einsum("ij,hjd->hid", vis.astype(np.float64), np.abs(v)) / den[..., None])
                        l64, l2 = np.broadcast_to(np.log(n)[None], den.shape), np.log(den)
                    assert not on[:, dead].any(), ((wl, wr), S, b)
                    want_dead = np.full((Hq, int(dead.sum())), -np.inf, np.float32) if sinks is None else np.repeat(sinks[:, None], dead.sum(), 1)
                    assert np.array_equal(ln[:, dead].view(np.int32), want_dead.view(np.int32)), ((wl, wr), S, b, "dead rows")
                    live = ~dead
                    if not live.any():
                        continue
                    # every score is 0: m = 0, l = the split's count, every probability 1 in the type. What is left: the fp32 sums over the n
                    # values, the merge, the fold, and the rounding of O to the type
                    bar_l = ks.merge_lse_term(S, l2) + (0.0 if sinks is None else sk.fold_term(l64, l2, sinks))
                    out_round = np.maximum(cb.U_OUT[dtype] * np.abs(o2), 2.0 ** -25 if dtype == "f16" else 0.0)
                    bar_o = out_round + 2.0 ** -24 * (n[None, :, None] + 8 + 2 * (S + 3)) * A + np.abs(o2) * bar_l[..., None]
                    ro = float((np.abs(on - o2)[:, live] / bar_o[:, live]).max())
                    rl = float((np.abs(ln[:, live] - l2[:, live]) / bar_l[:, live]).max())
                    assert ro <= 1.0 and rl <= 1.0, ((wl, wr), S, (Lq, Lk), sinks is not None, "error / bar", ro, rl)


# ---- 4. sinks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,heads", [MATRIX[0], MATRIX[3]])
def test_sinks_far_below_change_no_bit_and_far_out_stay_finite(fa, oracle_mod, dtype, D, heads):
    import torch

    d = data(oracle_mod, dtype, D, heads)
    n = int(d["cu_q"][-1])
    for k, (wl, wr) in enumerate(sk.WINDOWS):
        P, layout = POOLS[k % 2]
        for S in (2, 16):
            plain = split(fa, d, P, layout, (wl, wr), S)
            low = split(fa, d, P, layout, (wl, wr), S, np.full(heads[0], -1e4, np.float32))
            assert torch.equal(bits(low[0]), bits(plain[0])), ((wl, wr), S, "O under sinks of -1e4")
            live = torch.isfinite(plain[1])
            assert torch.equal(bits(low[1][live]), bits(plain[1][live])) and bool((low[1][~live] == -1e4).all()), ((wl, wr), S)
        for value in (100.0, -100.0):
            r = split(fa, d, P, layout, (wl, wr), 5, np.full(heads[0], value, np.float32))
            assert bool(torch.isfinite(r[0][:n].float()).all()) and bool(torch.isfinite(r[1][:, :n]).all()), ((wl, wr), value)


# ---- 5. footprint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,heads,P,layout", [("bf16", 64, (4, 4), 16, "HND"), ("f16", 128, (8, 2), 256, "NHD")])
def test_footprint(fa, oracle_mod, dtype, D, heads, P, layout):
    import torch

    d = data(oracle_mod, dtype, D, heads)
    Hq, Hkv = heads
    total, n = d["q"].shape[0], int(d["cu_q"][-1])
    B, max_q = len(d["lens"]), max(lq for lq, _ in d["lens"])
    pool = nan_pool(d, P, layout)
    sinks = sk.sinks_for(Hq)
    for S, (wl, wr), s in ((3, (127, 5), None), (16, (-1, 0), sinks), (2, (15, 0), None)):
        need = fa.varlen_paged_split_workspace_bytes(B, Hq, total, max_q, D, P, pool[2].shape[1], S)
        assert need == ks.workspace_bytes(S, Hq, total, D)
        plain = split(fa, d, P, layout, (wl, wr), S, s)
        raw = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda")  # 0xFFFFFFFF: a NaN in every float, and the canary
        out = torch.full_like(d["q"], SO)
        lse = torch.full((Hq, total), SL, dtype=torch.float32, device="cuda")
        r = split(fa, d, P, layout, (wl, wr), S, s, workspace=raw[:need], out=out, lse=lse)
        assert bool((raw[need:] == 0xFF).all()), (S, "bytes behind workspace_bytes were written")
        assert same_bits((r[0][:n], r[1][:, :n]), plain), (S, (wl, wr), "a NaN-filled workspace changed the result")
        assert bool((out[n:] == SO).all()) and bool((lse[:, n:] == SL).all()), "tokens nobody owns were written"
        assert not bool(torch.isnan(out[:n].float()).any()) and not bool(torch.isnan(lse[:, :n]).any())
        nol = split(fa, d, P, layout, (wl, wr), S, s, return_lse=False)
        assert nol[1] is None and torch.equal(bits(nol[0]), bits(plain[0])), (S, "lse = None")
        # q as a view of a packed QKV projection
        proj = torch.full((total, (Hq + 2 * Hkv) * D), float("nan"), dtype=d["q"].dtype, device="cuda")
        proj[:, :Hq * D] = d["q"].reshape(total, Hq * D)
        qv = proj[:, :Hq * D].unflatten(1, (Hq, D))
        o, l = fa.flash_attention_varlen_paged(qv, pool[0], pool[1], i32(d["cu_q"]), i32(pool[2]), i32([lk for _, lk in d["lens"]]), max_q, layout=layout,
                                               window=(wl, wr), sinks=None if s is None else dev(s), num_splits=S)
        torch.cuda.synchronize()
        assert o.stride() == qv.stride() and same_bits((o[:n].contiguous(), l[:, :n]), plain), (S, "q as a view")
        assert bool(torch.isnan(proj[:, Hq * D:].float()).all())


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------
def test_the_pair_of_launches_replays_in_a_graph(fa, oracle_mod):
    import torch

    B, Hq, Hkv, D, P, mp, total, max_q, S = 3, 8, 2, 64, 16, 40, 333, 200, 5
    num_pages = B * mp + 5
    rng = np.random.default_rng(226)
    win = (127, 0)
    steps = [([0, 100, 250, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [100, 400, 81]),
             ([0, 200, 200, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [480, 77, 130]),
             ([0, 1, 2, 3], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [300, 1, 640])]
    steps[1][1][1, 6] = num_pages + 9  # an entry outside the pool, behind the sequence's last page
    q = to_dev(vp.draw(oracle_mod.round_to, rng, "bf16", total, Hq, D), "bf16")
    kp, vpool = (to_dev(vp.draw(oracle_mod.round_to, rng, "bf16", num_pages, Hkv, P, D), "bf16") for _ in range(2))
    sinks_of = [dev(sk.sinks_for(Hq) + np.float32(j)) for j in range(len(steps))]
    cu, bt, sl, sinks = i32(steps[0][0]), i32(steps[0][1]), i32(steps[0][2]), sinks_of[0].clone()
    ws = torch.empty(fa.varlen_paged_split_workspace_bytes(B, Hq, total, max_q, D, P, mp, S), dtype=torch.uint8, device="cuda")

    def bufs():
        return torch.full_like(q, float("nan")), torch.full((Hq, total), float("nan"), device="cuda")

    def step(o_, lse_, ws_):
        fa.flash_attention_varlen_paged(q, kp, vpool, cu, bt, sl, max_q, window=win, sinks=sinks, out=o_, lse=lse_, num_splits=S, workspace=ws_)

    g = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*g, ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*g, ws)
    for j in (1, 0, 2, 1):
        c, t, l = steps[j]
        cu.copy_(i32(c))
        bt.copy_(i32(t))
        sl.copy_(i32(l))
        sinks.copy_(sinks_of[j])
        for dst, src in zip(g, bufs()):
            bits(dst).copy_(bits(src))
        graph.replay()
        torch.cuda.synchronize()
        e = bufs()
        step(*e, torch.empty_like(ws))
        torch.cuda.synchronize()
        n = c[-1]
        assert torch.equal(bits(g[0][:n]), bits(e[0][:n])) and torch.equal(bits(g[1][:, :n]), bits(e[1][:, :n])), j
        assert bool(torch.isnan(g[0][n:].float()).all()) and not bool(torch.isnan(g[0][:n].float()).any())
        # and the replay is the un-split sink call within one rounding of the type
        o1, _ = fa.flash_attention_varlen_paged(q, kp, vpool, cu, bt, sl, max_q, window=win, sinks=sinks)
        torch.cuda.synchronize()
        assert float((g[0][:n].float() - o1[:n].float()).abs().max()) < 2 * TOL_O["bf16"]


# ---- 7. the wrapper's errors -----------------------------------------------------------------------------------------------------------
def test_error_surface(fa, oracle_mod):
    import torch

    d = data(oracle_mod, "bf16", 64, (4, 4))
    with pytest.raises(ValueError, match="num_splits"):
        split(fa, d, 16, "HND", (-1, 0), -1)
    with pytest.raises(ValueError, match="num_splits"):
        split(fa, d, 16, "HND", (-1, 0), 2.0)
    with pytest.raises(ValueError, match="softcap"):
        split(fa, d, 16, "HND", (-1, 0), 2, softcap=30.0)
    with pytest.raises(fa.FaError, match="num_splits"):
        split(fa, d, 16, "HND", (-1, 0), ks.MAX_SPLITS + 1)
    with pytest.raises(ValueError, match="workspace"):
        split(fa, d, 16, "HND", (-1, 0), 2, workspace=torch.empty(1 << 20, dtype=torch.float32, device="cuda"))
    with pytest.raises(fa.FaError, match="workspace"):
        split(fa, d, 16, "HND", (-1, 0), 2, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="right side 0"):
        split(fa, d, 16, "HND", (63, 5), 2, causal=True)
    pool = nan_pool(d, 16, "HND")
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        paged(fa, d, 16, "HND", (-1, 0), pool=(pool[0].to(torch.float8_e4m3fn), pool[1].to(torch.float8_e4m3fn), pool[2]), num_splits=2)
