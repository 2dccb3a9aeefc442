"""GPU: the sliding-window entry points fa_fwd_varlen_window, fa_fwd_varlen_paged_window and fa_fwd_decode_paged_window (window=(left, right)
of flash_attention_varlen / _varlen_paged / _decode_paged). The cases live in tests/window.py (checked on the CPU by
tests/test_window_cases.py):
  1. parity with the fp64 reference of the visibility rule at util.o_tol / util.lse_tol; dead rows exactly 0 / -inf; the write footprint;
  2. the known answer of (0, 0): O = V[i + coff], LSE = scale q.k;
  3. (INT_MAX, 0) / (INT_MAX, INT_MAX) through the windowed kernels, bit for bit the causal / full un-windowed call;
  4. the shift identity: dropping the keys in front of the first tile changes no bit;
  5. keys no query sees hold +-6e4: no bit changes;
  6. routing by sign, window=None, return_lse=False;
  7. append + windowed prefill + windowed decode in one captured graph, replayed after the tables changed in place."""
import numpy as np
import pytest

import varlen_paged as vp
import window as wn
from test_gpu_decode_paged import to_layout
from util import TOL_O, lse_tol, o_tol, to_dev

pytestmark = pytest.mark.gpu
INT_MAX = wn.INT_MAX
MAX_Q = max(lq for lq, _ in wn.SEQS)
MAX_K = max(lk for _, lk in wn.SEQS)
CAP = 4096
DECODE_PAIRS = (("f16", "f16"), ("bf16", "bf16"), ("fp8", "fp8"), ("bf16", "fp8"))
DECODE_WINDOWS = ((0, 0), (31, 0), (64, 5), (200, -1), (INT_MAX, 0), (INT_MAX, INT_MAX))


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def i32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def bits(t):
    import torch

    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    import torch

    return torch.equal(bits(a[0]), bits(b[0])) and (a[1] is None or torch.equal(bits(a[1]), bits(b[1])))


def paged_config(n):
    return ((16, "HND"), (256, "NHD"), (16, "NHD"), (256, "HND"))[n % 4]


_DATA, _REF = {}, {}


def data(oracle, dtype, D, heads, lens=wn.SEQS, seed=0):
    """One batch: numpy sequences, the packed q / k / v on the device, cu_q / cu_k. Drawn once per key."""
    key = (dtype, D, heads, lens, seed)
    if key not in _DATA:
        rng = np.random.default_rng(14000 + 1000 * seed + D + 10 * heads[0] + heads[1] + (1 if dtype == "f16" else 0))
        seqs = wn.draw_seqs(oracle.round_to, rng, heads[0], heads[1], D, dtype, lens)
        qn, cu_q = vp.pack_rows([s[0] for s in seqs], tail=3)
        kn, cu_k = vp.pack_rows([s[1] for s in seqs], tail=1)
        vn, _ = vp.pack_rows([s[2] for s in seqs], tail=1)
        _DATA[key] = dict(seqs=seqs, q=to_dev(qn, dtype), k=to_dev(kn, dtype), v=to_dev(vn, dtype), cu_q=cu_q, cu_k=cu_k, kn=kn, vn=vn, lens=lens,
                          dtype=dtype)
    return _DATA[key]


def owned(d, r, kw):
    """The rows some sequence owns: the packed batch ends with tokens nobody owns, which no call writes (whatever the buffer held stays
    there, so they are no part of a bit comparison). A call into the caller's own buffers is returned whole."""
    if "out" in kw:
        return r
    n = int(d["cu_q"][-1])
    return r[0][:n], (None if r[1] is None else r[1][:, :n])


def varlen(fa, d, window=None, causal=False, k=None, v=None, cu_k=None, max_k=None, **kw):
    import torch

    lens = d["lens"]
    r = fa.flash_attention_varlen(d["q"], d["k"] if k is None else k, d["v"] if v is None else v, i32(d["cu_q"]),
                                  i32(d["cu_k"] if cu_k is None else cu_k), max(lq for lq, _ in lens), max_k or max(max(lk for _, lk in lens), 1),
                                  is_causal=causal, window=window, **kw)
    torch.cuda.synchronize()
    return owned(d, r, kw)


def pool_of(d, P, layout, ks=None, vs=None, seed=0):
    ks = [s[1] for s in d["seqs"]] if ks is None else ks
    vs = [s[2] for s in d["seqs"]] if vs is None else vs
    pool = vp.build_pool(ks, vs, P, rng=np.random.default_rng(P + seed), spare=2, fill=0.0)  # pages in random order
    return to_layout(pool["k"], d["dtype"], layout), to_layout(pool["v"], d["dtype"], layout), pool["table"]


def paged(fa, d, P, layout, window=None, causal=False, pool=None, lens_k=None, **kw):
    import torch

    kp, vpool, table = pool or pool_of(d, P, layout)
    r = fa.flash_attention_varlen_paged(d["q"], kp, vpool, i32(d["cu_q"]), i32(table), i32([lk for _, lk in d["lens"]] if lens_k is None else lens_k),
                                        max(lq for lq, _ in d["lens"]), is_causal=causal, layout=layout, window=window, **kw)
    torch.cuda.synchronize()
    return owned(d, r, kw)


def piece(r, cu_q, b):
    s, e = int(cu_q[b]), int(cu_q[b + 1])
    return r[0][s:e].transpose(0, 1), r[1][:, s:e]


def refs(d, wl, wr):
    key = (id(d), wl, wr)
    if key not in _REF:
        _REF[key] = [wn.reference(*s, wl, wr) for s in d["seqs"]]
    return _REF[key]


def check_parity(d, r, wl, wr, what):
    dtype = d["dtype"]
    for b, (Lq, Lk) in enumerate(d["lens"]):
        q, k, v = d["seqs"][b]
        ob, lb = piece(r, d["cu_q"], b)
        on, ln = ob.float().cpu().numpy(), lb.cpu().numpy()
        o64, l64 = refs(d, wl, wr)[b]
        dead = wn.dead_rows(Lq, Lk, wl, wr)
        assert np.array_equal(on[:, dead], np.zeros_like(on[:, dead])) and np.isneginf(ln[:, dead]).all(), (what, b, "dead rows")
        if dead.all():
            continue
        live = ~dead
        assert np.isfinite(on).all() and np.isfinite(ln[:, live]).all(), (what, b)
        err_o, err_l = np.abs(on - o64).max(), np.abs(ln[:, live] - l64[:, live]).max()
        bar_o, bar_l = o_tol(dtype, 1, q, k, v, None, TOL_O[dtype]), lse_tol(dtype, 1, q, k)
        print(f"WINDOW parity {what} seq {b} {(Lq, Lk)}: O {err_o:.2e} (bar {bar_o:.2e}) LSE {err_l:.2e} (bar {bar_l:.2e})")
        assert err_o < bar_o and err_l < bar_l, (what, b, err_o, bar_o, err_l, bar_l)


MATRIX = [(t, d) for t in ("f16", "bf16") for d in (64, 128)]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_parity_with_the_fp64_reference(fa, oracle_mod, dtype, D):
    for heads in wn.HEADS:
        d = data(oracle_mod, dtype, D, heads)
        for n, (name, _, wl, wr) in enumerate(wn.CASES):
            check_parity(d, varlen(fa, d, (wl, wr)), wl, wr, ("varlen", dtype, D, heads, name))
            P, layout = paged_config(n)
            check_parity(d, paged(fa, d, P, layout, (wl, wr)), wl, wr, ("paged", P, layout, dtype, D, heads, name))


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_write_footprint_is_the_unwindowed_calls(fa, oracle_mod, dtype, D):
    import torch

    d = data(oracle_mod, dtype, D, (8, 2))
    SO, SL = -3.0e4, 12345.0  # no output is near them: |O| <= 1, |LSE| < 100 or -inf

    def sentinels():
        return dict(out=torch.full_like(d["q"], SO), lse=torch.full((8, d["q"].shape[0]), SL, dtype=torch.float32, device="cuda"))

    for call in (lambda **kw: varlen(fa, d, **kw), lambda **kw: paged(fa, d, 16, "HND", **kw)):
        base = call(causal=True, **sentinels())
        for wl, wr in ((0, 0), (64, 5), (200, -1)):
            r = call(window=(wl, wr), **sentinels())
            assert torch.equal(r[0] == SO, base[0] == SO) and torch.equal(r[1] == SL, base[1] == SL), (wl, wr)
        assert bool((base[0][-3:] == SO).all()) and bool((base[1][:, -3:] == SL).all())  # the tokens nobody owns


# ---- 2. the known answer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_a_window_of_one_key_returns_that_keys_value(fa, oracle_mod, dtype, D):
    for heads in wn.HEADS:
        d = data(oracle_mod, dtype, D, heads)
        G = heads[0] // heads[1]
        for r, what in ((varlen(fa, d, (0, 0)), "varlen"), (paged(fa, d, 16, "NHD", (0, 0)), "paged")):
            for b, (Lq, Lk) in enumerate(d["lens"]):
                q, k, v = d["seqs"][b]
                on, ln = (x.float().cpu().numpy() for x in piece(r, d["cu_q"], b))
                rows = np.nonzero(~wn.dead_rows(Lq, Lk, 0, 0))[0]
                if not len(rows):
                    continue
                keys = rows + Lk - Lq
                ve, ke = np.repeat(v, G, axis=0), np.repeat(k, G, axis=0)
                assert np.array_equal(on[:, rows], ve[:, keys]), (what, heads, b, "O != V[i + coff]")
                s = (q[:, rows].astype(np.float64) * ke[:, keys]).sum(-1) * D ** -0.5
                assert np.abs(ln[:, rows] - s).max() < lse_tol(dtype, 1, q, k), (what, heads, b)


# ---- 3. identity to the old kernels through the new ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_an_unbinding_window_is_the_unwindowed_call_bit_for_bit(fa, oracle_mod, dtype, D):
    for heads in wn.HEADS:
        d = data(oracle_mod, dtype, D, heads)
        for causal, win in ((True, (INT_MAX, 0)), (False, (INT_MAX, INT_MAX))):
            for n, (new, old) in enumerate(((varlen(fa, d, win), varlen(fa, d, causal=causal)),
                                            (paged(fa, d, 16, "HND", win), paged(fa, d, 16, "HND", causal=causal)),
                                            (paged(fa, d, 256, "NHD", win), paged(fa, d, 256, "NHD", causal=causal)))):
                claimed = 0
                for b, (Lq, Lk) in enumerate(d["lens"]):
                    if wn.identity_claimed(Lq, Lk):
                        claimed += 1
                        assert same_bits(piece(new, d["cu_q"], b), piece(old, d["cu_q"], b)), (n, heads, causal, b)
                assert claimed == 5


# ---- 4. the shift identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_dropping_the_keys_in_front_of_the_first_tile_changes_no_bit(fa, oracle_mod, dtype, D):
    Lq, Lk, wl, drop = wn.SHIFT
    assert drop % wn.TILE == 0 and (max(0, Lk - Lq - wl) // wn.TILE) * wn.TILE == drop
    d = data(oracle_mod, dtype, D, (8, 2), lens=((Lq, Lk),), seed=1)
    q, k, v = d["seqs"][0]
    kd, vd = to_dev(d["kn"][drop:], dtype), to_dev(d["vn"][drop:], dtype)
    a = varlen(fa, d, (wl, 0))
    b = varlen(fa, d, (wl, 0), k=kd, v=vd, cu_k=[0, Lk - drop], max_k=Lk - drop)
    assert same_bits(a, b)
    check_parity(d, a, wl, 0, ("shift", dtype, D))
    for P in (16, 64):
        kp, vpool, table = pool_of(d, P, "HND")
        a = paged(fa, d, P, "HND", (wl, 0), pool=(kp, vpool, table))
        b = paged(fa, d, P, "HND", (wl, 0), pool=(kp, vpool, table[:, drop // P:]), lens_k=[Lk - drop])
        assert same_bits(a, b), P
        check_parity(d, a, wl, 0, ("shift paged", P, dtype, D))


# ---- 5. keys no query sees ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_keys_no_query_sees_do_not_matter(fa, oracle_mod, dtype, D):
    d = data(oracle_mod, dtype, D, (8, 2))
    for n, (wl, wr) in enumerate(((0, 0), (63, 0), (64, 64), (200, 0), (31, 5))):
        ks, vs, hidden = [], [], 0
        for (Lq, Lk), (_, k, v) in zip(d["lens"], d["seqs"]):
            un = wn.unseen_keys(Lq, Lk, wl, wr)
            hidden += int(un.sum())
            k2, v2 = k.copy(), v.copy()
            k2[:, un], v2[:, un] = 6e4, -6e4
            k2[:, un, ::2], v2[:, un, ::2] = -6e4, 6e4
            ks.append(oracle_mod.round_to(k2, dtype))
            vs.append(oracle_mod.round_to(v2, dtype))
        assert hidden > 0
        kn, _ = vp.pack_rows(ks, tail=1)
        vn, _ = vp.pack_rows(vs, tail=1)
        assert same_bits(varlen(fa, d, (wl, wr)), varlen(fa, d, (wl, wr), k=to_dev(kn, dtype), v=to_dev(vn, dtype))), (wl, wr)
        P, layout = paged_config(n)
        assert same_bits(paged(fa, d, P, layout, (wl, wr)), paged(fa, d, P, layout, (wl, wr), pool=pool_of(d, P, layout, ks, vs))), (wl, wr, P)


# ---- 6. routing and the wrapper ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_routing_by_sign_and_the_wrapper(fa, oracle_mod, dtype, D):
    import torch

    d = data(oracle_mod, dtype, D, (8, 2))
    for call in (lambda **kw: varlen(fa, d, **kw), lambda **kw: paged(fa, d, 16, "HND", **kw)):
        full, causal = call(causal=False), call(causal=True)
        assert same_bits(call(window=(-1, -1)), full) and same_bits(call(window=(-1, 0)), causal)
        assert same_bits(call(window=(-7, -2)), full) and same_bits(call(window=(-1, -1), causal=True), causal)
        assert same_bits(call(window=None), full) and same_bits(call(window=None, causal=True), causal)
        with_lse = call(window=(63, 5))
        without = call(window=(63, 5), return_lse=False)
        assert without[1] is None and torch.equal(bits(without[0]), bits(with_lse[0]))
        assert same_bits(call(window=(63, -1), causal=True), call(window=(63, 0)))
        with pytest.raises(ValueError):
            call(window=(63, 5), causal=True)


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def decode_batch(oracle, qdt, kvdt, D, Hq, Hkv, Nq, P, layout, lens=wn.DECODE_L, seed=0, unseen=None):
    """q [B, Hq, Nq, D], a paged cache of capacity 4096 with pages in random order; `unseen`: (wl, wr) whose unseen keys hold +-6e4."""
    rng = np.random.default_rng(14500 + seed + D + Nq + P)
    amp = 2.0 if kvdt == "fp8" else 1.0
    q = oracle.round_to(amp * rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, D)).astype(np.float32), qdt)
    ks = [oracle.round_to(amp * rng.uniform(-1.0, 1.0, (Hkv, L, D)).astype(np.float32), kvdt) for L in lens]
    vs = [oracle.round_to(amp * rng.uniform(-1.0, 1.0, (Hkv, L, D)).astype(np.float32), kvdt) for L in lens]
    return q, ks, vs


def decode_pool(ks, vs, kvdt, P, layout, seed=0):
    pool = vp.build_pool(ks, vs, P, rng=np.random.default_rng(P + seed), spare=2, fill=0.0, max_pages=CAP // P)
    return to_layout(pool["k"], kvdt, layout), to_layout(pool["v"], kvdt, layout), pool["table"]


def decode(fa, q, qdt, pool, lens, layout, window=None, causal=False, **kw):
    import torch

    kp, vpool, table = pool
    r = fa.flash_attention_decode_paged(to_dev(q, qdt), kp, vpool, i32(table), i32(lens), is_causal=causal, layout=layout, window=window, **kw)
    torch.cuda.synchronize()
    return r


DECODE_CASES = [  # qdt, kvdt, D, Hq, Hkv, Nq, P, layout: a group of 4 at Nq 1 and 4 (16 packed rows), a group of 8 at Nq 4 (32)
    ("f16", "f16", 64, 8, 2, 1, 16, "HND"), ("bf16", "bf16", 128, 8, 2, 4, 256, "NHD"), ("fp8", "fp8", 64, 8, 2, 4, 16, "NHD"),
    ("bf16", "fp8", 128, 8, 2, 1, 256, "HND"), ("bf16", "bf16", 64, 8, 1, 4, 16, "HND"), ("f16", "f16", 128, 16, 2, 4, 256, "NHD"),
]


@pytest.mark.parametrize("qdt,kvdt,D,Hq,Hkv,Nq,P,layout", DECODE_CASES)
def test_decode_parity_identity_and_unseen_keys(fa, oracle_mod, qdt, kvdt, D, Hq, Hkv, Nq, P, layout):
    lens = list(wn.DECODE_L)
    q, ks, vs = decode_batch(oracle_mod, qdt, kvdt, D, Hq, Hkv, Nq, P, layout)
    pool = decode_pool(ks, vs, kvdt, P, layout)
    bar = "bf16" if "fp8" in (qdt, kvdt) else qdt
    base_o = (2 if kvdt == "fp8" else 1) * TOL_O[bar]  # (an e4m3 cache at twice the amplitude: tests/test_gpu_decode_paged.py::test_paged_e4m3)
    for wl, wr in DECODE_WINDOWS:
        o, lse = decode(fa, q, qdt, pool, lens, layout, (wl, wr))
        on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
        for b, L in enumerate(lens):
            o64, l64 = wn.reference(q[b], ks[b], vs[b], wl, wr)
            dead = wn.dead_rows(Nq, L, wl, wr)
            assert np.array_equal(on[b][:, dead], np.zeros_like(on[b][:, dead])) and np.isneginf(ln[b][:, dead]).all(), (wl, wr, b)
            live = ~dead
            if not live.any():
                continue
            err_o, err_l = np.abs(on[b] - o64).max(), np.abs(ln[b][:, live] - l64[:, live]).max()
            bar_o, bar_l = o_tol(bar, 1, q[b], ks[b], vs[b], None, base_o), lse_tol(bar, 1, q[b], ks[b])
            print(f"WINDOW decode {qdt}/{kvdt} D={D} Nq={Nq} ({wl}, {wr}) L={L}: O {err_o:.2e} (bar {bar_o:.2e}) LSE {err_l:.2e} (bar {bar_l:.2e})")
            assert err_o < bar_o and err_l < bar_l, (wl, wr, b, err_o, err_l)
        if wl not in (INT_MAX,):  # keys nobody sees hold +-6e4 (e4m3: its largest finite value)
            big = 448.0 if kvdt == "fp8" else 6e4
            k2, v2, hidden = [], [], 0
            for L, k, v in zip(lens, ks, vs):
                un = wn.unseen_keys(Nq, L, wl, wr)
                hidden += int(un.sum())
                kk, vv = k.copy(), v.copy()
                kk[:, un], vv[:, un] = big, -big
                k2.append(oracle_mod.round_to(kk, kvdt))
                v2.append(oracle_mod.round_to(vv, kvdt))
            assert hidden > 0
            assert same_bits((o, lse), decode(fa, q, qdt, decode_pool(k2, v2, kvdt, P, layout), lens, layout, (wl, wr))), (wl, wr, "unseen keys")
    # through the windowed kernels, bit for bit the un-windowed call (every L >= Nq here except L = 1 < Nq = 4)
    keep = [b for b, L in enumerate(lens) if L >= Nq]
    for causal, win in ((True, (INT_MAX, 0)), (False, (INT_MAX, INT_MAX))):
        new, old = decode(fa, q, qdt, pool, lens, layout, win), decode(fa, q, qdt, pool, lens, layout, causal=causal)
        assert same_bits((new[0][keep], new[1][keep]), (old[0][keep], old[1][keep])), (causal, win)
    # routing by sign, and the wrapper
    full, causal = decode(fa, q, qdt, pool, lens, layout), decode(fa, q, qdt, pool, lens, layout, causal=True)
    assert same_bits(decode(fa, q, qdt, pool, lens, layout, (-1, -1)), full) and same_bits(decode(fa, q, qdt, pool, lens, layout, (-1, 0)), causal)
    assert same_bits(decode(fa, q, qdt, pool, lens, layout, (31, -1), causal=True), decode(fa, q, qdt, pool, lens, layout, (31, 0)))
    nol = decode(fa, q, qdt, pool, lens, layout, (31, 0), return_lse=False)
    assert nol[1] is None and same_bits((nol[0], None), decode(fa, q, qdt, pool, lens, layout, (31, 0)))


@pytest.mark.parametrize("qdt,kvdt,D", [("bf16", "bf16", 64), ("f16", "f16", 128), ("bf16", "fp8", 128)])
def test_decode_shift_identity(fa, oracle_mod, qdt, kvdt, D):
    L, Nq, wl, drop = wn.SHIFT_DECODE
    assert (max(0, L - Nq - wl) // wn.TILE) * wn.TILE == drop
    q, ks, vs = decode_batch(oracle_mod, qdt, kvdt, D, 8, 2, Nq, 16, "HND", lens=(L,), seed=2)
    for P in (16, 256):  # the same capacity in both calls: the same number of key splits
        kp, vpool, table = decode_pool(ks, vs, kvdt, P, "HND")
        a = decode(fa, q, qdt, (kp, vpool, table), [L], "HND", (wl, 0))
        k2, v2 = [ks[0][:, drop:]], [vs[0][:, drop:]]
        b = decode(fa, q, qdt, decode_pool(k2, v2, kvdt, P, "HND", seed=5), [L - drop], "HND", (wl, 0))
        assert same_bits(a, b), P


# ---- 7. graph replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_graph_replay_after_the_tables_change(fa, oracle_mod, dtype, D):
    import torch

    Hq, Hkv, P, mp, B, total, max_q = 8, 2, 16, 40, 3, 400, 200
    win, dwin = (100, 0), (150, 0)
    rng = np.random.default_rng(140 + D)
    q = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hq, D), dtype)
    kn = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hkv, D), dtype)
    vn = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hkv, D), dtype)
    qd = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, B, Hq, 1, D), dtype)
    num_pages = B * mp + 4
    init_k = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, num_pages, Hkv, P, D), dtype)  # every slot finite: any prefix is a cache
    init_v = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, num_pages, Hkv, P, D), dtype)
    steps = [  # (cu of the chunk, block table, lengths after the append)
        ([0, 100, 250, 400], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [100, 600, 151]),
        ([0, 200, 200, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [480, 77, 130]),
        ([0, 1, 2, 3], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [1, 300, 17]),
    ]
    cu, bt, sl = i32(steps[0][0]), i32(steps[0][1]), i32(steps[0][2])
    ws = torch.empty(fa.decode_paged_workspace_bytes(B, Hq, Hkv, 1, D, P, mp), dtype=torch.uint8, device="cuda")

    def bufs():
        return (init_k.clone(), init_v.clone(), torch.full_like(q, float("nan")), torch.full((Hq, total), float("nan"), device="cuda"),
                torch.full_like(qd, float("nan")), torch.full((B, Hq, 1), float("nan"), device="cuda"))

    def step(kp_, vp_, o_, lse_, od_, ld_):
        fa.kv_append_paged(kn, vn, kp_, vp_, cu, bt, sl, max_q)
        fa.flash_attention_varlen_paged(q, kp_, vp_, cu, bt, sl, max_q, window=win, out=o_, lse=lse_)
        fa.flash_attention_decode_paged(qd, kp_, vp_, bt, sl, window=dwin, out=od_, lse=ld_, workspace=ws)

    g = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*g)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*g)
    for c, t, l in (steps[1], steps[0], steps[2], steps[1]):
        cu.copy_(i32(c))
        bt.copy_(i32(t))
        sl.copy_(i32(l))
        for dst, src in zip(g, bufs()):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        e = bufs()
        step(*e)  # the same three calls eagerly, on fresh buffers
        torch.cuda.synchronize()
        n = c[-1]
        assert torch.equal(bits(g[0]), bits(e[0])) and torch.equal(bits(g[1]), bits(e[1])), "the appended pools"
        assert torch.equal(bits(g[2][:n]), bits(e[2][:n])) and torch.equal(bits(g[3][:, :n]), bits(e[3][:, :n])), "the windowed prefill"
        assert torch.equal(bits(g[4]), bits(e[4])) and torch.equal(bits(g[5]), bits(e[5])), "the windowed decode"
        assert bool(torch.isnan(g[2][n:].float()).all())  # tokens nobody owns stay untouched
        # and the replayed prefill is the operator: sequence 0 against the fp64 reference on its gathered cache
        L0, n0 = l[0], c[1] - c[0]
        if n0 and L0 <= mp * P:
            kg = vp.gather(g[0].float().cpu().numpy(), t[0], L0, P)
            vg = vp.gather(g[1].float().cpu().numpy(), t[0], L0, P)
            q0 = q[:n0].float().cpu().numpy().transpose(1, 0, 2)
            o64, l64 = wn.reference(q0, kg, vg, *win)
            on = g[2][:n0].float().cpu().numpy().transpose(1, 0, 2)
            live = ~wn.dead_rows(n0, L0, *win)
            assert np.abs(on - o64).max() < o_tol(dtype, 1, q0, kg, vg, None, TOL_O[dtype])
            assert np.abs(g[3][:, :n0].cpu().numpy()[:, live] - l64[:, live]).max() < lse_tol(dtype, 1, q0, kg)
