"""GPU: the MLA indexer (include/fa_mi355.h, "The MLA indexer") -- fa_mla_indexer_logits_paged, fa_mla_indexer_select and their composite
against numpy fp64: exact inputs (logits and lists must be equal), random inputs under the header's per-element bound, the select alone
on crafted rows, footprints and no-influence, the chain into the sparse decode, reproducibility and a captured graph, and an index pool
whose used pages lie past byte 2^32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TORCH = {"f16": "float16", "bf16": "bfloat16"}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def make(rng, dtype, Hi, P, seqs, exact, spare=3):
    """One batch, seqs = [(Lq_b, L_b)]: packed q / w, a pool of B * mp + spare pages under a shuffled block table, as fp64 numpy."""
    B, T = len(seqs), sum(lq for lq, _ in seqs)
    mp = max(1, max(-(-L // P) for _, L in seqs)) + 1
    num_pages = B * mp + spare
    if exact:  # small integers times powers of two: every partial sum an integer below 2^24 units, many equal logits
        q = rng.integers(-1, 2, (T, Hi, 128)) * 0.5
        k = rng.integers(-1, 2, (num_pages, P, 128)) * 2.0
        w = rng.integers(0, 3, (T, Hi)) * 0.25
    else:
        import torch

        rnd = lambda a: torch.from_numpy(a).to(getattr(torch, TORCH[dtype])).double().numpy()
        q, k = rnd(rng.standard_normal((T, Hi, 128))), rnd(rng.standard_normal((num_pages, P, 128)))
        w = rng.standard_normal((T, Hi)).astype(np.float32).astype(np.float64)
    bt = rng.permutation(num_pages)[:B * mp].reshape(B, mp).astype(np.int32)
    return dict(q=q, k=k, w=w, bt=bt, seqs=seqs, P=P, mp=mp, num_pages=num_pages, dtype=dtype, Hi=Hi, T=T, max_q=max(lq for lq, _ in seqs),
                cu=np.concatenate([[0], np.cumsum([lq for lq, _ in seqs])]).astype(np.int32), sk=np.array([L for _, L in seqs], np.int32))


def tokens(c):
    """(token, sequence, visible keys) of every owned token"""
    return [(c["cu"][b] + i, b, min(max(L - lq + i + 1, 0), L)) for b, (lq, L) in enumerate(c["seqs"]) for i in range(lq)]


def ref_logits(c):
    """{token: (fp64 logits of its visible keys, the bound's sum_h |w| sum_d |q| |k|)}; a page entry outside the pool is rows of zeros"""
    out = {}
    for t, b, v in tokens(c):
        j = np.arange(v)
        page = c["bt"][b][j // c["P"]]
        ok = (page >= 0) & (page < c["num_pages"])
        keys = np.where(ok[:, None], c["k"][np.where(ok, page, 0), j % c["P"]], 0.0)
        dots = c["q"][t] @ keys.T
        out[t] = ((c["w"][t][:, None] * np.maximum(dots, 0)).sum(0), (np.abs(c["w"][t])[:, None] * (np.abs(c["q"][t]) @ np.abs(keys).T)).sum(0))
    return out


def ref_select(c, rows, topk):
    """{token: slots}: lexsort on (-logit, position), the picked positions sorted, then the slots (-1 outside the pool)"""
    out = {}
    for t, b, v in tokens(c):
        j = np.sort(np.lexsort((np.arange(v), -rows[t][:v].astype(np.float64)))[:topk]) if v > topk else np.arange(v)
        page = c["bt"][b][j // c["P"]].astype(np.int64)
        out[t] = np.where((page >= 0) & (page < c["num_pages"]), page * c["P"] + j % c["P"], -1)
    return out


def dev(c):
    import torch

    td = getattr(torch, TORCH[c["dtype"]])
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    return dict(q=torch.from_numpy(c["q"]).to(td).cuda(), k=torch.from_numpy(c["k"]).to(td).cuda(), w=torch.from_numpy(c["w"]).float().cuda(),
                cu=i32(c["cu"]), bt=i32(c["bt"]), sk=i32(c["sk"]))


def topk_call(fa, c, d, topk, **kw):
    return fa.flash_attention_mla_indexer_topk(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], topk, c["max_q"], **kw)


def hold_lists(c, idx, cnt, want, topk, what):
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for t, _, v in tokens(c):
        assert cnt[t] == min(topk, v), (what, t, cnt[t], v)
        assert np.array_equal(idx[t, :cnt[t]], want[t]), (what, t, v, idx[t, :cnt[t]], want[t])


# sequences (Lq_b, L_b) around a longest query of `lq`: L_b in {0, 1, 63, 64, 65, 129}, a chunk offset (L_b > Lq_b), L_b < Lq_b (tokens that
# see nothing), and v = topk, topk + 1 for topk in {1, 48, 64, 65} (the one-token sequences: v = L_b)
def batch(lq):
    return [(lq, 129), (1, 64), (lq, lq - 1), (min(2, lq), 65), (lq, 63), (1, 0), (1, 1), (1, 2), (1, 48), (1, 49), (1, 66), (lq, 200), (min(3, lq), 64)]


@pytest.mark.parametrize("lq", [1, 2, 4, 5])  # every token-block form (1, 2, 4) and a ragged last block of four
@pytest.mark.parametrize("P", [16, 64, 256])
@pytest.mark.parametrize("dtype,Hi", [("bf16", 64), ("bf16", 32), ("f16", 64), ("f16", 32)])
def test_exact_inputs_give_exact_logits_and_the_reference_lists(fa, dtype, Hi, P, lq):
    c = make(np.random.default_rng(3200 + lq + P), dtype, Hi, P, batch(lq), exact=True)
    d, ref = dev(c), ref_logits(c)
    got = fa.mla_indexer_logits(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], c["max_q"]).cpu().numpy()
    for t, _, v in tokens(c):
        assert np.array_equal(got[t, :v].astype(np.float64), ref[t][0]), (t, v)
    for topk in (1, 48, 64, 65):
        idx, cnt = topk_call(fa, c, d, topk)
        hold_lists(c, idx, cnt, ref_select(c, {t: ref[t][0] for t in ref}, topk), topk, f"topk={topk}")


def test_a_sequence_over_several_key_chunks(fa):
    P, mp, seqs = 64, 40, [(1, 40 * 64 - 3), (1, 700)]
    chunk = fa.mla_indexer_chunk_keys(len(seqs), 1, P, mp + 1)  # (make adds one spare table column)
    assert 0 < 2 * chunk <= seqs[0][1], chunk
    c = make(np.random.default_rng(3210), "bf16", 64, P, seqs, exact=True)
    assert c["mp"] == mp + 1
    d, ref = dev(c), ref_logits(c)
    got = fa.mla_indexer_logits(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], 1).cpu().numpy()
    for t, _, v in tokens(c):
        assert np.array_equal(got[t, :v].astype(np.float64), ref[t][0]), t
    idx, cnt = topk_call(fa, c, d, 65)
    hold_lists(c, idx, cnt, ref_select(c, {t: ref[t][0] for t in ref}, 65), 65, "chunks")


@pytest.mark.parametrize("dtype,Hi", [("bf16", 64), ("f16", 32)])
def test_random_inputs_within_the_per_element_bound(fa, dtype, Hi):
    """|logit - fp64| <= 2^-15 sum_h |w_h| sum_d |q_hd| |k_d| per element: 2^-16 for the fp32 summation (127 + 63 adds, a product rounding,
    192 * 2^-24 to first order, rounded up), a factor 2 for the matrix core's internal rounding. Worst ratio of error to bound measured
    on an MI355X: see README.md, "The MLA indexer"."""
    c = make(np.random.default_rng(3220), dtype, Hi, 64, [(5, 333), (1, 129), (2, 64)], exact=False)
    d, ref = dev(c), ref_logits(c)
    got = fa.mla_indexer_logits(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], c["max_q"]).cpu().numpy()
    ratios = [np.abs(got[t, :v] - ref[t][0]) / (2.0 ** -15 * ref[t][1]) for t, _, v in tokens(c)]
    worst = max(r.max() for r in ratios)
    print(f"INDEXER {dtype} Hi={Hi}: worst error / bound = {worst:.4f}")
    assert worst <= 1.0, worst


def crafted(kind, rng, n):
    if kind == "low_byte":  # one exponent and high mantissa: only the lowest byte differs, all four radix passes decide
        return (np.uint32(0x3F800000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == "mixed":
        pool = np.array([0.0, -0.0, 1e-40, -1e-40, -np.inf, 1.5, -1.5, 3e38, -3e38, 2.0 ** -126, 7.0], np.float32)
        return pool[rng.integers(0, len(pool), n)]
    if kind == "all_equal":
        return np.full(n, 0.375, np.float32)
    row = rng.standard_normal(n).astype(np.float32)  # "nan"
    row[rng.integers(0, n, n // 3)] = np.nan
    row[rng.integers(0, n, 5)] = np.float32(np.uint32(0xFFC00001).view(np.float32))
    return row


@pytest.mark.parametrize("kind", ["low_byte", "mixed", "all_equal", "nan"])
def test_select_alone_on_crafted_rows(fa, kind):
    import torch

    rng = np.random.default_rng(3230)
    c = make(rng, "bf16", 32, 16, [(1, 700), (2, 300), (1, 65), (1, 5)], exact=True)
    d, cap = dev(c), c["mp"] * c["P"]
    rows = np.stack([crafted(kind, rng, cap) for _ in range(c["T"])])
    for topk in (1, 64, 65, 257):
        idx, cnt = fa.mla_indexer_select(torch.from_numpy(rows).cuda(), d["cu"], d["bt"], d["sk"], topk, c["max_q"], c["P"], c["num_pages"])
        if kind != "nan":
            hold_lists(c, idx, cnt, ref_select(c, rows, topk), topk, (kind, topk))
            continue
        idx, cnt, every = idx.cpu().numpy(), cnt.cpu().numpy(), ref_select(c, rows, 1 << 30)  # (every visible slot of the token)
        for t, _, v in tokens(c):
            got = idx[t, :cnt[t]]
            assert cnt[t] == min(topk, v) and len(set(got)) == len(got) and set(got) <= set(every[t]), (topk, t)


def test_footprints_and_what_has_no_influence(fa):
    import torch

    rng = np.random.default_rng(3240)
    c = make(rng, "bf16", 64, 16, [(4, 70), (1, 33), (2, 1), (3, 100)], exact=True)
    c["bt"][3, 2] = c["num_pages"] + 5  # keys 32 .. 47 of the last sequence: a page entry outside the pool
    c["bt"][1, 0] = -1
    d, ref, cap, T, topk = dev(c), ref_logits(c), c["mp"] * c["P"], c["T"], 24
    want = ref_select(c, {t: ref[t][0] for t in ref}, topk)
    assert any((want[t] == -1).any() for t in want) and all((ref[t][0][32:48] == 0).all() for t, b, v in tokens(c) if b == 3)
    pad = 2  # rows of tokens nobody owns, behind the last sequence
    q2, w2 = torch.cat([d["q"], d["q"][:pad]]), torch.cat([d["w"], d["w"][:pad]])
    logits = torch.full((T + pad, cap + 8), -7.5, device="cuda")
    fa.mla_indexer_logits(q2, w2, d["k"], d["cu"], d["bt"], d["sk"], c["max_q"], logits=logits)
    ln = logits.cpu().numpy()
    vis = {t: v for t, _, v in tokens(c)}
    for t in range(T + pad):
        v = vis.get(t, 0)
        assert np.array_equal(ln[t, :v].astype(np.float64), ref[t][0] if v else ln[t, :0]) and (ln[t, v:] == -7.5).all(), t
    idx = torch.full((T + pad, 32), -99, dtype=torch.int32, device="cuda")
    cnt = torch.full((T + pad,), -99, dtype=torch.int32, device="cuda")
    # NaN wherever nothing may be read: the workspace, pages no table lists, table columns and rows behind L_b
    kn, used = d["k"].clone(), np.zeros((c["num_pages"], c["P"]), bool)
    for b, (_, L) in enumerate(c["seqs"]):
        for j in range(L):
            if 0 <= c["bt"][b, j // c["P"]] < c["num_pages"]:
                used[c["bt"][b, j // c["P"]], j % c["P"]] = True
    kn[torch.from_numpy(~used).cuda()] = float("nan")
    ws = torch.full((fa.mla_indexer_workspace_bytes(T + pad, c["P"], c["mp"]),), 0xFF, dtype=torch.uint8, device="cuda")
    fa.flash_attention_mla_indexer_topk(q2, w2, kn, d["cu"], d["bt"], d["sk"], topk, c["max_q"], indices=idx, index_counts=cnt, workspace=ws)
    hold_lists(c, idx, cnt, want, topk, "footprint")
    idn, cn = idx.cpu().numpy(), cnt.cpu().numpy()
    for t in range(T + pad):
        n = cn[t] if t in vis else 0
        assert (idn[t, n:] == -99).all() and (t in vis or cn[t] == -99), t


def test_the_list_feeds_the_sparse_decode(fa):
    import torch

    rng = np.random.default_rng(3250)
    c = make(rng, "bf16", 64, 64, [(1, 300), (2, 130), (1, 40)], exact=True)
    d, ref, topk = dev(c), ref_logits(c), 64
    idx, cnt = topk_call(fa, c, d, topk)
    want = ref_select(c, {t: ref[t][0] for t in ref}, topk)
    ridx = np.zeros((c["T"], topk), np.int32)
    for t in want:
        ridx[t, :len(want[t])] = want[t]
    rcnt = torch.tensor([len(want[t]) for t in range(c["T"])], dtype=torch.int32, device="cuda")
    q = torch.from_numpy(rng.uniform(-1, 1, (c["T"], 16, 576))).bfloat16().cuda()
    kv = torch.from_numpy(rng.uniform(-1, 1, (c["num_pages"], c["P"], 576))).bfloat16().cuda()
    o1, l1 = fa.flash_attention_mla_decode_sparse(q, kv, idx, 0.07, index_counts=cnt)
    o2, l2 = fa.flash_attention_mla_decode_sparse(q, kv, torch.from_numpy(ridx).cuda(), 0.07, index_counts=rcnt)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))


def test_runs_alike_and_a_captured_graph_follows_its_tables(fa):
    import torch

    rng = np.random.default_rng(3260)
    seqs = [(4, 150), (1, 90), (2, 64)]
    c = make(rng, "bf16", 64, 32, seqs, exact=False)
    d, topk = dev(c), 48
    idx = torch.full((c["T"], topk), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((c["T"],), dtype=torch.int32, device="cuda")
    ws = torch.zeros((fa.mla_indexer_workspace_bytes(c["T"], c["P"], c["mp"]),), dtype=torch.uint8, device="cuda")
    kw = dict(indices=idx, index_counts=cnt, workspace=ws)
    topk_call(fa, c, d, topk, **kw)
    first = (idx.clone(), cnt.clone())
    topk_call(fa, c, d, topk, **kw)
    assert torch.equal(idx, first[0]) and torch.equal(cnt, first[1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        topk_call(fa, c, d, topk, **kw)
    torch.cuda.synchronize()
    # another step under the same scalars: lengths, the table and the keys change in place
    c2 = make(rng, "bf16", 64, 32, [(3, 97), (2, 140), (2, 33)], exact=False)
    c2["bt"] = np.concatenate([c2["bt"], np.zeros((3, c["mp"] - c2["mp"]), np.int32)], 1) if c2["mp"] < c["mp"] else c2["bt"]
    assert c2["bt"].shape == c["bt"].shape and c2["k"].shape == c["k"].shape and c2["T"] == c["T"]
    d2 = dev(c2)
    for name in ("q", "w", "k", "cu", "bt", "sk"):
        d[name].copy_(d2[name])
    ei, ec = fa.flash_attention_mla_indexer_topk(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], topk, c["max_q"])
    torch.cuda.synchronize()
    for _ in range(3):
        idx.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cnt, ec)
        for t in range(c["T"]):
            assert torch.equal(idx[t, :cnt[t]], ei[t, :ec[t]]), t


def test_used_pages_past_byte_2_32(fa):
    """The index pool is a little over 4 GiB and every listed page lies past byte 2^32 (the manner of
    tests/test_gpu_far_addresses_mla_sparse.py): logits are the compact pool's bits, slots the compact ones plus the offset."""
    import torch

    from test_gpu_far_addresses import Arena

    c = make(np.random.default_rng(3270), "bf16", 64, 256, [(1, 700), (4, 300)], exact=False, spare=0)
    d, first, topk = dev(c), (1 << 32) // (256 * 128 * 2) + 1, 65
    lc = fa.mla_indexer_logits(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], c["max_q"])
    ic, cc = topk_call(fa, c, d, topk)
    with Arena() as a:
        big = a.ints("bf16", (first + c["num_pages"]) * 256 * 128, sentinel=False).view(torch.bfloat16).view(-1, 256, 128)
        assert big.numel() * 2 > (1 << 32) and first * 256 * 128 * 2 > (1 << 32)
        big[first:] = d["k"]
        bt = d["bt"] + first
        lf = fa.mla_indexer_logits(d["q"], d["w"], big, d["cu"], bt, d["sk"], c["max_q"])
        jf, cf = fa.flash_attention_mla_indexer_topk(d["q"], d["w"], big, d["cu"], bt, d["sk"], topk, c["max_q"])
        torch.cuda.synchronize()
        assert torch.equal(cf, cc)
        for t, _, v in tokens(c):
            assert torch.equal(lf[t, :v].view(torch.int32), lc[t, :v].view(torch.int32)), t
            assert torch.equal(jf[t, :cf[t]], ic[t, :cc[t]] + first * 256), t
