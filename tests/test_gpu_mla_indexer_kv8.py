"""GPU: the MLA indexer over e4m3 index keys with a scale per key (include/fa_mi355.h, "The MLA indexer (e4m3 keys)") against numpy fp64,
at the shapes and with the helpers of test_gpu_mla_indexer.py: exact inputs (logits and lists must be equal), key chunks, random inputs
under the header's per-element bound, footprints and no-influence, the chain into the sparse decode, a captured graph, Python routing."""
import numpy as np
import pytest

from test_gpu_mla_indexer import batch, fa, hold_lists, make, ref_logits, ref_select, tokens  # noqa: F401  (fa: fixture)

pytestmark = pytest.mark.gpu


def make8(rng, Hi, P, seqs, exact, spare=3):
    """test_gpu_mla_indexer.make's batch on e4m3-representable values, plus a scale per pool slot: powers of two (exact) or random"""
    import torch

    c = make(rng, "bf16", Hi, P, seqs, exact=True, spare=spare)
    if not exact:
        rnd = lambda a: torch.from_numpy(a).float().to(torch.float8_e4m3fn).double().numpy()
        c["q"], c["k"] = rnd(rng.standard_normal(c["q"].shape)), rnd(rng.standard_normal(c["k"].shape))
        c["w"] = rng.standard_normal(c["w"].shape).astype(np.float32).astype(np.float64)
    shape = (c["num_pages"], P)
    c["ks"] = rng.choice([0.5, 1.0, 2.0, 4.0], shape) if exact else rng.uniform(0.01, 3.0, shape).astype(np.float32).astype(np.float64)
    return c


def ref8(c):
    """{token: (fp64 logits, the bound's k_scale_j sum_h |w| sum_d |q| |k|)}: the 16-bit reference times the key's scale"""
    out, base = {}, ref_logits(c)
    for t, b, v in tokens(c):
        j = np.arange(v)
        s = c["ks"][np.clip(c["bt"][b][j // c["P"]], 0, c["num_pages"] - 1), j % c["P"]]  # (a page outside the pool: the logit is 0)
        out[t] = (base[t][0] * s, base[t][1] * s)
    return out


def dev8(c, packed=False):
    """device tensors; packed: one uint8 pool of pages of P * 128 value bytes followed by P * 4 scale bytes, k and ks as views of it"""
    import torch

    f8, i32 = torch.float8_e4m3fn, lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    k, ks, P = torch.from_numpy(c["k"]).float().to(f8).cuda(), torch.from_numpy(c["ks"]).float().cuda(), c["P"]
    if packed:
        pool = torch.empty((c["num_pages"], 132 * P), dtype=torch.uint8, device="cuda")
        pool[:, :128 * P] = k.view(torch.uint8).view(-1, 128 * P)
        pool[:, 128 * P:] = ks.view(torch.uint8).view(-1, 4 * P)
        k, ks = pool[:, :128 * P].view(f8).unflatten(1, (P, 128)), pool[:, 128 * P:].view(torch.float32)
        assert k.stride() == (132 * P, 128, 1) and ks.stride() == (33 * P, 1)
    return dict(q=torch.from_numpy(c["q"]).float().to(f8).cuda(), k=k, ks=ks, w=torch.from_numpy(c["w"]).float().cuda(),
                cu=i32(c["cu"]), bt=i32(c["bt"]), sk=i32(c["sk"]))


def logits8(fa, c, d, **kw):
    return fa.mla_indexer_logits(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], c["max_q"], k_scale_pages=d["ks"], **kw)


def topk8(fa, c, d, topk, **kw):
    return fa.flash_attention_mla_indexer_topk(d["q"], d["w"], d["k"], d["cu"], d["bt"], d["sk"], topk, c["max_q"], k_scale_pages=d["ks"], **kw)


def hold_exact(fa, c, d, topks, what):
    ref = ref8(c)
    got = logits8(fa, c, d).cpu().numpy()
    for t, _, v in tokens(c):
        assert np.array_equal(got[t, :v].astype(np.float64), ref[t][0]), (what, t, v)
    for topk in topks:
        idx, cnt = topk8(fa, c, d, topk)
        hold_lists(c, idx, cnt, ref_select(c, {t: ref[t][0] for t in ref}, topk), topk, (what, topk))


@pytest.mark.parametrize("lq", [1, 2, 4, 5])  # every token-block form (1, 2, 4) and a ragged last block of four
@pytest.mark.parametrize("P", [16, 64, 256])
@pytest.mark.parametrize("Hi", [64, 32])
def test_exact_inputs_give_exact_logits_and_the_reference_lists(fa, Hi, P, lq):
    c = make8(np.random.default_rng(3300 + lq + P), Hi, P, batch(lq), exact=True)
    c["bt"][11, 0] = c["num_pages"] + 2  # keys 0 .. P - 1 of the 200-key sequence: a page entry outside the pool
    hold_exact(fa, c, dev8(c, packed=(Hi == 32 and lq == 5)), (1, 48, 64, 65), "exact")


def test_a_sequence_over_several_key_chunks(fa):
    P, mp, seqs = 64, 40, [(1, 40 * 64 - 3), (1, 700)]
    chunk = fa.mla_indexer_chunk_keys(len(seqs), 1, P, mp + 1)  # (make adds one spare table column)
    assert 0 < 2 * chunk <= seqs[0][1], chunk
    c = make8(np.random.default_rng(3310), 64, P, seqs, exact=True)
    assert c["mp"] == mp + 1
    hold_exact(fa, c, dev8(c), (65,), "chunks")


@pytest.mark.parametrize("Hi", [64, 32])
def test_random_inputs_within_the_per_element_bound(fa, Hi):
    """|logit - fp64| <= 2^-15 k_scale_j sum_h |w_h| sum_d |q_hd| |k_d| per element: the 16-bit call's bound times the scale (e4m3 products
    are exact in fp32, the summation is the same length plus one multiply). Worst ratio of error to bound measured on an MI355X: see
    README.md, "The MLA indexer over e4m3 keys"."""
    c = make8(np.random.default_rng(3320), Hi, 64, [(5, 333), (1, 129), (2, 64)], exact=False)
    ref = ref8(c)
    got = logits8(fa, c, dev8(c)).cpu().numpy()
    worst = max((np.abs(got[t, :v] - ref[t][0]) / (2.0 ** -15 * ref[t][1])).max() for t, _, v in tokens(c))
    print(f"INDEXER KV8 Hi={Hi}: worst error / bound = {worst:.4f}")
    assert worst <= 1.0, worst


def test_footprints_and_what_has_no_influence(fa):
    import torch

    rng = np.random.default_rng(3340)
    c = make8(rng, 64, 16, [(4, 70), (1, 33), (2, 1), (3, 100)], exact=True)
    c["bt"][3, 2] = c["num_pages"] + 5  # keys 32 .. 47 of the last sequence: a page entry outside the pool
    c["bt"][1, 0] = -1
    d, ref, cap, T, topk, pad = dev8(c), ref8(c), c["mp"] * c["P"], c["T"], 24, 2  # pad: rows of tokens nobody owns
    want = ref_select(c, {t: ref[t][0] for t in ref}, topk)
    assert any((want[t] == -1).any() for t in want)
    d["q"] = torch.cat([d["q"].view(torch.uint8), d["q"][:pad].view(torch.uint8)]).view(torch.float8_e4m3fn)
    d["w"] = torch.cat([d["w"], d["w"][:pad]])
    logits = torch.full((T + pad, cap + 8), -7.5, device="cuda")
    logits8(fa, c, d, logits=logits)
    ln, vis = logits.cpu().numpy(), {t: v for t, _, v in tokens(c)}
    for t in range(T + pad):
        v = vis.get(t, 0)
        assert np.array_equal(ln[t, :v].astype(np.float64), ref[t][0] if v else ln[t, :0]) and (ln[t, v:] == -7.5).all(), t
    # NaN wherever nothing may be read: key bytes and scales of every slot no visible key names, and the workspace
    used = np.zeros((c["num_pages"], c["P"]), bool)
    for b, (_, L) in enumerate(c["seqs"]):
        for j in range(L):
            if 0 <= c["bt"][b, j // c["P"]] < c["num_pages"]:
                used[c["bt"][b, j // c["P"]], j % c["P"]] = True
    free = torch.from_numpy(~used).cuda()
    kb = d["k"].view(torch.uint8).clone()
    kb[free] = torch.tensor([0x7F, 0xFF], dtype=torch.uint8, device="cuda").repeat(64)
    d["k"], d["ks"] = kb.view(torch.float8_e4m3fn), torch.where(free, float("nan"), d["ks"])
    idx = torch.full((T + pad, 32), -99, dtype=torch.int32, device="cuda")
    cnt = torch.full((T + pad,), -99, dtype=torch.int32, device="cuda")
    ws = torch.full((fa.mla_indexer_workspace_bytes(T + pad, c["P"], c["mp"]),), 0xFF, dtype=torch.uint8, device="cuda")
    topk8(fa, c, d, topk, indices=idx, index_counts=cnt, workspace=ws)
    hold_lists(c, idx, cnt, want, topk, "footprint")
    byhand = fa.mla_indexer_select(logits8(fa, c, d), d["cu"], d["bt"], d["sk"], topk, c["max_q"], c["P"], c["num_pages"])  # the two calls by hand
    idn, cn = idx.cpu().numpy(), cnt.cpu().numpy()
    for t in range(T + pad):
        n = cn[t] if t in vis else 0
        assert (idn[t, n:] == -99).all() and (t in vis or cn[t] == -99), t
        assert t not in vis or (byhand[1][t] == cnt[t] and torch.equal(byhand[0][t, :n], idx[t, :n])), t


def test_the_list_feeds_the_sparse_decode(fa):
    import torch

    rng = np.random.default_rng(3350)
    c = make8(rng, 64, 64, [(1, 300), (2, 130), (1, 40)], exact=True)
    ref, topk = ref8(c), 64
    idx, cnt = topk8(fa, c, dev8(c), topk)
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


def test_a_captured_graph_follows_tables_lengths_keys_and_scales(fa):
    import torch

    rng = np.random.default_rng(3360)
    c = make8(rng, 64, 32, [(4, 150), (1, 90), (2, 64)], exact=False)
    d, topk = dev8(c), 48
    idx = torch.full((c["T"], topk), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((c["T"],), dtype=torch.int32, device="cuda")
    ws = torch.zeros((fa.mla_indexer_workspace_bytes(c["T"], c["P"], c["mp"]),), dtype=torch.uint8, device="cuda")
    kw = dict(indices=idx, index_counts=cnt, workspace=ws)
    topk8(fa, c, d, topk, **kw)  # (warm: the first call loads the code object)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        topk8(fa, c, d, topk, **kw)
    torch.cuda.synchronize()
    # another step under the same scalars: lengths, the table, the key bytes and the scales change in place
    c2 = make8(rng, 64, 32, [(3, 97), (2, 140), (2, 33)], exact=False)
    assert c2["mp"] == c["mp"] and c2["k"].shape == c["k"].shape and c2["T"] == c["T"]
    d2 = dev8(c2)
    for name in d:
        d[name].view(torch.uint8).copy_(d2[name].view(torch.uint8))
    ei, ec = topk8(fa, c, d, topk)
    torch.cuda.synchronize()
    for _ in range(3):
        idx.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cnt, ec)
        for t in range(c["T"]):
            assert torch.equal(idx[t, :cnt[t]], ei[t, :ec[t]]), t


def test_python_routing_refuses_before_the_library(fa):
    c = make8(np.random.default_rng(3370), 32, 16, [(1, 20)], exact=True)
    import torch

    d = dev8(c)
    q16, k16 = torch.from_numpy(c["q"]).bfloat16().cuda(), torch.from_numpy(c["k"]).bfloat16().cuda()
    # e4m3 without scales, scales with 16-bit tensors, mixed types either way, scales of another type or shape
    for bad in (dict(ks=None), dict(q=q16, k=k16), dict(k=k16), dict(q=q16), dict(ks=d["ks"].double()), dict(ks=d["ks"][:, :8])):
        with pytest.raises(ValueError):
            logits8(fa, c, {**d, **bad})
        with pytest.raises(ValueError):
            topk8(fa, c, {**d, **bad}, 8)
