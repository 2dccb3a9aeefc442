"""GPU: fa_mla_indexer_select_split (include/fa_mi355.h, "The MLA indexer's select over several workgroups") against a plain numpy select
on the integer image of the logits, and bit for bit against fa_mla_indexer_select on the same buffers: every split count and page size
over random and crafted rows, footprints under two workspace fillings, a captured graph of logits + split select, and the Python
composite's select_splits=."""
import numpy as np
import pytest

from test_gpu_mla_indexer import crafted, dev, fa, make, topk_call  # noqa: F401  (fa: fixture)

pytestmark = pytest.mark.gpu
CAP = 2048  # segments of 1024, 704 and 256 keys under 2, 3 and 8 splits


def batch(P, topk, rng):
    """(Lq_b, L_b): v = 2040 ends inside the last segment of every split; v <= topk; v == topk + 1; no key at all; three tokens that
    share a table (v = 998, 999, 1000). Two table entries lie outside the pool."""
    seqs, mp = [(1, 2040), (1, topk), (1, topk + 1), (1, 0), (3, 1000)], CAP // P
    num_pages = len(seqs) * mp + 3
    bt = rng.permutation(num_pages)[:len(seqs) * mp].reshape(len(seqs), mp).astype(np.int32)
    bt[0, 3], bt[4, 1] = num_pages + 5, -1
    cu = np.concatenate([[0], np.cumsum([lq for lq, _ in seqs])]).astype(np.int32)
    toks = [(cu[b] + i, b, min(max(L - lq + i + 1, 0), L)) for b, (lq, L) in enumerate(seqs) for i in range(lq)]
    return dict(P=P, mp=mp, num_pages=num_pages, bt=bt, cu=cu, sk=np.array([L for _, L in seqs], np.int32), toks=toks, T=int(cu[-1]), max_q=3)


def rows_of(kind, rng, c, topk):
    if kind in ("low_byte", "mixed", "all_equal", "nan"):
        return np.stack([crafted(kind, rng, CAP) for _ in range(c["T"])])
    if kind == "late_ties":  # all equal behind 1000 lower keys: `need` cuts the equals inside a later segment of every split
        return np.tile(np.where(np.arange(CAP) < 1000, 0.25, 0.375).astype(np.float32), (c["T"], 1))
    rows = rng.standard_normal((c["T"], CAP)).astype(np.float32)
    for t, _, v in c["toks"]:  # the topk best in the first 256 keys (the first segment of every split), or the last topk below v
        if kind == "first_segment":
            rows[t, rng.permutation(256)[:topk]] += 100.0
        elif kind == "last_segment":
            rows[t, max(v - topk, 0):v] += 100.0
    return rows


def ref_lists(c, rows, topk):
    """{token: slots}: np.lexsort on (position, -image), -0 counted as +0; the picked positions ascending, as slots (-1 outside the pool)"""
    out = {}
    for t, b, v in c["toks"]:
        u = rows[t, :v].view(np.uint32).astype(np.int64)
        u[u == 0x80000000] = 0
        img = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
        j = np.sort(np.lexsort((np.arange(v), -img))[:topk])
        page = c["bt"][b][j // c["P"]].astype(np.int64)
        out[t] = np.where((page >= 0) & (page < c["num_pages"]), page * c["P"] + j % c["P"], -1)
    return out


def tables(c):
    import torch

    return [torch.from_numpy(c[n]).cuda() for n in ("cu", "bt", "sk")]


@pytest.mark.parametrize("P", [16, 64])
@pytest.mark.parametrize("S", [2, 3, 8])
def test_lists_are_the_references_and_the_one_workgroup_selects(fa, S, P):
    import torch

    rng = np.random.default_rng(3500 + S + P)
    for topk in (1, 64, 200):
        c = batch(P, topk, rng)
        cu, bt, sk = tables(c)
        for kind in ("random", "low_byte", "mixed", "all_equal", "late_ties", "first_segment", "last_segment", "nan"):
            rows = rows_of(kind, rng, c, topk)
            lg = torch.from_numpy(rows).cuda()
            idx, cnt = (x.cpu().numpy() for x in fa.mla_indexer_select(lg, cu, bt, sk, topk, 3, P, c["num_pages"], num_splits=S))
            one, ocnt = (x.cpu().numpy() for x in fa.mla_indexer_select(lg, cu, bt, sk, topk, 3, P, c["num_pages"]))
            want = ref_lists(c, rows, topk if kind != "nan" else CAP)  # (nan: every visible slot of the token)
            for t, _, v in c["toks"]:
                got, what = idx[t, :cnt[t]], (kind, topk, t, v)
                assert cnt[t] == min(topk, v) == ocnt[t], what
                if kind == "nan":  # distinct visible positions: distinct slots, and no more -1 than the keys outside the pool
                    real = got[got != -1]
                    assert len(set(real)) == len(real) and set(real) <= set(want[t]) and len(got) - len(real) <= (want[t] == -1).sum(), what
                else:
                    assert np.array_equal(got, want[t]) and np.array_equal(got, one[t, :cnt[t]]), (what, got, want[t])


def test_footprints_and_a_workspace_of_any_bytes(fa):
    import torch

    rng, topk, S, pad = np.random.default_rng(3510), 64, 8, 2
    c = batch(16, topk, rng)
    cu, bt, sk = tables(c)
    rows = np.concatenate([rows_of("random", rng, c, topk), np.zeros((pad, CAP), np.float32)])  # (two rows of tokens nobody owns)
    want, vis = ref_lists(c, rows, topk), {t: v for t, _, v in c["toks"]}
    for t in range(c["T"] + pad):
        rows[t, vis.get(t, 0):] = np.nan  # nothing at or behind column v may be read
    lg, lists = torch.from_numpy(rows).cuda(), []
    for fill in (0xFF, 0x00):
        idx = torch.full((c["T"] + pad, topk + 8), -99, dtype=torch.int32, device="cuda")
        cnt = torch.full((c["T"] + pad,), -99, dtype=torch.int32, device="cuda")
        ws = torch.full((fa.mla_indexer_select_split_workspace_bytes(c["T"] + pad, S),), fill, dtype=torch.uint8, device="cuda")
        fa.mla_indexer_select(lg, cu, bt, sk, topk, 3, 16, c["num_pages"], indices=idx, index_counts=cnt, num_splits=S, workspace=ws)
        lists.append((idx.cpu().numpy(), cnt.cpu().numpy()))
    assert np.array_equal(lists[0][0], lists[1][0]) and np.array_equal(lists[0][1], lists[1][1])
    idx, cnt = lists[0]
    for t in range(c["T"] + pad):
        n = min(topk, vis[t]) if t in vis else 0
        assert (idx[t, n:] == -99).all() and cnt[t] == (n if t in vis else -99), t
        assert t not in vis or np.array_equal(idx[t, :n], want[t]), t


def test_a_captured_graph_and_the_python_composite(fa):
    import torch

    rng, topk, S = np.random.default_rng(3520), 48, 3
    c = make(rng, "bf16", 64, 32, [(4, 1500), (1, 900), (2, 64)], exact=False)
    d = dev(c)
    idx = torch.full((c["T"], topk), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((c["T"],), dtype=torch.int32, device="cuda")
    need = fa.mla_indexer_workspace_bytes(c["T"], c["P"], c["mp"]) + fa.mla_indexer_select_split_workspace_bytes(c["T"], S)
    kw = dict(indices=idx, index_counts=cnt, workspace=torch.zeros((need,), dtype=torch.uint8, device="cuda"), select_splits=S)
    topk_call(fa, c, d, topk, **kw)  # the composite with select_splits= against today's composite
    ei, ec = topk_call(fa, c, d, topk)
    assert torch.equal(cnt, ec) and all(torch.equal(idx[t, :ec[t]], ei[t, :ec[t]]) for t in range(c["T"]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        topk_call(fa, c, d, topk, **kw)
    torch.cuda.synchronize()
    # another step under the same scalars: lengths, the table, the queries and the keys (so the logits) change in place
    c2 = make(rng, "bf16", 64, 32, [(3, 1100), (2, 1504), (2, 33)], exact=False)
    assert c2["bt"].shape == c["bt"].shape and c2["k"].shape == c["k"].shape and c2["T"] == c["T"]
    for name, t in dev(c2).items():
        d[name].copy_(t)
    ei, ec = topk_call(fa, c, d, topk)
    torch.cuda.synchronize()
    for _ in range(3):
        idx.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cnt, ec) and all(torch.equal(idx[t, :ec[t]], ei[t, :ec[t]]) for t in range(c["T"]))
