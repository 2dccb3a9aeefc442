"""The cases of fa_fwd_varlen_paged / fa_kv_append_paged (pure numpy; shared by tests/test_varlen_paged_cases.py on the CPU, which checks
that every case is what it claims to be, and tests/test_gpu_varlen_paged.py on the GPU).

The edges: the page (16 slots, and 64 / 256), the 64-key tile, the 128-row block and its four 32-row waves. BASE is the batch every
parity / identity test runs, in this order; Lq_b queries against a cache of L_b keys (the chunk already appended)."""
import numpy as np

TILE, BLOCK, WAVE = 64, 128, 32
PAGE_SIZES = (16, 64, 256)
HEADS = ((4, 4), (8, 2), (4, 1))  # (Hq, Hkv)
BASE = (
    (1, 1),       # smallest case
    (17, 17),     # just past the 16-slot page
    (33, 15),     # causal: rows 0-17 see no key; a partial first page
    (64, 200),    # 64-key tile edge
    (129, 129),   # a second block that holds one row
    (130, 401),   # the last key alone in its page at P = 16
    (5, 0),       # no keys
    (0, 77),      # no queries
    (128, 1024),  # sixteen tiles: the table prefetch across many pages
)


def dead_rows(Lq, L, causal):
    """Rows 0 .. dead-1 of a sequence see no key: all of them without keys; under the mask (key j visible to query i iff
    j <= i + L - Lq) the first Lq - L."""
    if L == 0:
        return Lq
    return max(Lq - L, 0) if causal else 0


def identity_claimed(Lq, L, causal):
    """The header's bit-identity to fa_fwd_varlen on the gathered cache: L >= Lq >= 1 under the mask, both >= 1 without."""
    return Lq >= 1 and (L >= Lq if causal else L >= 1)


def draw(round_to, rng, dtype, *shape):
    return round_to(rng.uniform(-1.0, 1.0, shape).astype(np.float32), dtype)


def draw_seqs(round_to, rng, Hq, Hkv, D, dtype, lens):
    """[(q [Hq, Lq, D], k [Hkv, L, D], v [Hkv, L, D])]: fp32 arrays that hold values of `dtype`."""
    return [(draw(round_to, rng, dtype, Hq, Lq, D), draw(round_to, rng, dtype, Hkv, L, D), draw(round_to, rng, dtype, Hkv, L, D)) for Lq, L in lens]


def pack_rows(xs, tail=0):
    """[H, n_b, D] per sequence -> ([total + tail, H, D], cu [B + 1]); the tail tokens belong to nobody (zeros)."""
    H, _, D = xs[0].shape
    rows = np.concatenate([x.transpose(1, 0, 2) for x in xs] + [np.zeros((tail, H, D), np.float32)])
    return rows, np.cumsum([0] + [x.shape[1] for x in xs]).astype(np.int32)


def pages_of(L, P):
    return (L + P - 1) // P


def build_pool(ks, vs, P, rng=None, spare=2, max_pages=None, fill=np.nan, unused="spare"):
    """The logical caches ks / vs ([Hkv, L_b, D] each) laid into pools [num_pages, Hkv, P, D] (HND, fp32) and a block table
    [B, max_pages]. rng: the pool's pages are dealt in a random order (None: in table order, sequence after sequence). `spare` pages at the
    end of the deal belong to nobody. Whatever no key occupies -- slots >= L_b of a last page, the spare pages -- holds `fill`.
    Table entries past a sequence's last page (`unused`): "spare" names a spare page, "minus1" -1, "beyond" num_pages, "zero" page 0.
    Returns dict(k, v, table, pages=[page ids per sequence], spare=[ids], num_pages, P)."""
    Hkv, _, D = ks[0].shape
    npb = [pages_of(k.shape[1], P) for k in ks]
    mp = max_pages or max(max(npb), 1)
    assert mp >= max(npb) and spare >= 1
    num_pages = sum(npb) + spare
    order = np.arange(num_pages) if rng is None else rng.permutation(num_pages)
    kpool = np.full((num_pages, Hkv, P, D), fill, np.float32)
    vpool = np.full((num_pages, Hkv, P, D), fill, np.float32)
    spare_ids = [int(x) for x in order[sum(npb):]]
    filler = {"spare": spare_ids[-1], "minus1": -1, "beyond": num_pages, "zero": 0}[unused]
    table = np.full((len(ks), mp), filler, np.int32)
    pages, used = [], 0
    for b, (k, v) in enumerate(zip(ks, vs)):
        ids = order[used:used + npb[b]]
        used += npb[b]
        table[b, :npb[b]] = ids
        for j, pg in enumerate(ids):
            n = min(P, k.shape[1] - j * P)
            kpool[pg, :, :n] = k[:, j * P:j * P + n]
            vpool[pg, :, :n] = v[:, j * P:j * P + n]
        pages.append([int(x) for x in ids])
    return dict(k=kpool, v=vpool, table=table, pages=pages, spare=spare_ids, num_pages=num_pages, P=P)


def gather(pool, row, L, P):
    """Keys 0 .. L-1 of one sequence out of an HND pool through its table row, as the header defines it: key j is slot j % P of page
    row[j // P]; a page index outside the pool reads as zeros. -> [Hkv, L, D]."""
    num_pages, Hkv, _, D = pool.shape
    out = np.zeros((Hkv, L, D), np.float32)
    for j in range(L):
        pg = int(row[j // P])
        if 0 <= pg < num_pages:
            out[:, j] = pool[pg, :, j % P]
    return out


def append_positions(n, L_after, cap):
    """Key positions of the n new tokens of a sequence whose length after the append is L_after; None where the contract skips one
    (below 0, at or above the capacity)."""
    return [(p if 0 <= p < cap else None) for p in range(L_after - n, L_after)]


def chunks(total, size):
    """(start, n) of the chunks of a prompt of `total` tokens fed `size` at a time."""
    return [(s, min(size, total - s)) for s in range(0, total, size)]
