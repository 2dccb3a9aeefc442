"""Far addresses (test side only; Python ints, torch only inside the checker): where every call of tests/test_gpu_far_addresses.py
(cases()) and of tests/test_gpu_far_addresses_mla.py (mla_cases(): the MLA family) puts its tensors, which 32-bit thresholds those
placements cross, and a checker of what a call wrote into a sentinel-filled buffer.

The planner restates the host rules of include/fa_mi355.h and returns, per case, the scalars of the call and, per tensor it touches, the
rows it owns as blocks (start, rows, row length, pitch) in ELEMENTS of the allocation (whose element `base`, 0 unless the tensor is a
view into a wider buffer, is the one the call's pointer names), so that the smallest and largest element and byte offset from that base
follow in exact integers. A case names the thresholds it claims to cross (byte offset 2^31 / 2^32 / 2^33, element offset
2^30 / 2^31 / 2^32); tests/test_far_cases.py holds every claim to the integers, on the CPU.

The checker (footprint) walks an integer view of an output buffer in chunks: every element outside the owned rows must still hold the
sentinel, every owned row must have lost it somewhere. A far owned row that is untouched is looked for at its offset modulo the wrap
modulus (2^32 on the GPU: a truncated 32-bit offset), so that a wrapped store is named, not only noticed."""

BYTE_THRESHOLDS = (1 << 31, 1 << 32, 1 << 33)
ELEM_THRESHOLDS = (1 << 30, 1 << 31, 1 << 32)
ITEMSIZE = {"f32": 4, "f16": 2, "bf16": 2, "fp8": 1, "u8": 1}
GIB = 1 << 30


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
class Tensor:
    """One tensor of a call: `numel` elements of `itemsize` bytes are allocated; the call touches `blocks`, each (start, rows, row_len,
    pitch): `rows` rows of `row_len` contiguous elements, row i at element start + i * pitch of the allocation. role: "load" or "store".
    base: the element of the allocation the call's pointer names (a half-view of a wider buffer: 128); lo / hi and every crossing are
    offsets from it, as the kernel forms them."""

    def __init__(self, name, kind, numel, role, blocks, base=0):
        self.name, self.kind, self.itemsize, self.numel, self.role, self.base = name, kind, ITEMSIZE[kind], int(numel), role, int(base)
        self.blocks = [tuple(int(x) for x in b) for b in blocks]
        assert self.blocks and all(n >= 1 and ln >= 1 and (n == 1 or p >= ln) for _, n, ln, p in self.blocks), name
        self.lo_elem = min(s for s, _, _, _ in self.blocks) - self.base
        self.hi_elem = max(s + (n - 1) * p + ln - 1 for s, n, ln, p in self.blocks) - self.base
        self.lo_byte, self.hi_byte = self.lo_elem * self.itemsize, self.hi_elem * self.itemsize + self.itemsize - 1
        assert 0 <= self.lo_elem and self.base + self.hi_elem < self.numel, (name, "touched outside its allocation", self.hi_elem, self.numel)

    def crosses(self, unit, threshold):
        return (self.hi_byte if unit == "byte" else self.hi_elem) >= threshold

    def crossings(self):
        return [("byte", t) for t in BYTE_THRESHOLDS if self.crosses("byte", t)] + [("elem", t) for t in ELEM_THRESHOLDS if self.crosses("elem", t)]

    def rows_at_or_past(self, unit, threshold):
        """How many touched rows START at or past the threshold."""
        per = self.itemsize if unit == "byte" else 1
        count = 0
        for s, n, _, p in self.blocks:
            s -= self.base
            if n == 1 or p == 0:
                count += n if s * per >= threshold else 0
                continue
            first = max(0, -(-(threshold - s * per) // (p * per)))
            count += max(0, n - first)
        return count

    def nbytes(self):
        return self.numel * self.itemsize


class Plan:
    """One case: `scalars` (everything the call takes besides pointers, and the tables as lists), `tensors` by name, `claims` as
    (tensor name, "byte" | "elem", threshold), `rules` as (text, holds)."""

    def __init__(self, name, scalars, tensors, claims, rules):
        self.name, self.scalars, self.claims, self.rules = name, scalars, list(claims), list(rules)
        self.tensors = {t.name: t for t in tensors}

    def __getitem__(self, key):
        return self.scalars[key]

    def legal(self):
        return all(ok for _, ok in self.rules)

    def device_bytes(self):
        return sum(t.nbytes() for t in self.tensors.values())

    def table(self):
        """case -> tensor -> thresholds, as text lines."""
        def show(c):
            return f"{c[0]} 2^{c[1].bit_length() - 1}"
        lines = [f"{self.name}: {self.device_bytes() / GIB:.2f} GiB placed far"]
        for t in self.tensors.values():
            claimed = [show((u, th)) for n, u, th in self.claims if n == t.name]
            lines.append(f"  {t.name:<10} {t.kind:<4} {t.role:<5} elements {t.lo_elem} .. {t.hi_elem}  bytes {t.lo_byte} .. {t.hi_byte}  crosses "
                         f"{', '.join(show(c) for c in t.crossings()) or 'nothing'}" + (f"  (claimed: {', '.join(claimed)})" if claimed else ""))
        return lines


def stride_rules(what, row_stride, head_stride, D, itemsize=2):
    unit = 16 // itemsize if itemsize == 1 else 8
    return [(f"{what}: strides multiples of {unit} and at least D", row_stride % unit == 0 and head_stride % unit == 0 and min(row_stride, head_stride) >= D)]


def sequence_rule(what, max_seqlen, row_stride):
    return [(f"{what}: (max_seqlen + 128) * row_stride * 2 < 2^32", (max_seqlen + 128) * row_stride * 2 < (1 << 32))]


def grid_rule(blocks):
    return [("the grid fits an int", 0 < blocks < (1 << 31))]


def pool_rules(P, D, ps, hs, rs, itemsize, max_pages):
    unit = 16 if itemsize == 1 else 8
    return [("a page of one head below 2^31 bytes", P * rs * itemsize < (1 << 31)),
            (f"pool strides multiples of {unit} and at least D", all(s % unit == 0 and s >= D for s in (ps, hs, rs))),
            ("capacity at most 2^30", P * max_pages <= (1 << 30))]


def seq_blocks(starts_lens, H, D, row_stride, head_stride):
    """Blocks of the rows that sequences [(first token, rows)] own in a [total, H, D]-addressed tensor: one block per sequence and head."""
    return [(t0 * row_stride + h * head_stride, L, D, row_stride) for t0, L in starts_lens if L for h in range(H)]


L_SEQ, L_LAST = 300, 257  # the clamped first sequence and the last one of a packed far placement


def packed(name, side, layout="THD", dtype="bf16", D=128, Hq=16, Hkv=8, backward=False):
    """Cases A and B: packed sequences with one side far. side "q": q / o (and d_o, dq) hold total_q tokens, above 4 GiB in 16 bits;
    sequence 0 starts at token 0 and is clamped to max_seqlen_q = 300 rows, sequence 1 is the last 257 tokens; K / V are compact. side "kv": the same
    for k / v (and dk, dv) with two sequences of 300 keys, the queries compact. layout "THD" [total, H, D] or "HTD" [H, total, D]."""
    H = Hq if side == "q" else Hkv
    total = (1 << 32) // (H * D * 2) + 512  # 512 tokens past 4 GiB
    last = L_LAST if side == "q" else L_SEQ
    rs, hs = (H * D, D) if layout == "THD" else (D, total * D)
    owned = [(0, L_SEQ), (total - last, last)]
    blocks = seq_blocks(owned, H, D, rs, hs)
    numel = total * H * D
    other = [L_SEQ, L_SEQ] if side == "q" else [L_SEQ, L_LAST]  # the compact side's lengths
    cu_far, cu_near = [0, total - last, total], [0, other[0], other[0] + other[1]]
    sc = dict(side=side, layout=layout, dtype=dtype, D=D, Hq=Hq, Hkv=Hkv, total=total, row_stride=rs, head_stride=hs, owned=owned,
              cu_far=cu_far, cu_near=cu_near, max_far=L_SEQ, max_near=L_SEQ, lens_far=[L_SEQ, last], lens_near=other)
    names = (("q", "load"), ("o", "store")) if side == "q" else (("k", "load"), ("v", "load"))
    if backward:
        names = ((("q", "load"), ("o", "load"), ("d_o", "load")) if side == "q" else names)
    tensors = [Tensor(n, dtype, numel, r, blocks) for n, r in names]
    claims = [(n, "byte", 1 << 32) for n, _ in names] + [(n, "elem", 1 << 31) for n, _ in names]
    if backward:
        g = ("dq",) if side == "q" else ("dk", "dv")
        tensors += [Tensor(n, "f32", numel, "store", blocks) for n in g]
        claims += [(n, "byte", 1 << 33) for n in g]
    Bn = 2
    rules = (stride_rules(side, rs, hs, D) + sequence_rule(side, L_SEQ, rs) + [("max_seqlen <= total", L_SEQ <= total), ("total fits an int", total < (1 << 31))]
             + grid_rule(Bn * Hq * ((L_SEQ + 127) // 128)))
    return Plan(name, sc, tensors, claims, rules)


WIDE_STRIDE = 1 << 22


def wide(name, side, dtype="bf16", D=128, Hq=4, Hkv=2, backward=False):
    """Case C: one sequence of 300 rows under a row stride of 2^22 elements, heads adjacent inside a row: in-sequence offsets of 2 - 4 GiB
    in 16 bits, up to 5 GiB in fp32. side "q", "kv" or "both" (the forward)."""
    L, rs = L_SEQ, WIDE_STRIDE
    numel = L * rs
    tensors, claims, rules = [], [], [("max_seqlen <= total", True)] + grid_rule(Hq * ((L + 127) // 128))
    if side in ("q", "both"):
        blocks = seq_blocks([(0, L)], Hq, D, rs, D)
        names = (("q", "load"), ("o", "load"), ("d_o", "load")) if backward else (("q", "load"), ("o", "store"))
        tensors += [Tensor(n, dtype, numel, r, blocks) for n, r in names]
        claims += [(n, "byte", 1 << 31) for n, _ in names]
        if backward:
            tensors.append(Tensor("dq", "f32", numel, "store", blocks))
            claims += [("dq", "byte", 1 << 31), ("dq", "byte", 1 << 32)]
        rules += stride_rules("q", rs, D, D) + sequence_rule("q", L, rs)
    if side in ("kv", "both"):
        blocks = seq_blocks([(0, L)], Hkv, D, rs, D)
        tensors += [Tensor(n, dtype, numel, "load", blocks) for n in ("k", "v")]
        claims += [(n, "byte", 1 << 31) for n in ("k", "v")]
        if backward:
            tensors += [Tensor(n, "f32", numel, "store", blocks) for n in ("dk", "dv")]
            claims += [(n, "byte", t) for n in ("dk", "dv") for t in (1 << 31, 1 << 32)]
        rules += stride_rules("kv", rs, D, D) + sequence_rule("kv", L, rs)
    sc = dict(side=side, dtype=dtype, D=D, Hq=Hq, Hkv=Hkv, L=L, row_stride=rs, head_stride=D, total=L)
    return Plan(name, sc, tensors, claims, rules)


POOL_LENS = [(130, 700), (40, 300)]  # (new query rows, keys in the cache) per sequence, as the existing 4.5 GiB pool tests


def pool(name, kind, layout, gib_halves, Hkv=8, P=256, D=128, store=False):
    """Cases D, E, F: a pool pair of gib_halves / 2 GiB whose used pages start three pages past ELEMENT offset 2^32. Sequence b's keys
    fill consecutive pages; `store`: the case appends into them (the last n_b keys of every sequence)."""
    isz = ITEMSIZE[kind]
    ps = Hkv * P * D
    hs, rs = (P * D, D) if layout == "HND" else (D, Hkv * D)
    num_pages = (gib_halves << 29) // (ps * isz)
    first = (1 << 32) // ps + 3
    pages, tables, blocks, new_blocks = first, [], [], []
    for n_new, L in POOL_LENS:
        mine = list(range(pages, pages + (L + P - 1) // P))
        pages += len(mine)
        tables.append(mine)
        for j, pg in enumerate(mine):
            n = min(P, L - j * P)
            blocks += [(pg * ps + h * hs, n, D, rs) for h in range(Hkv)]
            lo = max(L - n_new - j * P, 0)  # slots of this page the append writes
            if lo < n:
                new_blocks += [(pg * ps + h * hs + lo * rs, n - lo, D, rs) for h in range(Hkv)]
    max_pages = max(len(t) for t in tables)
    numel = num_pages * ps
    role = "store" if store else "load"
    tensors = [Tensor(n, kind, numel, role, new_blocks if store else blocks) for n in ("k_pages", "v_pages")]
    claims = [(n, u, 1 << 32) for n in ("k_pages", "v_pages") for u in ("byte", "elem")]
    rules = pool_rules(P, D, ps, hs, rs, isz, max_pages) + [("the pages lie inside the pool", pages <= num_pages)]
    sc = dict(kind=kind, layout=layout, Hkv=Hkv, P=P, D=D, num_pages=num_pages, first_page=first, used_pages=pages - first, tables=tables,
              max_pages=max_pages, page_stride=ps, head_stride=hs, row_stride=rs, lens=POOL_LENS)
    return Plan(name, sc, tensors, claims, rules)


def ksplit(name, S=64, Hq=16, Hkv=2, D=128, Lq=16512, Lk=4096, P=256):
    """Case G: the key-split workspace, S * Hq * total_q * (D + 1) floats: o_s [S, Hq, total_q, D] then lse2_s [S, Hq, total_q]."""
    n_o, n_l = S * Hq * Lq * D, S * Hq * Lq
    nbytes = (4 * (n_o + n_l) + 15) // 16 * 16
    tensors = [Tensor("workspace", "f32", nbytes // 4, "store", [(0, S * Hq * Lq, D, D), (n_o, S * Hq, Lq, Lq)])]
    tiles = (Lk + 63) // 64
    rules = (sequence_rule("q", Lq, Hq * D) + stride_rules("q", Hq * D, D, D) + pool_rules(P, D, Hkv * P * D, P * D, D, 2, Lk // P)
             + grid_rule(S * Hq * ((Lq + 127) // 128)) + [("every split owns one tile", tiles == S), ("at most 64 splits", S <= 64)])
    sc = dict(S=S, Hq=Hq, Hkv=Hkv, D=D, Lq=Lq, Lk=Lk, P=P, workspace_bytes=nbytes, o_elems=n_o)
    return Plan(name, sc, tensors, [("workspace", "elem", 1 << 31), ("workspace", "byte", 1 << 33)], rules)


def dense(name, kind, side, D=64, B=2, H=2, N=300, backward=False):
    """Case H: [B, H, N, D] with heads back to back and batch entry 1 one 4 GiB-plus stride behind entry 0: the batch stride is
    2^32 bytes plus 1 MiB in every type. side "both" (the forwards), "q" or "kv" (fa_bwd_ex with that side wide)."""
    isz = ITEMSIZE[kind]
    bs, hs = ((1 << 32) + (1 << 20)) // isz, N * D
    blocks = [(b * bs + h * hs, N, D, D) for b in range(B) for h in range(H)]
    numel = (B - 1) * bs + H * hs
    okind = "bf16" if kind == "fp8" else kind  # o shares q's ELEMENT strides: e4m3's bf16 output lies 8 GiB apart
    tensors, claims = [], []
    q_names = (("q", "load"), ("o", "load"), ("d_o", "load")) if backward else (("q", "load"), ("o", "store"))
    if side in ("q", "both"):
        for n, r in q_names:
            k2 = kind if n == "q" else okind
            tensors.append(Tensor(n, k2, numel, r, blocks))
            claims.append((n, "byte", 1 << 32))
        if backward:
            tensors.append(Tensor("dq", "f32", numel, "store", blocks))
            claims.append(("dq", "byte", 1 << 33))
    if side in ("kv", "both"):
        tensors += [Tensor(n, kind, numel, "load", blocks) for n in ("k", "v")]
        claims += [(n, "byte", 1 << 32) for n in ("k", "v")]
        if backward:
            tensors += [Tensor(n, "f32", numel, "store", blocks) for n in ("dk", "dv")]
            claims += [(n, "byte", 1 << 33) for n in ("dk", "dv")]
    unit = 16 if isz == 1 else 8
    rules = [("strides multiples of 8 (16 for e4m3) and at least D", bs % unit == 0 and hs % unit == 0 and hs >= D),
             ("one head below 4 GiB with the 128-row margin", (N + 128) * D * max(isz, 2) < (1 << 32))] + grid_rule(B * H * ((N + 127) // 128))
    sc = dict(kind=kind, side=side, B=B, H=H, N=N, D=D, batch_stride=bs, head_stride=hs)
    return Plan(name, sc, tensors, claims, rules)


def cases():
    """Every case of tests/test_gpu_far_addresses.py by name."""
    out = [
        packed("A-packed-forward-q-far", "q"),
        packed("A-packed-forward-q-far-head-major-f16", "q", layout="HTD", dtype="f16", D=64),
        packed("B-packed-backward-q-far", "q", backward=True),
        packed("B-packed-backward-kv-far", "kv", backward=True),
    ]
    for dtype, D in (("bf16", 128), ("f16", 64)):
        out += [wide(f"C-wide-forward-{dtype}", "both", dtype, D), wide(f"C-wide-backward-q-{dtype}", "q", dtype, D, backward=True),
                wide(f"C-wide-backward-kv-{dtype}", "kv", dtype, D, backward=True)]
    out += [pool(f"D-e4m3-pool-{lay}", "fp8", lay, 9) for lay in ("HND", "NHD")]
    out += [pool("E-bf16-pool-HND", "bf16", "HND", 17)]
    out += [pool("F-append-e4m3-pool-HND", "fp8", "HND", 9, store=True), pool("F-append-bf16-pool-HND", "bf16", "HND", 17, store=True)]
    out += [ksplit("G-ksplit-workspace")]
    out += [dense(f"H-dense-forward-{k}", k, "both") for k in ("f32", "f16", "bf16", "fp8")]
    out += [dense("H-dense-backward-q-bf16", "bf16", "q", backward=True), dense("H-dense-backward-kv-bf16", "bf16", "kv", backward=True)]
    return {p.name: p for p in out}


# ---- the MLA family: fa_fwd_mla_decode_paged / _wide / _kv8, fa_fwd_varlen_mla, fa_bwd_varlen_mla ------------------------------------------
MLA_DQK, MLA_DV = 576, 512    # the decode: a latent row, and the part of it that is the value
MLA_PQK, MLA_PV = 192, 128    # the prefill and its backward: q / k rows, v / o rows
MLA_ROW = {"q": MLA_PQK, "k": MLA_PQK, "v": MLA_PV, "o": MLA_PV, "d_o": MLA_PV, "dq": MLA_PQK, "dk": MLA_PQK, "dv": MLA_PV}
MLA_IST = 16 * (MLA_DV + 2)   # floats of one 16-row slot of the decode workspace: [16][512] O, then [16][2] (m, l)


def latent_pool_rules(P, ps, rs, itemsize, max_pages):
    """The one-head pool [num_pages, P, 576]: no head stride, so the row stride stands in for it (fa_fwd_decode_paged's rules)."""
    return pool_rules(P, MLA_DQK, ps, rs, rs, itemsize, max_pages)


def decode_stride_rules(what, B, D, bs, hs, rs):
    return [(f"{what}: three strides, multiples of 8, at least D (batch: >= 0 when B = 1)",
             rs >= D and hs >= D and bs >= 0 and (B == 1 or bs >= D) and bs % 8 == 0 and hs % 8 == 0 and rs % 8 == 0)]


def decode_grid_rule(B, Hq, Nq):
    rblk = (Hq * Nq + 15) // 16
    return [("B * Hq * Nq and B * 256 * rblk fit an int", 0 < B * Hq * Nq < (1 << 31) and B * 256 * rblk < (1 << 31))]


def prefill_rules(strides, max_q, max_k, total_q, total_k, B, Hq):
    """fa_fwd_varlen_mla / fa_bwd_varlen_mla: a stride pair and the 4 GiB sequence rule PER TENSOR. strides: name -> (row, head)."""
    out = []
    for n in ("q", "k", "v", "o"):
        rs, hs = strides[n]
        out += stride_rules(n, rs, hs, MLA_ROW[n]) + sequence_rule(n, max_q if n in "qo" else max_k, rs)
    return out + [("max_seqlen <= total", max_q <= total_q and max_k <= total_k), ("totals fit an int", max(total_q, total_k) < (1 << 31))] + \
        grid_rule(B * Hq * ((max_q + 127) // 128))


def mla_packed(name, side, layout="THD", dtype="bf16", Hq=16, Hkv=8, backward=False):
    """Cases M-A and M-B: packed sequences with one side far, as packed(): sequence 0 at token 0, clamped to max_seqlen = 300 rows,
    sequence 1 the last tokens. The forward's token count is set by the NARROWEST row pitch of the far side, 512 tokens past 4 GiB in 16
    bits, so that every tensor of the side crosses byte 2^32 and element 2^31: o's (Hq * 128) on the q side; on the kv side v is the
    upper half of a [total_k, Hkv, 256] buffer (head stride 256, base 128), whose rows are wider than k's, so k's (Hkv * 192).
    The backward's q side is the forward's, with d_o beside o and dq an fp32 store past byte 2^33 (26 GiB). The backward's kv side: v
    is a plain [total_k, Hkv, 128] and k sets the total: k and dk cross 2^32 / 2^33 bytes, v crosses 2^31 and dv 2^32 (20 GiB).
    NOT COVERED: dv past byte 2^33. That needs 2^33 / (8 * 128 * 4) = 2 Mi tokens, at which dk alone is 12 GiB and the case 30 GiB
    before its compact twin and the checker's temporaries: it does not fit under the 32 GiB peak limit, and the limit stays."""
    half_v = side == "kv" and not backward
    H = Hq if side == "q" else Hkv
    width = dict(q=MLA_PQK, o=MLA_PV, k=MLA_PQK, v=2 * MLA_PV if half_v else MLA_PV)
    mine = ("q", "o") if side == "q" else ("k", "v")
    total = (1 << 32) // (H * min(width[n] for n in mine if not (backward and n == "v")) * 2) + 512
    last = L_LAST if side == "q" else L_SEQ
    owned = [(0, L_SEQ), (total - last, last)]
    other = [L_SEQ, L_SEQ] if side == "q" else [L_SEQ, L_LAST]
    strides, base = {}, {}
    for n in mine:
        strides[n] = (H * width[n], width[n]) if layout == "THD" else (width[n], total * width[n])
        base[n] = MLA_PV if (n == "v" and half_v) else 0
    tensors, claims = [], []

    def add(n, like, kind, role, past):
        rs, hs = strides[like]
        blocks = [(s + base[like], r, ln, p) for s, r, ln, p in seq_blocks(owned, H, MLA_ROW[n], rs, hs)]
        tensors.append(Tensor(n, kind, total * H * width[like], role, blocks, base=base[like]))
        claims.extend((n, u, t) for u, t in past)
    both = (("byte", 1 << 32), ("elem", 1 << 31))
    if side == "q":
        add("q", "q", dtype, "load", both)
        add("o", "o", dtype, "load" if backward else "store", both)
        if backward:
            add("d_o", "o", dtype, "load", both)
            add("dq", "q", "f32", "store", (("byte", 1 << 33),))
    else:
        add("k", "k", dtype, "load", both)
        add("v", "v", dtype, "load", (("byte", 1 << 31),) if backward else both)
        if backward:
            add("dk", "k", "f32", "store", (("byte", 1 << 33),))
            add("dv", "v", "f32", "store", (("byte", 1 << 32),))
    near = {n: ((Hq if n in "qo" else Hkv) * MLA_ROW[n], MLA_ROW[n]) for n in ("q", "k", "v", "o")}
    tq, tk = (total, sum(other)) if side == "q" else (sum(other), total)
    rules = prefill_rules({**near, **strides}, L_SEQ, L_SEQ, tq, tk, 2, Hq)
    sc = dict(side=side, layout=layout, dtype=dtype, Hq=Hq, Hkv=Hkv, total=total, strides=strides, base=base, owned=owned, half_v=half_v,
              cu_far=[0, total - last, total], cu_near=[0, other[0], other[0] + other[1]], max_far=L_SEQ, max_near=L_SEQ,
              lens_far=[L_SEQ, last], lens_near=other)
    return Plan(name, sc, tensors, claims, rules)


# four different row strides near 2^22, one per tensor: a load or a store made under a neighbour's stride lands between the rows
MLA_WIDE_STRIDES = {"q": (1 << 22) + 3 * 256, "k": (1 << 22) + 5 * 256, "v": (1 << 22) + 2 * 256, "o": (1 << 22) + 7 * 256}


def mla_wide(name, side, dtype="bf16", Hq=4, Hkv=2, backward=False):
    """Case M-C: one sequence of 300 rows, heads adjacent inside a row, FOUR different row strides near 2^22 elements: in-sequence offsets
    of 2 - 4 GiB in 16 bits, up to 5 GiB in fp32. v is the upper half of a buffer whose heads are 256 wide (head stride 256, base 128).
    side "both" (the forward), "q" or "kv" (the backward with that side wide)."""
    L = L_SEQ
    strides = {n: (MLA_WIDE_STRIDES[n], 2 * MLA_PV if n == "v" else MLA_ROW[n]) for n in ("q", "k", "v", "o")}
    base = {"q": 0, "k": 0, "v": MLA_PV, "o": 0}
    tensors, claims = [], []

    def add(n, like, kind, role, past):
        rs, hs = strides[like]
        H = Hq if like in "qo" else Hkv
        blocks = [(s + base[like], r, ln, p) for s, r, ln, p in seq_blocks([(0, L)], H, MLA_ROW[n], rs, hs)]
        tensors.append(Tensor(n, kind, L * rs, role, blocks, base=base[like]))
        claims.extend((n, "byte", t) for t in past)
    if side in ("q", "both"):
        add("q", "q", dtype, "load", (1 << 31,))
        add("o", "o", dtype, "load" if backward else "store", (1 << 31,))
        if backward:
            add("d_o", "o", dtype, "load", (1 << 31,))
            add("dq", "q", "f32", "store", (1 << 31, 1 << 32))
    if side in ("kv", "both"):
        add("k", "k", dtype, "load", (1 << 31,))
        add("v", "v", dtype, "load", (1 << 31,))
        if backward:
            add("dk", "k", "f32", "store", (1 << 31, 1 << 32))
            add("dv", "v", "f32", "store", (1 << 31, 1 << 32))
    near = {n: ((Hq if n in "qo" else Hkv) * MLA_ROW[n], MLA_ROW[n]) for n in ("q", "k", "v", "o")}
    far_names = {"both": "qkvo", "q": "qo", "kv": "kv"}[side]
    used = {n: (strides[n] if n in far_names else near[n]) for n in near}
    rules = prefill_rules(used, L, L, L, L, 1, Hq) + [("four different row strides", len({s[0] for s in strides.values()}) == 4)]
    sc = dict(side=side, dtype=dtype, Hq=Hq, Hkv=Hkv, L=L, strides=strides, base=base, total=L)
    return Plan(name, sc, tensors, claims, rules)


MLA_POOL_LENS = [700, 300]         # keys per sequence of every pool case (POOL_LENS' key counts)
MLA_POOL_NEW = [130, 40]           # ... of which the append cases write the last ones (POOL_LENS' new rows)
# (Hq, Nq, causal, wide) of the decode calls on the far pools: 16 rows and 32 rows on one-wave items, 32 rows again through the wide call
# (NW = 2), 33 and 128 rows (NW = 4); causal with Nq = 2 in every call. The e4m3 pool takes the rows of the kv8 call.
MLA_POOL_CALLS = {"bf16": [(8, 2, True, False), (16, 2, True, False), (16, 2, True, True), (33, 1, False, True), (64, 2, True, True)],
                  "fp8": [(8, 2, True, None), (33, 1, False, None), (64, 2, True, None)]}


def mla_pool(name, kind, gib_halves, rs=MLA_DQK, pad_page=False, P=256, store=False):
    """Cases M-D and M-F: ONE latent pool [num_pages, P, 576] of gib_halves / 2 GiB whose used pages start three pages past ELEMENT
    offset 2^32, as pool(). rs: the row stride (640: padded rows); pad_page: a page stride of one row more than P. store: the case
    appends the last MLA_POOL_NEW keys of every sequence."""
    isz = ITEMSIZE[kind]
    ps = (P + (1 if pad_page else 0)) * rs
    num_pages = (gib_halves << 29) // (ps * isz)
    first = (1 << 32) // ps + 3
    pages, tables, blocks, new_blocks = first, [], [], []
    for n_new, L in zip(MLA_POOL_NEW, MLA_POOL_LENS):
        mine = list(range(pages, pages + (L + P - 1) // P))
        pages += len(mine)
        tables.append(mine)
        for j, pg in enumerate(mine):
            n = min(P, L - j * P)
            blocks.append((pg * ps, n, MLA_DQK, rs))
            lo = max(L - n_new - j * P, 0)
            if lo < n:
                new_blocks.append((pg * ps + lo * rs, n - lo, MLA_DQK, rs))
    max_pages = max(len(t) for t in tables)
    tensors = [Tensor("kv_pages", kind, num_pages * ps, "store" if store else "load", new_blocks if store else blocks)]
    claims = [("kv_pages", u, 1 << 32) for u in ("byte", "elem")]
    rules = latent_pool_rules(P, ps, rs, isz, max_pages) + [("the pages lie inside the pool", pages + 1 <= num_pages)]
    for Hq, Nq, _, _ in MLA_POOL_CALLS[kind]:
        rules += decode_grid_rule(len(MLA_POOL_LENS), Hq, Nq)
    sc = dict(kind=kind, P=P, num_pages=num_pages, first_page=first, used_pages=pages - first, tables=tables, max_pages=max_pages,
              page_stride=ps, row_stride=rs, pad_page=pad_page, lens=MLA_POOL_LENS, new=MLA_POOL_NEW, calls=MLA_POOL_CALLS[kind])
    return Plan(name, sc, tensors, claims, rules)


def mla_batch(name, call, token_major, Hq, Nq):
    """Case M-H: q and o of a decode call with batch entry 1 lying 2^32 bytes plus 1 MiB behind entry 0, for q and independently for o.
    Head-major [B, Hq, Nq, D] with rows back to back, or token-major [B, Nq, Hq, D] where o's rows are 576 apart (the first 512 columns
    of a [B, Nq, Hq, 576] buffer): rows of 512 are written, never 576. The pool is small and compact."""
    B, R = 2, Hq * Nq
    bs = ((1 << 32) + (1 << 20)) // 2
    o_row = MLA_DQK if token_major else MLA_DV
    q_st = (bs, MLA_DQK, Hq * MLA_DQK) if token_major else (bs, Nq * MLA_DQK, MLA_DQK)
    o_st = (bs, o_row, Hq * o_row) if token_major else (bs, Nq * o_row, o_row)
    tensors = [Tensor("q", "bf16", bs + R * MLA_DQK, "load", [(b * bs, R, MLA_DQK, MLA_DQK) for b in range(B)]),
               Tensor("o", "bf16", bs + R * o_row, "store", [(b * bs, R, MLA_DV, o_row) for b in range(B)])]
    rules = (decode_stride_rules("q", B, MLA_DQK, *q_st) + decode_stride_rules("o", B, MLA_DV, *o_st) + decode_grid_rule(B, Hq, Nq)
             + [("the row count fits the call", R <= (32 if call == "one" else 128))])
    sc = dict(call=call, token_major=token_major, B=B, Hq=Hq, Nq=Nq, q_strides=q_st, o_strides=o_st, batch_stride=bs, o_row=o_row,
              lens=MLA_POOL_LENS, P=64)
    return Plan(name, sc, tensors, [("q", "byte", 1 << 32), ("o", "byte", 1 << 32)], rules)


def mla_workspace(name, B=32768, Hq=64, Nq=2, P=256, o_row=520):
    """Case M-G: the wide decode's workspace, B * S * rows16 * 514 floats, above 2^31 floats: 128 packed rows and B = 32768, where the
    split rule gives S = 1 (the test takes S from the library's size function and asserts it). All but three sequences are empty; the
    live ones lie at batch indices whose workspace slots start past element 2^31 and whose q and o rows start past byte 2^32 (o's rows
    are 520 elements apart: back to back, entry 32767 would end exactly at byte 2^32). The grid rule B * 256 * rblk < 2^31 and the peak
    limit both admit this shape: neither rows16 nor B was shrunk."""
    R = Hq * Nq
    rows16 = 16 * ((R + 15) // 16)
    S = 1
    live = {0: 300, 32700: 700, 32767: 257}  # batch index -> keys
    ws = B * S * rows16 * (MLA_DV + 2)
    q_st, o_st = (R * MLA_DQK, Nq * MLA_DQK, MLA_DQK), (R * o_row, Nq * o_row, o_row)
    tensors = [Tensor("workspace", "f32", ws, "store", [(0, B * S * rows16 // 16, MLA_IST, MLA_IST)]),
               Tensor("q", "bf16", B * R * MLA_DQK, "load", [(b * q_st[0], R, MLA_DQK, MLA_DQK) for b in live]),
               Tensor("o", "bf16", B * R * o_row, "store", [(0, B * R, MLA_DV, o_row)])]
    far_live = [b for b in live if b]
    rules = (decode_stride_rules("q", B, MLA_DQK, *q_st) + decode_stride_rules("o", B, MLA_DV, *o_st) + decode_grid_rule(B, Hq, Nq)
             + latent_pool_rules(P, P * MLA_DQK, MLA_DQK, 2, 3)
             + [("the far live sequences' slots start past element 2^31", all(b * S * rows16 * (MLA_DV + 2) >= (1 << 31) for b in far_live)),
                ("... and their q and o rows past byte 2^32", all(b * q_st[0] * 2 >= (1 << 32) and b * o_st[0] * 2 >= (1 << 32) for b in far_live))])
    sc = dict(B=B, Hq=Hq, Nq=Nq, P=P, S=S, rows16=rows16, live=live, q_strides=q_st, o_strides=o_st, o_row=o_row, workspace_bytes=4 * ws,
              max_pages=3)
    claims = [("workspace", "elem", 1 << 31), ("workspace", "byte", 1 << 33), ("q", "byte", 1 << 32), ("o", "byte", 1 << 32)]
    return Plan(name, sc, tensors, claims, rules)


def mla_cases():
    """Every case of tests/test_gpu_far_addresses_mla.py by name."""
    out = [
        mla_packed("M-A-prefill-q-far", "q"),
        mla_packed("M-A-prefill-kv-far", "kv"),
        mla_packed("M-A-prefill-q-far-head-major-f16", "q", layout="HTD", dtype="f16"),
        mla_packed("M-A-prefill-kv-far-head-major-f16", "kv", layout="HTD", dtype="f16"),
        mla_packed("M-B-backward-q-far", "q", backward=True),
        mla_packed("M-B-backward-kv-far", "kv", backward=True),
    ]
    for dtype in ("bf16", "f16"):
        out += [mla_wide(f"M-C-wide-forward-{dtype}", "both", dtype), mla_wide(f"M-C-wide-backward-q-{dtype}", "q", dtype, backward=True),
                mla_wide(f"M-C-wide-backward-kv-{dtype}", "kv", dtype, backward=True)]
    out += [mla_pool("M-D-bf16-pool", "bf16", 17), mla_pool("M-D-bf16-pool-padded", "bf16", 17, rs=640, pad_page=True),
            mla_pool("M-D-e4m3-pool", "fp8", 9)]
    out += [mla_pool("M-F-append-bf16-pool", "bf16", 17, store=True), mla_pool("M-F-append-e4m3-pool", "fp8", 9, store=True)]
    out += [mla_workspace("M-G-wide-workspace")]
    for call, Hq, Nq in (("one", 16, 2), ("wide", 64, 2), ("kv8", 33, 2)):
        out += [mla_batch(f"M-H-decode-{call}-{'token' if tm else 'head'}-major", call, tm, Hq, Nq) for tm in (False, True)]
    return {p.name: p for p in out}


# ---- the footprint checker -----------------------------------------------------------------------------------------------------------------
class Report:
    """outside: (count, first positions) of elements outside the owned rows that lost the sentinel; untouched: per owned row that still
    holds it entirely (start, offset from the base, that offset modulo the modulus or None for a near row, data found there)."""

    def __init__(self):
        self.outside_count, self.outside, self.untouched = 0, [], []

    @property
    def ok(self):
        return self.outside_count == 0 and not self.untouched

    def describe(self):
        out = []
        if self.outside_count:
            out.append(f"{self.outside_count} elements written outside the owned rows, first at {self.outside[:8]}")
        for start, off, wrapped, found in self.untouched[:8]:
            msg = f"owned row at element {start} (offset {off} from the base) untouched"
            if wrapped is not None:
                msg += f"; offset mod modulus = {wrapped}: " + ("the data sits there: a wrapped store" if found else "nothing written there either")
            out.append(msg)
        if len(self.untouched) > 8:
            out.append(f"... and {len(self.untouched) - 8} more untouched rows")
        return "; ".join(out) or "clean"


def _rows_in(block, c0, c1):
    """(first row, rows) of the block's rows that lie wholly inside [c0, c1)."""
    s, n, ln, p = block
    if n == 1:
        return (0, 1) if c0 <= s and s + ln <= c1 else (0, 0)
    i0 = max(0, -(-(c0 - s) // p))
    i1 = min(n, (c1 - ln - s) // p + 1) if c1 - ln - s >= 0 else 0
    return i0, max(0, i1 - i0)


def _straddler(block, c):
    """Start of the block's row that element position c cuts in two, or None."""
    s, n, ln, p = block
    if c <= s:
        return None
    i = min((c - s) // p, n - 1) if n > 1 else 0
    r = s + i * p
    return r if r < c < r + ln else None


def footprint(buf, sentinel, blocks, modulus=1 << 32, base=0, chunk=1 << 27, keep=64):
    """buf: a flat integer view of a whole allocation that was filled with `sentinel` before the call; blocks: the owned rows, (start,
    rows, row_len, pitch) in elements of buf, disjoint; base: the element of buf the call's pointer named (offsets wrap relative to
    it); modulus: the wrap to look for, in ELEMENTS of buf, or several of them (a 32-bit byte offset wraps at 2^32 / itemsize elements, a
    32-bit element offset at 2^32): the one at which the data is found is named, else the first. Works chunk by chunk: temporaries are
    chunk-sized booleans."""
    import torch

    assert buf.dim() == 1 and buf.is_contiguous()
    moduli = (modulus,) if isinstance(modulus, int) else tuple(modulus)
    blocks = [tuple(int(x) for x in b) for b in blocks]
    n, rep, c0 = buf.numel(), Report(), 0
    while c0 < n:
        c1 = min(c0 + chunk, n)
        moved = True
        while moved and c1 < n:  # never cut an owned row in two
            moved = False
            for b in blocks:
                r = _straddler(b, c1)
                if r is not None:
                    assert r > c0, "an owned row longer than a chunk"
                    c1, moved = r, True
        ne = buf[c0:c1] != sentinel
        for b in blocks:
            i0, rows = _rows_in(b, c0, c1)
            if not rows:
                continue
            s, _, ln, p = b
            view = ne.as_strided((rows, ln), (p if rows > 1 else ln, 1), s + i0 * p - c0)
            idle = torch.nonzero(~view.any(1)).flatten().tolist()
            for i in idle:
                start = s + (i0 + i) * p
                off = start - base
                wrapped, found = None, False
                for m in moduli:
                    if found or 0 <= off < m:
                        continue
                    w = base + off % m
                    found = bool(0 <= w and w + ln <= n and (buf[w:w + ln] != sentinel).any())
                    wrapped = off % m if found or wrapped is None else wrapped
                rep.untouched.append((start, off, wrapped, found))
            view.fill_(False)
        if bool(ne.any()):
            idx = torch.nonzero(ne).flatten()
            rep.outside_count += idx.numel()
            rep.outside += (idx[:max(0, keep - len(rep.outside))] + c0).tolist()
        del ne
        c0 = c1
    return rep
