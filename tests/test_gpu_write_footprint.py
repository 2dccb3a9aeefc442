"""What the library writes, and nothing else: sentinels around every output, LSE and workspace of the C-ABI (include/fa_mi355.h).

Every output lives inside a larger allocation filled with one bit pattern (compared as integers: the patterns are NaNs): a guard
block in front of the base pointer, `PAD` spare rows behind row N of every head, a spare head per batch entry, a guard behind the last
element. After the call no element of the output proper holds the pattern, and EVERY element outside it still does. LSE and the
workspaces get a guard in front and one behind B*H*N floats / the size their *_workspace_bytes() function returns. Inputs sit in
the same kind of padded buffer (the pattern in their padding) and are compared with clones taken before the call. A store past row N
of a head that the owning workgroup of the next head overwrites -- invisible to a parity test -- lands in the spare rows here.
All allocations are real and as large as the sizes passed: nothing here can fault. test_checker_reports_a_row_declared_missing shows on
the test side that the checker sees a single row.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD, GUARD = 8, 2048  # spare rows per head; guard elements in front of and behind a buffer (a multiple of 16 bytes for every type)
KIND = {  # name -> (torch dtype name, integer view, sentinel)
    "f32": ("float32", "int32", 0x7FC5A5A5), "f16": ("float16", "int16", 0x7E5A), "bf16": ("bfloat16", "int16", 0x7FA5),
    "fp8": ("float8_e4m3fn", "int8", 0x7F), "u8": ("uint8", "uint8", 0xA5), "i32": ("int32", "int32", 0x5A5A5A5A),
}
FA_DTYPE = {"f32": 0, "f16": 1, "bf16": 2, "fp8": 3}
OUT_KIND = {"f32": "f32", "f16": "f16", "bf16": "bf16", "fp8": "bf16"}
VARIANTS = {"auto": 0, "naive": 1, "tiled": 2, "tiled_v2": 3, "mfma": 4, "mfma_pp": 5, "mfma_splitkv": 6, "mfma_split2": 7,
            "mfma_exact": 8, "mfma_h64s2": 9, "mfma16": 10, "mfma_fp8pv": 11}


@pytest.fixture(scope="module")
def lib():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available()
    return fa.load_library()


class Guarded:
    """A tensor of `shape` ([B,H,N,D]: padded rows and a spare head; anything else: flat) inside a sentinel-filled allocation."""

    def __init__(self, kind, shape, values=None, pad=PAD, spare=1):
        import torch

        tname, iname, self.sentinel = KIND[kind]
        idt = getattr(torch, iname)
        if len(shape) == 4:
            B, H, N, D = shape
            outer = (B, H + spare, N + pad, D)
        else:
            outer = (int(np.prod(shape)),)
        n = int(np.prod(outer))
        self.raw = torch.full((GUARD + n + GUARD,), self.sentinel, dtype=idt, device="cuda")
        body = self.raw[GUARD:GUARD + n].view(outer)
        self.ints = body[:, :shape[1], :shape[2]] if len(shape) == 4 else body
        self.t = self.ints.view(getattr(torch, tname))  # the tensor proper (a view)
        self.inside = torch.zeros_like(self.raw, dtype=torch.bool)
        ins = self.inside[GUARD:GUARD + n].view(outer)
        (ins[:, :shape[1], :shape[2]] if len(shape) == 4 else ins).fill_(True)
        self.outer, self.shape = outer, tuple(shape)
        if values is not None:
            self.t.copy_(values.to(self.t.dtype) if hasattr(values, "to") else torch.from_numpy(np.ascontiguousarray(values)).to(self.t.dtype))
        self.before = self.raw.clone()

    def ptr(self):
        return self.t.data_ptr()

    def strides(self):
        """(batch stride, head stride) in elements."""
        _, H1, N1, D = self.outer
        return H1 * N1 * D, N1 * D

    def where(self, idx):
        """flat raw indices -> a short description (guard / (b, h, row) of the padded layout)."""
        out = []
        for i in idx[:6].tolist():
            j = i - GUARD
            if j < 0 or j >= int(np.prod(self.outer)):
                out.append(f"guard{'-front' if j < 0 else '-back'}[{j if j < 0 else j - int(np.prod(self.outer))}]")
            elif len(self.outer) == 4:
                _, H1, N1, D = self.outer
                out.append(f"(b{j // (H1 * N1 * D)}, h{j // (N1 * D) % H1}, row{j // D % N1}, d{j % D})")
            else:
                out.append(f"[{j}]")
        return out

    def touched_outside(self, inside=None):
        """raw indices outside the region whose bits changed."""
        import torch

        inside = self.inside if inside is None else inside
        return torch.nonzero((self.raw != self.sentinel) & ~inside).flatten()

    def unwritten_inside(self):
        import torch

        return torch.nonzero((self.raw == self.sentinel) & self.inside).flatten()

    def check_written(self, what, full=True):
        """An output: everything outside untouched; with full=True no element inside still holds the sentinel."""
        import torch

        torch.cuda.synchronize()
        out = self.touched_outside()
        assert out.numel() == 0, (what, "wrote outside its output", out.numel(), self.where(out))
        if full:
            un = self.unwritten_inside()
            assert un.numel() == 0, (what, "left output elements unwritten", un.numel(), self.where(un))

    def check_unchanged(self, what):
        """An input (or a refused call's output): bit-identical to what it held before the call."""
        import torch

        torch.cuda.synchronize()
        assert torch.equal(self.raw, self.before), (what, "was modified", self.where(torch.nonzero(self.raw != self.before).flatten()))


def rand_in(kind, shape, seed, amp=1.0):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    return Guarded(kind, shape, (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * amp)


def no_nan(gd, what):
    import torch

    assert not torch.isnan(gd.t.float()).any(), (what, "NaN in the output: the inputs' padding was read")


def test_checker_reports_a_row_declared_missing(lib):
    """The checker itself: fa_fwd writes N rows per head; told that the output has N - 1, it reports exactly row N - 1 of every head."""
    import torch

    B, H, N, D = 2, 3, 129, 64
    q, k, v = (rand_in("bf16", (B, H, N, D), s) for s in (1, 2, 3))
    o, lse = Guarded("bf16", (B, H, N, D)), Guarded("f32", (B * H * N,))
    bs, hs = q.strides()
    assert lib.fa_fwd(q.ptr(), k.ptr(), v.ptr(), o.ptr(), lse.ptr(), B, H, N, D, D ** -0.5, bs, hs, 1, 2, 0, None) == 0
    o.check_written("fa_fwd")
    short = torch.zeros_like(o.inside)
    short[GUARD:GUARD + int(np.prod(o.outer))].view(o.outer)[:, :H, :N - 1] = True
    idx = o.touched_outside(short)
    assert idx.numel() == B * H * D
    j = idx - GUARD
    _, H1, N1, _ = o.outer
    assert (j // D % N1 == N - 1).all() and (j // (N1 * D) % H1 < H).all()
    lshort = torch.zeros_like(lse.inside)
    lshort[GUARD:GUARD + B * H * N - 1] = True
    assert lse.touched_outside(lshort).tolist() == [GUARD + B * H * N - 1]


NS = (1, 63, 129, 200, 333)


@pytest.mark.parametrize("D", [8, 32, 40, 64, 96, 120, 128, 256])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16", "fp8"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fa_fwd_footprint(lib, variant, dtype, D):
    ok = lib.fa_supported(FA_DTYPE[dtype], VARIANTS[variant], D)
    B, H = 2, 3
    for n, N in enumerate(NS if ok else (129,)):
        for causal in ((0, 1) if ok else (1,)):
            q, k, v = (rand_in(dtype, (B, H, N, D), 10 * n + s) for s in (1, 2, 3))
            o, lse = Guarded(OUT_KIND[dtype], (B, H, N, D)), Guarded("f32", (B * H * N,))
            bs, hs = q.strides()
            st = lib.fa_fwd(q.ptr(), k.ptr(), v.ptr(), o.ptr(), lse.ptr(), B, H, N, D, D ** -0.5, bs, hs, causal, FA_DTYPE[dtype],
                            VARIANTS[variant], None)
            what = ("fa_fwd", variant, dtype, D, N, causal)
            if not ok:  # no kernel (or, for e4m3, a head stride that is no multiple of 16): refused, and nothing written
                assert st < 0, what
                o.check_unchanged(what)
                lse.check_unchanged(what)
                continue
            assert st == 0, (what, lib.fa_last_error())
            o.check_written(what)
            lse.check_written(what)
            no_nan(o, what)
            for x in (q, k, v):
                x.check_unchanged(what)


@pytest.mark.parametrize("D", [8, 40, 64, 120, 128, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "fp8"])
@pytest.mark.parametrize("variant", ["auto", "mfma", "mfma_exact", "mfma16", "mfma_splitkv"])
def test_fa_fwd_exv_footprint(lib, variant, dtype, D):
    """Grouped heads and Nq != Nk; a combination without a kernel is refused and writes nothing."""
    served = 0
    for (B, Hq, Hkv, Nq, Nk, causal) in ((2, 4, 2, 63, 129, 1), (1, 6, 1, 200, 333, 1), (2, 2, 2, 129, 63, 0), (1, 8, 2, 1, 200, 0), (1, 2, 1, 333, 333, 1)):
        q = rand_in(dtype, (B, Hq, Nq, D), 1)
        k, v = (Guarded(dtype, (B, Hkv, Nk, D), rand_in(dtype, (B, Hkv, Nk, D), s).t, pad=24, spare=2) for s in (2, 3))
        o, lse = Guarded(OUT_KIND[dtype], (B, Hq, Nq, D)), Guarded("f32", (B * Hq * Nq,))
        st = lib.fa_fwd_exv(q.ptr(), k.ptr(), v.ptr(), o.ptr(), lse.ptr(), B, Hq, Hkv, Nq, Nk, D, D ** -0.5, *q.strides(), *k.strides(),
                            causal, FA_DTYPE[dtype], VARIANTS[variant], None)
        what = ("fa_fwd_exv", variant, dtype, D, (B, Hq, Hkv, Nq, Nk), causal)
        if st != 0:  # refused (no kernel for the combination; e4m3 under a head stride that is no multiple of 16): nothing written
            assert st < 0, (what, st, lib.fa_last_error())
            o.check_unchanged(what)
            lse.check_unchanged(what)
            continue
        served += 1
        o.check_written(what)
        lse.check_written(what)
        no_nan(o, what)
        for x in (q, k, v):
            x.check_unchanged(what)
    # what the header promises: auto serves every f16 / bf16 multiple of 8 up to 128 and 256 (e4m3: 64, 128, 256); the 128-row kernel by
    # name 64, 128, 256 (the head dims on zero-padded rows belong to the 16x16x32 kernel)
    if (variant == "auto" and (dtype != "fp8" or D in (64, 128, 256))) or (variant == "mfma" and D in (64, 128, 256)):
        assert served == 5, (variant, dtype, D, served)


DECODE_SHAPES = [(2, 32, 8, 1, 333), (1, 16, 2, 2, 1000), (3, 8, 8, 4, 63), (1, 4, 1, 7, 4097), (2, 8, 4, 1, 1)]  # B, Hq, Hkv, Nq, Nk


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", ["f16", "bf16", "fp8", "kv8"])
def test_fa_fwd_decode_footprint(lib, mode, D):
    for (B, Hq, Hkv, Nq, Nk) in DECODE_SHAPES:
        for causal in (0, 1):
            if causal and Nk < Nq:
                continue
            qk, kk = ("bf16", "fp8") if mode == "kv8" else (mode, mode)
            q = rand_in(qk, (B, Hq, Nq, D), 1)
            k, v = (rand_in(kk, (B, Hkv, Nk, D), s) for s in (2, 3))
            o, lse = Guarded(OUT_KIND[qk], (B, Hq, Nq, D)), Guarded("f32", (B * Hq * Nq,))
            need = lib.fa_fwd_decode_workspace_bytes(B, Hq, Hkv, Nq, Nk, D)
            assert need > 0
            ws = Guarded("u8", (need,))
            fn = lib.fa_fwd_decode_kv8 if mode == "kv8" else lib.fa_fwd_decode
            st = fn(q.ptr(), k.ptr(), v.ptr(), o.ptr(), lse.ptr(), B, Hq, Hkv, Nq, Nk, D, D ** -0.5, *q.strides(), *k.strides(), causal,
                    FA_DTYPE[qk], ws.ptr(), need, None)
            what = ("fa_fwd_decode", mode, D, (B, Hq, Hkv, Nq, Nk), causal)
            assert st == 0, (what, lib.fa_last_error())
            o.check_written(what)
            lse.check_written(what)
            ws.check_written(what, full=False)
            no_nan(o, what)
            for x in (q, k, v):
                x.check_unchanged(what)


@pytest.mark.parametrize("P", [16, 64, 256])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mode", ["f16", "bf16", "fp8", "kv8"])
def test_fa_fwd_decode_paged_footprint(lib, mode, D, P):
    """Mixed lengths, an empty sequence, a page index outside the pool in a slot that is used: O, LSE and the workspace tail are
    written and nothing else; both pools, the table and the lengths are bit-identical afterwards."""
    import torch

    qk, kk = ("bf16", "fp8") if mode == "kv8" else (mode, mode)
    rng = np.random.default_rng(P + D)
    for (Hq, Hkv, Nq, layout) in ((16, 4, 1, "HND"), (8, 2, 3, "NHD")):
        lens = [0, 1, P + 1, 333, 1000, 5 * P - 1]
        B = len(lens)
        mp = max((L + P - 1) // P for L in lens) + 1
        num_pages = sum((L + P - 1) // P for L in lens) + 2
        table = rng.integers(0, num_pages, (B, mp)).astype(np.int32)
        table[3, 0] = num_pages + 7  # used slots naming pages outside the pool: read as zeros
        table[4, 1] = -1
        shape = (num_pages, Hkv, P, D) if layout == "HND" else (num_pages, P, Hkv, D)
        kp, vp = (rand_in(kk, (int(np.prod(shape)),), s) for s in (2, 3))
        ps = Hkv * P * D
        hs, rs = (P * D, D) if layout == "HND" else (D, Hkv * D)
        tb = Guarded("i32", (B * mp,), table.reshape(-1))
        sl = Guarded("i32", (B,), np.asarray(lens, np.int32))
        for causal in (0, 1):
            q = rand_in(qk, (B, Hq, Nq, D), 1)
            o, lse = Guarded(OUT_KIND[qk], (B, Hq, Nq, D)), Guarded("f32", (B * Hq * Nq,))
            need = lib.fa_fwd_decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp)
            assert need > 0
            ws = Guarded("u8", (need,))
            st = lib.fa_fwd_decode_paged(q.ptr(), kp.ptr(), vp.ptr(), o.ptr(), lse.ptr(), tb.ptr(), sl.ptr(), B, Hq, Hkv, Nq, D, P, num_pages,
                                         mp, D ** -0.5, *q.strides(), ps, hs, rs, mp, causal, FA_DTYPE[qk], FA_DTYPE[kk], ws.ptr(), need, None)
            what = ("fa_fwd_decode_paged", mode, D, P, layout, causal)
            assert st == 0, (what, lib.fa_last_error())
            o.check_written(what)
            lse.check_written(what)
            ws.check_written(what, full=False)
            no_nan(o, what)
            assert torch.isneginf(lse.t.view(B, Hq, Nq)[0]).all() and (o.t[0].float() == 0).all(), what  # L_b = 0: O = 0, LSE = -inf
            for x in (q, kp, vp, tb, sl):
                x.check_unchanged(what)


def _bwd_case(lib, dtype, B, Hq, Hkv, Nq, Nk, D, causal, ex, exact_ws):
    import torch

    odt = OUT_KIND[dtype]
    amp = 2.0 if dtype == "fp8" else 1.0
    q, o_, do = rand_in(dtype, (B, Hq, Nq, D), 1, amp), rand_in(odt, (B, Hq, Nq, D), 4, 0.3), rand_in(odt, (B, Hq, Nq, D), 5)
    k, v = (Guarded(dtype, (B, Hkv, Nk, D), rand_in(dtype, (B, Hkv, Nk, D), s, amp).t, pad=8 if not ex else 24, spare=1 if not ex else 2)
            for s in (2, 3))
    lse = Guarded("f32", (B * Hq * Nq,), torch.full((B * Hq * Nq,), float(np.log(Nk)), device="cuda"))
    dq = Guarded("f32", (B, Hq, Nq, D))
    dk, dv = (Guarded("f32", (B, Hkv, Nk, D), pad=k.outer[2] - Nk, spare=k.outer[1] - Hkv) for _ in range(2))
    need = lib.fa_bwd_workspace_bytes_ex(FA_DTYPE[dtype], B, Hq, Hkv, Nq, Nk, D, *q.strides(), *k.strides())
    if exact_ws:  # f16 / bf16: the header asks for fa_bwd_workspace_bytes(B, Hq, Nq) = B*Hq*Nq floats, no more
        assert dtype != "fp8"
        need = lib.fa_bwd_workspace_bytes(B, Hq, Nq)
        assert need == 4 * B * Hq * Nq
    ws = Guarded("u8", (need,))
    what = ("fa_bwd_ex" if ex else "fa_bwd", dtype, D, (B, Hq, Hkv, Nq, Nk), causal, "ws", need)
    if ex:
        st = lib.fa_bwd_ex(q.ptr(), k.ptr(), v.ptr(), o_.ptr(), do.ptr(), lse.ptr(), dq.ptr(), dk.ptr(), dv.ptr(), ws.ptr(), B, Hq, Hkv, Nq, Nk,
                           D, D ** -0.5, *q.strides(), *k.strides(), causal, FA_DTYPE[dtype], None)
    else:
        assert k.strides() == q.strides()
        st = lib.fa_bwd(q.ptr(), k.ptr(), v.ptr(), o_.ptr(), do.ptr(), lse.ptr(), dq.ptr(), dk.ptr(), dv.ptr(), ws.ptr(), B, Hq, Nq, D, D ** -0.5,
                        *q.strides(), causal, FA_DTYPE[dtype], None)
    assert st == 0, (what, lib.fa_last_error())
    for g in (dq, dk, dv):  # written, not accumulated: the sentinel they were pre-filled with is gone, and it was a NaN
        g.check_written(what)
        no_nan(g, what)
    ws.check_written(what, full=False)
    torch.cuda.synchronize()
    delta = ws.raw[GUARD:GUARD + 4 * B * Hq * Nq].view(torch.float32)  # delta [B,Hq,Nq] leads the workspace: every entry written
    ref = (do.t.float() * o_.t.float()).sum(-1).reshape(-1)
    assert torch.allclose(delta, ref, rtol=1e-4, atol=1e-4), what
    for x in (q, k, v, o_, do, lse):
        x.check_unchanged(what)


@pytest.mark.parametrize("D", [8, 40, 64, 120, 128, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fa_bwd_footprint(lib, dtype, D):
    for n, N in enumerate(NS):
        _bwd_case(lib, dtype, 2, 3, 3, N, N, D, n % 2, ex=False, exact_ws=True)
        _bwd_case(lib, dtype, 2, 3, 3, N, N, D, 1 - n % 2, ex=False, exact_ws=True)


@pytest.mark.parametrize("D", [8, 40, 64, 120, 128, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fa_bwd_ex_footprint(lib, dtype, D):
    for (B, Hq, Hkv, Nq, Nk, causal) in ((2, 4, 2, 63, 129, 1), (1, 6, 1, 200, 333, 1), (2, 2, 2, 129, 63, 0), (1, 8, 2, 1, 200, 0),
                                         (1, 2, 1, 333, 333, 1), (1, 4, 2, 129, 1, 0)):
        _bwd_case(lib, dtype, B, Hq, Hkv, Nq, Nk, D, causal, ex=True, exact_ws=True)
    _bwd_case(lib, dtype, 2, 4, 2, 63, 129, D, 1, ex=True, exact_ws=False)  # the size fa_bwd_workspace_bytes_ex returns (rounded up)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_fa_bwd_e4m3_footprint(lib, D):
    """e4m3 Q, K, V: the widened bf16 copies live in the workspace behind delta, at the size fa_bwd_workspace_bytes_ex computes
    from the (padded) strides; a guard behind exactly that size."""
    for (B, Hq, Hkv, Nq, Nk, causal) in ((2, 4, 2, 63, 129, 1), (1, 6, 1, 200, 333, 1), (2, 2, 2, 129, 63, 0), (1, 2, 2, 333, 333, 1)):
        _bwd_case(lib, "fp8", B, Hq, Hkv, Nq, Nk, D, causal, ex=True, exact_ws=False)
    _bwd_case(lib, "fp8", 2, 3, 3, 200, 200, D, 1, ex=False, exact_ws=False)
