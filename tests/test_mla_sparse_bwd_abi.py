"""CPU: the C-ABI of fa_bwd_mla_sparse -- symbols against the header, support table, size function, its own rules with status and text (fake
aligned pointers: nothing may launch), and every rule of fa_fwd_mla_decode_sparse textually identical after the function name."""
from test_mla_abi import BF16, F16, F32, FP8, INT_OK, INT_ODD, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fixtures)
from test_mla_sparse_abi import SHARED, sparse_call

BWD, SPARSE = "fa_bwd_mla_sparse", "fa_fwd_mla_decode_sparse"


def bwd_call(lib, q=OK, kv=OK, o=OK, do=OK, lse=INT_OK, dq=OK, dkv=OK, idx=OK, cnt=INT_OK, ws=OK, T=2, Hq=16, Dqk=576, Dv=512, topk=320, P_=64,
             num_pages=100, scale=0.0722, qs=None, os_=None, kps=64 * 576, krs=576, dps=64 * 576, drs=576, ist=320, dtype=BF16, wsb=None):
    qs = (Hq * 576, 576) if qs is None else qs
    os_ = (Hq * 512, 512) if os_ is None else os_
    wsb = lib.fa_bwd_mla_sparse_workspace_bytes(2, 16) if wsb is None else wsb
    return lib.fa_bwd_mla_sparse(q, kv, o, do, lse, dq, dkv, idx, cnt, T, Hq, Dqk, Dv, topk, P_, num_pages, scale, *qs, *os_, kps, krs, dps, drs, ist,
                                 dtype, ws, wsb, None)


def test_symbols_support_table_and_size(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((BWD, 30), (BWD + "_workspace_bytes", 2), (BWD + "_supported", 5)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds) and hasattr(lib, name), name
    assert header_args(BWD + "_supported") == header_args(SPARSE + "_supported") and lib.fa_version() == 400
    sup, fwd = lib.fa_bwd_mla_sparse_supported, lib.fa_fwd_mla_decode_sparse_supported
    for args in [(d, 576, 512, hq, p) for d in (F16, BF16, F32, FP8, 9) for hq in (-1, 0, 1, 17, 64, 128, 129) for p in (0, 8, 16, 32, 48, 64, 128, 256, 512)]:
        assert sup(*args) == fwd(*args) == int(args[0] in (F16, BF16) and 1 <= args[3] <= 128 and args[4] in (16, 32, 64, 128, 256)), args
    assert not sup(BF16, 192, 128, 16, 64) and not sup(BF16, 576, 576, 16, 64) and not sup(BF16, 512, 512, 16, 64)
    size = lib.fa_bwd_mla_sparse_workspace_bytes
    assert size(2, 16) == 128 and size(1, 1) == 16 and size(3, 33) == 400 and size(4096, 128) == 4096 * 128 * 4 and size(1 << 24, 127) == (1 << 26) * 127
    assert all(size(t, h) % 16 == 0 and size(t, h) >= 4 * t * h for t in (1, 5, 7) for h in (1, 3, 128))
    assert all(size(*bad) == 0 for bad in ((0, 16), (-1, 16), (2, 0), (2, 129), (2, -4), (1 << 30, 128)))


def test_rules_of_its_own(lib):
    need = lib.fa_bwd_mla_sparse_workspace_bytes(2, 16)
    own = [({"do": None}, "null pointer"), ({"lse": None}, "null pointer"), ({"dq": None}, "null pointer"), ({"dkv": None}, "null pointer"),
           ({"ws": None}, "null pointer"), ({"drs": 572}, "bad dkv strides (page 36864, row 572)"), ({"drs": 578, "dps": 64 * 580}, "bad dkv strides"),
           ({"dps": 64 * 576 + 2}, "bad dkv strides"), ({"dps": 512}, "bad dkv strides"),
           ({"P_": 256, "kps": 256 * 576, "drs": 1 << 21, "dps": 1 << 29}, "one page of dkv exceeds 2 GiB"),
           ({"do": ODD}, "d_o, dq and dkv must be 16-byte aligned"), ({"dq": ODD}, "d_o, dq and dkv must be 16-byte aligned"),
           ({"dkv": P(0x1004)}, "d_o, dq and dkv must be 16-byte aligned"), ({"lse": INT_ODD}, "lse must be fp32-aligned"),
           ({"wsb": need - 1}, f"workspace of {need - 1} bytes, fa_bwd_mla_sparse_workspace_bytes() asks for {need}")]
    for kw, word in own:
        assert bwd_call(lib, **kw) == -1 and lib.fa_last_error().decode().startswith(BWD + ": ") and word in lib.fa_last_error().decode(), (kw, lib.fa_last_error())
    for kw in ({}, {"cnt": None}, {"drs": 580, "dps": 65 * 580}, {"Hq": 128}, {"Hq": 1}, {"P_": 16, "kps": 16 * 576, "dps": 16 * 576}, {"dtype": F16}):
        assert bwd_call(lib, wsb=1, **kw) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode(), kw


def test_the_forwards_rules_keep_status_and_text(lib):
    lists = [({"idx": None}, "null pointer"), ({"topk": 0}, "sizes must be >= 1"), ({"ist": 316}, "indices_stride=316 must be a multiple of 4 and >= topk=320"),
             ({"idx": ODD}, "indices must be 16-byte aligned"), ({"cnt": INT_ODD}, "index_counts must be int32-aligned"),
             ({"num_pages": (1 << 24) + 1}, "slots, above 2^30"), ({"topk": (1 << 30) + 1, "ist": (1 << 30) + 4, "wsb": 1 << 60}, "capacity above 2^30 keys"),
             ({"dtype": FP8}, "dtype=fp8_e4m3"), ({"Dv": 576}, "Dv=576")]
    for kw, word in SHARED + lists:
        st = bwd_call(lib, **kw)
        mine = lib.fa_last_error().decode()
        assert sparse_call(lib, **kw) == st and st in (-1, -2), kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith(BWD + ": ") and theirs.startswith(SPARSE + ": ") and word in mine and mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (kw, mine, theirs)

