"""CPU: the C-ABI of fa_mla_sparse_head_probs and fa_mla_indexer_loss_sparse -- symbols against the header, the support tables, each rule of
their own with status and text (fake aligned pointers: nothing may launch), and the rules they share with fa_fwd_mla_decode_sparse and
fa_mla_indexer_logits_paged textually identical after the function name."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, INT_ODD, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fixtures)
from test_mla_sparse_abi import SHARED, sparse_call

PROBS, LOSS, SPARSE, LOGITS = "fa_mla_sparse_head_probs", "fa_mla_indexer_loss_sparse", "fa_fwd_mla_decode_sparse", "fa_mla_indexer_logits_paged"


def probs_call(lib, q=OK, kv=OK, lse=INT_OK, probs=INT_OK, idx=OK, cnt=INT_OK, T=2, Hq=16, Dqk=576, Dv=512, topk=320, P_=64, num_pages=100,
               scale=0.0722, qs=None, kps=64 * 576, krs=576, ist=320, pst=320, dtype=BF16, **_):
    qs = (Hq * 576, 576) if qs is None else qs
    return lib.fa_mla_sparse_head_probs(q, kv, lse, probs, idx, cnt, T, Hq, Dqk, Dv, topk, P_, num_pages, scale, *qs, kps, krs, ist, pst, dtype, None)


def loss_call(lib, q=OK, w=INT_OK, k=OK, idx=OK, cnt=INT_OK, tgt=INT_OK, lg=None, loss=INT_OK, dq=OK, dw=INT_OK, dk=OK, T=2, Hi=64, Di=128,
              topk=320, P_=64, num_pages=100, qs=(64 * 128, 128), wrs=64, kps=64 * 128, krs=128, dps=64 * 128, drs=128, ist=320, tst=320, dtype=BF16):
    return lib.fa_mla_indexer_loss_sparse(q, w, k, idx, cnt, tgt, lg, loss, dq, dw, dk, T, Hi, Di, topk, P_, num_pages, *qs, wrs, kps, krs, dps, drs,
                                          ist, tst, dtype, None)


def logits_call(lib, q=OK, w=INT_OK, k=OK, Hi=64, Di=128, P_=64, num_pages=100, qs=(64 * 128, 128), wrs=64, kps=64 * 128, krs=128, dtype=BF16, **_):
    return lib.fa_mla_indexer_logits_paged(q, w, k, INT_OK, INT_OK, INT_OK, INT_OK, 1, Hi, 2, 2, Di, P_, num_pages, 5, *qs, wrs, kps, krs, 8, 320, dtype, None)


def same_text(lib, mine_fn, mine, theirs_fn, theirs, kw, word, statuses=(-1, -2)):
    st = mine(lib, **kw)
    a = lib.fa_last_error().decode()
    assert theirs(lib, **kw) == st and st in statuses, (kw, a)
    b = lib.fa_last_error().decode()
    assert a.startswith(mine_fn + ": ") and b.startswith(theirs_fn + ": ") and word in a and a.split(": ", 1)[1] == b.split(": ", 1)[1], (kw, a, b)


def test_symbols_and_support_tables(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((PROBS, 22), (PROBS + "_supported", 5), (LOSS, 28), (LOSS + "_supported", 5)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds) and hasattr(lib, name), name
    assert header_args(PROBS + "_supported") == header_args(SPARSE + "_supported") and lib.fa_version() == 400
    for args in [(d, 576, 512, hq, p) for d in (F16, BF16, F32, FP8, 9) for hq in (0, 1, 33, 128, 129) for p in (0, 16, 48, 64, 256, 512)]:
        assert lib.fa_mla_sparse_head_probs_supported(*args) == lib.fa_fwd_mla_decode_sparse_supported(*args), args
    for d in (F16, BF16, F32, FP8):
        for hi in (16, 32, 64, 128):
            for p in (8, 16, 256, 512):
                for topk in (0, 1, 2048, 4096, 4097):
                    assert lib.fa_mla_indexer_loss_sparse_supported(d, hi, 128, p, topk) == int(lib.fa_mla_indexer_supported(d, hi, 128, p) and 1 <= topk <= 4096)
    assert not lib.fa_mla_indexer_loss_sparse_supported(BF16, 64, 64, 64, 2048)
    assert loss_call(lib, topk=4097, ist=4100, tst=4100) == -2 and "topk=4097 above the 4096 list entries" in lib.fa_last_error().decode()


@pytest.mark.parametrize("kw,word", [({"lse": None}, "null pointer"), ({"probs": None}, "null pointer"), ({"pst": 319}, "probs_stride=319 < topk=320"),
                                     ({"lse": INT_ODD}, "lse must be fp32-aligned"), ({"probs": INT_ODD}, "probs must be fp32-aligned")])
def test_head_probs_rules_of_its_own(lib, kw, word):
    assert probs_call(lib, **kw) == -1 and lib.fa_last_error().decode().startswith(PROBS + ": ") and word in lib.fa_last_error().decode(), lib.fa_last_error()


def test_head_probs_shares_the_forwards_rules(lib):
    lists = [({"idx": None}, "null pointer"), ({"topk": 0}, "sizes must be >= 1"), ({"ist": 316}, "indices_stride=316 must be a multiple of 4 and >= topk=320"),
             ({"idx": ODD}, "indices must be 16-byte aligned"), ({"cnt": INT_ODD}, "index_counts must be int32-aligned"),
             ({"num_pages": (1 << 24) + 1}, "slots, above 2^30"), ({"dtype": FP8}, "dtype=fp8_e4m3"), ({"Dv": 576}, "Dv=576"), ({"Hq": 129}, "Hq=129")]
    for kw, word in [s for s in SHARED if not {"o", "ws", "os_"} & set(s[0])] + lists:  # (the call has no o and no workspace)
        same_text(lib, PROBS, probs_call, SPARSE, sparse_call, kw, word)


@pytest.mark.parametrize("kw,word", [({"tgt": None}, "null pointer"), ({"loss": None}, "null pointer"), ({"tst": 319}, "target_stride=319 < topk=320"),
                                     ({"tgt": INT_ODD}, "target, loss_grad and loss must be fp32-aligned"), ({"lg": INT_ODD}, "fp32-aligned"),
                                     ({"dq": None}, "all three"), ({"dw": None, "dk": None}, "all three"), ({"drs": 124}, "bad dk strides (page 8192, row 124)"),
                                     ({"dps": 64 * 128 + 2}, "bad dk strides"), ({"P_": 256, "kps": 256 * 128, "drs": 1 << 21, "dps": 1 << 29}, "one page of dk exceeds 2 GiB"),
                                     ({"dq": ODD}, "dq_idx and dk_idx must be 16-byte aligned"), ({"dw": INT_ODD}, "dw must be fp32-aligned")])
def test_indexer_loss_rules_of_its_own(lib, kw, word):
    assert loss_call(lib, **kw) == -1 and lib.fa_last_error().decode().startswith(LOSS + ": ") and word in lib.fa_last_error().decode(), lib.fa_last_error()


def test_indexer_loss_shares_the_indexers_and_the_forwards_rules(lib):
    for kw, word in [({"q": None}, "null pointer"), ({"Hi": 48}, "Hi=48"), ({"dtype": F32}, "dtype=f32"), ({"P_": 48}, "page_size=48"), ({"Di": 64}, "Di=64"),
                     ({"qs": (64 * 128, 120)}, "bad strides"), ({"qs": (64 * 128 + 4, 128)}, "bad strides"), ({"krs": 120}, "bad page strides"),
                     ({"kps": 64 * 128 + 4}, "bad page strides"), ({"q": ODD}, "tensors must be 16-byte aligned"), ({"k": ODD}, "16-byte aligned"),
                     ({"w": INT_ODD}, "w must be fp32-aligned"), ({"wrs": 63}, "w_row_stride=63 < Hi=64")]:
        same_text(lib, LOSS, loss_call, LOGITS, logits_call, kw, word)
    for kw, word in [({"idx": None}, "null pointer"), ({"ist": 316}, "indices_stride=316 must be a multiple of 4 and >= topk=320"),
                     ({"idx": ODD}, "indices must be 16-byte aligned"), ({"cnt": INT_ODD}, "index_counts must be int32-aligned"),
                     ({"num_pages": (1 << 24) + 1}, "slots, above 2^30")]:
        assert loss_call(lib, **kw) == -1
        a = lib.fa_last_error().decode()
        assert sparse_call(lib, **kw) == -1
        b = lib.fa_last_error().decode()
        assert word in a and a.split(": ", 1)[1] == b.split(": ", 1)[1], (kw, a, b)
