"""CPU: the C-ABI of the MLA indexer (include/fa_mi355.h, "The MLA indexer") -- the six symbols against the header's argument lists, the
support table, every argument rule with its status and text (fake aligned pointers: nothing may launch), the rules shared with
fa_fwd_varlen_paged and fa_fwd_mla_decode_sparse textually identical after the function name on the same bad argument, and the
workspace and chunk size functions on legal and illegal inputs."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, INT_ODD, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)

LOGITS, SELECT, TOPK = "fa_mla_indexer_logits_paged", "fa_mla_indexer_select", "fa_mla_indexer_topk_paged"
F_ODD = P(0x1002)  # not 4-byte aligned


def logits_call(lib, q=OK, w=OK, k=OK, lg=OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, Hi=64, T=8, mq=4, Di=128, P_=64, num_pages=100, mp=8,
                qs=(64 * 128, 128), wrs=64, kps=64 * 128, krs=128, bts=8, ls=512, dtype=BF16, **_):
    return lib.fa_mla_indexer_logits_paged(q, w, k, lg, cu, bt, sl, B, Hi, T, mq, Di, P_, num_pages, mp, *qs, wrs, kps, krs, bts, ls, dtype, None)


def select_call(lib, lg=OK, idx=OK, cnt=INT_OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, T=8, mq=4, topk=64, P_=64, num_pages=100, mp=8, ls=512,
                ist=64, bts=8, **_):
    return lib.fa_mla_indexer_select(lg, idx, cnt, cu, bt, sl, B, T, mq, topk, P_, num_pages, mp, ls, ist, bts, None)


def topk_call(lib, q=OK, w=OK, k=OK, idx=OK, cnt=INT_OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, Hi=64, T=8, mq=4, Di=128, topk=64, P_=64,
              num_pages=100, mp=8, qs=(64 * 128, 128), wrs=64, kps=64 * 128, krs=128, bts=8, ist=64, dtype=BF16, ws=OK, wsb=8 * 512 * 4, **_):
    return lib.fa_mla_indexer_topk_paged(q, w, k, idx, cnt, cu, bt, sl, B, Hi, T, mq, Di, topk, P_, num_pages, mp, *qs, wrs, kps, krs, bts, ist,
                                         dtype, ws, wsb, None)


def paged_twin(lib, q=OK, k=OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, T=8, mq=4, Di=128, P_=64, num_pages=100, mp=8, qs=(64 * 128, 128),
               kps=64 * 128, krs=128, bts=8, dtype=BF16, **_):
    """the same arguments as fa_fwd_varlen_paged sees them: one key head, the pool's row stride as its head stride"""
    return lib.fa_fwd_varlen_paged(q, k, k, OK, None, cu, bt, sl, B, 64, 1, T, mq, Di, P_, num_pages, mp, 0.1, *qs, kps, krs, krs, bts, 1, dtype, None)


def sparse_twin(lib, idx=OK, cnt=INT_OK, topk=64, P_=64, num_pages=100, ist=64, **_):
    wsb = lib.fa_fwd_mla_decode_sparse_workspace_bytes(8, 16, 512, topk)
    return lib.fa_fwd_mla_decode_sparse(OK, OK, OK, None, idx, cnt, 8, 16, 576, 512, topk, P_, num_pages, 0.1, 16 * 576, 576, 16 * 512, 512,
                                        P_ * 576, 576, ist, BF16, OK, wsb, None)


def text(lib, name):
    msg = lib.fa_last_error().decode()
    assert msg.startswith(name + ": "), msg
    return msg[len(name) + 2:]


def test_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((LOGITS, 24), (SELECT, 17), (TOPK, 28), (TOPK + "_workspace_bytes", 3), ("fa_mla_indexer_chunk_keys", 4),
                        ("fa_mla_indexer_supported", 4)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name


def test_support_table_and_refusals_that_name_what_was_given(lib):
    sup = lib.fa_mla_indexer_supported
    assert all(sup(d, h, 128, p) == 1 for d in (F16, BF16) for h in (32, 64) for p in (16, 32, 64, 128, 256))
    assert not any(sup(*a) for a in ((F32, 64, 128, 64), (FP8, 64, 128, 64), (BF16, 16, 128, 64), (BF16, 48, 128, 64), (BF16, 128, 128, 64),
                                     (BF16, 64, 64, 64), (BF16, 64, 128, 48), (BF16, 64, 128, 8), (BF16, 64, 128, 512)))
    for kw, word in (({"Hi": 48}, "Hi=48"), ({"Di": 64}, "Di=64"), ({"dtype": F32}, "dtype=f32"), ({"P_": 48}, "page_size=48")):
        for call, name in ((logits_call, LOGITS), (topk_call, TOPK)):
            assert call(lib, **kw) == -2 and word in text(lib, name), (name, kw)
    assert select_call(lib, P_=48) == -2 and "page_size=48" in text(lib, SELECT)


PAGED = [({"q": None}, "null pointer"), ({"k": None}, "null pointer"), ({"cu": None}, "null pointer"), ({"bt": None}, "null pointer"),
         ({"sl": None}, "null pointer"), ({"B": 0}, "sizes must be >= 1"), ({"T": 0}, "sizes must be >= 1"), ({"mp": 0}, "sizes must be >= 1"),
         ({"num_pages": 0}, "sizes must be >= 1"), ({"mq": 9}, "max_seqlen_q=9 exceeds the token count 8"),
         ({"qs": (64 * 128, 120)}, "bad strides"), ({"qs": (64 * 128 + 4, 128)}, "bad strides"), ({"bts": 7}, "block_table_stride=7"),
         ({"krs": 120}, "bad page strides"), ({"kps": 64 * 128 + 4}, "bad page strides"),
         ({"P_": 256, "krs": 1 << 22, "kps": 1 << 30, "ls": 2048, "wsb": 1 << 40}, "one page of one head exceeds 2 GiB"),
         ({"bt": INT_ODD}, "int32-aligned"), ({"sl": INT_ODD}, "int32-aligned"), ({"cu": INT_ODD}, "cu_seqlens_q must be int32-aligned"),
         ({"mp": 1 << 25, "bts": 1 << 25, "ls": 1 << 31, "wsb": 1 << 60}, "capacity above 2^30 keys"),
         ({"q": ODD}, "tensors must be 16-byte aligned"), ({"k": ODD}, "tensors must be 16-byte aligned")]
SPARSE = [({"ist": 60}, "indices_stride=60 must be a multiple of 4 and >= topk=64"), ({"ist": 66}, "indices_stride=66"),
          ({"idx": ODD}, "indices must be 16-byte aligned"), ({"cnt": INT_ODD}, "index_counts must be int32-aligned"),
          ({"num_pages": 1 << 25}, "slots, above 2^30")]


@pytest.mark.parametrize("twin,rules,mine", [(paged_twin, PAGED, (logits_call, LOGITS)), (paged_twin, PAGED, (topk_call, TOPK)),
                                             (sparse_twin, SPARSE, (select_call, SELECT)), (sparse_twin, SPARSE, (topk_call, TOPK))])
def test_shared_rules_carry_the_other_calls_status_and_text(lib, twin, rules, mine):
    twin_name = "fa_fwd_varlen_paged" if twin is paged_twin else "fa_fwd_mla_decode_sparse"
    for kw, word in rules:
        assert mine[0](lib, **kw) == -1, (mine[1], kw)
        got = text(lib, mine[1])
        assert twin(lib, **kw) == -1 and got == text(lib, twin_name) and word in got, (kw, got)


def test_rules_of_their_own(lib):
    own = [(logits_call, LOGITS, {"w": None}, "null pointer"), (logits_call, LOGITS, {"lg": None}, "null pointer"),
           (logits_call, LOGITS, {"w": F_ODD}, "w must be fp32-aligned"), (logits_call, LOGITS, {"lg": F_ODD}, "logits must be fp32-aligned"),
           (logits_call, LOGITS, {"wrs": 63}, "w_row_stride=63 < Hi=64"), (logits_call, LOGITS, {"ls": 511}, "logits_stride=511 < max_pages_per_seq * page_size = 512"),
           (logits_call, LOGITS, {"B": 1 << 30, "mq": 8}, "grid too large"),
           (select_call, SELECT, {"lg": None}, "null pointer"), (select_call, SELECT, {"idx": None}, "null pointer"),
           (select_call, SELECT, {"cnt": None}, "null pointer"), (select_call, SELECT, {"topk": 0}, "sizes must be >= 1"),
           (select_call, SELECT, {"lg": F_ODD}, "logits must be fp32-aligned"), (select_call, SELECT, {"ls": 511}, "logits_stride=511"),
           (select_call, SELECT, {"mq": 9}, "max_seqlen_q=9 exceeds the token count 8"), (select_call, SELECT, {"bts": 7}, "block_table_stride=7"),
           (select_call, SELECT, {"mp": 1 << 25, "bts": 1 << 25, "ls": 1 << 31}, "capacity above 2^30 keys"),
           (select_call, SELECT, {"B": 1 << 30, "T": 1 << 30, "mq": 2}, "grid too large"),
           (topk_call, TOPK, {"ws": None}, "null pointer"), (topk_call, TOPK, {"w": F_ODD}, "w must be fp32-aligned"),
           (topk_call, TOPK, {"ws": F_ODD}, "logits must be fp32-aligned"), (topk_call, TOPK, {"topk": 0}, "sizes must be >= 1"),
           (topk_call, TOPK, {"wsb": 8 * 512 * 4 - 1}, "workspace of 16383 bytes, fa_mla_indexer_topk_paged_workspace_bytes() asks for 16384")]
    for call, name, kw, word in own:
        assert call(lib, **kw) == -1 and word in text(lib, name), (name, kw, lib.fa_last_error())


def test_size_functions(lib):
    size, chunk = lib.fa_mla_indexer_topk_paged_workspace_bytes, lib.fa_mla_indexer_chunk_keys
    assert size(8, 64, 8) == 8 * 512 * 4 and size(1, 16, 1) == 64 and size(1 << 20, 256, 1 << 22) == (1 << 20) * (1 << 30) * 4
    assert all(size(*a) == 0 for a in ((0, 64, 8), (8, 48, 8), (8, 64, 0), (8, 256, (1 << 22) + 1), (-1, 64, 8)))
    # as few chunks as give 1024 items, none shorter than 8 tiles where the capacity has them
    assert chunk(1, 1, 64, 2048) == 64 * 8          # one decode token, 128k keys: 256 chunks of 8 tiles
    assert chunk(128, 1, 64, 2048) == 64 * 256      # 128 sequences: 8 chunks
    assert chunk(1, 2048, 64, 1024) == 64 * 512     # a prefill chunk of 512 token blocks: 2 chunks
    assert chunk(4096, 1, 16, 8) == 128 and chunk(2, 1, 64, 41) == 64 * 9
    assert all(chunk(*a) == 0 for a in ((0, 1, 64, 8), (1, 0, 64, 8), (1, 1, 48, 8), (1, 1, 64, 0), (1, 1, 256, (1 << 22) + 1)))
