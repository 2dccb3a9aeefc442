"""CPU: the C-ABI of fa_mla_indexer_select_split (include/fa_mi355.h, "The MLA indexer's select over several workgroups") -- the three
symbols against the header's argument lists, the call's own rules with status and text (fake aligned pointers: nothing may launch), every
rule of fa_mla_indexer_select textually identical after the function name on the same bad argument, and the two size functions."""
import pytest

from test_mla_abi import INT_OK, INT_ODD, ODD, OK, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)
from test_mla_indexer_abi import F_ODD, SELECT, select_call, text

SPLIT = "fa_mla_indexer_select_split"


def split_call(lib, lg=OK, idx=OK, cnt=INT_OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, T=8, mq=4, topk=64, P_=64, num_pages=100, mp=8, ls=512,
               ist=64, bts=8, S=4, ws=OK, wsb=1 << 20, **_):
    return lib.fa_mla_indexer_select_split(lg, idx, cnt, cu, bt, sl, B, T, mq, topk, P_, num_pages, mp, ls, ist, bts, S, ws, wsb, None)


def test_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((SPLIT, 20), (SPLIT + "_workspace_bytes", 2), ("fa_mla_indexer_select_num_splits", 4)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
    assert header_args(SPLIT)[1][:16] == header_args(SELECT)[1][:16]


def test_rules_of_its_own(lib):
    need = lib.fa_mla_indexer_select_split_workspace_bytes(8, 4)
    own = [({"S": 0}, "num_splits=0 outside 1 .. 64"), ({"S": 65}, "num_splits=65 outside 1 .. 64"), ({"S": -3}, "num_splits=-3"),
           ({"ws": None}, "workspace is null with num_splits=4"), ({"ws": ODD}, "workspace must be 16-byte aligned"),
           ({"ws": ODD, "S": 1}, "workspace must be 16-byte aligned"),
           ({"wsb": need - 1}, f"workspace of {need - 1} bytes, fa_mla_indexer_select_split_workspace_bytes() asks for {need}"),
           ({"B": 1 << 28, "T": 1 << 30, "mq": 4, "S": 2, "wsb": 1 << 62}, "grid too large")]
    for kw, word in own:
        assert split_call(lib, **kw) == -1 and word in text(lib, SPLIT), (kw, lib.fa_last_error())


SHARED = [({"lg": None}, "null pointer"), ({"idx": None}, "null pointer"), ({"cnt": None}, "null pointer"), ({"cu": None}, "null pointer"),
          ({"topk": 0}, "sizes must be >= 1"), ({"B": 0}, "sizes must be >= 1"), ({"P_": 48}, "page_size=48"),
          ({"ist": 60}, "indices_stride=60 must be a multiple of 4 and >= topk=64"), ({"mq": 9}, "max_seqlen_q=9 exceeds the token count 8"),
          ({"bts": 7}, "block_table_stride=7"), ({"mp": 1 << 25, "bts": 1 << 25, "ls": 1 << 31}, "capacity above 2^30 keys"),
          ({"bt": INT_ODD}, "int32-aligned"), ({"cu": INT_ODD}, "cu_seqlens_q must be int32-aligned"), ({"idx": ODD}, "indices must be 16-byte aligned"),
          ({"cnt": INT_ODD}, "index_counts must be int32-aligned"), ({"num_pages": 1 << 25}, "slots, above 2^30"),
          ({"lg": F_ODD}, "logits must be fp32-aligned"), ({"ls": 511}, "logits_stride=511"),
          ({"B": 1 << 30, "T": 1 << 30, "mq": 2}, "grid too large")]


@pytest.mark.parametrize("S", [1, 4])
def test_the_selects_rules_keep_status_and_text(lib, S):
    for kw, word in SHARED:
        st = split_call(lib, S=S, **kw)
        got = text(lib, SPLIT)
        assert select_call(lib, **kw) == st and st in (-1, -2) and got == text(lib, SELECT) and word in got, (kw, got)


def test_size_functions(lib):
    size, splits = lib.fa_mla_indexer_select_split_workspace_bytes, lib.fa_mla_indexer_select_num_splits
    # histograms [4][T][S][256], states [4][T][2], carries [T][S], in ints, rounded up to 16 bytes
    assert size(8, 4) == 4 * (4 * 8 * 4 * 256 + 4 * 8 * 2 + 8 * 4) and size(1, 3) == (4 * (4 * 3 * 256 + 8 + 3) + 15) // 16 * 16
    assert size(1 << 30, 64) > 1 << 48 and all(size(t, s) % 16 == 0 and size(t, s) > 0 for t in (1, 5) for s in (1, 2, 64))
    assert all(size(*a) == 0 for a in ((0, 4), (-1, 4), (8, 0), (8, 65), (8, -1)))
    assert all(splits(*a) == 0 for a in ((0, 1, 64, 8), (1, 0, 64, 8), (1, 1, 48, 8), (1, 1, 64, 0), (1, 1, 256, (1 << 22) + 1)))
    assert splits(512, 1, 64, 2048) == 1 and splits(128, 4, 64, 2048) == 1 and splits(4096, 1, 16, 8) == 1
    assert 2 <= splits(1, 1, 64, 2048) <= 64
