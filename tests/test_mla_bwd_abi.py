"""CPU: the C-ABI of fa_bwd_varlen_mla (include/fa_mi355.h, "Multi-head latent attention (prefill, backward)") -- the two symbols against
the header's argument lists, the support table (the two existing backward tables unmoved), every argument rule with its status and its
text (fake aligned pointers: nothing may launch), the rules it shares with fa_fwd_varlen_mla and with fa_bwd_varlen textually identical
after the function name on the same bad argument, each of the four stride pairs refused on its own, the null gradients / workspace / lse
-- and the errors of the Python wrapper and the op's Meta shapes."""
import os

import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_ODD, INT_OK, ODD, OK, header_args
from test_mla_prefill_abi import mla_call as fwd_call

NAME = "fa_bwd_varlen_mla"
TENSORS = ("q", "k", "v", "o")
WHAT = {"q": "", "k": "key ", "v": "value ", "o": "output "}  # how varlen_strides_ok names the operand
ROW = {"q": 192, "k": 192, "v": 128, "o": 128}
ODD4 = INT_ODD  # 2-byte aligned: not fp32-aligned


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


@pytest.fixture(scope="module")
def lib(fa):
    return fa.load_library()


def bwd_call(lib, q=OK, k=OK, v=OK, o=OK, d_o=OK, lse=OK, dq=OK, dk=OK, dv=OK, ws=OK, cu_q=INT_OK, cu_k=INT_OK, B=3, Hq=8, Hkv=2, total_q=700,
             total_k=900, max_q=400, max_k=500, Dqk=192, Dv=128, scale=0.0722, strides=None, causal=1, dtype=BF16):
    s = {"q": (Hq * 192, 192), "k": (Hkv * 192, 192), "v": (Hkv * 128, 128), "o": (Hq * 128, 128)}
    s.update(strides or {})
    return lib.fa_bwd_varlen_mla(q, k, v, o, d_o, lse, dq, dk, dv, ws, cu_q, cu_k, B, Hq, Hkv, total_q, total_k, max_q, max_k, Dqk, Dv, scale,
                                 *s["q"], *s["k"], *s["v"], *s["o"], causal, dtype, None)


def varlen_bwd_call(lib, q=OK, k=OK, v=OK, o=OK, d_o=OK, lse=OK, dq=OK, dk=OK, dv=OK, ws=OK, cu_q=INT_OK, cu_k=INT_OK, B=3, Hq=8, Hkv=2,
                    total_q=700, total_k=900, max_q=400, max_k=500, scale=0.0722, strides=None, causal=1, dtype=BF16, **_):
    s = {"q": (Hq * 128, 128), "k": (Hkv * 128, 128)}
    s.update(strides or {})
    return lib.fa_bwd_varlen(q, k, v, o, d_o, lse, dq, dk, dv, ws, cu_q, cu_k, B, Hq, Hkv, total_q, total_k, max_q, max_k, 128, scale, *s["q"],
                             *s["k"], causal, dtype, None)


def test_two_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((NAME, 33), (NAME + "_supported", 3)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
        assert hasattr(lib, name)
    assert lib.fa_version() == 400
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fa_mi355.h")).read()
    assert "Multi-head latent attention (prefill, backward)" in header
    assert "fa_bwd_varlen_workspace_bytes(Hq, total_q) bytes; it holds delta" in header and "no size function of its own" in header


def test_support_table_and_the_existing_tables_unmoved(lib, fa):
    sup = lib.fa_bwd_varlen_mla_supported
    assert sup(F16, 192, 128) == 1 and sup(BF16, 192, 128) == 1
    for dtype, dqk, dv in ((F32, 192, 128), (FP8, 192, 128), (9, 192, 128), (BF16, 128, 128), (BF16, 192, 192), (BF16, 576, 512), (BF16, 128, 192),
                           (BF16, 192, 64), (BF16, 0, 0), (BF16, 256, 128)):
        assert not sup(dtype, dqk, dv), (dtype, dqk, dv)
    assert fa.varlen_mla_backward_supported("bf16", 192, 128) and not fa.varlen_mla_backward_supported("f32", 192, 128)
    # fa_bwd_varlen_supported: f16 / bf16 at 64 | 128; fa_bwd_supported: multiples of 8 up to 128, and 256 -- neither takes 192
    for d in range(8, 264, 8):
        assert bool(lib.fa_bwd_varlen_supported(BF16, d)) == (d in (64, 128)) and bool(lib.fa_bwd_varlen_supported(F16, d)) == (d in (64, 128)), d
        assert bool(lib.fa_bwd_supported(BF16, d)) == (d <= 128 or d == 256), d
    assert not lib.fa_bwd_varlen_supported(F32, 128) and not lib.fa_bwd_varlen_supported(FP8, 128)


# the rules the call applies through the shared helpers: what to break, the status, a word of the message
SHARED_FWD = [({"q": None}, -1, "null pointer"), ({"o": None}, -1, "null pointer"), ({"cu_k": None}, -1, "null pointer"),
              ({"B": 0}, -1, "sizes must be >= 1"), ({"total_k": 0}, -1, "sizes must be >= 1"), ({"max_q": -1}, -1, "sizes must be >= 1"),
              ({"Dv": 0}, -1, "sizes must be >= 1"),
              ({"Hq": 8, "Hkv": 3}, -1, "Hq=8 must be a multiple of Hkv=3"),
              ({"scale": 0.0}, -1, "scale"), ({"scale": float("nan")}, -1, "scale"),
              ({"Dqk": 128}, -2, "Dqk=128 Dv=128"), ({"dtype": F32}, -2, "dtype=f32"),
              ({"max_q": 701}, -1, "max_seqlen (701, 500) exceeds the token count (700, 900)"), ({"max_k": 901}, -1, "exceeds the token count"),
              ({"strides": {"v": (2 * 128 + 4, 128)}}, -1, "bad value strides"), ({"strides": {"o": (8 * 128, 120)}}, -1, "bad output strides"),
              ({"q": ODD}, -1, "tensors must be 16-byte aligned"), ({"v": ODD}, -1, "tensors must be 16-byte aligned"),
              ({"cu_q": INT_ODD}, -1, "int32-aligned"), ({"cu_k": INT_ODD}, -1, "int32-aligned"),
              ({"strides": {"q": (1 << 23, 1 << 24)}}, -1, "one head exceeds 4 GiB (one sequence of max_seqlen_q rows)"),
              ({"strides": {"v": (1 << 23, 1 << 24)}}, -1, "one head exceeds 4 GiB (one sequence of max_seqlen_k rows)"),
              ({"B": 1 << 23, "Hq": 1 << 8, "Hkv": 1 << 8}, -1, "grid too large")]
SHARED_BWD = [({"d_o": None}, -1, "null pointer"), ({"lse": None}, -1, "null pointer"), ({"dq": None}, -1, "null pointer"),
              ({"dk": None}, -1, "null pointer"), ({"dv": None}, -1, "null pointer"), ({"ws": None}, -1, "null pointer"),
              ({"B": 0}, -1, "sizes must be >= 1"), ({"Hq": 8, "Hkv": 3}, -1, "Hq=8 must be a multiple of Hkv=3"),
              ({"scale": -1.0}, -1, "scale"), ({"max_k": 901}, -1, "exceeds the token count"),
              ({"d_o": ODD}, -1, "tensors must be 16-byte aligned"), ({"dq": ODD}, -1, "tensors must be 16-byte aligned"),
              ({"dk": ODD}, -1, "tensors must be 16-byte aligned"), ({"dv": ODD}, -1, "tensors must be 16-byte aligned"),
              ({"cu_q": INT_ODD}, -1, "int32-aligned"),
              ({"lse": ODD4}, -1, "lse / workspace must be fp32-aligned"), ({"ws": ODD4}, -1, "lse / workspace must be fp32-aligned"),
              ({"B": 1 << 23, "Hq": 1 << 8, "Hkv": 1 << 8}, -1, "grid too large"),
              ({"B": 1 << 22, "Hq": 1, "Hkv": 1, "total_k": 1 << 20, "max_k": 1 << 20}, -1, "grid too large")]  # the dK/dV kernel's grid alone


def _same_text(lib, mine_call, their_call, their_name, rules):
    for kw, status, word in rules:
        assert mine_call(lib, **kw) == status, kw
        mine = lib.fa_last_error().decode()
        assert their_call(lib, **kw) == status, kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith(NAME + ": ") and theirs.startswith(their_name + ": ") and word in mine, (kw, mine, theirs)
        assert mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (kw, mine, theirs)


def test_rules_shared_with_fa_fwd_varlen_mla_have_its_status_and_text(lib):
    _same_text(lib, bwd_call, fwd_call, "fa_fwd_varlen_mla", SHARED_FWD)


def test_rules_shared_with_fa_bwd_varlen_have_its_status_and_text(lib):
    _same_text(lib, bwd_call, varlen_bwd_call, "fa_bwd_varlen", SHARED_BWD)


def test_unsupported_pairs_and_types_say_what_was_given(lib):
    for kw, word in (({"Dqk": 128}, "Dqk=128 Dv=128"), ({"Dv": 192}, "Dqk=192 Dv=192"), ({"Dqk": 576, "Dv": 512}, "Dqk=576 Dv=512"),
                     ({"Dqk": 256, "Dv": 256}, "Dqk=256 Dv=256"), ({"dtype": F32}, "dtype=f32"), ({"dtype": FP8}, "fp8_e4m3")):
        assert bwd_call(lib, **kw) == -2, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(NAME + ": needs f16 / bf16 and (Dqk, Dv) = (192, 128), got ") and word in msg, (kw, msg)
    assert bwd_call(lib, dtype=F16, q=None) == -1  # f16 passes the table and meets the next rule


@pytest.mark.parametrize("t", TENSORS)
def test_each_stride_pair_is_refused_on_its_own(lib, t):
    d = ROW[t]
    good = {"q": (8 * 192, 192), "k": (2 * 192, 192), "v": (2 * 128, 128), "o": (8 * 128, 128)}[t]
    for bad in ((d - 8, good[1]), (good[0], d - 8), (good[0] + 4, good[1]), (good[0], good[1] + 4)):  # too small (row, head); not a multiple of 8
        assert bwd_call(lib, strides={t: bad}) == -1, (t, bad)
        assert lib.fa_last_error().decode() == (f"{NAME}: bad {WHAT[t]}strides (row {bad[0]}, head {bad[1]}): a row holds {d} elements, "
                                                "strides are multiples of 8"), (t, bad)
    # a misaligned base
    assert bwd_call(lib, **{t: ODD}) == -1
    assert lib.fa_last_error().decode() == f"{NAME}: tensors must be 16-byte aligned"
    # the 4 GiB rule, (max_seqlen + 128) * row_stride * 2 bytes: q and o by max_seqlen_q = 400, k and v by max_seqlen_k = 500
    rows = (400 if t in "qo" else 500) + 128
    edge = -(-(1 << 31) // rows)  # the smallest row stride (elements) that reaches 4 GiB
    edge = (edge + 7) // 8 * 8
    assert bwd_call(lib, strides={t: (edge, good[1])}) == -1, t
    assert lib.fa_last_error().decode() == f"{NAME}: one head exceeds 4 GiB (one sequence of max_seqlen_{'q' if t in 'qo' else 'k'} rows)"
    # ... and one step below it the call passes on to the next rule, the last before the launch
    assert bwd_call(lib, strides={t: (edge - 8, good[1])}, B=1 << 23, Hq=1 << 8, Hkv=1 << 8) == -1
    assert lib.fa_last_error().decode() == f"{NAME}: grid too large"


def test_python_wrapper_refuses_bad_arguments(fa):
    import torch

    bf = torch.bfloat16
    q, k, v = torch.zeros(10, 4, 192, dtype=bf), torch.zeros(12, 2, 192, dtype=bf), torch.zeros(12, 2, 128, dtype=bf)
    o = torch.zeros(10, 4, 128, dtype=bf)
    lse = torch.zeros(4, 10)
    cu = torch.tensor([0, 10], dtype=torch.int32)
    call = fa.flash_attention_varlen_mla_backward
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(q, k, v, o, o, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="got"):
        call(q[0], k, v, o, o, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="got"):
        call(q, k, v, o, o[:9], lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="incompatible shapes"):
        call(q, k[:, :, :128], v, o, o, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="incompatible shapes"):
        call(q, k, v[:11], o, o, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="incompatible shapes"):  # o rows of 192
        call(q, k, v, q, q, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="dtypes"):
        call(q, k, v, o, o.half(), lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="unit element stride"):
        call(q, k, torch.zeros(12, 2, 256, dtype=bf)[:, :, ::2], o, o, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="o and d_o must share"):
        call(q, k, v, o, torch.zeros(4, 10, 128, dtype=bf).transpose(0, 1), lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="int32"):
        call(q, k, v, o, o, lse, cu.long(), cu, 10, 12)
    with pytest.raises(ValueError, match=r"both be \[B \+ 1\]"):
        call(q, k, v, o, o, lse, cu, torch.tensor([0, 5, 12], dtype=torch.int32), 10, 12)
    with pytest.raises(ValueError, match="lse must be contiguous fp32"):
        call(q, k, v, o, o, lse.T, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="lse must be contiguous fp32"):
        call(q, k, v, o, o, lse.double(), cu, cu, 10, 12)


def test_the_op_is_registered_with_meta_shapes():
    import torch

    from flash_attention_metal_amd import torch_op  # noqa: F401 (registers the op)

    q = torch.empty(50, 8, 192, dtype=torch.bfloat16, device="meta")
    k = torch.empty(70, 2, 192, dtype=torch.bfloat16, device="meta")
    v = torch.empty(70, 2, 256, dtype=torch.bfloat16, device="meta")[:, :, 128:]
    cu = torch.empty(3, dtype=torch.int32, device="meta")
    o, lse = torch.ops.fa_mi355.attention_varlen_mla(q, k, v, cu, cu, 30, 40, True, 0.0)
    assert o.shape == (50, 8, 128) and o.dtype == torch.bfloat16 and o.is_contiguous()
    assert lse.shape == (8, 50) and lse.dtype == torch.float32
    schema = str(torch.ops.fa_mi355.attention_varlen_mla.default._schema)
    assert "bool is_causal=False" in schema and "float scale=0." in schema
    assert callable(torch_op.attention_varlen_mla)
