"""The references of tests/kv8.py are what include/fa_mi355.h ("e4m3 pools in the prefill") says (CPU only): the widening of the 254
finite e4m3 codes is exact and lands on bf16 values; the quantisation reference -- clamp in fp32, then torch's CPU cast -- over EVERY finite
bf16 and f16 bit pattern and the multipliers 1, 0.25 and 3 equals a nearest-value search with ties to the even code done here in fp64, is
monotone, symmetric in sign, saturates at +-448 and never gives a NaN byte; ties go to even at subnormal and normal midpoints; and each
planted mistake differs on a named pattern."""
import numpy as np
import pytest
import torch

import kv8

MULS = (1.0, 0.25, 3.0)
TYPES = (torch.bfloat16, torch.float16)
GRID = np.array([kv8.decode_by_hand(c) for c in range(0x7F)])  # the non-negative values: code order is value order


def from_bits(pattern, dtype):
    return torch.tensor([pattern - 65536 if pattern >= 32768 else pattern], dtype=torch.int16).view(dtype)


def test_widening_is_exact_and_stays_inside_bf16():
    codes = kv8.FINITE_CODES
    assert len(codes) == 254
    w = kv8.widen(codes)
    assert np.array_equal(w.astype(np.float64), np.array([kv8.decode_by_hand(int(c)) for c in codes]))
    assert np.signbit(w[codes == 0x80]).all() and not np.signbit(w[codes == 0x00]).any()  # -0 and +0
    t = torch.from_numpy(codes.copy()).view(kv8.E4M3).to(torch.float32).to(torch.bfloat16)
    assert np.array_equal(t.to(torch.float32).numpy().view(np.int32), w.view(np.int32))  # every e4m3 value is a bf16 value, bit for bit
    assert np.isnan(kv8.widen(np.array(kv8.NAN_CODES, np.uint8))).all()
    assert np.all(np.diff(GRID) > 0) and GRID[-1] == kv8.MAX and GRID[1] == 2.0 ** -9 and GRID[8] == 2.0 ** -6


def nearest_even(y32):
    """fp32 values -> codes, in fp64: clamp, the nearest grid value, a tie to the even code, the sign bit kept (also of -0)."""
    a = np.minimum(np.abs(y32.astype(np.float64)), kv8.MAX)
    lo = np.searchsorted(GRID, a, side="right") - 1
    hi = np.minimum(lo + 1, len(GRID) - 1)
    dl, dh = a - GRID[lo], GRID[hi] - a
    up = (dh < dl) | ((dh == dl) & (lo % 2 == 1))
    code = np.where(up & (hi > lo), hi, lo).astype(np.uint8)
    return code | (np.signbit(y32).astype(np.uint8) << 7)


@pytest.mark.parametrize("dtype", TYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("mul", MULS)
def test_reference_over_every_finite_pattern(dtype, mul):
    x, finite = kv8.all_patterns(dtype)
    assert int(finite.sum()) == {torch.bfloat16: 65536 - 2 * 128, torch.float16: 65536 - 2 * 1024}[dtype]
    x = x[finite]
    got = kv8.quant_reference(x, mul)
    with np.errstate(over="ignore"):
        y = x.to(torch.float32).numpy() * np.float32(mul)  # one fp32 multiply (bf16 * 3 may reach inf: the clamp takes it)
    assert np.array_equal(got, nearest_even(y)), "torch's cast behind the clamp is not round-to-nearest-even"
    assert not np.isin(got, kv8.NAN_CODES).any()
    # monotone in the input's value
    order = np.argsort(x.to(torch.float32).numpy(), kind="stable")
    assert np.all(np.diff(kv8.widen(got[order])) >= 0)
    # symmetric in sign: the pattern with the sign bit flipped gives the code with the sign bit flipped
    bits = x.view(torch.int16).numpy().astype(np.int32) & 0xFFFF
    table = np.zeros(65536, np.int32) - 1
    table[bits] = got
    assert np.array_equal(table[bits ^ 0x8000], got ^ 0x80)
    # saturation, both ends, and the sign of zero
    big = np.abs(y) >= kv8.MAX
    assert big.any() and np.array_equal(got[big], np.where(y[big] > 0, 0x7E, 0xFE))
    assert table[0x0000] == 0x00 and table[0x8000] == 0x80


@pytest.mark.parametrize("dtype", TYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("mul", (1.0, 0.25))
def test_ties_go_to_the_even_code(dtype, mul):
    # the midpoint of every pair of neighbours, subnormal (codes 0 .. 8) and normal: a 4-bit mantissa, exact in both input types, and so
    # is the midpoint divided by the multiplier
    mids = (GRID[:-1] + GRID[1:]) / 2
    x = torch.tensor(mids / mul, dtype=torch.float64).to(dtype)
    assert np.array_equal(x.to(torch.float64).numpy() * mul, mids)
    want = np.array([c if c % 2 == 0 else c + 1 for c in range(len(mids))], np.uint8)
    assert np.array_equal(kv8.quant_reference(x, mul), want)
    assert np.array_equal(kv8.quant_reference(-x, mul), want | 0x80)
    assert want[0] == 0 and want[7] == 8  # 2^-10 -> 0; 7.5 * 2^-9 -> the smallest normal


PLANTED = (  # mistake, input type, pattern, multiplier, the right byte, the mistake's byte
    ("truncate", torch.bfloat16, 0x3A81, 1.0, 0x01, 0x00),            # just above half the smallest subnormal
    ("truncate", torch.float16, 0x3C67, 1.0, 0x39, 0x38),             # 1.1006: nearer to 1.125 than to 1
    ("clamp_after", torch.bfloat16, 0x43E9, 1.0, 0x7E, 0x7F),         # 466: the bare cast gives NaN past 464
    ("clamp_after", torch.float16, 0x58D6, 3.0, 0x7E, 0x7F),          # 154.75 * 3
    ("mul_after_rounding", torch.bfloat16, 0x39AB, 3.0, 0x01, 0x00),  # 3 x lies above the tie 2^-10, its bf16 rounding on it
    ("mul_after_rounding", torch.float16, 0x0D56, 3.0, 0x01, 0x00),
)


@pytest.mark.parametrize("bug,dtype,pattern,mul,right,wrong", PLANTED, ids=[f"{p[0]}-{p[2]:04x}" for p in PLANTED])
def test_planted_mistakes_differ_on_a_named_pattern(bug, dtype, pattern, mul, right, wrong):
    x = from_bits(pattern, dtype)
    assert kv8.quant_reference(x, mul)[0] == right
    assert kv8.quant_reference(x, mul, bug)[0] == wrong


def test_twin_pools_agree_and_hide_nan_where_nobody_reads():
    import varlen_paged as vp

    rng = np.random.default_rng(5)
    lens = (40, 0, 17)
    ks = [kv8.draw_e4m3(rng, 2, L, 64) for L in lens]
    vs = [kv8.draw_e4m3(rng, 2, L, 64) for L in lens]
    t = kv8.twin_pools(ks, vs, 16, np.random.default_rng(6), max_pages=4)
    for b, L in enumerate(lens):
        for n8, n16, x in (("k8", "k16", ks[b]), ("v8", "v16", vs[b])):
            assert np.array_equal(vp.gather(kv8.widen(t[n8]), t["table"][b], L, 16), x)
            assert np.array_equal(vp.gather(t[n16], t["table"][b], L, 16), x)
        past = t["table"][b, vp.pages_of(L, 16)]
        assert past < 0 or past >= t["num_pages"]
    nan8 = np.isin(t["k8"], kv8.NAN_CODES)
    assert np.array_equal(nan8, np.isnan(t["k16"])) and (t["k8"] == 0x7F).any() and (t["k8"] == 0xFF).any()
    assert nan8[:, :, 8:].any() and nan8.reshape(len(nan8), -1).all(1).sum() >= 2  # tails of last pages, and whole spare pages
