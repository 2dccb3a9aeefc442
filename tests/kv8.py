"""Helpers of the e4m3-pool prefill and the quantising append (fa_fwd_varlen_paged_kv8, fa_kv_append_paged_quant; include/fa_mi355.h,
"e4m3 pools in the prefill"). CPU only: torch's CPU casts are the references, tests/test_kv8_cases.py checks that they are what the
header says (exact widening of the 254 finite codes; round to nearest even with subnormals; NaN -- not saturation -- past 464, hence the
clamp first), tests/test_gpu_varlen_paged_kv8.py holds the kernels to them.

  * widen(codes): OCP e4m3 (e4m3fn) bytes -> fp32, exact; every such value is a bf16 value too;
  * quant_reference(x, mul): e4m3_rne(clamp(fp32(x) * mul, -448, 448)) as bytes;
  * twin_pools(...): an e4m3 pool and its bf16 twin on top of varlen_paged.build_pool: identical page order, spare pages, NaN in every
    slot nobody may read (bytes 0x7F and 0xFF in the e4m3 pool), one table entry outside the pool past each sequence's last page."""
import numpy as np
import torch

import varlen_paged as vp

E4M3 = torch.float8_e4m3fn
NAN_CODES = (0x7F, 0xFF)
FINITE_CODES = np.array([c for c in range(256) if c not in NAN_CODES], np.uint8)  # 254 of them; 0x00 and 0x80 are +0 and -0
MAX = 448.0  # 0x7E / 0xFE


def widen(codes):
    """uint8 e4m3 codes -> fp32 values (NaN for 0x7F / 0xFF)."""
    c = torch.from_numpy(np.ascontiguousarray(codes, np.uint8))
    return c.view(E4M3).to(torch.float32).numpy()


def decode_by_hand(code):
    """The value of one finite code from the format's definition (bias 7, 3 mantissa bits, subnormals below 2^-6)."""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    mag = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -mag if s else mag


def to_e4m3_bytes(x):
    """fp32 values that are e4m3 values (or NaN) -> their codes; NaN becomes 0x7F."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(E4M3).view(torch.uint8).numpy()


def quant_reference(x, mul, bug=None):
    """The stored byte of every element of x (a torch f16 / bf16 tensor, finite): clamp in fp32, then torch's CPU cast (RNE, subnormals).
    bug plants one mistake: "truncate" (round toward zero), "clamp_after" (the cast first: NaN above 464), "mul_after_rounding" (the
    product rounded to the input type before the conversion)."""
    m = torch.tensor(mul, dtype=torch.float32)
    y = x.to(torch.float32) * m
    if bug == "mul_after_rounding":
        y = y.to(x.dtype).to(torch.float32)
    if bug == "clamp_after":
        return y.to(E4M3).to(torch.float32).clamp(-MAX, MAX).to(E4M3).view(torch.uint8).numpy()
    y = y.clamp(-MAX, MAX)
    if bug == "truncate":
        grid = torch.from_numpy(np.sort(widen(FINITE_CODES[FINITE_CODES < 0x7F]))).to(torch.float32)  # the non-negative values, ascending
        idx = torch.searchsorted(grid, y.abs().contiguous(), right=True) - 1
        t = grid[idx.clamp(min=0)]
        y = torch.where(torch.signbit(y), -t, t)
    return y.to(E4M3).view(torch.uint8).numpy()


def all_patterns(dtype):
    """All 65536 bit patterns of a 16-bit float type as a tensor of that type, and the mask of the finite ones."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    x = bits.view(dtype)
    return x, torch.isfinite(x.to(torch.float32))


def draw_e4m3(rng, *shape):
    """U(-1, 1) rounded to the e4m3 grid, as fp32 (so a pool built from it is exact in e4m3 and in bf16)."""
    x = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    return widen(to_e4m3_bytes(x))


def twin_pools(ks, vs, P, rng, spare=2, max_pages=None):
    """dict(k8, v8: uint8 [num_pages, Hkv, P, D] codes; k16, v16: fp32 holding the same values widened (NaN where the codes are NaN);
    table; num_pages). ks / vs must hold e4m3 values. Unused slots and spare pages: NaN, alternating 0x7F / 0xFF in the e4m3 pool.
    The first table entry past a sequence's last page names a page outside the pool (num_pages + 3 or -2); later ones a spare page."""
    pool = vp.build_pool(ks, vs, P, rng=rng, spare=spare, max_pages=max_pages, fill=np.nan, unused="spare")
    out = dict(table=pool["table"].copy(), num_pages=pool["num_pages"], P=P)
    for b, k in enumerate(ks):
        n = vp.pages_of(k.shape[1], P)
        if n < out["table"].shape[1]:
            out["table"][b, n] = pool["num_pages"] + 3 if b % 2 else -2
    for name in ("k", "v"):
        x = pool[name]
        codes = to_e4m3_bytes(x)
        assert np.array_equal(widen(codes)[~np.isnan(x)], x[~np.isnan(x)]), "the caches must hold e4m3 values"
        nan = np.isnan(x)
        flip = nan & (np.arange(x.size).reshape(x.shape) % 2 == 1)
        codes[flip] = 0xFF
        out[name + "8"], out[name + "16"] = codes, widen(codes)
    return out
