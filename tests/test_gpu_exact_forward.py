"""GPU: every forward entry point on exact-arithmetic inputs (tests/exact_forward.py), EVERY element of O and
LSE held to the per-element bar: the rounding of O to its type plus the epilogue's few fp32 operations (family A, rows the criterion
proves), plus n * 2^-24 * sum p |v| where fp32 partial sums may round (family B, unproven rows). The reference is fp64 numpy of the
same operator; nothing comes from the kernels' output. Each test prints its worst error / bar ("EXACT ..." lines; above 1 fails).

Every family-A case must be PROVEN exact on every row it checks (hold() asserts it): bar A is never replaced silently by the wider one.
The cases come from the catalogue in tests/exact_forward.py, which tests/test_exact_forward_cases.py walks on the CPU.
Not covered here, on purpose: the scalar variants (natural exp: not exact on these inputs)."""
import numpy as np
import pytest

import exact_forward as ef
from util import MFMA_VARIANTS, need, to_dev

pytestmark = pytest.mark.gpu

SPLITS = {"mfma_splitkv": 8, "mfma_split2": 2, "mfma_h64s2": 2}  # key splits the kernel merges (each with a maximum of its own)
SPLIT_ANY = 8  # AUTO of the generalised entry points may pick the split-KV kernel: its criterion (2 * span) and its merge terms (S = 8)
WORST = {}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    yield fa
    # the summary README and profiles/ quote: worst error / bar per entry point, dtype and family over what this module ran
    for (entry, dtype, family), w in sorted(WORST.items()):
        print(f"EXACT-SUMMARY {entry} {dtype} family {family}: worst O error / bar {w['o']:.3f}, worst LSE error / bar {w['lse']:.3f}")


def resolved(fa, variant, dtype, B, H, N, D, causal):
    if variant != "auto":
        return variant
    names = {v: k for k, v in fa.VARIANTS.items()}
    return names[fa.load_library().fa_resolve_variant_for(fa.DTYPES[{"fp8": "fp8_e4m3"}.get(dtype, dtype)], D, B, H, N, int(causal))]


def hold(case, o, lse, heads, entry, what, split=0, shift=0.0, rows=None):
    """Every element of the given heads against the bar; records and prints the worst ratio. Family A: every row proven, or it fails."""
    worst = dict(o=0.0, lse=0.0, proven=1.0)
    for (b, h) in heads:
        ref = ef.reference_head(case, b, h, rows)
        oh, lh = o[b, h].float().cpu().numpy(), lse[b, h].cpu().numpy()
        if rows is not None:
            oh, lh = oh[rows], lh[rows]
        r = ef.ratios(case, ref, oh, lh, split, shift)
        assert r["o"] <= 1.0 and r["lse"] <= 1.0, (entry, what, case.family, (b, h), r)
        assert case.family == "B" or r["proven"] == 1.0, (entry, what, (b, h), "a family-A row is not proven exact: bar A would not apply")
        worst = dict(o=max(worst["o"], r["o"]), lse=max(worst["lse"], r["lse"]), proven=min(worst["proven"], r["proven"]))
    key = (entry, case.dtype, case.family)
    w = WORST.setdefault(key, dict(o=0.0, lse=0.0))
    w["o"], w["lse"] = max(w["o"], worst["o"]), max(w["lse"], worst["lse"])
    print(f"EXACT {entry} {case.dtype} {case.family} {what}: O {worst['o']:.3f} LSE {worst['lse']:.3f} of bar (rows proven exact: {worst['proven']:.2f})")
    return worst


def padded(x):
    """x inside a larger zero buffer: padded batch / head strides."""
    import torch

    B, H, N, D = x.shape
    buf = torch.zeros(B, H + 1, N + 8, D, dtype=torch.float32, device="cuda").to(x.dtype)
    view = buf[:, :H, :N, :]
    view.copy_(x)
    return view


def device(case, q_dtype=None, pad=False):
    qd, kd, vd = to_dev(case.q, q_dtype or case.dtype), to_dev(case.k, case.dtype), to_dev(case.v, case.dtype)
    return (padded(qd), padded(kd), padded(vd)) if pad else (qd, kd, vd)


def forward(fa, case, variant="auto", pad=False):
    import torch

    qd, kd, vd = device(case)
    if pad:
        qd, kd, vd = padded(qd), padded(kd), padded(vd)
    o, lse = fa.flash_attention_forward(qd, kd, vd, is_causal=case.causal, variant=variant, scale=case.scale)
    torch.cuda.synchronize()
    return o, lse


# ---- fa_fwd: every matrix-core variant, both sides of every tile / wave / block edge -------------------------------------------
@pytest.mark.parametrize("variant", MFMA_VARIANTS + ["auto"])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "fp8"])
@pytest.mark.parametrize("D", ef.GRID_D)
@pytest.mark.parametrize("causal", [False, True])
def test_fa_fwd_exact(fa, dtype, D, causal, variant):
    need(fa, dtype, variant, D)
    for spec in ef.grid_specs(dtype, D, causal):
        name = resolved(fa, variant, dtype, spec.B, spec.Hq, spec.Nq, D, causal)
        split, shift = SPLITS.get(name, 0), ef.reference_shift(name, dtype)
        case = ef.make(spec, split > 0 or variant == "auto", name == "mfma_fp8pv")  # (auto: the depth the split kernels need, whatever it picks)
        o, lse = forward(fa, case, variant)
        hold(case, o, lse, ef.heads_of(spec), "fa_fwd", f"{variant}->{name} D={D} N={spec.Nq} causal={causal} k={spec.kexp}", split, shift)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fa_fwd_exact_padded_strides(fa, dtype):
    for spec in ef.padded_specs("fa_fwd", dtype):
        name = resolved(fa, "auto", dtype, spec.B, spec.Hq, spec.Nq, spec.D, True)
        case = ef.make(spec, True)
        o, lse = forward(fa, case, "auto", pad=True)
        hold(case, o, lse, ef.heads_of(spec), "fa_fwd", f"padded strides auto->{name}", SPLITS.get(name, 0), ef.reference_shift(name, dtype))


# ---- the full-size shapes: code paths small shapes never reach (all rows of two heads; config 4's shard: sampled rows) ---------
def _full(fa, B, H, N, D, dtype, causal, variant, heads, want=None, kernel_suffix=None):
    name = resolved(fa, variant, dtype, B, H, N, D, causal)
    if want is not None:
        assert name == want, (name, want)
    if kernel_suffix is not None:
        kn = fa.forward_kernel_name({"fp8": "fp8_e4m3"}.get(dtype, dtype), D, causal, B, H, N)
        assert kn.endswith(kernel_suffix), kn
    split, shift = SPLITS.get(name, 0), ef.reference_shift(name, dtype)
    spec = ef.full_spec(B, H, N, D, dtype, causal, heads)
    case = ef.make(spec, split > 0, name == "mfma_fp8pv")
    o, lse = forward(fa, case, variant)
    hold(case, o, lse, heads, "fa_fwd", f"full {variant}->{name} {B}x{H}x{N} D={D} causal={causal}", split, shift, spec.rows)


@pytest.mark.parametrize("full", ef.FULL, ids=[f[0] for f in ef.FULL])
def test_full_size_exact(fa, full):
    _, B, H, N, D, dtype, causal, variant, heads, want, suffix = full
    _full(fa, B, H, N, D, dtype, causal, variant, heads, want, suffix)


@pytest.mark.parametrize("B,H,N,D,dtype,causal,want", ef.ROUTES)
def test_auto_routes_exact(fa, B, H, N, D, dtype, causal, want):
    # one shape per kernel AUTO can pick (the shapes of test_auto_routes_reach_every_kernel_and_match_the_oracle), through AUTO
    _full(fa, B, H, N, D, dtype, causal, "auto", [(0, 0), (0, H - 1)], want=want)


# ---- fa_fwd_ex / fa_fwd_exv: grouped heads, Nq != Nk ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_generalised_forward_exact(fa, dtype):
    for spec in ef.generalised_specs(dtype):
        D = spec.D
        for variant in ["auto", "mfma", "mfma_exact"] + (["mfma16"] if D in (64, 128) else []) + (["mfma_splitkv"] if D == 64 else []):
            # AUTO's choice is not asked for here: its cases take the stricter criterion and the merge terms of the split-KV kernel
            split = SPLIT_ANY if variant == "auto" else SPLITS.get(variant, 0)
            shifts = [ef.reference_shift(variant, dtype)] if variant != "auto" else [0.0, ef.reference_shift("mfma16", dtype)]
            case = ef.make(spec, split > 0)
            o, lse = forward(fa, case, variant)
            what = f"{variant} {tuple(spec[2:10])}"
            hold(case, o, lse, ef.heads_of(spec), "fa_fwd_exv", what, split, max(shifts))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fa_fwd_ex_c_entry_exact(fa, dtype):
    # fa_fwd_ex itself (the wrapper goes through fa_fwd_exv): the C entry point, AUTO only
    import torch

    lib = fa.load_library()
    for spec in ef.generalised_specs(dtype, 200, 1, ef.GENERALISED[:11]):
        case = ef.make(spec, True)
        qd, kd, vd = device(case)
        B, Hq, Hkv, Nq, Nk, D = spec.B, spec.Hq, spec.Hkv, spec.Nq, spec.Nk, spec.D
        o = torch.empty_like(qd)
        lse = torch.empty(B, Hq, Nq, dtype=torch.float32, device="cuda")
        st = lib.fa_fwd_ex(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), lse.data_ptr(), B, Hq, Hkv, Nq, Nk, D, case.scale,
                           Hq * Nq * D, Nq * D, Hkv * Nk * D, Nk * D, int(spec.causal), fa.DTYPES[dtype], torch.cuda.current_stream().cuda_stream)
        assert st == 0, lib.fa_last_error()
        torch.cuda.synchronize()
        hold(case, o, lse, ef.heads_of(spec), "fa_fwd_ex", f"{tuple(spec[2:10])}", SPLIT_ANY, ef.reference_shift("mfma16", dtype))


def test_generalised_forward_exact_padded_strides(fa):
    import torch

    for spec in ef.padded_specs("fa_fwd_exv"):
        for variant in ("mfma", "mfma16", "mfma_splitkv"):
            case = ef.make(spec, variant in SPLITS)
            qd, kd, vd = device(case, pad=True)
            o, lse = fa.flash_attention_forward(qd, kd, vd, is_causal=True, variant=variant, scale=case.scale)
            torch.cuda.synchronize()
            hold(case, o, lse, ef.heads_of(spec), "fa_fwd_exv", f"padded strides {variant}", SPLITS.get(variant, 0), ef.reference_shift(variant, "bf16"))


# ---- the decode entry points (dtype "kv8": bf16 queries on an e4m3 cache, fa_fwd_decode_kv8) ------------------------------------
def q_dtype(dtype):
    return "bf16" if dtype == "kv8" else dtype


@pytest.mark.parametrize("dtype", ["f16", "bf16", "fp8", "kv8"])
def test_decode_exact(fa, dtype):
    import torch

    for spec in ef.decode_specs(dtype):
        case = ef.make(spec, True)
        qd, kd, vd = device(case, q_dtype(dtype))
        o, lse = fa.flash_attention_decode(qd, kd, vd, is_causal=spec.causal, scale=case.scale)
        torch.cuda.synchronize()
        hold(case, o, lse, ef.heads_of(spec), "fa_fwd_decode_kv8" if dtype == "kv8" else "fa_fwd_decode", f"{tuple(spec[2:10])}",
             ef.decode_splits(spec.Nk))


@pytest.mark.parametrize("dtype", ["bf16", "kv8"])
def test_decode_exact_padded_strides(fa, dtype):
    import torch

    for spec in ef.padded_specs("decode", "fp8" if dtype == "kv8" else dtype):
        case = ef.make(spec, True)
        qd, kd, vd = device(case, q_dtype(dtype), pad=True)
        o, lse = fa.flash_attention_decode(qd, kd, vd, is_causal=True, scale=case.scale)
        torch.cuda.synchronize()
        hold(case, o, lse, ef.heads_of(spec), "fa_fwd_decode_kv8" if dtype == "kv8" else "fa_fwd_decode", "padded strides", ef.decode_splits(spec.Nk))


def paged_pools(case, P, layout, rng, spare=3):
    """The case's K / V scattered over shuffled pages (NaN in every unreferenced page and every slot past a sequence's length)."""
    B, Hkv, Nk, D = case.k.shape
    lens = case.lens
    npb = [(L + P - 1) // P for L in lens]
    mp = max(max(npb), 1)
    num_pages = sum(npb) + spare
    perm = rng.permutation(num_pages)
    kpool = np.full((num_pages, Hkv, P, D), np.nan, np.float32)
    vpool = np.full((num_pages, Hkv, P, D), np.nan, np.float32)
    table = np.full((B, mp), perm[-1], np.int32)
    used = 0
    for b, L in enumerate(lens):
        pages = perm[used:used + npb[b]]
        used += npb[b]
        table[b, :npb[b]] = pages
        for j, pg in enumerate(pages):
            n = min(P, L - j * P)
            kpool[pg, :, :n] = case.k[b, :, j * P:j * P + n]
            vpool[pg, :, :n] = case.v[b, :, j * P:j * P + n]
    lay = (lambda x: x) if layout == "HND" else (lambda x: x.transpose(0, 2, 1, 3))
    return to_dev(lay(kpool), case.dtype), to_dev(lay(vpool), case.dtype), table


@pytest.mark.parametrize("P", ef.PAGE_SIZES)
@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "fp8", "kv8"])
def test_decode_paged_exact(fa, P, layout, dtype):
    import torch

    rng = np.random.default_rng(P)
    for spec in ef.paged_specs(dtype, P):
        case = ef.make(spec, True)
        kp, vp, table = paged_pools(case, P, layout, rng)
        o, lse = fa.flash_attention_decode_paged(to_dev(case.q, q_dtype(dtype)), kp, vp, torch.from_numpy(table).cuda(),
                                                 torch.tensor(spec.lens, dtype=torch.int32).cuda(), is_causal=spec.causal, scale=case.scale, layout=layout)
        torch.cuda.synchronize()
        hold(case, o, lse, ef.heads_of(spec), "fa_fwd_decode_paged" + ("(kv8)" if dtype == "kv8" else ""), f"P={P} {layout} {tuple(spec[3:10])}",
             ef.decode_splits(spec.Nk))
