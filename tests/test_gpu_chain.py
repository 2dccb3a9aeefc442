"""The backward on the FORWARD's own O and LSE, element by element -- the chain every caller runs (training, torch.ops.fa_mi355).

The other per-element backward tests (test_gpu_backward_rows.py, test_gpu_backward_probes.py) feed the kernels the fp64 oracle's O and
LSE. Here a forward kernel of ours writes them, and every case computes two ratios per tensor, worst |g - ref| / bound over all elements:
  given  the kernels' gradients against the given-input reference of tests/backward_bound.py: the documented gradient formula in fp64 on
         the very O and LSE the backward was fed. Judges the backward alone, on inputs the oracle-fed tests never produce.
  true   the same gradients against the fp64 gradient of the operator, under the bound of backward_bound.py with the lse_err / o_err that
         tests/chain_bound.py derives from what include/fa_mi355.h documents for the forward route (never from a kernel's output).
Both must be at most 1.0 on every element; every case prints both ("CHAIN ..."). tests/test_chain_bound_model.py shows on the CPU that a
model of the kernels' roundings stays inside both bounds and which sabotaged O / LSE leave them.
given > 1: the backward itself is at fault. given <= 1 < true: a forward route delivers an O or LSE outside what the header documents.

Families: (a) fa_fwd by name into fa_bwd; (b) fa_fwd_exv into fa_bwd_ex, grouped rectangular shapes, contiguous and as NaN-padded views;
(c) the dense custom op through torch.autograd (gradients in the input dtype: one more rounding, u |g| (+ 2^-25 for f16), with
|g| <= |ref| + bound); (d) e4m3 inputs; (e) the ramp of tests/score_range.py, rows the forward's reference had to climb for.
f16 mfma16's low-probability term (header, "LSE accuracy") is asserted to be zero per case in (a)-(c) and added from the fp64 scores in (e).

"Nq != Nk full scale 0.3" of (c) keeps head_dim 128, where three f16 scores lie more than 11 log2 units below their row maximum: that
one case takes the term from the fp64 scores as (e) does (LOW_TERM) instead of moving to a shape that avoids it.
The printed forward figures (fwd lse, o) are |kernel - exact| / lse_err, o_err, over the elements with a bound; where o_err is exactly 0
(e4m3 inputs: O and sum_j P |v| both 0) the error is asserted to be 0.

No measured ratio is recorded here yet: this file has not had a passing run on the MI355X, so there is no table of worst ratios and no
log under profiles/. (The CPU model of tests/test_chain_bound_model.py: given 0.36, true 0.36.)
"""
import numpy as np
import pytest

import backward_bound as bb
import chain_bound as cb
import score_range as sr
from test_gpu_backward_rows import inputs, padded
from util import TORCH_DTYPE, need, to_dev

pytestmark = pytest.mark.gpu
WORST = {}  # (family, dtype, kind) -> [dq, dk, dv]


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available()
    fa.load_library()
    yield fa
    for (family, dtype, kind), r in sorted(WORST.items()):
        print(f"CHAIN WORST {family} {dtype:4s} {kind:5s} dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")


def resolve(fa, route, dtype, B, H, N, D, causal):
    """The kernel a route of fa_fwd runs, by name (AUTO: fa_resolve_variant_for)."""
    if route != "auto":
        return route
    v = fa.load_library().fa_resolve_variant_for(fa.DTYPES[{"fp8": "fp8_e4m3"}.get(dtype, dtype)], D, B, H, N, int(causal))
    name = {n: s for s, n in fa.VARIANTS.items()}[v]
    assert name in cb.KERNELS, (name, "AUTO left the matrix-core kernels")
    return name


def bwd_square(fa, q, k, v, o, do, lse, causal, scale, dtype):
    """fa_bwd itself (flash_attention_backward goes through fa_bwd_ex): contiguous [B,H,N,D] tensors, one stride pair."""
    import torch

    lib = fa.load_library()
    B, H, N, D = q.shape
    assert all(t.is_contiguous() and t.shape == q.shape for t in (q, k, v, o, do)) and lse.is_contiguous() and lse.shape == (B, H, N)
    dq, dk, dv = (torch.empty((B, H, N, D), dtype=torch.float32, device=q.device) for _ in range(3))
    ws = torch.empty(max(int(lib.fa_bwd_workspace_bytes(B, H, N)), 16), dtype=torch.uint8, device=q.device)
    st = lib.fa_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                    dv.data_ptr(), ws.data_ptr(), B, H, N, D, float(scale), H * N * D, N * D, int(causal), fa.DTYPES[dtype],
                    torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.fa_last_error().decode()
    return dq, dk, dv


def worst_ratio(err, bound, tag):
    """max err / bound over the elements with a bound; where the bound is exactly 0 (e4m3 inputs: O and sum_j P |v| both 0) so is the error."""
    pos = bound > 0
    assert (err[~pos] == 0).all(), (tag, "an error where the bound is exactly 0")
    return float((err[pos] / bound[pos]).max())


def judge(family, tag, q, k, v, do, dtype, causal, scale, kernels, o_t, lse_t, grads, rounded_to=None, low_term=False):
    """Both ratios of one chain: o_t / lse_t the tensors the backward consumed, grads its three gradients (torch); rounded_to: the 16-bit
    type the gradients were rounded to on their way out (the custom op), which the bounds then allow for. f16 mfma16's documented
    low-probability term n * 2^-22 (chain_bound adds it from the fp64 scores) is asserted to be zero unless the case says low_term."""
    import torch

    torch.cuda.synchronize()
    D = q.shape[-1]
    scale = bb.default_scale(D) if scale is None else float(scale)
    if dtype == "f16" and "mfma16" in kernels:
        n_low = cb.low_probability_rows(q, k, causal, scale)
        if low_term:
            print(f"CHAIN {family} f16 {tag}: at most {n_low} visible scores of a row lie more than 11 log2 units below its maximum (n * 2^-22 in lse_err)")
        else:
            assert n_low == 0, (tag, "f16 mfma16: a visible score more than 11 log2 units below its row maximum")
    le, oe = cb.errors(q, k, v, causal, scale, dtype, kernels)
    o_in, lse_in = o_t.float().cpu().numpy().astype(np.float64), lse_t.cpu().numpy().astype(np.float64)
    assert np.isfinite(o_in).all() and np.isfinite(lse_in).all(), tag
    X = bb.Bounds(q, k, v, do, causal, scale, dtype, lse_err=le, o_err=oe, o_in=o_in, lse_in=lse_in)
    g = [t.float().cpu().numpy() for t in grads]
    assert g[0].shape == q.shape and g[1].shape == k.shape and g[2].shape == k.shape
    out = {}
    for kind, ref, bound in (("given", X.given_ref, X.given_bound), ("true", X.ref, X.bound)):
        if rounded_to is not None:
            bound = [b + bb.U[rounded_to] * (np.abs(r) + b) + bb.TINY[rounded_to] for r, b in zip(ref, bound)]
        out[kind] = bb.ratios(g, ref, bound)
        w = WORST.setdefault((family, dtype, kind), [0.0, 0.0, 0.0])
        w[:] = [max(a, b) for a, b in zip(w, out[kind])]
    fwd = (worst_ratio(np.abs(lse_in - X.lse), le, tag), worst_ratio(np.abs(o_in - X.o), oe, tag))
    print(f"CHAIN {family} {dtype} {tag} Hq{q.shape[1]} Hkv{k.shape[1]} Nq{q.shape[2]} Nk{k.shape[2]} D{D} causal={int(causal)} kernels={'/'.join(kernels)}"
          f" | fwd lse {fwd[0]:.3f} o {fwd[1]:.3f} | given dq {out['given'][0]:.3f} dk {out['given'][1]:.3f} dv {out['given'][2]:.3f}"
          f" | true dq {out['true'][0]:.3f} dk {out['true'][1]:.3f} dv {out['true'][2]:.3f}")
    for x in g:
        assert np.isfinite(x).all(), tag
    for kind in ("given", "true"):
        assert max(out[kind]) <= 1.0, (family, kind, dtype, tag, q.shape, k.shape, causal, kernels, out[kind])
    return out


MHA = ((1, 2, 65), (2, 2, 203), (1, 2, 520))  # one tile + 1; two 128-row blocks with a ragged tail, two batch entries; five blocks
RECT = ((1, 4, 2, 130, 200), (2, 8, 1, 66, 129))  # B, Hq, Hkv, Nq, Nk


@pytest.mark.parametrize("D", [64, 128, 96, 40, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("route", ["mfma", "mfma_exact", "mfma16", "mfma_splitkv", "mfma_split2", "mfma_h64s2", "auto"])
def test_fa_fwd_into_fa_bwd(fa, oracle_mod, route, dtype, D):
    """(a) fa_fwd by name (and AUTO, resolved with fa_resolve_variant_for) into fa_bwd."""
    need(fa, dtype, route, D)
    for (B, H, N) in MHA:
        q, k, v, do = inputs(oracle_mod, dtype, B, H, H, N, N, D)
        qd, kd, vd, dod = (to_dev(x, dtype) for x in (q, k, v, do))
        for causal in (False, True):
            o, lse = fa.flash_attention_forward(qd, kd, vd, is_causal=causal, variant=route)
            grads = bwd_square(fa, qd, kd, vd, o, dod, lse, causal, D ** -0.5, dtype)
            judge("a", route, q, k, v, do, dtype, causal, None, [resolve(fa, route, dtype, B, H, N, D, causal)], o, lse, grads)


@pytest.mark.parametrize("D", [64, 128, 40, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("route", ["auto", "mfma", "mfma_exact", "mfma16", "mfma_splitkv"])
def test_fa_fwd_exv_into_fa_bwd_ex(fa, oracle_mod, route, dtype, D):
    """(b) grouped heads on rectangular problems, contiguous and as views (Q / O / dO under one stride pair, K / V under another, NaN in
    the padding). AUTO of fa_fwd_ex has no exported resolver: the largest term over the kernels its rule may pick."""
    import torch

    need(fa, dtype, route, D)
    kernels = cb.kernels_of(route, dtype, ex=True)
    for (B, Hq, Hkv, Nq, Nk) in RECT:
        q, k, v, do = inputs(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D)
        for pad in (False, True):
            if pad:
                qd, dod, od = padded(q, dtype, 8, 1), padded(do, dtype, 8, 1), padded(np.zeros_like(q), dtype, 8, 1)
                kd, vd = padded(k, dtype, 24, 2), padded(v, dtype, 24, 2)
                assert qd.stride() == od.stride() == dod.stride() and kd.stride() == vd.stride() and not qd.is_contiguous()
            else:
                qd, kd, vd, dod = (to_dev(x, dtype) for x in (q, k, v, do))
                od = torch.empty_like(qd)
            for causal in (False, True):
                o, lse = fa.flash_attention_forward(qd, kd, vd, is_causal=causal, variant=route, out=od)
                assert o.data_ptr() == od.data_ptr()
                grads = fa.flash_attention_backward(qd, kd, vd, o, dod, lse, is_causal=causal)
                judge("b", f"{route}{' padded' if pad else ''}", q, k, v, do, dtype, causal, None, kernels, o, lse, grads)


OP_CASES = {  # name -> (B, Hq, Hkv, Nq, Nk, D, causal, scale, padded view)
    "mha": (2, 2, 2, 203, 203, 64, True, None, False),
    "mha full D=128 scale 0.3": (1, 2, 2, 203, 203, 128, False, 0.3, False),
    "grouped heads": (1, 4, 2, 203, 203, 64, True, None, False),
    "Nq != Nk D=128": (1, 4, 2, 130, 200, 128, True, None, False),
    # (at scale 0.3 and head_dim 128 three f16 scores of this shape lie more than 11 log2 units below their row maximum: the one case
    # of this family that takes the header's n * 2^-22 instead of asserting it away, see LOW_TERM)
    "Nq != Nk full scale 0.3": (2, 8, 1, 66, 129, 128, False, 0.3, False),
    "padded view": (2, 4, 2, 130, 200, 64, True, None, True),
    "padded view mha D=40": (2, 2, 2, 203, 203, 40, True, None, True),
}


LOW_TERM = ("Nq != Nk full scale 0.3",)


def through_the_op(fa, q, k, v, do, dtype, causal, scale, pad):
    """(O, LSE, (dQ, dK, dV)) of torch.ops.fa_mi355.attention_forward under autograd; the O and LSE come from a SECOND call of the op on
    the same tensors (the forward is bitwise reproducible: asserted)."""
    import torch

    import flash_attention_metal_amd.torch_op  # noqa: F401  (registers the op)

    odt = "bf16" if dtype == "fp8" else dtype
    if pad:  # (equal shapes go to fa_fwd, which takes one stride pair for Q, K and V)
        kpad = (8, 1) if q.shape == k.shape else (24, 2)
        qd, kd, vd, dod = padded(q, dtype, 8, 1), padded(k, dtype, *kpad), padded(v, dtype, *kpad), padded(do, odt, 8, 1)
    else:
        qd, kd, vd, dod = to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype), to_dev(do, odt)
    leaves = [t.detach().requires_grad_() for t in (qd, kd, vd)]
    assert all(a.stride() == b.stride() for a, b in zip(leaves, (qd, kd, vd)))
    s = 0.0 if scale is None else float(scale)
    o, lse = torch.ops.fa_mi355.attention_forward(*leaves, causal, s)
    o.backward(dod)
    with torch.no_grad():
        o2, lse2 = torch.ops.fa_mi355.attention_forward(qd, kd, vd, causal, s)
    torch.cuda.synchronize()
    assert torch.equal(o.detach().view(torch.int16), o2.view(torch.int16)) and torch.equal(lse.detach(), lse2), "the forward is not bitwise reproducible"
    grads = [t.grad for t in leaves]
    assert all(g is not None and g.dtype == getattr(torch, TORCH_DTYPE[dtype]) for g in grads)
    return o2, lse2, grads


@pytest.mark.parametrize("case", list(OP_CASES))
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dense_op_autograd(fa, oracle_mod, dtype, case):
    """(c) MHA, grouped heads, Nq != Nk, padded views, scale given and default; gradients in the input dtype."""
    B, Hq, Hkv, Nq, Nk, D, causal, scale, pad = OP_CASES[case]
    q, k, v, do = inputs(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D)
    o, lse, grads = through_the_op(fa, q, k, v, do, dtype, causal, scale, pad)
    square = (Hq, Nq) == (Hkv, Nk)  # (equal shapes: fa_fwd and its AUTO; else fa_fwd_ex's)
    kernels = [resolve(fa, "auto", dtype, B, Hq, Nq, D, causal)] if square else cb.kernels_of("auto", dtype, ex=True)
    judge("c", case, q, k, v, do, dtype, causal, scale, kernels, o, lse, grads, rounded_to=dtype, low_term=case in LOW_TERM)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("route", ["mfma", "mfma_exact", "mfma_fp8pv", "op"])
def test_e4m3_inputs(fa, oracle_mod, route, D):
    """(d) e4m3 Q, K, V (the suite's e4m3 family: U(-1,1) x 2), bf16 O and dO: the forward by name into fa_bwd_ex, and the custom op
    (its AUTO resolved; gradients come back in e4m3 there, which is no 16-bit rounding the bound knows: the op's case judges the fp32
    gradients of flash_attention_backward on the op's O and LSE and asserts that the op returns exactly their e4m3 roundings)."""
    import torch

    dtype = "fp8"
    if route != "op":
        need(fa, dtype, route, D)
    for (B, Hq, Hkv, Nq, Nk) in ((2, 2, 2, 203, 203), (1, 4, 2, 130, 200) if route in ("mfma", "mfma_exact", "op") else (1, 2, 2, 520, 520)):
        q, k, v, do = inputs(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D, amp=2.0)
        for causal in (False, True):
            qd, kd, vd, dod = to_dev(q, dtype), to_dev(k, dtype), to_dev(v, dtype), to_dev(do, "bf16")
            square = (Hq, Nq) == (Hkv, Nk)
            if route == "op":
                o, lse, op_grads = through_the_op(fa, q, k, v, do, dtype, causal, None, False)
                kernels = [resolve(fa, "auto", dtype, B, Hq, Nq, D, causal)] if square else cb.kernels_of("auto", dtype, ex=True)
            else:
                o, lse = fa.flash_attention_forward(qd, kd, vd, is_causal=causal, variant=route)
                kernels = [route]
            assert o.dtype == torch.bfloat16
            grads = fa.flash_attention_backward(qd, kd, vd, o, dod, lse, is_causal=causal)
            judge("d", route, q, k, v, do, dtype, causal, None, kernels, o, lse, grads)
            if route == "op":
                for a, b in zip(op_grads, grads):
                    assert torch.equal(a.float(), b.to(a.dtype).float())


@pytest.mark.parametrize("route", ["mfma16", "auto"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_ramp_rows_the_reference_climbs_for(fa, oracle_mod, dtype, route):
    """(e) sr.ramp at N = 300 (every 32-row group holds rows from depth 0 to -20 log2 units): the forward's first tile starts from an
    assumed maximum of 0 and has to find the row's own. Held to the same two bounds, element by element (the whole-tensor
    test_backward_on_the_forward_lse_of_a_ramp stays beside it)."""
    c = sr.ramp(oracle_mod.round_to, dtype, 300, -20.0)
    B, H, N, D = c.q.shape
    do = oracle_mod.round_to(np.random.default_rng(10).uniform(-1, 1, c.q.shape).astype(np.float32), dtype)
    qd, kd, vd, dod = (to_dev(x, dtype) for x in (c.q, c.k, c.v, do))
    for causal in (False, True):
        kernel = resolve(fa, route, dtype, B, H, N, D, causal)
        o, lse = fa.flash_attention_forward(qd, kd, vd, is_causal=causal, variant=route)
        grads = bwd_square(fa, qd, kd, vd, o, dod, lse, causal, D ** -0.5, dtype)
        judge("e", route, c.q, c.k, c.v, do, dtype, causal, None, [kernel], o, lse, grads, low_term=True)
