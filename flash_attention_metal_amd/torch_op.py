"""torch.library custom op over the C-ABI.

    torch.ops.fa_mi355.attention_forward(q, k, v, is_causal, scale) -> (o, lse)

Lets the gfx950 kernel be called like any other torch operator (dispatcher, torch.compile graphs,
fake-tensor shape propagation) and compared in-process with scaled_dot_product_attention. The op is
registered for the CUDA/HIP device only -- there is deliberately no CPU implementation.

Autograd: the op carries a backward formula that saves (q, k, v, o, lse) and calls fa_bwd()
(csrc/fa_bwd_kernels.hip; the math of /root/reference/kernels.metal:905-1265, which consumes the
forward's LSE), through fa_bwd_ex: grouped-query heads (Hq % Hkv == 0) and Nq != Nk (causal: Nk >= Nq) are
differentiated too. Shapes fa_bwd_ex has no kernel for (head dims above 128 or not a multiple of 8, fp32 inputs)
raise instead of returning a silent zero gradient; so does a gradient flowing into the LSE output.

    torch.ops.fa_mi355.attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, scale) -> (o, lse)

The same over packed variable-length sequences (fa_fwd_varlen / fa_bwd_varlen): q [total_q, Hq, D], k / v [total_k, Hkv, D], lse
[Hq, total_q]. Its backward writes into zero-initialised fp32 buffers, so tokens that belong to no sequence get a zero gradient, and
returns the gradients in the input dtype.

    torch.ops.fa_mi355.attention_varlen_window(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right,
                                               scale) -> (o, lse)

attention_varlen under a sliding window (fa_fwd_varlen_window / fa_bwd_varlen_window; a negative side is unbounded), differentiable in the
same way. attention_varlen(..., window=(left, right)) dispatches to it.

    torch.ops.fa_mi355.attention_varlen_sink(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left,
                                             window_right, scale) -> (o, lse)

attention_varlen_window with one learnt sink logit per query head in every softmax denominator (fa_fwd_varlen_sink / fa_bwd_varlen_sink):
sinks [Hq], any float dtype. Autograd gives q, k, v AND sinks their gradients, the sinks' in the parameter's own dtype.
attention_varlen(..., sinks=) dispatches to it.

    torch.ops.fa_mi355.attention_varlen_mla(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, scale) -> (o, lse)

The MLA prefill (fa_fwd_varlen_mla / fa_bwd_varlen_mla): q [total_q, Hq, 192], k [total_k, Hkv, 192], v [total_k, Hkv, 128], o
[total_q, Hq, 128], each under its own strides; scale = 0.0 means 192 ** -0.5. Differentiable in q, k, v like attention_varlen.
"""
from __future__ import annotations

from typing import Tuple

import torch

from .ops import (_TORCH2FA, FaError, _out_dtype, _sink_window, _window, flash_attention_backward, flash_attention_forward, flash_attention_varlen,
                  flash_attention_varlen_backward, flash_attention_varlen_mla, flash_attention_varlen_mla_backward, load_library)

_LIB = torch.library.Library("fa_mi355", "DEF")
_LIB.define("attention_forward(Tensor q, Tensor k, Tensor v, bool is_causal=False, float scale=0.0) -> (Tensor, Tensor)")


def _impl(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, is_causal: bool = False, scale: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    o, lse = flash_attention_forward(q, k, v, is_causal=is_causal, scale=(scale if scale > 0 else None))
    return o, lse


def _meta(q, k, v, is_causal=False, scale=0.0):
    B, H, N, _ = q.shape
    return torch.empty_like(q, dtype=_out_dtype(q.dtype)), q.new_empty((B, H, N), dtype=torch.float32)


_LIB.impl("attention_forward", _impl, "CUDA")
_LIB.impl("attention_forward", _meta, "Meta")


def _setup_context(ctx, inputs, output):
    q, k, v, is_causal, scale = inputs
    o, lse = output
    ctx.save_for_backward(q, k, v, o, lse)
    ctx.is_causal, ctx.scale = bool(is_causal), float(scale)
    ctx.set_materialize_grads(False)


def _backward(ctx, grad_o, grad_lse):
    q, k, v, o, lse = ctx.saved_tensors
    if grad_lse is not None:
        raise NotImplementedError("fa_mi355::attention_forward: no gradient through the LSE output")
    if grad_o is None:
        return None, None, None, None, None
    B, H, N, D = q.shape
    gqa_ok = k.dim() == 4 and (k.shape[0], k.shape[3]) == (B, D) and H % k.shape[1] == 0 and not (ctx.is_causal and k.shape[2] < N)
    if not gqa_ok or q.dtype not in _TORCH2FA or not load_library().fa_bwd_supported(_TORCH2FA[q.dtype], D):
        raise FaError(-2, f"no backward kernel for q {tuple(q.shape)} k {tuple(k.shape)} {q.dtype} "
                          "(f16 / bf16 / e4m3, Hq % Hkv == 0, causal needs Nk >= Nq, head_dim a multiple of 8 up to 128, or 256)", "fa_bwd_ex")
    go = grad_o.to(o.dtype)  # (e4m3 inputs: O and its gradient are bf16)
    if go.stride() != q.stride():
        go = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(go)
    dq, dk, dv = flash_attention_backward(q, k, v, o, go, lse, is_causal=ctx.is_causal,
                                          scale=(ctx.scale if ctx.scale > 0 else None))
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype), None, None


torch.library.register_autograd("fa_mi355::attention_forward", _backward, setup_context=_setup_context, lib=_LIB)


def attention_forward(q, k, v, is_causal: bool = False, scale: float = 0.0):
    return torch.ops.fa_mi355.attention_forward(q, k, v, is_causal, scale)


_LIB.define("attention_varlen(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
            "bool is_causal=False, float scale=0.0) -> (Tensor, Tensor)")


def _varlen_impl(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False, scale=0.0):
    # (O zero-initialised: tokens owned by no sequence are not written by the kernel, and the op's outputs are fully defined)
    out = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device).zero_()
    lse = torch.full((q.shape[1], q.shape[0]), float("-inf"), dtype=torch.float32, device=q.device)
    return flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=is_causal,
                                  scale=(scale if scale > 0 else None), out=out, lse=lse)


def _varlen_meta(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False, scale=0.0):
    return torch.empty_like(q), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)


_LIB.impl("attention_varlen", _varlen_impl, "CUDA")
_LIB.impl("attention_varlen", _varlen_meta, "Meta")


def _varlen_setup_context(ctx, inputs, output):
    q, k, v, cu_q, cu_k, max_q, max_k, is_causal, scale = inputs
    o, lse = output
    ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
    ctx.max_q, ctx.max_k, ctx.is_causal, ctx.scale = int(max_q), int(max_k), bool(is_causal), float(scale)
    ctx.set_materialize_grads(False)


def _varlen_backward(ctx, grad_o, grad_lse):
    q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
    if grad_lse is not None:
        raise NotImplementedError("fa_mi355::attention_varlen: no gradient through the LSE output")
    none = (None,) * 9
    if grad_o is None:
        return none
    if q.dtype not in _TORCH2FA or not load_library().fa_bwd_varlen_supported(_TORCH2FA[q.dtype], q.shape[2]):
        raise FaError(-2, f"no varlen backward kernel for q {tuple(q.shape)} {q.dtype} (f16 / bf16, head_dim 64 or 128)", "fa_bwd_varlen")
    go = grad_o.to(o.dtype)
    if go.stride() != q.stride():  # d_o is addressed under q's strides
        go = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(go)
    if o.stride() != q.stride():
        o = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(o)
    # zero-initialised: tokens owned by no sequence are not written by the kernels and get a zero gradient
    dq = torch.empty_strided(q.shape, q.stride(), dtype=torch.float32, device=q.device).zero_()
    dk = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    dv = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    flash_attention_varlen_backward(q, k, v, o, go, lse, cu_q, cu_k, ctx.max_q, ctx.max_k, is_causal=ctx.is_causal,
                                    scale=(ctx.scale if ctx.scale > 0 else None), dq=dq, dk=dk, dv=dv)
    return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)) + none[3:]


torch.library.register_autograd("fa_mi355::attention_varlen", _varlen_backward, setup_context=_varlen_setup_context, lib=_LIB)


_LIB.define("attention_varlen_window(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, "
            "int max_seqlen_k, int window_left, int window_right, float scale=0.0) -> (Tensor, Tensor)")


def _varlen_window_impl(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right, scale=0.0):
    out = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device).zero_()
    lse = torch.full((q.shape[1], q.shape[0]), float("-inf"), dtype=torch.float32, device=q.device)
    return flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale=(scale if scale > 0 else None),
                                  out=out, lse=lse, window=(window_left, window_right))


def _varlen_window_meta(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right, scale=0.0):
    return torch.empty_like(q), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)


_LIB.impl("attention_varlen_window", _varlen_window_impl, "CUDA")
_LIB.impl("attention_varlen_window", _varlen_window_meta, "Meta")


def _varlen_window_setup_context(ctx, inputs, output):
    q, k, v, cu_q, cu_k, max_q, max_k, window_left, window_right, scale = inputs
    o, lse = output
    ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
    ctx.max_q, ctx.max_k, ctx.window, ctx.scale = int(max_q), int(max_k), (int(window_left), int(window_right)), float(scale)
    ctx.set_materialize_grads(False)


def _varlen_window_backward(ctx, grad_o, grad_lse):
    q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
    if grad_lse is not None:
        raise NotImplementedError("fa_mi355::attention_varlen_window: no gradient through the LSE output")
    none = (None,) * 10
    if grad_o is None:
        return none
    if q.dtype not in _TORCH2FA or not load_library().fa_bwd_varlen_supported(_TORCH2FA[q.dtype], q.shape[2]):
        raise FaError(-2, f"no varlen backward kernel for q {tuple(q.shape)} {q.dtype} (f16 / bf16, head_dim 64 or 128)", "fa_bwd_varlen_window")
    go = grad_o.to(o.dtype)
    if go.stride() != q.stride():  # d_o is addressed under q's strides
        go = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(go)
    if o.stride() != q.stride():
        o = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(o)
    # zero-initialised: tokens owned by no sequence are not written by the kernels and get a zero gradient
    dq = torch.empty_strided(q.shape, q.stride(), dtype=torch.float32, device=q.device).zero_()
    dk = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    dv = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    flash_attention_varlen_backward(q, k, v, o, go, lse, cu_q, cu_k, ctx.max_q, ctx.max_k, scale=(ctx.scale if ctx.scale > 0 else None),
                                    dq=dq, dk=dk, dv=dv, window=ctx.window)
    return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)) + none[3:]


torch.library.register_autograd("fa_mi355::attention_varlen_window", _varlen_window_backward, setup_context=_varlen_window_setup_context,
                                lib=_LIB)


_LIB.define("attention_varlen_sink(Tensor q, Tensor k, Tensor v, Tensor sinks, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, "
            "int max_seqlen_k, int window_left, int window_right, float scale=0.0) -> (Tensor, Tensor)")


def _varlen_sink_impl(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right, scale=0.0):
    out = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device).zero_()
    lse = torch.full((q.shape[1], q.shape[0]), float("-inf"), dtype=torch.float32, device=q.device)
    return flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale=(scale if scale > 0 else None),
                                  out=out, lse=lse, window=(window_left, window_right), sinks=sinks)


def _varlen_sink_meta(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right, scale=0.0):
    return torch.empty_like(q), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)


_LIB.impl("attention_varlen_sink", _varlen_sink_impl, "CUDA")
_LIB.impl("attention_varlen_sink", _varlen_sink_meta, "Meta")


def _varlen_sink_setup_context(ctx, inputs, output):
    q, k, v, sinks, cu_q, cu_k, max_q, max_k, window_left, window_right, scale = inputs
    o, lse = output
    ctx.save_for_backward(q, k, v, sinks, o, lse, cu_q, cu_k)
    ctx.max_q, ctx.max_k, ctx.window, ctx.scale = int(max_q), int(max_k), (int(window_left), int(window_right)), float(scale)
    ctx.set_materialize_grads(False)


def _varlen_sink_backward(ctx, grad_o, grad_lse):
    q, k, v, sinks, o, lse, cu_q, cu_k = ctx.saved_tensors
    if grad_lse is not None:
        raise NotImplementedError("fa_mi355::attention_varlen_sink: no gradient through the LSE output")
    none = (None,) * 11
    if grad_o is None:
        return none
    if q.dtype not in _TORCH2FA or not load_library().fa_bwd_varlen_supported(_TORCH2FA[q.dtype], q.shape[2]):
        raise FaError(-2, f"no varlen backward kernel for q {tuple(q.shape)} {q.dtype} (f16 / bf16, head_dim 64 or 128)", "fa_bwd_varlen_sink")
    go = grad_o.to(o.dtype)
    if go.stride() != q.stride():  # d_o is addressed under q's strides
        go = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(go)
    if o.stride() != q.stride():
        o = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(o)
    # zero-initialised: tokens owned by no sequence are not written by the kernels and get a zero gradient
    dq = torch.empty_strided(q.shape, q.stride(), dtype=torch.float32, device=q.device).zero_()
    dk = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    dv = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    _, _, _, dsinks = flash_attention_varlen_backward(q, k, v, o, go, lse, cu_q, cu_k, ctx.max_q, ctx.max_k,
                                                      scale=(ctx.scale if ctx.scale > 0 else None), dq=dq, dk=dk, dv=dv, window=ctx.window,
                                                      sinks=sinks)
    return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype), dsinks.to(sinks.dtype)) + none[4:]


torch.library.register_autograd("fa_mi355::attention_varlen_sink", _varlen_sink_backward, setup_context=_varlen_sink_setup_context, lib=_LIB)


_LIB.define("attention_varlen_softcap(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, "
            "int max_seqlen_k, int window_left, int window_right, float softcap, float scale=0.0) -> (Tensor, Tensor)")


def _varlen_softcap_impl(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right, softcap, scale=0.0):
    if not softcap > 0:  # (0.0 would quietly be the call without a cap in the wrapper)
        raise ValueError("fa_mi355::attention_varlen_softcap: softcap must be finite and > 0")
    out = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device).zero_()
    lse = torch.full((q.shape[1], q.shape[0]), float("-inf"), dtype=torch.float32, device=q.device)
    return flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scale=(scale if scale > 0 else None),
                                  out=out, lse=lse, window=(window_left, window_right), softcap=softcap)


def _varlen_softcap_meta(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window_left, window_right, softcap, scale=0.0):
    return torch.empty_like(q), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)


_LIB.impl("attention_varlen_softcap", _varlen_softcap_impl, "CUDA")
_LIB.impl("attention_varlen_softcap", _varlen_softcap_meta, "Meta")


def _varlen_softcap_setup_context(ctx, inputs, output):
    q, k, v, cu_q, cu_k, max_q, max_k, window_left, window_right, softcap, scale = inputs
    o, lse = output
    ctx.save_for_backward(q, k, v, o, lse, cu_q, cu_k)
    ctx.max_q, ctx.max_k, ctx.window, ctx.scale = int(max_q), int(max_k), (int(window_left), int(window_right)), float(scale)
    ctx.softcap = float(softcap)
    ctx.set_materialize_grads(False)


def _varlen_softcap_backward(ctx, grad_o, grad_lse):
    q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
    if grad_lse is not None:
        raise NotImplementedError("fa_mi355::attention_varlen_softcap: no gradient through the LSE output")
    none = (None,) * 11  # (the cap is a host scalar: no gradient)
    if grad_o is None:
        return none
    if q.dtype not in _TORCH2FA or not load_library().fa_bwd_varlen_supported(_TORCH2FA[q.dtype], q.shape[2]):
        raise FaError(-2, f"no varlen backward kernel for q {tuple(q.shape)} {q.dtype} (f16 / bf16, head_dim 64 or 128)", "fa_bwd_varlen_softcap")
    go = grad_o.to(o.dtype)
    if go.stride() != q.stride():  # d_o is addressed under q's strides
        go = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(go)
    if o.stride() != q.stride():
        o = torch.empty_strided(q.shape, q.stride(), dtype=o.dtype, device=q.device).copy_(o)
    # zero-initialised: tokens owned by no sequence are not written by the kernels and get a zero gradient
    dq = torch.empty_strided(q.shape, q.stride(), dtype=torch.float32, device=q.device).zero_()
    dk = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    dv = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    flash_attention_varlen_backward(q, k, v, o, go, lse, cu_q, cu_k, ctx.max_q, ctx.max_k, scale=(ctx.scale if ctx.scale > 0 else None),
                                    dq=dq, dk=dk, dv=dv, window=ctx.window, softcap=ctx.softcap)
    return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)) + none[3:]


torch.library.register_autograd("fa_mi355::attention_varlen_softcap", _varlen_softcap_backward, setup_context=_varlen_softcap_setup_context,
                                lib=_LIB)


_LIB.define("attention_varlen_mla(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
            "bool is_causal=False, float scale=0.0) -> (Tensor, Tensor)")


def _varlen_mla_impl(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False, scale=0.0):
    # (O zero-initialised and LSE -inf-initialised: tokens owned by no sequence are not written by the kernel)
    out = torch.zeros((q.shape[0], q.shape[1], v.shape[2]), dtype=q.dtype, device=q.device)
    lse = torch.full((q.shape[1], q.shape[0]), float("-inf"), dtype=torch.float32, device=q.device)
    return flash_attention_varlen_mla(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=is_causal,
                                      scale=(scale if scale > 0 else None), out=out, lse=lse)


def _varlen_mla_meta(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False, scale=0.0):
    return q.new_empty((q.shape[0], q.shape[1], v.shape[2])), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)


_LIB.impl("attention_varlen_mla", _varlen_mla_impl, "CUDA")
_LIB.impl("attention_varlen_mla", _varlen_mla_meta, "Meta")


def _varlen_mla_backward(ctx, grad_o, grad_lse):
    q, k, v, o, lse, cu_q, cu_k = ctx.saved_tensors
    if grad_lse is not None:
        raise NotImplementedError("fa_mi355::attention_varlen_mla: no gradient through the LSE output")
    none = (None,) * 9
    if grad_o is None:
        return none
    if q.dtype not in _TORCH2FA or not load_library().fa_bwd_varlen_mla_supported(_TORCH2FA[q.dtype], q.shape[2], v.shape[2]):
        raise FaError(-2, f"no MLA backward kernel for q {tuple(q.shape)} v {tuple(v.shape)} {q.dtype} (f16 / bf16, head dims 192 / 128)",
                      "fa_bwd_varlen_mla")
    go = grad_o.to(o.dtype)
    if go.stride() != o.stride():  # d_o is addressed under o's strides
        go = torch.empty_strided(o.shape, o.stride(), dtype=o.dtype, device=q.device).copy_(go)
    # zero-initialised: tokens owned by no sequence are not written by the kernels and get a zero gradient
    dq = torch.empty_strided(q.shape, q.stride(), dtype=torch.float32, device=q.device).zero_()
    dk = torch.empty_strided(k.shape, k.stride(), dtype=torch.float32, device=q.device).zero_()
    dv = torch.empty_strided(v.shape, v.stride(), dtype=torch.float32, device=q.device).zero_()
    flash_attention_varlen_mla_backward(q, k, v, o, go, lse, cu_q, cu_k, ctx.max_q, ctx.max_k, is_causal=ctx.is_causal,
                                        scale=(ctx.scale if ctx.scale > 0 else None), dq=dq, dk=dk, dv=dv)
    return (dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)) + none[3:]


# (the context is attention_varlen's: the same inputs, outputs and host scalars)
torch.library.register_autograd("fa_mi355::attention_varlen_mla", _varlen_mla_backward, setup_context=_varlen_setup_context, lib=_LIB)


def attention_varlen_mla(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q: int, max_seqlen_k: int, is_causal: bool = False, scale: float = 0.0):
    """fa_mi355::attention_varlen_mla: the MLA prefill (head dims 192 / 128), differentiable in q, k, v through fa_bwd_varlen_mla."""
    return torch.ops.fa_mi355.attention_varlen_mla(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, scale)


def attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q: int, max_seqlen_k: int, is_causal: bool = False, scale: float = 0.0,
                     window=None, sinks=None, softcap=None):
    """window=(left, right): fa_mi355::attention_varlen_window (differentiable through fa_bwd_varlen_window); None: the op above.
    sinks=[Hq] logits: fa_mi355::attention_varlen_sink (differentiable in q, k, v and sinks; window=None is (-1, 0) under is_causal, else
    (-1, -1)). softcap=a positive float: fa_mi355::attention_varlen_softcap (differentiable in q, k, v through fa_bwd_varlen_softcap; the
    window maps as with sinks; not together with sinks); None or 0.0: the ops above."""
    if softcap is not None and float(softcap) != 0.0:
        if sinks is not None:
            raise ValueError("softcap together with sinks is not supported")
        left, right = _sink_window(window, is_causal)
        return torch.ops.fa_mi355.attention_varlen_softcap(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, left, right,
                                                           float(softcap), scale)
    if sinks is not None:
        left, right = _sink_window(window, is_causal)
        return torch.ops.fa_mi355.attention_varlen_sink(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, left, right, scale)
    if window is None:
        return torch.ops.fa_mi355.attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, scale)
    left, right = _window(window, is_causal)
    return torch.ops.fa_mi355.attention_varlen_window(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, left, right, scale)
