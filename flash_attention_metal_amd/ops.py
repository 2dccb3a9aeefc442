"""The operator: flash_attention_forward(Q, K, V, is_causal) -> (O, LSE).

Argument meaning follows the reference binding table
(/root/reference/kernels.metal:600-613, host side /root/reference/main.mm:821-852):
tensors are ``[B, H, N, D]`` with rows contiguous; batch/head strides are taken
from the tensors; ``scale`` defaults to ``1/sqrt(D)`` (main.mm:13); ``lse`` is
``[B, H, N]`` fp32 (kernels.metal:611). Errors follow the C-ABI: a negative
status becomes :class:`FaError` carrying ``fa_last_error()``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ._lib import load_library

DTYPES = {"f32": 0, "f16": 1, "bf16": 2, "fp8_e4m3": 3}
VARIANTS = {"auto": 0, "naive": 1, "tiled": 2, "tiled_v2": 3, "mfma": 4, "mfma_pp": 5, "mfma_splitkv": 6, "mfma_split2": 7, "mfma_exact": 8, "mfma_h64s2": 9, "mfma16": 10, "mfma_fp8pv": 11}

_FP8 = getattr(torch, "float8_e4m3fn", None)  # (None on torch builds without it)
_TORCH2FA = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
if _FP8 is not None:
    _TORCH2FA[_FP8] = 3


class FaError(RuntimeError):
    def __init__(self, status: int, msg: str, entry: str = "fa_fwd"):
        super().__init__(f"{entry} failed ({status}): {msg}")
        self.status = status


def supported(dtype: str, variant: str, D: int) -> bool:
    return bool(load_library().fa_supported(DTYPES[dtype], VARIANTS[variant], D))


def algorithmic_flops(B: int, H: int, N: int, D: int, is_causal: bool) -> float:
    return float(load_library().fa_algorithmic_flops(B, H, N, D, int(is_causal)))


def algorithmic_bytes(B: int, H: int, N: int, D: int, dtype: str) -> float:
    return float(load_library().fa_algorithmic_bytes(B, H, N, D, DTYPES[dtype]))


def forward_kernel_name(dtype: str, D: int, is_causal: bool, B: int = 4, H: int = 16, N: int = 4096) -> str:
    """Name (as rocprofv3 prints it) of the device kernel variant "auto" launches for the problem."""
    return load_library().fa_fwd_kernel_name(DTYPES[dtype], D, B, H, N, int(is_causal)).decode()


def _strides(t: torch.Tensor) -> Tuple[int, int]:
    """(batch_stride, head_stride) in elements; size-1 dims get the dense value."""
    B, H, N, D = t.shape
    sb, sh, sn, sd = t.stride()
    if sd != 1 or sn != D:
        raise ValueError("rows must be contiguous with pitch D (kernels.metal:622: offset = b*bs + h*hs)")
    hs = sh if H > 1 else N * D
    bs = sb if B > 1 else H * hs
    return bs, hs


def _kv_strides(k: torch.Tensor, v: torch.Tensor) -> Tuple[int, int]:
    ks = _strides(k)
    if _strides(v) != ks:
        raise ValueError("k and v must share batch/head strides")
    return ks


def _on_device(entry: str, *tensors: torch.Tensor) -> None:
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{entry} needs device tensors: there is no CPU path "
                           "(the CPU oracle lives in oracle/ and is test infrastructure only)")


def _out_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.bfloat16 if dtype == _FP8 else dtype  # e4m3 inputs: bf16 output


def _out(out: Optional[torch.Tensor], q: torch.Tensor, q_strides: Tuple[int, int]) -> torch.Tensor:
    """O, allocated or checked: the kernels write it with q's shape and strides, anything else lands in the wrong place or out of bounds."""
    if out is None:
        return torch.empty_strided(q.shape, q.stride(), dtype=_out_dtype(q.dtype), device=q.device)
    if (not out.is_cuda or out.device != q.device or out.dtype != _out_dtype(q.dtype) or out.shape != q.shape
            or _strides(out) != q_strides):
        raise ValueError("out must be a device tensor with q's shape/strides (bf16 for fp8 inputs)")
    return out


def _lse(lse: Optional[torch.Tensor], return_lse: bool, q: torch.Tensor) -> Optional[torch.Tensor]:
    B, H, N, _ = q.shape
    if lse is None:
        return torch.empty((B, H, N), dtype=torch.float32, device=q.device) if return_lse else None
    if not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H * N:
        raise ValueError("lse must be contiguous fp32 [B,H,N] on q's device")
    return lse


def _workspace(workspace: Optional[torch.Tensor], need: int, device: torch.device) -> torch.Tensor:
    if workspace is None:
        return torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    if not workspace.is_cuda or workspace.device != device or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 device tensor")
    return workspace


def _scale(scale: Optional[float], D: int) -> float:
    return 1.0 / math.sqrt(D) if scale is None else float(scale)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return t.data_ptr() if t is not None else None


def _call(lib, entry: str, args: tuple, device: torch.device, stream: Optional[int]) -> None:
    """Call the C entry point `entry` with `args` and the stream (default: the current torch stream of `device`); a refusal raises FaError."""
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    fn = getattr(lib, entry)
    if device.index == torch.cuda.current_device():  # the common case: no device switch (it costs microseconds,
        st = fn(*args, stream)                       # as much as a short-sequence kernel runs)
    else:
        with torch.cuda.device(device):
            st = fn(*args, stream)
    if st != 0:
        raise FaError(st, lib.fa_last_error().decode(), entry)


def _prepare_forward(q, k, v, is_causal, scale, variant, return_lse, out, lse):
    """Validate one forward call and return (entry point, its arguments without the stream, out, lse). q [B,Hq,Nq,D], k / v
    [B,Hkv,Nk,D]: equal shapes go to fa_fwd, grouped heads / Nq != Nk to fa_fwd_exv (include/fa_mi355.h; Hq % Hkv == 0, causal
    bottom-right aligned: key j visible to query i iff j <= i + Nk - Nq), whose `variant` is auto, mfma, mfma_exact, mfma16 or
    mfma_splitkv -- the kernels that take that problem; any other raises FaError (unsupported), never a silent substitute."""
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape:
        raise ValueError(f"q [B,Hq,Nq,D] and k, v one [B,Hkv,Nk,D] shape, got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    B, Hq, Nq, D = q.shape
    Bk, Hkv, Nk, Dk = k.shape
    if Bk != B or Dk != D or Hq % Hkv:
        raise ValueError(f"incompatible shapes q {tuple(q.shape)} k/v {tuple(k.shape)}")
    _on_device("flash_attention_forward", q, k, v)
    if q.dtype not in _TORCH2FA or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k.dtype} {v.dtype}")
    qs, ks = _strides(q), _kv_strides(k, v)
    out, lse = _out(out, q, qs), _lse(lse, return_lse, q)
    ptrs = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(lse))
    tail = (int(bool(is_causal)), _TORCH2FA[q.dtype], VARIANTS[variant])
    if q.shape != k.shape:
        return "fa_fwd_exv", ptrs + (B, Hq, Hkv, Nq, Nk, D, _scale(scale, D), *qs, *ks) + tail, out, lse
    if ks != qs:
        raise ValueError("q, k, v must share batch/head strides (one stride pair in the binding table)")
    return "fa_fwd", ptrs + (B, Hq, Nq, D, _scale(scale, D), *qs) + tail, out, lse


def flash_attention_forward(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    is_causal: bool = False,
    scale: Optional[float] = None,
    variant: str = "auto",
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Launch the gfx950 kernel on the current torch stream (asynchronous). k / v may carry fewer heads than q and another
    sequence length (fa_fwd_exv, see _prepare_forward)."""
    lib = load_library()
    entry, args, out, lse = _prepare_forward(q, k, v, is_causal, scale, variant, return_lse, out, lse)
    _call(lib, entry, args, q.device, stream)
    return out, lse


class ForwardPlan:
    """One validated forward call on fixed tensors, launched many times: the argument table is checked and encoded
    once (what the reference host does per dispatch, /root/reference/main.mm:821-852), ``launch()`` only issues
    ``fa_fwd``. For launch-bound shapes -- short sequences, where the Python-side checks of
    ``flash_attention_forward`` cost as much as the kernel runs -- and for replaying a step loop. The plan keeps the
    tensors alive; it does not notice if they are resized or freed behind its back (``Tensor.set_`` / ``resize_``)."""

    def __init__(self, q, k, v, is_causal=False, scale=None, variant="auto", return_lse=True, out=None, lse=None):
        self._lib = load_library()
        if q.shape != k.shape or q.shape != v.shape:
            raise ValueError(f"q, k, v must share one [B,H,N,D] shape, got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
        _, self._args, self.out, self.lse = _prepare_forward(q, k, v, is_causal, scale, variant, return_lse, out, lse)
        self._keep = (q, k, v)
        self._device = q.device

    def launch(self, stream: Optional[int] = None) -> None:
        """Issue the kernel on ``stream`` (default: the current torch stream of the tensors' device); asynchronous."""
        _call(self._lib, "fa_fwd", self._args, self._device, stream)


def decode_workspace_bytes(B: int, Hq: int, Hkv: int, Nq: int, Nk: int, D: int) -> int:
    return int(load_library().fa_fwd_decode_workspace_bytes(B, Hq, Hkv, Nq, Nk, D))


def flash_attention_decode(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    is_causal: bool = False,
    scale: Optional[float] = None,
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    workspace: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Few query rows against a long key sequence (include/fa_mi355.h fa_fwd_decode): q [B,Hq,Nq,D], k/v [B,Hkv,Nk,D] with
    (Hq / Hkv) * Nq <= 32, f16 / bf16 / e4m3 -- or bf16 queries on an e4m3 k / v cache --, D = 64 | 128; the same operator as
    flash_attention_forward on these shapes, laid out for the HBM roofline. `workspace`: a uint8 device tensor of at least decode_workspace_bytes(...) bytes (allocated here if None --
    the C entry point itself allocates nothing)."""
    lib = load_library()
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape:
        raise ValueError("q [B,Hq,Nq,D], k / v [B,Hkv,Nk,D]")
    B, Hq, Nq, D = q.shape
    Bk, Hkv, Nk, Dk = k.shape
    if Bk != B or Dk != D or Hq % Hkv:
        raise ValueError(f"incompatible shapes q {tuple(q.shape)} k/v {tuple(k.shape)}")
    _on_device("flash_attention_decode", q, k, v)
    kv8 = _FP8 is not None and k.dtype == _FP8 and v.dtype == _FP8 and q.dtype == torch.bfloat16  # an e4m3 KV cache under bf16 queries (fa_fwd_decode_kv8)
    if q.dtype not in (torch.float16, torch.bfloat16, _FP8) or v.dtype != k.dtype or (k.dtype != q.dtype and not kv8):
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k.dtype} {v.dtype} (one of f16 / bf16 / e4m3, or bf16 queries on an e4m3 cache)")
    qs, ks = _strides(q), _kv_strides(k, v)
    out, lse = _out(out, q, qs), _lse(lse, return_lse, q)
    ws = _workspace(workspace, decode_workspace_bytes(B, Hq, Hkv, Nq, Nk, D), q.device)
    _call(lib, "fa_fwd_decode_kv8" if kv8 else "fa_fwd_decode",
          (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(lse), B, Hq, Hkv, Nq, Nk, D, _scale(scale, D), *qs, *ks,
           int(bool(is_causal)), _TORCH2FA[q.dtype], ws.data_ptr(), ws.numel()), q.device, stream)
    return out, lse


def _window(window, is_causal: bool) -> Tuple[int, int]:
    """(window_left, window_right) of a *_window entry point (include/fa_mi355.h, "Sliding window"): negative = unbounded on that side.
    is_causal=True turns an unbounded right side into 0 and refuses any other right side that is not 0."""
    try:
        left, right = (int(x) for x in window)
    except (TypeError, ValueError):
        raise ValueError(f"window must be a (left, right) pair of ints, got {window!r}") from None
    if max(left, right) > 2 ** 31 - 1:
        raise ValueError(f"window sides are ints up to 2**31 - 1, got {window!r}")
    left, right = max(left, -1), max(right, -1)
    if is_causal:
        if right > 0:
            raise ValueError(f"is_causal=True needs window right side 0 (or negative: then it is 0), got {right}")
        right = 0
    return left, right


def _sinks(sinks: torch.Tensor, Hq: int, device: torch.device) -> torch.Tensor:
    """The sinks of a *_sink entry point (include/fa_mi355.h, "Attention sinks"): one logit per query head, as contiguous fp32 on `device`."""
    if not isinstance(sinks, torch.Tensor) or sinks.dim() != 1 or sinks.shape[0] != Hq:
        raise ValueError(f"sinks must be a [Hq] = [{Hq}] tensor, one logit per query head")
    if not sinks.is_cuda or sinks.device != device:
        raise ValueError("sinks must be on q's device: the kernels read them, the host never does")
    return sinks.detach().to(torch.float32).contiguous()


def _sink_window(window, is_causal: bool) -> Tuple[int, int]:
    """The window of a call with sinks: None is (-1, 0) under is_causal and (-1, -1) without."""
    return ((-1, 0) if is_causal else (-1, -1)) if window is None else _window(window, is_causal)


def _softcap(softcap, sinks) -> Optional[float]:
    """The cap of a *_softcap entry point (include/fa_mi355.h, "Logit soft-capping"): None or 0.0 is the call without a cap; otherwise a
    finite positive host scalar (the library refuses anything else), which does not combine with sinks."""
    if softcap is None or float(softcap) == 0.0:
        return None
    if sinks is not None:
        raise ValueError("softcap together with sinks is not supported")
    return float(softcap)


def decode_paged_workspace_bytes(B: int, Hq: int, Hkv: int, Nq: int, D: int, page_size: int, max_pages_per_seq: int) -> int:
    return int(load_library().fa_fwd_decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, page_size, max_pages_per_seq))


def flash_attention_decode_paged(
    q: torch.Tensor,
    k_pages: torch.Tensor,
    v_pages: torch.Tensor,
    block_table: torch.Tensor,
    seqlens_k: torch.Tensor,
    is_causal: bool = False,
    scale: Optional[float] = None,
    layout: str = "HND",
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    workspace: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
    window: Optional[Tuple[int, int]] = None,
    sinks: Optional[torch.Tensor] = None,
    softcap: Optional[float] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """A decode step against a paged KV cache (include/fa_mi355.h fa_fwd_decode_paged): q [B,Hq,Nq,D]; k_pages / v_pages one pool
    each, [num_pages, Hkv, P, D] (layout "HND") or [num_pages, P, Hkv, D] ("NHD"), P in {16, 32, 64, 128, 256}; block_table int32
    [B, max_pages_per_seq] and seqlens_k int32 [B], both contiguous on q's device and read by the kernels only -- nothing here
    synchronises or reads device values, so the call can be captured in a graph and replayed after the tables change in place.
    dtypes as flash_attention_decode (f16, bf16, e4m3, or bf16 queries on an e4m3 pool). A row with no visible key gets O = 0 and
    LSE = -inf. `workspace`: a uint8 device tensor of at least decode_paged_workspace_bytes(...) bytes (allocated here if None).
    window=(left, right): a sliding window (fa_fwd_decode_paged_window: key j visible to query i iff i + L_b - Nq - left <= j <=
    i + L_b - Nq + right; negative = unbounded; with is_causal=True right must be 0 or negative). None: the call above, untouched.
    sinks: a [Hq] tensor of per-head sink logits (fa_fwd_decode_paged_sink: exp(sinks[h]) joins every softmax denominator of head h and
    carries no value; a row with no visible key then gets O = 0 and LSE = sinks[h]). None: the calls above, untouched.
    softcap: a finite positive float (fa_fwd_decode_paged_softcap: every score becomes softcap * tanh(scale * s / softcap) before the mask
    and the softmax; window=None is then (-1, 0) under is_causal, else (-1, -1); not together with sinks). None or 0.0: the calls above."""
    lib = load_library()
    cap = _softcap(softcap, sinks)  # (first: a cap that cannot be served is refused whatever else is wrong)
    if q.dim() != 4 or k_pages.dim() != 4 or k_pages.shape != v_pages.shape:
        raise ValueError("q [B,Hq,Nq,D], k_pages / v_pages one [num_pages,Hkv,P,D] (HND) or [num_pages,P,Hkv,D] (NHD) shape")
    if layout not in ("HND", "NHD"):
        raise ValueError(f"layout must be 'HND' or 'NHD', got {layout!r}")
    if not all(t.is_cuda and t.device == q.device for t in (q, k_pages, v_pages, block_table, seqlens_k)):
        raise ValueError("flash_attention_decode_paged needs q, the pools and both tables on one device: there is no CPU path")
    B, Hq, Nq, D = q.shape
    if layout == "HND":
        num_pages, Hkv, P, Dk = k_pages.shape
        ps, hs, rs, es = k_pages.stride()
    else:
        num_pages, P, Hkv, Dk = k_pages.shape
        ps, rs, hs, es = k_pages.stride()
    if Dk != D or Hq % Hkv or es != 1 or v_pages.stride() != k_pages.stride():
        raise ValueError(f"incompatible q {tuple(q.shape)} and pools {tuple(k_pages.shape)} (same D, Hq % Hkv == 0, unit element stride, "
                         "k_pages and v_pages with one set of strides)")
    if (block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B or not block_table.is_contiguous()
            or seqlens_k.dtype != torch.int32 or seqlens_k.shape != (B,) or not seqlens_k.is_contiguous()):
        raise ValueError("block_table must be a contiguous int32 [B, max_pages_per_seq] tensor and seqlens_k a contiguous int32 [B] one")
    pairs = {(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (_FP8, _FP8), (torch.bfloat16, _FP8)}
    if v_pages.dtype != k_pages.dtype or (q.dtype, k_pages.dtype) not in pairs:
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k_pages.dtype} {v_pages.dtype} (one of f16 / bf16 / e4m3, or bf16 queries on "
                         "an e4m3 pool)")
    qs = _strides(q)
    max_pages = block_table.shape[1]
    out, lse = _out(out, q, qs), _lse(lse, return_lse, q)
    ws = _workspace(workspace, decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, max(max_pages, 1)), q.device)
    mask = (int(bool(is_causal)),) if window is None else _window(window, is_causal)
    entry = "fa_fwd_decode_paged" if window is None else "fa_fwd_decode_paged_window"
    if sinks is not None:
        sinks = _sinks(sinks, Hq, q.device)
        entry, mask = "fa_fwd_decode_paged_sink", _sink_window(window, is_causal) + (sinks.data_ptr(),)
    if cap is not None:
        entry, mask = "fa_fwd_decode_paged_softcap", _sink_window(window, is_causal) + (cap,)
    _call(lib, entry,
          (q.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(), out.data_ptr(), _ptr(lse), block_table.data_ptr(), seqlens_k.data_ptr(),
           B, Hq, Hkv, Nq, D, P, num_pages, max_pages, _scale(scale, D), *qs, ps, hs, rs, block_table.stride(0), *mask,
           _TORCH2FA[q.dtype], _TORCH2FA[k_pages.dtype], ws.data_ptr(), ws.numel()), q.device, stream)
    return out, lse


def mla_decode_paged_supported(dtype: str, d_qk: int, d_v: int, Hq: int, Nq: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_mla_decode_paged_supported(DTYPES[dtype], d_qk, d_v, Hq, Nq, page_size))


def mla_decode_paged_workspace_bytes(B: int, Hq: int, Nq: int, d_v: int, page_size: int, max_pages_per_seq: int) -> int:
    return int(load_library().fa_fwd_mla_decode_paged_workspace_bytes(B, Hq, Nq, d_v, page_size, max_pages_per_seq))


def mla_decode_paged_wide_supported(dtype: str, d_qk: int, d_v: int, Hq: int, Nq: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_mla_decode_paged_wide_supported(DTYPES[dtype], d_qk, d_v, Hq, Nq, page_size))


def mla_decode_paged_wide_workspace_bytes(B: int, Hq: int, Nq: int, d_v: int, page_size: int, max_pages_per_seq: int) -> int:
    return int(load_library().fa_fwd_mla_decode_paged_wide_workspace_bytes(B, Hq, Nq, d_v, page_size, max_pages_per_seq))


def mla_decode_paged_kv8_supported(q_dtype: str, kv_dtype: str, d_qk: int, d_v: int, Hq: int, Nq: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_mla_decode_paged_kv8_supported(DTYPES[q_dtype], DTYPES[kv_dtype], d_qk, d_v, Hq, Nq, page_size))


def mla_decode_paged_kv8_workspace_bytes(B: int, Hq: int, Nq: int, d_v: int, page_size: int, max_pages_per_seq: int) -> int:
    return int(load_library().fa_fwd_mla_decode_paged_kv8_workspace_bytes(B, Hq, Nq, d_v, page_size, max_pages_per_seq))


def flash_attention_mla_decode_paged(
    q: torch.Tensor,
    kv_pages: torch.Tensor,
    block_table: torch.Tensor,
    seqlens_k: torch.Tensor,
    scale: float,
    d_v: int = 512,
    is_causal: bool = False,
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    workspace: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
    wide: Optional[bool] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The absorbed MLA decode step over a paged latent cache (include/fa_mi355.h fa_fwd_mla_decode_paged and
    fa_fwd_mla_decode_paged_wide): q [B,Hq,Nq,576] under any strides with a unit last stride (head-major or a token-major view), up to 128
    rows Hq * Nq; kv_pages ONE pool [num_pages, P, 576] or
    [num_pages, P, 1, 576], f16 / bf16 like q, P in {16, 32, 64, 128, 256}: all 576 columns of a row enter the score, the first d_v = 512
    are the value. block_table int32 [B, max_pages_per_seq] and seqlens_k int32 [B] are contiguous device tensors read by the kernels only:
    nothing here synchronises, the call can be captured in a graph. `scale` is required (the model's, e.g. (128 + 64) ** -0.5 * mscale ** 2:
    the head dim of the model is not 576). Returns O [B,Hq,Nq,d_v] (allocated head-major if `out` is None; any strides with a unit last
    stride otherwise) and LSE [B,Hq,Nq] fp32 or None. A row with no visible key gets O = 0 and LSE = -inf. `workspace`: a uint8 device
    tensor of at least mla_decode_paged_workspace_bytes(...) bytes (allocated here if None). `wide` chooses the entry point: None sends
    Hq * Nq <= 32 to fa_fwd_mla_decode_paged (one-wave items) and more rows to fa_fwd_mla_decode_paged_wide (workgroups of two or four waves
    over a shared tile); True forces the wide call for any row count it supports, False the other. The wide call's workspace is sized by
    mla_decode_paged_wide_workspace_bytes(...).
    A torch.float8_e4m3fn pool under bf16 q goes to fa_fwd_mla_decode_paged_kv8 for every row count up to 128 (no scales: the bytes are
    read as plain e4m3 values; a caller that appended with k_mul = v_mul = 1 / s passes scale * s and multiplies O by s). O is bf16, the
    workspace is sized by mla_decode_paged_kv8_workspace_bytes(...); `wide` is ignored there, except that wide=False raises ValueError
    (that pool has no one-wave form), and f16 q on such a pool raises ValueError."""
    lib = load_library()
    if scale is None:
        raise ValueError("flash_attention_mla_decode_paged needs the model's scale: there is no default (the head dim of the model is not 576)")
    if q.dim() != 4 or kv_pages.dim() not in (3, 4) or (kv_pages.dim() == 4 and kv_pages.shape[2] != 1):
        raise ValueError("q [B,Hq,Nq,576], kv_pages one [num_pages,P,576] or [num_pages,P,1,576] latent pool")
    kv8 = _FP8 is not None and kv_pages.dtype == _FP8
    if kv8 and q.dtype != torch.bfloat16:
        raise ValueError(f"unsupported dtypes {q.dtype} {kv_pages.dtype}: a float8_e4m3fn latent pool takes bf16 queries only")
    if kv8 and wide is not None and not wide:
        raise ValueError("wide=False on a float8_e4m3fn latent pool: fa_fwd_mla_decode_paged_kv8 has no one-wave form")
    if not all(t.is_cuda and t.device == q.device for t in (q, kv_pages, block_table, seqlens_k)):
        raise ValueError("flash_attention_mla_decode_paged needs q, the pool and both tables on one device: there is no CPU path")
    B, Hq, Nq, Dqk = q.shape
    num_pages, P, Dk = kv_pages.shape[0], kv_pages.shape[1], kv_pages.shape[-1]
    ps, rs, es = kv_pages.stride(0), kv_pages.stride(1), kv_pages.stride(-1)
    if Dk != Dqk or es != 1 or q.stride(3) != 1:
        raise ValueError(f"incompatible q {tuple(q.shape)} and pool {tuple(kv_pages.shape)} (same last dim, unit element strides)")
    if (block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B or not block_table.is_contiguous()
            or seqlens_k.dtype != torch.int32 or seqlens_k.shape != (B,) or not seqlens_k.is_contiguous()):
        raise ValueError("block_table must be a contiguous int32 [B, max_pages_per_seq] tensor and seqlens_k a contiguous int32 [B] one")
    if not kv8 and (q.dtype not in (torch.float16, torch.bfloat16) or kv_pages.dtype != q.dtype):
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {kv_pages.dtype} (f16 or bf16, q and the pool alike)")
    d_v = int(d_v)
    if out is None:
        out = torch.empty((B, Hq, Nq, d_v), dtype=q.dtype, device=q.device)
    elif not out.is_cuda or out.device != q.device or out.dtype != q.dtype or out.shape != (B, Hq, Nq, d_v) or out.stride(3) != 1:
        raise ValueError("out must be a [B,Hq,Nq,d_v] device tensor of q's dtype with a unit last stride")
    lse = _lse(lse, return_lse, q)
    max_pages = block_table.shape[1]
    if kv8:
        ws = _workspace(workspace, mla_decode_paged_kv8_workspace_bytes(B, Hq, Nq, d_v, P, max(max_pages, 1)), q.device)
        _call(lib, "fa_fwd_mla_decode_paged_kv8",
              (q.data_ptr(), kv_pages.data_ptr(), out.data_ptr(), _ptr(lse), block_table.data_ptr(), seqlens_k.data_ptr(), B, Hq, Nq, Dqk, d_v,
               P, num_pages, max_pages, float(scale), q.stride(0), q.stride(1), q.stride(2), out.stride(0), out.stride(1), out.stride(2), ps,
               rs, block_table.stride(0), int(bool(is_causal)), _TORCH2FA[q.dtype], _TORCH2FA[kv_pages.dtype], ws.data_ptr(), ws.numel()),
              q.device, stream)
        return out, lse
    wide = Hq * Nq > 32 if wide is None else bool(wide)
    need = (mla_decode_paged_wide_workspace_bytes if wide else mla_decode_paged_workspace_bytes)(B, Hq, Nq, d_v, P, max(max_pages, 1))
    ws = _workspace(workspace, need, q.device)
    _call(lib, "fa_fwd_mla_decode_paged_wide" if wide else "fa_fwd_mla_decode_paged",
          (q.data_ptr(), kv_pages.data_ptr(), out.data_ptr(), _ptr(lse), block_table.data_ptr(), seqlens_k.data_ptr(), B, Hq, Nq, Dqk, d_v, P,
           num_pages, max_pages, float(scale), q.stride(0), q.stride(1), q.stride(2), out.stride(0), out.stride(1), out.stride(2), ps, rs,
           block_table.stride(0), int(bool(is_causal)), _TORCH2FA[q.dtype], ws.data_ptr(), ws.numel()), q.device, stream)
    return out, lse


def mla_decode_sparse_supported(dtype: str, d_qk: int, d_v: int, Hq: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_mla_decode_sparse_supported(DTYPES[dtype], d_qk, d_v, Hq, page_size))


def mla_decode_sparse_workspace_bytes(T: int, Hq: int, d_v: int, topk: int) -> int:
    return int(load_library().fa_fwd_mla_decode_sparse_workspace_bytes(T, Hq, d_v, topk))


def mla_decode_sparse_kv8_supported(q_dtype: str, kv_dtype: str, d_qk: int, d_v: int, Hq: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_mla_decode_sparse_kv8_supported(DTYPES[q_dtype], DTYPES[kv_dtype], d_qk, d_v, Hq, page_size))


def mla_decode_sparse_kv8_workspace_bytes(T: int, Hq: int, d_v: int, topk: int) -> int:
    return int(load_library().fa_fwd_mla_decode_sparse_kv8_workspace_bytes(T, Hq, d_v, topk))


def flash_attention_mla_decode_sparse(
    q: torch.Tensor,
    kv_pages: torch.Tensor,
    indices: torch.Tensor,
    scale: float,
    index_counts: Optional[torch.Tensor] = None,
    d_v: int = 512,
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    workspace: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The absorbed MLA step over a list of keys per query token (include/fa_mi355.h fa_fwd_mla_decode_sparse): q [T,Hq,576] under any
    strides with a unit last stride, up to 128 heads; kv_pages ONE pool [num_pages, P, 576] or [num_pages, P, 1, 576], f16 / bf16 like q,
    P in {16, 32, 64, 128, 256}. indices int32 [T, topk] with a unit last stride (the row stride a multiple of 4, the base 16-byte
    aligned) names token t's keys by SLOT, page * P + row; index_counts int32 [T] contiguous says how many entries of each row count
    (None: all topk). Both are device tensors read by the kernels only: nothing here synchronises, the call can be captured in a graph.
    A slot named twice enters twice; an entry among the counted ones outside the pool is a key of zeros; entries behind the count are
    never read. `scale` is required (the model's: the head dim of the model is not 576). Returns O [T,Hq,d_v] (allocated contiguous if
    `out` is None; any strides with a unit last stride otherwise) and LSE [T,Hq] fp32 or None. A token with no key gets O = 0 and
    LSE = -inf. `workspace`: a uint8 device tensor of at least mla_decode_sparse_workspace_bytes(T, Hq, d_v, topk) bytes (allocated here
    if None).
    A torch.float8_e4m3fn pool under bf16 q goes to fa_fwd_mla_decode_sparse_kv8 (no scales: the bytes are read as plain e4m3 values; a
    caller that appended with k_mul = v_mul = 1 / s passes scale * s and multiplies O by s). The pool's strides are then bytes, a SLOT
    is still page * P + row, O is bf16 and the workspace is sized by mla_decode_sparse_kv8_workspace_bytes(...), the same number; f16 q
    on such a pool raises ValueError."""
    lib = load_library()
    if scale is None:
        raise ValueError("flash_attention_mla_decode_sparse needs the model's scale: there is no default (the head dim of the model is not 576)")
    if q.dim() != 3 or kv_pages.dim() not in (3, 4) or (kv_pages.dim() == 4 and kv_pages.shape[2] != 1):
        raise ValueError("q [T,Hq,576], kv_pages one [num_pages,P,576] or [num_pages,P,1,576] latent pool")
    kv8 = _FP8 is not None and kv_pages.dtype == _FP8
    if kv8 and q.dtype != torch.bfloat16:
        raise ValueError(f"unsupported dtypes {q.dtype} {kv_pages.dtype}: a float8_e4m3fn latent pool takes bf16 queries only")
    tensors = (q, kv_pages, indices) + (() if index_counts is None else (index_counts,))
    if not all(t.is_cuda and t.device == q.device for t in tensors):
        raise ValueError("flash_attention_mla_decode_sparse needs q, the pool, the index lists and their counts on one device: there is no CPU path")
    T, Hq, Dqk = q.shape
    num_pages, P, Dk = kv_pages.shape[0], kv_pages.shape[1], kv_pages.shape[-1]
    ps, rs, es = kv_pages.stride(0), kv_pages.stride(1), kv_pages.stride(-1)
    if Dk != Dqk or es != 1 or q.stride(2) != 1:
        raise ValueError(f"incompatible q {tuple(q.shape)} and pool {tuple(kv_pages.shape)} (same last dim, unit element strides)")
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[0] != T or indices.shape[1] < 1 or indices.stride(1) != 1:
        raise ValueError("indices must be an int32 [T, topk] tensor with a unit last stride")
    if index_counts is not None and (index_counts.dtype != torch.int32 or index_counts.shape != (T,) or not index_counts.is_contiguous()):
        raise ValueError("index_counts must be a contiguous int32 [T] tensor, or None")
    if not kv8 and (q.dtype not in (torch.float16, torch.bfloat16) or kv_pages.dtype != q.dtype):
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {kv_pages.dtype} (f16 or bf16, q and the pool alike)")
    d_v = int(d_v)
    topk = indices.shape[1]
    if out is None:
        out = torch.empty((T, Hq, d_v), dtype=q.dtype, device=q.device)
    elif not out.is_cuda or out.device != q.device or out.dtype != q.dtype or out.shape != (T, Hq, d_v) or out.stride(2) != 1:
        raise ValueError("out must be a [T,Hq,d_v] device tensor of q's dtype with a unit last stride")
    if lse is None:
        lse = torch.empty((T, Hq), dtype=torch.float32, device=q.device) if return_lse else None
    elif not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.shape != (T, Hq):
        raise ValueError("lse must be contiguous fp32 [T,Hq] on q's device")
    # (one row: its stride addresses nothing, and torch reports any value for a dimension of size 1)
    istride = indices.stride(0) if T > 1 else (topk + 3) // 4 * 4
    if kv8:  # (the pool's strides come from the tensor: bytes)
        ws = _workspace(workspace, mla_decode_sparse_kv8_workspace_bytes(T, Hq, d_v, topk), q.device)
        _call(lib, "fa_fwd_mla_decode_sparse_kv8",
              (q.data_ptr(), kv_pages.data_ptr(), out.data_ptr(), _ptr(lse), indices.data_ptr(), _ptr(index_counts), T, Hq, Dqk, d_v, topk, P,
               num_pages, float(scale), q.stride(0), q.stride(1), out.stride(0), out.stride(1), ps, rs, istride,
               _TORCH2FA[q.dtype], _TORCH2FA[kv_pages.dtype], ws.data_ptr(), ws.numel()), q.device, stream)
        return out, lse
    ws = _workspace(workspace, mla_decode_sparse_workspace_bytes(T, Hq, d_v, topk), q.device)
    _call(lib, "fa_fwd_mla_decode_sparse",
          (q.data_ptr(), kv_pages.data_ptr(), out.data_ptr(), _ptr(lse), indices.data_ptr(), _ptr(index_counts), T, Hq, Dqk, d_v, topk, P,
           num_pages, float(scale), q.stride(0), q.stride(1), out.stride(0), out.stride(1), ps, rs, istride,
           _TORCH2FA[q.dtype], ws.data_ptr(), ws.numel()), q.device, stream)
    return out, lse


def varlen_supported(dtype: str, D: int) -> bool:
    return bool(load_library().fa_fwd_varlen_supported(DTYPES[dtype], D))


def flash_attention_varlen(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    is_causal: bool = False,
    scale: Optional[float] = None,
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
    window: Optional[Tuple[int, int]] = None,
    sinks: Optional[torch.Tensor] = None,
    softcap: Optional[float] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The forward over packed variable-length sequences (include/fa_mi355.h fa_fwd_varlen): q [total_q, Hq, D], k / v
    [total_k, Hkv, D], f16 / bf16, D = 64 | 128. Strides are taken from the tensors: any view with unit element stride works ([H, total, D]
    storage transposed, slices of one packed QKV projection), k and v must share theirs. cu_seqlens_q / cu_seqlens_k: contiguous int32
    [B + 1] on q's device, read by the kernel only -- nothing here synchronises or reads device values, so the call can be captured in a
    graph and replayed after the tables change in place (same B, totals and max_seqlen_*). Sequence b owns query tokens
    cu_seqlens_q[b] .. cu_seqlens_q[b+1) and attends to keys cu_seqlens_k[b] .. cu_seqlens_k[b+1); causal is bottom-right aligned per
    sequence; a row with no visible key gets O = 0 and LSE = -inf; tokens at or past cu_seqlens_q[B] and rows beyond max_seqlen_q of a
    sequence are not written. window=(left, right): a sliding window (fa_fwd_varlen_window: key j visible to query i iff
    i + Lk_b - Lq_b - left <= j <= i + Lk_b - Lq_b + right; negative = unbounded; with is_causal=True right must be 0 or negative);
    None: the call above, untouched. sinks: a [Hq] tensor of per-head sink logits (fa_fwd_varlen_sink: exp(sinks[h]) joins every softmax
    denominator of head h and carries no value -- natural-log units, the scale is not applied to it; a row with no visible key then gets
    O = 0 and LSE = sinks[h]; window=None with sinks is (-1, 0) under is_causal, else (-1, -1)); None: the calls above, untouched.
    softcap: a finite positive float (fa_fwd_varlen_softcap, "Logit soft-capping": every score becomes softcap * tanh(scale * s / softcap)
    before the mask and the softmax, LSE is that of the capped scores; window=None is then (-1, 0) under is_causal, else (-1, -1); not
    together with sinks); None or 0.0: the calls above, untouched.
    Returns (out, lse): out like q ([total_q, Hq, D], q's strides unless `out` is given), lse [Hq, total_q]."""
    lib = load_library()
    cap = _softcap(softcap, sinks)  # (first: a cap that cannot be served is refused whatever else is wrong)
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape:
        raise ValueError(f"q [total_q,Hq,D] and k, v one [total_k,Hkv,D] shape, got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    total_q, Hq, D = q.shape
    total_k, Hkv, Dk = k.shape
    if Dk != D or Hkv < 1 or Hq % Hkv:
        raise ValueError(f"incompatible shapes q {tuple(q.shape)} k/v {tuple(k.shape)}")
    if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k.dtype} {v.dtype} (f16 or bf16)")
    if q.stride(2) != 1 or k.stride(2) != 1 or v.stride(2) != 1:
        raise ValueError("q, k, v need a unit element stride (a head of a token is D contiguous elements)")
    if v.stride() != k.stride():
        raise ValueError("k and v must share row/head strides")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if cu.dtype != torch.int32 or cu.dim() != 1 or cu.shape[0] < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 [B + 1] tensor")
    if cu_seqlens_k.shape != cu_seqlens_q.shape:
        raise ValueError("cu_seqlens_q and cu_seqlens_k must both be [B + 1]")
    B = cu_seqlens_q.shape[0] - 1
    if not all(t.is_cuda and t.device == q.device for t in (q, k, v, cu_seqlens_q, cu_seqlens_k)):
        raise RuntimeError("flash_attention_varlen needs q, k, v and both cu_seqlens on one device: there is no CPU path")
    if out is None:
        out = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device)
    elif (not out.is_cuda or out.device != q.device or out.dtype != q.dtype or out.shape != q.shape or out.stride() != q.stride()):
        raise ValueError("out must be a device tensor with q's dtype, shape and strides (the kernel writes it under q's strides)")
    if lse is None:
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=q.device) if return_lse else None
    elif not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.shape != (Hq, total_q):
        raise ValueError("lse must be contiguous fp32 [Hq, total_q] on q's device")
    mask = (int(bool(is_causal)),) if window is None else _window(window, is_causal)
    entry = "fa_fwd_varlen" if window is None else "fa_fwd_varlen_window"
    if sinks is not None:
        sinks = _sinks(sinks, Hq, q.device)
        entry, mask = "fa_fwd_varlen_sink", _sink_window(window, is_causal) + (sinks.data_ptr(),)
    if cap is not None:
        entry, mask = "fa_fwd_varlen_softcap", _sink_window(window, is_causal) + (cap,)
    _call(lib, entry,
          (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(),
           B, Hq, Hkv, total_q, total_k, int(max_seqlen_q), int(max_seqlen_k), D, _scale(scale, D), q.stride(0), q.stride(1),
           k.stride(0), k.stride(1), *mask, _TORCH2FA[q.dtype]), q.device, stream)
    return out, lse


def varlen_mla_supported(dtype: str, d_qk: int, d_v: int) -> bool:
    return bool(load_library().fa_fwd_varlen_mla_supported(DTYPES[dtype], int(d_qk), int(d_v)))


def flash_attention_varlen_mla(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    is_causal: bool = False,
    scale: Optional[float] = None,
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The MLA prefill forward over packed variable-length sequences (include/fa_mi355.h fa_fwd_varlen_mla): the non-absorbed form of
    a latent-attention layer, q [total_q, Hq, 192], k [total_k, Hkv, 192] (128 "nope" + 64 rotary columns), v [total_k, Hkv, 128],
    f16 / bf16. Strides are taken from EACH tensor, the element stride must be 1: q may be a slice of a wider projection, v the upper
    half of the [total_k, Hkv, 256] output of the kv up-projection. cu_seqlens_* and everything they imply are flash_attention_varlen's:
    int32 [B + 1] on q's device, read by the kernel only, so the call can be captured and replayed after the tables change in place;
    causal is bottom-right aligned per sequence; a row with no visible key gets O = 0 and LSE = -inf; unowned tokens are not written.
    scale=None means 192 ** -0.5 (nothing is derived from the value head dim). out: [total_q, Hq, 128], contiguous by default; any
    strided tensor of that shape with unit element stride is written in place (a slice of a wider buffer). The backward is
    flash_attention_varlen_mla_backward; torch.ops.fa_mi355.attention_varlen_mla is the differentiable op. The chunked-context recipe (an un-masked call per cached chunk, a causal call on the new tokens, the LSE merge) is in
    INTEGRATION.md, "Latent-attention layers: prefill".
    Returns (out, lse): out [total_q, Hq, 128], lse [Hq, total_q]."""
    lib = load_library()
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError(f"q [total_q,Hq,192], k [total_k,Hkv,192] and v [total_k,Hkv,128], got {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    total_q, Hq, Dqk = q.shape
    total_k, Hkv, Dk = k.shape
    Dv = v.shape[2]
    if Dk != Dqk or tuple(v.shape[:2]) != (total_k, Hkv) or Hkv < 1 or Hq % Hkv:
        raise ValueError(f"incompatible shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k.dtype} {v.dtype} (f16 or bf16)")
    if q.stride(2) != 1 or k.stride(2) != 1 or v.stride(2) != 1:
        raise ValueError("q, k, v need a unit element stride (a head of a token is contiguous elements)")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if cu.dtype != torch.int32 or cu.dim() != 1 or cu.shape[0] < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 [B + 1] tensor")
    if cu_seqlens_k.shape != cu_seqlens_q.shape:
        raise ValueError("cu_seqlens_q and cu_seqlens_k must both be [B + 1]")
    B = cu_seqlens_q.shape[0] - 1
    if not all(t.is_cuda and t.device == q.device for t in (q, k, v, cu_seqlens_q, cu_seqlens_k)):
        raise RuntimeError("flash_attention_varlen_mla needs q, k, v and both cu_seqlens on one device: there is no CPU path")
    if out is None:
        out = torch.empty((total_q, Hq, Dv), dtype=q.dtype, device=q.device)
    elif (not out.is_cuda or out.device != q.device or out.dtype != q.dtype or tuple(out.shape) != (total_q, Hq, Dv) or out.stride(2) != 1):
        raise ValueError("out must be a device tensor of q's dtype and shape [total_q, Hq, d_v] with a unit element stride")
    if lse is None:
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=q.device) if return_lse else None
    elif not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.shape != (Hq, total_q):
        raise ValueError("lse must be contiguous fp32 [Hq, total_q] on q's device")
    _call(lib, "fa_fwd_varlen_mla",
          (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(),
           B, Hq, Hkv, total_q, total_k, int(max_seqlen_q), int(max_seqlen_k), Dqk, Dv, _scale(scale, Dqk), q.stride(0), q.stride(1),
           k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1), int(bool(is_causal)), _TORCH2FA[q.dtype]),
          q.device, stream)
    return out, lse


def varlen_paged_supported(dtype: str, D: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_varlen_paged_supported(DTYPES[dtype], D, int(page_size)))


def varlen_paged_kv8_supported(q_dtype: str, kv_dtype: str, D: int, page_size: int) -> bool:
    return bool(load_library().fa_fwd_varlen_paged_kv8_supported(DTYPES[q_dtype], DTYPES[kv_dtype], D, int(page_size)))


def varlen_paged_num_splits(B: int, Hq: int, max_seqlen_q: int, D: int, page_size: int, max_pages_per_seq: int) -> int:
    """What num_splits=0 resolves to in flash_attention_varlen_paged (fa_fwd_varlen_paged_num_splits; host scalars only; 0: invalid)."""
    return int(load_library().fa_fwd_varlen_paged_num_splits(B, Hq, int(max_seqlen_q), D, int(page_size), int(max_pages_per_seq)))


def varlen_paged_split_workspace_bytes(B: int, Hq: int, total_q: int, max_seqlen_q: int, D: int, page_size: int, max_pages_per_seq: int,
                                       num_splits: int = 0) -> int:
    """Bytes of workspace flash_attention_varlen_paged(num_splits=...) needs (fa_fwd_varlen_paged_split_workspace_bytes; 0 for one split
    and for invalid sizes)."""
    return int(load_library().fa_fwd_varlen_paged_split_workspace_bytes(B, Hq, total_q, int(max_seqlen_q), D, int(page_size),
                                                                        int(max_pages_per_seq), int(num_splits)))


def _pool(entry: str, k_pages: torch.Tensor, v_pages: torch.Tensor, layout: str):
    """(num_pages, Hkv, P, D, page stride, head stride, row stride) of a pool pair in layout HND / NHD."""
    if k_pages.dim() != 4 or k_pages.shape != v_pages.shape:
        raise ValueError(f"{entry}: k_pages / v_pages one [num_pages,Hkv,P,D] (HND) or [num_pages,P,Hkv,D] (NHD) shape")
    if layout not in ("HND", "NHD"):
        raise ValueError(f"layout must be 'HND' or 'NHD', got {layout!r}")
    if layout == "HND":
        num_pages, Hkv, P, D = k_pages.shape
        ps, hs, rs, es = k_pages.stride()
    else:
        num_pages, P, Hkv, D = k_pages.shape
        ps, rs, hs, es = k_pages.stride()
    if es != 1 or v_pages.stride() != k_pages.stride() or v_pages.dtype != k_pages.dtype:
        raise ValueError(f"{entry}: k_pages and v_pages need one dtype, a unit element stride and one set of strides")
    return num_pages, Hkv, P, D, ps, hs, rs


def _tables(entry: str, cu: torch.Tensor, cu_name: str, block_table: torch.Tensor, seqlens_k: torch.Tensor) -> int:
    if cu.dtype != torch.int32 or cu.dim() != 1 or cu.shape[0] < 2 or not cu.is_contiguous():
        raise ValueError(f"{cu_name} must be a contiguous int32 [B + 1] tensor")
    B = cu.shape[0] - 1
    if (block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] < 1
            or not block_table.is_contiguous() or seqlens_k.dtype != torch.int32 or seqlens_k.shape != (B,) or not seqlens_k.is_contiguous()):
        raise ValueError("block_table must be a contiguous int32 [B, max_pages_per_seq] tensor and seqlens_k a contiguous int32 [B] one")
    return B


def flash_attention_varlen_paged(
    q: torch.Tensor,
    k_pages: torch.Tensor,
    v_pages: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    block_table: torch.Tensor,
    seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    is_causal: bool = False,
    scale: Optional[float] = None,
    layout: str = "HND",
    return_lse: bool = True,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
    window: Optional[Tuple[int, int]] = None,
    sinks: Optional[torch.Tensor] = None,
    softcap: Optional[float] = None,
    num_splits: Optional[int] = None,
    workspace: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Packed queries against a paged KV cache (include/fa_mi355.h fa_fwd_varlen_paged): chunked prefill, prefix caching, verification of
    many speculated tokens. q [total_q, Hq, D] as in flash_attention_varlen (any view with a unit element stride), cu_seqlens_q int32
    [B + 1]; k_pages / v_pages, block_table [B, max_pages_per_seq] and seqlens_k [B] as in flash_attention_decode_paged (layout "HND" or
    "NHD", P in {16, 32, 64, 128, 256}); f16 / bf16 with q and the pools of one type, D = 64 | 128. seqlens_k[b] is the cache length
    with the chunk already appended (kv_append_paged): causal is bottom-right aligned per sequence, which makes a causal call a
    chunked-prefill step. The tables are read by the kernel only -- nothing here synchronises or reads device values, so the call can be
    captured in a graph and replayed after the tables change in place. A row with no visible key gets O = 0 and LSE = -inf; tokens at or
    past cu_seqlens_q[B] and rows beyond max_seqlen_q of a sequence are not written. An inference path: no torch custom op and no
    backward. window=(left, right): a sliding window as in flash_attention_varlen, with seqlens_k[b] in Lk_b's place
    (fa_fwd_varlen_paged_window); None: the call above, untouched. sinks: [Hq] per-head sink logits as in flash_attention_varlen
    (fa_fwd_varlen_paged_sink); None: the calls above, untouched. bf16 q on float8_e4m3fn pools (fa_fwd_varlen_paged_kv8, "e4m3 pools in
    the prefill"): the pool of flash_attention_decode_paged, read as plain e4m3 values -- no scales: fold a K scale into `scale`, a V scale
    into what consumes `out`; window, is_causal and sinks mean what they mean with sinks, and the result is bit for bit the bf16 call on
    the widened pool. softcap: as in flash_attention_varlen (fa_fwd_varlen_paged_softcap; f16 / bf16 pools only: with sinks or with e4m3
    pools it raises ValueError); None or 0.0: the calls above, untouched. num_splits: an int >= 0 takes the key-split call
    (fa_fwd_varlen_paged_split, "Key split in the paged prefill": the keys of every 128-row block are dealt to that many workgroups and
    combined in a second launch -- for a chunk or a few speculated tokens on one or a few long sequences, where the blocks alone cannot fill
    the chip); 0 asks varlen_paged_num_splits; window, is_causal and sinks mean what they mean with sinks; with softcap or with e4m3 pools it
    raises ValueError. `workspace`: a uint8 device tensor of at least varlen_paged_split_workspace_bytes(...) bytes (allocated here if
    None). None: the calls above, untouched. Returns (out, lse): out like q, lse [Hq, total_q]."""
    lib = load_library()
    cap = _softcap(softcap, sinks)  # (first: a cap that cannot be served is refused whatever else is wrong)
    if num_splits is not None:
        if isinstance(num_splits, bool) or not isinstance(num_splits, int) or num_splits < 0:
            raise ValueError(f"num_splits must be None or an int >= 0 (0: the heuristic), got {num_splits!r}")
        if cap is not None:
            raise ValueError("num_splits together with softcap is not supported (fa_fwd_varlen_paged_split has no cap)")
    entry = "flash_attention_varlen_paged"
    if q.dim() != 3:
        raise ValueError(f"q [total_q,Hq,D], got {tuple(q.shape)}")
    num_pages, Hkv, P, Dk, ps, hs, rs = _pool(entry, k_pages, v_pages, layout)
    total_q, Hq, D = q.shape
    if Dk != D or Hkv < 1 or Hq % Hkv:
        raise ValueError(f"incompatible q {tuple(q.shape)} and pools {tuple(k_pages.shape)} (same D, Hq % Hkv == 0)")
    kv8 = _FP8 is not None and q.dtype == torch.bfloat16 and k_pages.dtype == _FP8
    if cap is not None and kv8:
        raise ValueError("softcap on float8_e4m3fn pools is not supported in the prefill (fa_fwd_varlen_paged_kv8 has no cap)")
    if num_splits is not None and kv8:
        raise ValueError("num_splits on float8_e4m3fn pools is not supported (fa_fwd_varlen_paged_split takes f16 / bf16 pools)")
    if not kv8 and (q.dtype not in (torch.float16, torch.bfloat16) or k_pages.dtype != q.dtype):
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k_pages.dtype} {v_pages.dtype} (f16 or bf16, q and the pools alike; or bf16 q "
                         "on float8_e4m3fn pools)")
    if q.stride(2) != 1:
        raise ValueError("q needs a unit element stride (a head of a token is D contiguous elements)")
    B = _tables(entry, cu_seqlens_q, "cu_seqlens_q", block_table, seqlens_k)
    if not all(t.is_cuda and t.device == q.device for t in (q, k_pages, v_pages, cu_seqlens_q, block_table, seqlens_k)):
        raise RuntimeError("flash_attention_varlen_paged needs q, the pools and the tables on one device: there is no CPU path")
    if out is None:
        out = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device)
    elif (not out.is_cuda or out.device != q.device or out.dtype != q.dtype or out.shape != q.shape or out.stride() != q.stride()):
        raise ValueError("out must be a device tensor with q's dtype, shape and strides (the kernel writes it under q's strides)")
    if lse is None:
        lse = torch.empty((Hq, total_q), dtype=torch.float32, device=q.device) if return_lse else None
    elif not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or not lse.is_contiguous() or lse.shape != (Hq, total_q):
        raise ValueError("lse must be contiguous fp32 [Hq, total_q] on q's device")
    mask = (int(bool(is_causal)),) if window is None else _window(window, is_causal)
    entry = "fa_fwd_varlen_paged" if window is None else "fa_fwd_varlen_paged_window"
    if sinks is not None:
        sinks = _sinks(sinks, Hq, q.device)
        entry, mask = "fa_fwd_varlen_paged_sink", _sink_window(window, is_causal) + (sinks.data_ptr(),)
    if cap is not None:
        entry, mask = "fa_fwd_varlen_paged_softcap", _sink_window(window, is_causal) + (cap,)
    dtypes = (_TORCH2FA[q.dtype],)
    if kv8:  # one entry point with or without sinks; the mask as the sink path maps it
        entry, mask = "fa_fwd_varlen_paged_kv8", _sink_window(window, is_causal) + (_ptr(sinks),)
        dtypes = (_TORCH2FA[q.dtype], _TORCH2FA[k_pages.dtype])
    if num_splits is not None:  # the mask as the sink path maps it; sinks may be absent
        need = varlen_paged_split_workspace_bytes(B, Hq, total_q, int(max_seqlen_q), D, P, block_table.shape[1], num_splits)
        ws = _workspace(workspace, need, q.device)
        entry, mask = "fa_fwd_varlen_paged_split", _sink_window(window, is_causal) + (_ptr(sinks),)
        dtypes = (_TORCH2FA[q.dtype], num_splits, ws.data_ptr(), ws.numel())
    _call(lib, entry,
          (q.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(), block_table.data_ptr(),
           seqlens_k.data_ptr(), B, Hq, Hkv, total_q, int(max_seqlen_q), D, P, num_pages, block_table.shape[1], _scale(scale, D),
           q.stride(0), q.stride(1), ps, hs, rs, block_table.stride(0), *mask, *dtypes), q.device, stream)
    return out, lse


def kv_append_paged(
    k_new: torch.Tensor,
    v_new: torch.Tensor,
    k_pages: torch.Tensor,
    v_pages: torch.Tensor,
    cu_seqlens_new: torch.Tensor,
    block_table: torch.Tensor,
    seqlens_k: torch.Tensor,
    max_seqlen_new: int,
    layout: str = "HND",
    stream: Optional[int] = None,
    k_mul: float = 1.0,
    v_mul: float = 1.0,
) -> None:
    """Write new K / V rows into the page pools, in place (include/fa_mi355.h fa_kv_append_paged): k_new / v_new [total_new, Hkv, D] views
    with one set of strides, f16 / bf16 / e4m3 like the pools; token i of sequence b (tokens cu_seqlens_new[b] .. cu_seqlens_new[b+1)) goes to
    key position seqlens_k[b] - n_b + i, i.e. seqlens_k holds the lengths AFTER the append -- the table flash_attention_varlen_paged and
    flash_attention_decode_paged then read. Positions outside the capacity or on table entries outside the pool are skipped; nothing else
    is written. Nothing here synchronises or reads device values: graph-capturable. An inference path: no torch custom op, no backward.
    f16 / bf16 new rows with float8_e4m3fn pools: the quantising append (fa_kv_append_paged_quant), every element stored as
    e4m3_rne(clamp(fp32(x) * mul, -448, 448)) with mul = k_mul / v_mul (> 0, finite; host scalars), placed by the same rules. Equal dtypes
    stay the byte copy, which takes no multipliers (anything but 1.0 is refused there)."""
    lib = load_library()
    entry = "kv_append_paged"
    num_pages, Hkv, P, D, ps, hs, rs = _pool(entry, k_pages, v_pages, layout)
    if k_new.dim() != 3 or k_new.shape != v_new.shape or k_new.shape[1:] != (Hkv, D):
        raise ValueError(f"k_new / v_new one [total_new,Hkv,D] shape matching the pools, got {tuple(k_new.shape)} {tuple(v_new.shape)} "
                         f"for pools {tuple(k_pages.shape)}")
    quant = _FP8 is not None and k_pages.dtype == _FP8 and k_new.dtype in (torch.float16, torch.bfloat16) and v_new.dtype == k_new.dtype
    if not quant and (float(k_mul) != 1.0 or float(v_mul) != 1.0):
        raise ValueError("k_mul / v_mul belong to the quantising append (16-bit new rows, float8_e4m3fn pools): the byte copy has none")
    if not quant and (k_pages.dtype not in (torch.float16, torch.bfloat16, _FP8) or k_new.dtype != k_pages.dtype or v_new.dtype != k_pages.dtype):
        raise ValueError(f"unsupported / mixed dtypes {k_new.dtype} {v_new.dtype} {k_pages.dtype} (f16 / bf16 / e4m3, new rows and pools alike; "
                         "or f16 / bf16 new rows into e4m3 pools)")
    if k_new.stride(2) != 1 or v_new.stride() != k_new.stride():
        raise ValueError("k_new and v_new need a unit element stride and one set of row/head strides")
    B = _tables(entry, cu_seqlens_new, "cu_seqlens_new", block_table, seqlens_k)
    if not all(t.is_cuda and t.device == k_pages.device for t in (k_new, v_new, k_pages, v_pages, cu_seqlens_new, block_table, seqlens_k)):
        raise RuntimeError("kv_append_paged needs the new rows, the pools and the tables on one device: there is no CPU path")
    tail = (_TORCH2FA[k_new.dtype], float(k_mul), float(v_mul)) if quant else (_TORCH2FA[k_pages.dtype],)
    _call(lib, "fa_kv_append_paged_quant" if quant else "fa_kv_append_paged",
          (k_new.data_ptr(), v_new.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(), cu_seqlens_new.data_ptr(), block_table.data_ptr(),
           seqlens_k.data_ptr(), B, Hkv, k_new.shape[0], int(max_seqlen_new), D, P, num_pages, block_table.shape[1], k_new.stride(0),
           k_new.stride(1), ps, hs, rs, block_table.stride(0), *tail), k_pages.device, stream)


def varlen_backward_supported(dtype: str, D: int) -> bool:
    return bool(load_library().fa_bwd_varlen_supported(DTYPES[dtype], D))


def varlen_backward_workspace_bytes(Hq: int, total_q: int) -> int:
    return int(load_library().fa_bwd_varlen_workspace_bytes(Hq, total_q))


def flash_attention_varlen_backward(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    o: torch.Tensor,
    d_o: torch.Tensor,
    lse: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    is_causal: bool = False,
    scale: Optional[float] = None,
    dq: Optional[torch.Tensor] = None,
    dk: Optional[torch.Tensor] = None,
    dv: Optional[torch.Tensor] = None,
    workspace: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
    window: Optional[Tuple[int, int]] = None,
    sinks: Optional[torch.Tensor] = None,
    dsinks: Optional[torch.Tensor] = None,
    softcap: Optional[float] = None,
):
    """The backward over packed variable-length sequences (include/fa_mi355.h fa_bwd_varlen), the counterpart of
    flash_attention_varlen: q, o, d_o [total_q, Hq, D] under one set of strides, k, v [total_k, Hkv, D] under another, f16 / bf16,
    D = 64 | 128; lse the forward's [Hq, total_q]; the tables as in flash_attention_varlen. Returns (dq, dk, dv) in fp32 under the
    ELEMENT strides of q / k (allocated so unless given: three views of one fp32 [total, Hq + 2*Hkv, D] buffer serve a packed QKV
    projection). Only tokens owned by a sequence are written (allocate with zeros if the rest is read); a query row without a visible
    key gets dQ = 0 and adds nothing to dK / dV. With dq, dk, dv and `workspace` (uint8, at least
    varlen_backward_workspace_bytes(Hq, total_q) bytes) given the call allocates nothing, and it never synchronises or reads a device
    value: it can be captured in a graph and replayed after the tables change in place.
    window=(left, right): the backward of flash_attention_varlen(window=...) (fa_bwd_varlen_window: key j visible to query i iff
    i + Lk_b - Lq_b - left <= j <= i + Lk_b - Lq_b + right, a negative side unbounded; with is_causal the right side is 0); a key no
    query sees gets dK = dV = 0. None: the call above, untouched.
    sinks: the [Hq] sink logits of the forward that wrote o and lse (fa_bwd_varlen_sink). The call then returns (dq, dk, dv, dsinks):
    dsinks fp32 [Hq] (written, not accumulated; allocated unless given), dq / dk / dv bit for bit those of the call without sinks on the
    same tensors. None: the calls above, untouched, three gradients.
    softcap: the cap of the forward that wrote o and lse (fa_bwd_varlen_softcap: dS = P (dP - delta) (1 - tanh^2); the cap itself gets no
    gradient; not together with sinks). None or 0.0: the calls above, untouched."""
    lib = load_library()
    cap = _softcap(softcap, sinks)  # (first: a cap that cannot be served is refused whatever else is wrong)
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or o.shape != q.shape or d_o.shape != q.shape:
        raise ValueError(f"q, o, d_o one [total_q,Hq,D] shape and k, v one [total_k,Hkv,D] shape, got {tuple(q.shape)} {tuple(o.shape)} "
                         f"{tuple(d_o.shape)} {tuple(k.shape)} {tuple(v.shape)}")
    total_q, Hq, D = q.shape
    total_k, Hkv, Dk = k.shape
    if Dk != D or Hkv < 1 or Hq % Hkv:
        raise ValueError(f"incompatible shapes q {tuple(q.shape)} k/v {tuple(k.shape)}")
    if q.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q.dtype for t in (k, v, o, d_o)):
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k.dtype} {v.dtype} {o.dtype} {d_o.dtype} (f16 or bf16)")
    if q.stride(2) != 1 or k.stride(2) != 1:
        raise ValueError("q, k, v need a unit element stride (a head of a token is D contiguous elements)")
    if o.stride() != q.stride() or d_o.stride() != q.stride():
        raise ValueError("q, o and d_o must share row/head strides")
    if v.stride() != k.stride():
        raise ValueError("k and v must share row/head strides")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if cu.dtype != torch.int32 or cu.dim() != 1 or cu.shape[0] < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 [B + 1] tensor")
    if cu_seqlens_k.shape != cu_seqlens_q.shape:
        raise ValueError("cu_seqlens_q and cu_seqlens_k must both be [B + 1]")
    B = cu_seqlens_q.shape[0] - 1
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.shape != (Hq, total_q):
        raise ValueError("lse must be contiguous fp32 [Hq, total_q]")
    if not all(t.is_cuda and t.device == q.device for t in (q, k, v, o, d_o, lse, cu_seqlens_q, cu_seqlens_k)):
        raise RuntimeError("flash_attention_varlen_backward needs every tensor and both cu_seqlens on one device: there is no CPU path")
    grads = []
    for name, g, like in (("dq", dq, q), ("dk", dk, k), ("dv", dv, k)):
        if g is None:
            g = torch.empty_strided(like.shape, like.stride(), dtype=torch.float32, device=q.device)
        elif not g.is_cuda or g.device != q.device or g.dtype != torch.float32 or g.shape != like.shape or g.stride() != like.stride():
            raise ValueError(f"{name} must be an fp32 device tensor with the shape and element strides of {'q' if like is q else 'k'} "
                             "(the kernels write it under those strides)")
        grads.append(g)
    dq, dk, dv = grads
    need = varlen_backward_workspace_bytes(Hq, total_q)
    ws = _workspace(workspace, need, q.device)
    if ws.numel() < need:
        raise ValueError(f"workspace of {ws.numel()} bytes, varlen_backward_workspace_bytes() asks for {need}")
    mask = (int(bool(is_causal)),) if window is None else _window(window, is_causal)
    entry = "fa_bwd_varlen" if window is None else "fa_bwd_varlen_window"
    if sinks is not None:
        sinks = _sinks(sinks, Hq, q.device)
        if dsinks is None:
            dsinks = torch.empty(Hq, dtype=torch.float32, device=q.device)
        elif not dsinks.is_cuda or dsinks.device != q.device or dsinks.dtype != torch.float32 or dsinks.shape != (Hq,) or not dsinks.is_contiguous():
            raise ValueError("dsinks must be a contiguous fp32 [Hq] tensor on q's device")
        entry, mask = "fa_bwd_varlen_sink", _sink_window(window, is_causal) + (sinks.data_ptr(), dsinks.data_ptr())
    elif dsinks is not None:
        raise ValueError("dsinks without sinks")
    if cap is not None:
        entry, mask = "fa_bwd_varlen_softcap", _sink_window(window, is_causal) + (cap,)
    _call(lib, entry,
          (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
           dv.data_ptr(), ws.data_ptr(), cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), B, Hq, Hkv, total_q, total_k,
           int(max_seqlen_q), int(max_seqlen_k), D, _scale(scale, D), q.stride(0), q.stride(1), k.stride(0), k.stride(1),
           *mask, _TORCH2FA[q.dtype]), q.device, stream)
    return (dq, dk, dv) if sinks is None else (dq, dk, dv, dsinks)


def varlen_mla_backward_supported(dtype: str, d_qk: int, d_v: int) -> bool:
    return bool(load_library().fa_bwd_varlen_mla_supported(DTYPES[dtype], int(d_qk), int(d_v)))


def flash_attention_varlen_mla_backward(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    o: torch.Tensor,
    d_o: torch.Tensor,
    lse: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    is_causal: bool = False,
    scale: Optional[float] = None,
    dq: Optional[torch.Tensor] = None,
    dk: Optional[torch.Tensor] = None,
    dv: Optional[torch.Tensor] = None,
    workspace: Optional[torch.Tensor] = None,
    stream: Optional[int] = None,
):
    """The backward of flash_attention_varlen_mla (include/fa_mi355.h fa_bwd_varlen_mla): q [total_q, Hq, 192], k [total_k, Hkv, 192],
    v [total_k, Hkv, 128], o and d_o [total_q, Hq, 128], f16 / bf16; lse the forward's [Hq, total_q]; the tables as in the forward.
    Strides are taken from EACH of q, k, v, o (unit element stride); d_o must have o's strides. Returns (dq, dk, dv) in fp32 under the
    ELEMENT strides of q / k / v respectively (allocated so unless given: with v the upper half of a [total_k, Hkv, 256] up-projection,
    dv is the upper half of an fp32 buffer of that shape). Only tokens owned by a sequence are written (allocate with zeros if the rest
    is read); a query row without a visible key gets dQ = 0 and adds nothing to dK / dV; a key no query sees gets dK = dV = 0.
    scale=None means 192 ** -0.5. With dq, dk, dv and `workspace` (uint8, at least varlen_backward_workspace_bytes(Hq, total_q) bytes)
    given the call allocates nothing, and it never synchronises or reads a device value: it can be captured in a graph and replayed
    after the tables change in place."""
    lib = load_library()
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or o.dim() != 3 or d_o.shape != o.shape:
        raise ValueError(f"q [total_q,Hq,192], k [total_k,Hkv,192], v [total_k,Hkv,128], o and d_o [total_q,Hq,128], got {tuple(q.shape)} "
                         f"{tuple(k.shape)} {tuple(v.shape)} {tuple(o.shape)} {tuple(d_o.shape)}")
    total_q, Hq, Dqk = q.shape
    total_k, Hkv, Dk = k.shape
    Dv = v.shape[2]
    if Dk != Dqk or tuple(v.shape[:2]) != (total_k, Hkv) or tuple(o.shape) != (total_q, Hq, Dv) or Hkv < 1 or Hq % Hkv:
        raise ValueError(f"incompatible shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} o {tuple(o.shape)}")
    if q.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q.dtype for t in (k, v, o, d_o)):
        raise ValueError(f"unsupported / mixed dtypes {q.dtype} {k.dtype} {v.dtype} {o.dtype} {d_o.dtype} (f16 or bf16)")
    if q.stride(2) != 1 or k.stride(2) != 1 or v.stride(2) != 1 or o.stride(2) != 1:
        raise ValueError("q, k, v, o need a unit element stride (a head of a token is contiguous elements)")
    if d_o.stride() != o.stride():
        raise ValueError("o and d_o must share row/head strides")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if cu.dtype != torch.int32 or cu.dim() != 1 or cu.shape[0] < 2 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 [B + 1] tensor")
    if cu_seqlens_k.shape != cu_seqlens_q.shape:
        raise ValueError("cu_seqlens_q and cu_seqlens_k must both be [B + 1]")
    B = cu_seqlens_q.shape[0] - 1
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.shape != (Hq, total_q):
        raise ValueError("lse must be contiguous fp32 [Hq, total_q]")
    if not all(t.is_cuda and t.device == q.device for t in (q, k, v, o, d_o, lse, cu_seqlens_q, cu_seqlens_k)):
        raise RuntimeError("flash_attention_varlen_mla_backward needs every tensor and both cu_seqlens on one device: there is no CPU path")
    grads = []
    for name, g, like, like_name in (("dq", dq, q, "q"), ("dk", dk, k, "k"), ("dv", dv, v, "v")):
        if g is None:
            g = torch.empty_strided(like.shape, like.stride(), dtype=torch.float32, device=q.device)
        elif not g.is_cuda or g.device != q.device or g.dtype != torch.float32 or g.shape != like.shape or g.stride() != like.stride():
            raise ValueError(f"{name} must be an fp32 device tensor with the shape and element strides of {like_name} "
                             "(the kernels write it under those strides)")
        grads.append(g)
    dq, dk, dv = grads
    need = varlen_backward_workspace_bytes(Hq, total_q)
    ws = _workspace(workspace, need, q.device)
    if ws.numel() < need:
        raise ValueError(f"workspace of {ws.numel()} bytes, varlen_backward_workspace_bytes() asks for {need}")
    _call(lib, "fa_bwd_varlen_mla",
          (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
           dv.data_ptr(), ws.data_ptr(), cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), B, Hq, Hkv, total_q, total_k,
           int(max_seqlen_q), int(max_seqlen_k), Dqk, Dv, _scale(scale, Dqk), q.stride(0), q.stride(1), k.stride(0), k.stride(1),
           v.stride(0), v.stride(1), o.stride(0), o.stride(1), int(bool(is_causal)), _TORCH2FA[q.dtype]), q.device, stream)
    return dq, dk, dv


def flash_attention_backward(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    o: torch.Tensor,
    d_o: torch.Tensor,
    lse: torch.Tensor,
    is_causal: bool = False,
    scale: Optional[float] = None,
    stream: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(Q,K,V,O,dO,LSE) -> (dQ,dK,dV) in fp32, laid out like their inputs (binding table of
    /root/reference/kernels.metal:905-921; gradients are written, not accumulated). k / v may carry fewer heads than q and
    another sequence length (include/fa_mi355.h fa_bwd_ex, the counterpart of fa_fwd_ex): dK / dV have k's shape."""
    lib = load_library()
    if q.dim() != 4 or any(t.shape != q.shape for t in (o, d_o)) or k.dim() != 4 or v.shape != k.shape:
        raise ValueError("q, o, d_o must share one [B,Hq,N,D] shape and k, v one [B,Hkv,N,D] shape")
    _on_device("flash_attention_backward", q, k, v, o, d_o, lse)
    if q.dtype == _FP8:  # e4m3 Q, K, V with the bf16 O the forward wrote for them (and a bf16 dO)
        if any(t.dtype != q.dtype for t in (k, v)) or any(t.dtype != torch.bfloat16 for t in (o, d_o)):
            raise ValueError("backward with e4m3 q needs e4m3 k, v and bf16 o, d_o")
    elif q.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q.dtype for t in (k, v, o, d_o)):
        raise ValueError("backward supports f16 / bf16 tensors of one dtype (or e4m3 q, k, v with bf16 o, d_o)")
    B, H, N, D = q.shape
    Bk, Hkv, Nk, Dk = k.shape
    if (Bk, Dk) != (B, D) or H % Hkv:
        raise ValueError(f"k/v shape {tuple(k.shape)} does not fit q {tuple(q.shape)} (same B, D; Hq % Hkv == 0)")
    qs, ks = _strides(q), _kv_strides(k, v)
    if any(_strides(t) != qs for t in (o, d_o)):
        raise ValueError("q, o, d_o must share batch/head strides, and so must k, v")
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H * N:
        raise ValueError("lse must be contiguous fp32 [B,H,N]")
    dq = torch.empty_strided((B, H, N, D), q.stride(), dtype=torch.float32, device=q.device)
    dk, dv = (torch.empty_strided((B, Hkv, Nk, D), k.stride(), dtype=torch.float32, device=q.device) for _ in range(2))
    ws = _workspace(None, lib.fa_bwd_workspace_bytes_ex(_TORCH2FA[q.dtype], B, H, Hkv, N, Nk, D, *qs, *ks), q.device)
    _call(lib, "fa_bwd_ex", (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                             dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), B, H, Hkv, N, Nk, D, _scale(scale, D), *qs, *ks,
                             int(bool(is_causal)), _TORCH2FA[q.dtype]), q.device, stream)
    return dq, dk, dv
