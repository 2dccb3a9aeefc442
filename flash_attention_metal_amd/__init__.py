"""MI355X-native attention forward: (Q, K, V, is_causal) -> O (+ LSE).

Host-side mirror of the reference operator (the Metal binding table of
``flash_attention_v4_half_kernel``, /root/reference/kernels.metal:600-613, as
the host binds it at /root/reference/main.mm:821-852) over the C-ABI in
``include/fa_mi355.h``. The compute is hand-written HIP for gfx950 in
``csrc/``; torch is used for device memory and streams only. There is no CPU
fallback: importing works anywhere, calling the operator without the built
library or without a GPU raises.
"""
from ._lib import LibraryNotBuilt, lib_path, load_library, build_library  # noqa: F401
from .ops import (  # noqa: F401
    DTYPES,
    VARIANTS,
    FaError,
    ForwardPlan,
    algorithmic_bytes,
    algorithmic_flops,
    decode_paged_workspace_bytes,
    decode_workspace_bytes,
    flash_attention_backward,
    flash_attention_decode,
    flash_attention_decode_paged,
    flash_attention_forward,
    flash_attention_mla_decode_paged,
    flash_attention_mla_decode_sparse,
    flash_attention_varlen,
    flash_attention_varlen_backward,
    flash_attention_varlen_mla,
    flash_attention_varlen_mla_backward,
    flash_attention_varlen_paged,
    forward_kernel_name,
    kv_append_paged,
    mla_decode_paged_kv8_supported,
    mla_decode_paged_kv8_workspace_bytes,
    mla_decode_paged_supported,
    mla_decode_paged_wide_supported,
    mla_decode_paged_wide_workspace_bytes,
    mla_decode_paged_workspace_bytes,
    mla_decode_sparse_kv8_supported,
    mla_decode_sparse_kv8_workspace_bytes,
    mla_decode_sparse_supported,
    mla_decode_sparse_workspace_bytes,
    supported,
    varlen_backward_supported,
    varlen_backward_workspace_bytes,
    varlen_mla_backward_supported,
    varlen_mla_supported,
    varlen_paged_kv8_supported,
    varlen_paged_num_splits,
    varlen_paged_split_workspace_bytes,
    varlen_paged_supported,
    varlen_supported,
)
from .shard import shard_heads  # noqa: F401

__version__ = "0.4.0"
