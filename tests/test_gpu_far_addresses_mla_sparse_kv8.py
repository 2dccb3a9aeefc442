"""GPU: fa_fwd_mla_decode_sparse_kv8 on an e4m3 latent pool of a little over 4 GiB whose listed slots all lie past byte 2^32 (the manner
of tests/test_gpu_far_addresses_mla_sparse.py). The big pool is 0x7F everywhere but in the listed rows; what the call returns must be,
bit for bit, what it returns on a compact pool that holds the same pages (the same T, Hq and topk: the same split count and
workspace), and that is held to fp64. A slot address formed in 32 bits lands in the low, 0x7F-filled part of the pool or outside the
listed pages and cannot give those bits. The peak stays under 6 GiB (the family's files allow 32)."""
import numpy as np
import pytest

import far
import mla
import mla_sparse
import mla_sparse_kv8 as msk
from test_gpu_far_addresses import Arena, bits, fa, same, typed  # noqa: F401  (fa: the fixture)
from test_gpu_mla_decode import _dev, _i32, _np
from test_gpu_mla_decode_kv8 import _pool8

pytestmark = pytest.mark.gpu
DQK, DV, SCALE, DTYPE = mla.DQK, mla.DV, mla.SCALE, msk.DTYPE


def test_listed_slots_past_byte_2_32(fa, oracle_mod):
    import torch

    P, T, Hq, topk = 256, 4, 33, 320
    page = P * DQK                                  # bytes of a page (compact rows and pages)
    first = -(-(1 << 32) // page) + 1               # the first page that lies wholly past byte 2^32, and one more
    used = 23                                       # pages the lists draw from
    num_pages = first + used
    assert first * page > (1 << 32) and 4 * far.GIB < num_pages * page < 4.1 * far.GIB
    rng = np.random.default_rng(3551)
    indices = mla_sparse.make_lists(rng, T, topk, topk, used * P, "perm")
    indices[0, :2] = [0, used * P - 1]  # the first listed page's first slot and the pool's last slot
    counts = np.array([320, 65, 1, 200], np.int32)
    codes, twin = msk.make_pools(rng, P, used * P, indices, counts, topk)
    c = {"Hq": Hq, "topk": topk, "P": P, "dtype": DTYPE, "T": T, "kind": "perm", "codes": codes, "pool": twin, "indices": indices, "counts": counts,
         "q": oracle_mod.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)}
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    qd, cnt = _dev(c["q"], DTYPE), _i32(counts)
    raw, compact = _pool8(codes, P)
    torch.cuda.reset_peak_memory_stats()
    o_c, l_c = fa.flash_attention_mla_decode_sparse(qd, compact, _i32(indices), SCALE, index_counts=cnt)
    torch.cuda.synchronize()
    on, ln = _np(o_c, l_c)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(c["q"]), c["kvs"], c["lens"], False, DTYPE, "FAR sparse kv8, compact")
    with Arena() as a:
        ints = a.ints("fp8", num_pages * page)  # 0x7F everywhere: only the listed rows are written
        big = typed(ints, "fp8").view(num_pages, P, DQK)
        far_idx = indices.astype(np.int64) + first * P
        assert far_idx.max() < num_pages * P < (1 << 30) and far_idx.min() * DQK >= (1 << 32)
        for t in range(T):
            rows = torch.from_numpy(indices[t, :c["lens"][t]].astype(np.int64)).cuda()
            bits(big.view(-1, DQK))[rows + first * P] = bits(compact.reshape(-1, DQK))[rows]
        o_f, l_f = fa.flash_attention_mla_decode_sparse(qd, big, _i32(far_idx), SCALE, index_counts=cnt)
        torch.cuda.synchronize()
        assert same(o_f, o_c) and same(l_f, l_c), "the far pool differs from the compact one"
    peak = torch.cuda.max_memory_allocated()
    print(f"FAR sparse kv8: pool {num_pages * page / far.GIB:.3f} GiB, first listed byte 2^32 + {first * page - (1 << 32)}, peak {peak / far.GIB:.2f} GiB")
    assert peak < 6 * far.GIB, peak
