"""GPU: fa_fwd_mla_decode_sparse on a latent pool of a little over 4 GiB whose listed slots all lie past byte 2^32 and element 2^31 (the
manner of tests/test_gpu_far_addresses_mla.py, case M-D). Only the listed rows of the big pool are initialised; what the call returns
must be, bit for bit, what it returns on a compact pool that holds the same pages (the same T, Hq and topk: the same split count and
workspace), and that is held to fp64. A slot address formed in 32 bits -- elements or bytes -- lands in the uninitialised low part of
the pool or outside the listed pages and cannot give those bits. The peak stays under 6 GiB."""
import numpy as np
import pytest

import far
import mla
import mla_sparse
from test_gpu_far_addresses import Arena, bits, fa, same, typed  # noqa: F401  (fa: the fixture)
from test_gpu_mla_decode import _dev, _i32, _np

pytestmark = pytest.mark.gpu
DQK, DV, SCALE = mla.DQK, mla.DV, mla.SCALE


def test_listed_slots_past_byte_2_32(fa, oracle_mod):
    import torch

    dtype, P, T, Hq, topk = "bf16", 256, 4, 33, 320
    page = P * DQK                                  # elements of a page (compact rows and pages)
    first = -(-(1 << 31) // page) + 1               # the first page that lies wholly past element 2^31 = byte 2^32, and one more
    used = 23                                       # pages the lists draw from
    num_pages = first + used
    assert first * page * 2 > (1 << 32) and first * page > (1 << 31) and 4 * far.GIB < num_pages * page * 2 < 4.1 * far.GIB
    rng = np.random.default_rng(3501)
    c = {"Hq": Hq, "topk": topk, "P": P, "dtype": dtype, "T": T, "kind": "perm",
         "q": oracle_mod.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), dtype),
         "pool": mla_sparse.make_pool(oracle_mod, rng, P, used * P, dtype),
         "indices": mla_sparse.make_lists(rng, T, topk, topk, used * P, "perm"),
         "counts": np.array([320, 65, 1, 200], np.int32)}
    c["indices"][0, :2] = [0, used * P - 1]  # the first listed page's first slot and the pool's last slot
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    qd, cnt, compact = _dev(c["q"], dtype), _i32(c["counts"]), _dev(c["pool"], dtype)
    torch.cuda.reset_peak_memory_stats()
    o_c, l_c = fa.flash_attention_mla_decode_sparse(qd, compact, _i32(c["indices"]), SCALE, index_counts=cnt)
    torch.cuda.synchronize()
    on, ln = _np(o_c, l_c)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(c["q"]), c["kvs"], c["lens"], False, dtype, "FAR sparse, compact")
    with Arena() as a:
        ints = a.ints(dtype, num_pages * page, sentinel=False)  # left as allocated: only the listed rows are written
        big = typed(ints, dtype).view(num_pages, P, DQK)
        far_idx = c["indices"].astype(np.int64) + first * P
        assert far_idx.max() < num_pages * P < (1 << 30) and far_idx.min() * DQK >= (1 << 31)
        for t in range(T):
            rows = torch.from_numpy(c["indices"][t, :c["lens"][t]].astype(np.int64)).cuda()
            bits(big.view(-1, DQK))[rows + first * P] = bits(compact.view(-1, DQK))[rows]
        o_f, l_f = fa.flash_attention_mla_decode_sparse(qd, big, _i32(far_idx), SCALE, index_counts=cnt)
        torch.cuda.synchronize()
        assert same(o_f, o_c) and same(l_f, l_c), "the far pool differs from the compact one"
    peak = torch.cuda.max_memory_allocated()
    print(f"FAR sparse: pool {num_pages * page * 2 / far.GIB:.3f} GiB, first listed byte 2^32 + {first * page * 2 - (1 << 32)}, peak {peak / far.GIB:.2f} GiB")
    assert peak < 6 * far.GIB, peak
