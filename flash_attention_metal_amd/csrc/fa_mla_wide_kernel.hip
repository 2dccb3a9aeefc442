// fa_mla_wide_kernel.hip -- the absorbed latent-attention decode for up to 128 packed query rows: entry point fa_fwd_mla_decode_paged_wide.
//
// fa_mla_kernel.hip gives every 16 packed rows a one-wave item of their own that streams the sequence's 72-KiB tiles through a private
// double buffer: 32 rows stream every latent row twice, and the one wave issues all 72 LDS-DMA pieces of a tile between its own 200 LDS
// reads and 136 MFMAs. Here a WORKGROUP of NW waves (2 up to 32 rows, 4 above) shares ONE double buffer:
//   * wave w of row block wb IS that one-wave item on rows r = 16 (wb NW + w) + c = h * Nq + iq: the text of fa_mla_body.h, so the same
//     Q~ fragments, the same 18 k-steps in the same order, the same mask, online softmax, 64 PV steps and partial store -- the same bits;
//   * the image and its two swizzles are fa_mla_kernel.hip's (every wave's read pattern is the one whose conflict-freedom is argued at
//     the head of that file); each latent row is streamed once for 16 NW query rows;
//   * the kernel IS that file's, one text at NW waves (fa_mla_paged_partial.inc): wave w stages latent rows (64 / NW) w .. + 64 / NW - 1
//     of every tile and the rotary pieces over the same rows, under the same descriptor rules; one barrier per tile behind the explicit
//     wait, met by every wave in every iteration, padding waves included. The piece split, the descriptor rules and the argument for the
//     barrier's uniformity stand at the head of that text;
//   * the workspace keeps fa_mla_kernel.hip's format, [B . S][RBLK = ceil(Hq Nq / 16)][MLA_IST] with wave w of block wb on 16-row slot
//     wb NW + w, so that file's combine kernel serves this call unchanged (launch_mla_combine).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "fa_mfma_common.h"

namespace fa {

#define FA_MLA_BODY_PART 0
#include "fa_mla_body.h"  // the tile's shape and image, the MFMA types, the launch tail

// workgroup (b, s) x row block wb, wave w: rows r = 16 (wb NW + w) + c of the packed block, keys of tiles [t0, t1) of sequence b
template <typename Tag, bool CAUSAL, int NW>
__global__ __launch_bounds__(64 * NW) void mla_wide_partial_kernel(MlaDecodeParams p) {
// (this spelling and not fa_mla_kernel.hip's initialiser: with the initialiser the NW = 2 kernels move)
#define FA_MLA_PG_DECL int pg[MAXPG]; _Pragma("unroll") for (int k = 0; k < MAXPG; ++k) pg[k] = -1;
#include "fa_mla_paged_partial.inc"
}

long long mla_decode_wide_workspace_bytes(int B, int Hq, int Nq, int Nk) {
  const int rows = Hq * Nq, rblk = (rows + 15) / 16, nw = mla_wide_waves(rows);
  return (long long)B * mla_decode_splits(B, (rblk + nw - 1) / nw, Nk) * rblk * MLA_IST * 4;
}

// One call: the partial kernel over B . S items x ceil(RBLK / NW) row blocks of NW waves, then fa_mla_kernel.hip's combine kernel over
// the output rows, on the same stream
hipError_t launch_mla_decode_paged_wide(const MlaDecodeParams &p, int dtype, hipStream_t s) {
  return with_tag(dtype, [&](auto tag) {
    using Tag = decltype(tag);
    auto go = [&](auto partial, int nw) { return launch_mla_partial_and_combine(partial, dim3(p.B * p.S, (p.RBLK + nw - 1) / nw), nw, p, p, dtype, s); };
    if (mla_wide_waves(p.Hq * p.Nq) == 2) return p.is_causal ? go(mla_wide_partial_kernel<Tag, true, 2>, 2) : go(mla_wide_partial_kernel<Tag, false, 2>, 2);
    return p.is_causal ? go(mla_wide_partial_kernel<Tag, true, 4>, 4) : go(mla_wide_partial_kernel<Tag, false, 4>, 4);
  });
}

}  // namespace fa
