// The fused statistics pooling of the layer-chain kernels (kernels_tdnn_chain.hip, _chainx, _chainm, tools/kernels_tdnn_chain4.hip):
// a tile of rows publishes, per utterance it holds ("segment slot") and lane half, the moments of the last layer's output about a
// pivot,
//   P[tile][segment slot][lh][3 = sum (u - pv), sum (u - pv)^2, pv][channel],
// which pool_finish_kernel (kernels_pool.hip) merges in row order (Chan et al.) and to which it adds the BN shift.
#pragma once
#include "device_utils.h"

namespace asv {

// The utterance of segment slot 0 of the tile that starts at `row0`: that of its first row that belongs to one (utterances are
// separated by kHalo gap rows, marked -1 in p.row_seg); -1 for a tile of gap rows only.
__device__ __forceinline__ int pool_first_seg(const TdnnChainParams &p, int row0) {
  int first_seg = -1;
#pragma unroll
  for (int k = 0; k < kHalo + 1; ++k)
    if (first_seg < 0 && row0 + k < p.rows) first_seg = p.row_seg[row0 + k];
  return first_seg;
}

// Publication of utterance cur_seg's moments by one lane: channels cb + lr and cb + 32 + lr, lane half lh.  The BN scale sc
// multiplies the three moments here (u = scale * act(acc): moments about a pivot are linear / quadratic in it).
__device__ __forceinline__ void pool_publish_moments(const TdnnChainParams &p, int tile, int first_seg, int cur_seg, int cb, int lr, int lh,
                                                     const float (&ps)[2], const float (&pq)[2], const float (&pv)[2], const float (&sc)[2]) {
  const int slot = cur_seg - first_seg;
  if (cur_seg >= 0 && slot >= 0 && slot < p.pool_slots) {
    float *dst = p.pool_partial + ((size_t)((tile * p.pool_slots + slot) * 2 + lh) * 3) * p.ld_partial + cb + lr;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (cb + j * 32 + lr < p.ld_partial) {
        dst[j * 32] = ps[j] * sc[j];
        dst[j * 32 + p.ld_partial] = pq[j] * sc[j] * sc[j];
        dst[j * 32 + 2 * p.ld_partial] = pv[j] * sc[j];
      }
  }
}

// Pooling epilogue of a 64-channel unit of the last layer in the 64-frame chains (kernels_tdnn_chainx.hip, kernels_tdnn_chainm.hip),
// registers only.  acc[i][j][r] = channel cb + j*32 + lr, frame i*32 + 8 (r >> 2) + 4 lh + (r & 3), still carrying the weight scale
// (`unscale` = 1 / w_scale); rowseg = the utterance of row `lane` of the tile.  A lane sums its own frames per utterance about a
// pivot and the two lane halves publish separate partials.  (kernels_tdnn_chain.hip has the same walk with packed f32 arithmetic,
// another summation order and a fast path for whole fragments: its results differ in the last bits, so it keeps its own.)
//
// The pivot rule: the pivot is the lane's FIRST frame of the utterance, in whichever fragment of the tile that frame lies.  Until
// round 5 it was only taken in the utterance's first fragment: a lane half without a frame there - an utterance that starts in the
// last rows of a fragment - kept the PREVIOUS utterance's pivot for the rest of the tile.  Harmless between utterances of like
// scale; next to one whose activations are 1e5 x larger the sums about that pivot cancelled and the embedding depended on its
// batch neighbour: tests/test_gpu_xvector.py::test_pooled_moments_ignore_the_neighbour.
__device__ __forceinline__ void chain64_pool_epilogue(const f32x16_t (&acc)[2][2], const TdnnChainParams &p, const TdnnChainLayer &L, int cb, int tile,
                                                      int first_seg, int rowseg, int lr, int lh, float unscale, float act_lo) {
  const float sc[2] = {L.scale != nullptr ? L.scale[cb + lr] : 1.0f, L.scale != nullptr ? L.scale[cb + 32 + lr] : 1.0f};
  float ps[2] = {0.f, 0.f}, pq[2] = {0.f, 0.f}, pv[2] = {0.f, 0.f};
  int cur_seg = -1;                      // uniform: all lanes walk the utterances of the tile together
  bool have = false;                     // per lane: pv is a frame of cur_seg (the lane has had a frame of it in this tile)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int shift = i * 32;
    uint32_t rem = (uint32_t)(__builtin_amdgcn_ballot_w64(rowseg >= 0) >> shift);       // rows of the fragment that belong to an utterance
    if (rem == 0) continue;                                                              // gap rows only
    float u[2][16];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) u[j][r] = max_lo(acc[i][j][r] * unscale, act_lo);
    while (rem != 0) {                                       // one run per utterance present, in row order
      const int sg = __builtin_amdgcn_readlane(rowseg, shift + __builtin_ctz(rem));
      const uint32_t bits = (uint32_t)(__builtin_amdgcn_ballot_w64(rowseg == sg) >> shift) & rem;
      rem &= ~bits;
      const bool fresh = sg != cur_seg;
      if (fresh) {
        pool_publish_moments(p, tile, first_seg, cur_seg, cb, lr, lh, ps, pq, pv, sc);
        cur_seg = sg;
        have = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) { ps[j] = 0.0f; pq[j] = 0.0f; }
      }
      // register r of this lane holds frame 8 (r >> 2) + 4 lh + (r & 3) -> bit r of the lane's mask
      const uint32_t x = bits >> (4 * lh);
      const uint32_t lm = (x & 0xfu) | ((x >> 4) & 0xf0u) | ((x >> 8) & 0xf00u) | ((x >> 12) & 0xf000u);
      const bool need = !have && lm != 0;                    // the pivot rule above
      if (__builtin_amdgcn_ballot_w64(need) != 0) {
        const int rsel = need ? __builtin_ctz(lm) : 16;
#pragma unroll
        for (int r = 15; r >= 0; --r) {
          const bool hit = rsel == r;
          pv[0] = hit ? u[0][r] : pv[0];
          pv[1] = hit ? u[1][r] : pv[1];
        }
        have = have || need;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tm = (int)(lm << (31 - r)) >> 31;          // all ones where the frame is in the run
        const float da = __int_as_float(__float_as_int(u[0][r] - pv[0]) & tm), db = __int_as_float(__float_as_int(u[1][r] - pv[1]) & tm);
        ps[0] += da; pq[0] = fmaf(da, da, pq[0]);
        ps[1] += db; pq[1] = fmaf(db, db, pq[1]);
      }
    }
  }
  pool_publish_moments(p, tile, first_seg, cur_seg, cb, lr, lh, ps, pq, pv, sc);
}

}  // namespace asv
