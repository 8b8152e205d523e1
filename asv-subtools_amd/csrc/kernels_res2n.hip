// The Res2 block of the 64-channel-wide ECAPA-TDNN trunks (model/ecapa-tdnn-xvector.py at channels = 512: Res2Conv1dReluBn; the wiring of
// model/ecapa_tdnn_xvector.py at C = 512 as well) as ONE kernel.
//
//   x_0 .. x_n = the n + 1 groups of 64 channels of the block input; group `pass_group` passes through: y_p = x_p.  The other groups, in
//   ascending order, form the chain: the first  y = BN(ReLU(TDNN_{[-d, 0, d]}(x))),  every later one  y_g = BN(ReLU(TDNN(y_prev + x_g)));
//   output = cat(y_0 .. y_n).  Bias optional.  1 <= d <= 4, n <= 7.
//
// As n launches each 64 -> 64 convolution reads two and writes one [rows][64] slice through HBM / L2 for 24 kFLOP per row and waits for
// the one before it.  Here a workgroup owns 192 output rows and walks the chain with the running tensor in LDS:
//   * window = 192 rows + 32 recomputed rows on each side (branch i needs y_{i-1} at rows +-d: after seven branches 7 d <= 28 rows of
//     the margin are stale, the 192 central rows are exact; 75 % of the matrix work is output);
//   * ONE LDS image A of the window, [row][64 ch] 16-bit = 128-byte rows with the 16-byte slots swizzled (lds_dma.h lds_swz), 4 zero rows
//     above and below: the input of the running convolution, read with the three taps as shifted rows.  The epilogue rounds y to the
//     element type, stores the central rows, adds the next group (fetched into registers in the accumulator layout BEFORE the K loop, so
//     the loads fly behind it) and writes round(round(y) + x) back into A: the roundings of the per-layer path, so the results differ
//     from it by the f32 summation order only;
//   * 4 waves = 2 channel fragments x 2 row halves, each 128 rows x 32 channels (4 accumulators), K = 3 taps x 64 as 12 k-groups; a
//     branch's 12 weight fragments per wave (48 registers, fragment order of pack_tdnn_weight_frags) come from L2, fetched during the
//     previous branch's epilogue.  At this width a row is 128 B and a branch's weights are 24 KB: plain loads whose waits the compiler
//     counts, no LDS-DMA and no inline assembly - the image is 33 KiB, so several workgroups share a CU and cover each other's barriers
//     and load latencies (designed for 2 waves per SIMD: <= 256 registers);
//   * the epilogue is the per-layer kernels' arithmetic - bias added behind the sum, in IEEE half the last multiply-add rounded ONCE to half -,
//     so on the same operands the results are the per-branch path's bits (tests/test_gpu_res2n_kernel.py);
//   * two barriers per branch.
// Every output row is computed from the same operands in the same order whichever workgroup owns it and whatever its neighbours hold:
// rows outside the matrix and gap rows are zeros, as in the row layout itself.
#include "lds_dma.h"

namespace asv {
namespace {

constexpr int NW = kRes2nWidth;            // 64 channels per group
constexpr int NROWB = NW * 2;              // 128 B per row
constexpr int NWIN = 256;                  // window rows
constexpr int NMARGIN = 32;                // recomputed rows per side (>= 7 branches x dilation 4)
constexpr int NM = NWIN - 2 * NMARGIN;     // 192 output rows per workgroup
constexpr int NPAD = 4;                    // zero rows around the image (taps of the outermost window rows)
constexpr int NFRAG = 4;                   // 32-row fragments per wave
static_assert(7 * kHalo <= NMARGIN && kHalo <= NPAD, "margin must cover seven branches of the largest dilation");
static_assert(ASV_RES2N_TILE_ROWS == NM, "the tile asv_amd.h documents");

__device__ __forceinline__ uint32_t img_off(int row, int slot) { return (uint32_t)(row * NROWB + (lds_swz(row, slot) << 4)); }

template <int ET>
__global__ __launch_bounds__(256, 2) void res2n_chain_kernel(const Res2nKernelParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[(NWIN + 2 * NPAD) * NROWB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nf = wave & 1, rh = wave >> 1;                 // channel fragment, row half
  const int lr = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * NM;
  const int rbase = rh * NFRAG * 32;                        // first window row of this wave
  const int d = p.dilation, pg = p.pass_group;
  const unsigned char *xg = reinterpret_cast<const unsigned char *>(p.x);
  unsigned char *yg = reinterpret_cast<unsigned char *>(p.y);
  const size_t x_pitch = (size_t)p.ldx * 2, y_pitch = (size_t)p.ldy * 2;
  auto group_of = [&](int b) { return b < pg ? b : b + 1; };       // the b-th convolved group

  // weight fragments of one branch: [n-fragment][tap][k-group] blocks of 1 KiB, 12 per 32-channel fragment
  uint4 wf[12];
  auto load_weights = [&](int b) {
    const unsigned char *wb = reinterpret_cast<const unsigned char *>(p.wfrag) + ((size_t)b * 2 + nf) * (12 * 1024) + (size_t)lane * 16;
#pragma unroll
    for (int k = 0; k < 12; ++k) wf[k] = *reinterpret_cast<const uint4 *>(wb + k * 1024);
  };
  load_weights(0);
  // A = the window of the first convolved group; rows outside the matrix are zeros
  {
    const int g = group_of(0);
#pragma unroll
    for (int it = 0; it < NWIN * 8 / 256; ++it) {
      const int idx = it * 256 + tid, r = idx >> 3, slot = idx & 7, grow = m0 - NMARGIN + r;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (grow >= 0 && grow < p.rows) v = *reinterpret_cast<const uint4 *>(xg + (size_t)grow * x_pitch + (size_t)g * NROWB + slot * 16);
      *reinterpret_cast<uint4 *>(lds + img_off(NPAD + r, slot)) = v;
    }
    if (tid < 2 * NPAD * 8) {
      const int r = tid >> 3, row = r < NPAD ? r : NWIN + r;
      *reinterpret_cast<uint4 *>(lds + img_off(row, tid & 7)) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  // the pass-through group
#pragma unroll
  for (int it = 0; it < NM * 8 / 256; ++it) {
    const int idx = it * 256 + tid, row = m0 + (idx >> 3), slot = idx & 7;
    if (row < p.rows)
      *reinterpret_cast<uint4 *>(yg + (size_t)row * y_pitch + (size_t)pg * NROWB + slot * 16) =
          *reinterpret_cast<const uint4 *>(xg + (size_t)row * x_pitch + (size_t)pg * NROWB + slot * 16);
  }
  // this lane's four window rows: inside the matrix / holding a frame (gap rows and rows outside produce zeros)
  bool inside[NFRAG], valid[NFRAG];
#pragma unroll
  for (int rf = 0; rf < NFRAG; ++rf) {
    const int grow = m0 - NMARGIN + rbase + rf * 32 + lr;
    inside[rf] = grow >= 0 && grow < p.rows;
    valid[rf] = inside[rf] && ((p.row_valid[grow >> 5] >> (grow & 31)) & 1u);
  }
  __syncthreads();

#pragma unroll 1
  for (int b = 0; b < p.branches; ++b) {
    const int g = group_of(b);
    const bool more = b + 1 < p.branches;
    const int cbase = nf * 32 + 4 * lh;                     // channel of acc[.][4 q + e]: cbase + 8 q + e
    // the next group in the accumulator layout: 8 bytes per (fragment, q), consumed by the epilogue
    uint2 xn[NFRAG][4];
    if (more) {
      const size_t goff = (size_t)group_of(b + 1) * NROWB + (size_t)cbase * 2;
#pragma unroll
      for (int rf = 0; rf < NFRAG; ++rf) {
        const int grow = m0 - NMARGIN + rbase + rf * 32 + lr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          xn[rf][q] = make_uint2(0u, 0u);
          if (inside[rf]) xn[rf][q] = *reinterpret_cast<const uint2 *>(xg + (size_t)grow * x_pitch + goff + q * 16);
        }
      }
    }
    f32x16_t acc[NFRAG];
#pragma unroll
    for (int rf = 0; rf < NFRAG; ++rf)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[rf][e] = 0.0f;
    // K loop: k-group (tap t, 16-channel group kg); lane half lh holds channels kg * 16 + lh * 8 .. + 7 of its row
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int kg = 0; kg < 4; ++kg) {
        uint4 xr[NFRAG];
#pragma unroll
        for (int rf = 0; rf < NFRAG; ++rf) xr[rf] = *reinterpret_cast<const uint4 *>(lds + img_off(NPAD + rbase + rf * 32 + lr + (t - 1) * d, kg * 2 + lh));
#pragma unroll
        for (int rf = 0; rf < NFRAG; ++rf) acc[rf] = mfma16<ET>(wf[t * 4 + kg], xr[rf], acc[rf]);
      }
    }
    if (more) load_weights(b + 1);                           // the fragment registers are free: the next branch's fly during the epilogue
    __syncthreads();                                         // nobody reads the image any more

    // epilogue: y = BN(ReLU(acc + bias)) (zeros in gap rows), rounded -> HBM (central rows); round(y) + x_next -> the image
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 sc4 = *reinterpret_cast<const float4 *>(p.scale + b * NW + cbase + 8 * q), sh4 = *reinterpret_cast<const float4 *>(p.shift + b * NW + cbase + 8 * q);
      float4 b4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (p.bias != nullptr) b4 = *reinterpret_cast<const float4 *>(p.bias + b * NW + cbase + 8 * q);
      const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w}, bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int rf = 0; rf < NFRAG; ++rf) {
        const int rw = rbase + rf * 32 + lr, grow = m0 - NMARGIN + rw;
        uint2 pk;
        if constexpr (ET == ET_F16) {
          // IEEE half: the last multiply-add and the conversion as ONE rounding (v_fma_mix*_f16: f32 sources, half result) - what hipcc
          // makes of the per-layer kernels' "store_elem(epilogue)"; f32 first and half second would move a value by one unit in the last
          // place now and then.  The instruction is written out: packing two results makes hipcc choose the two-step form here.
          uint32_t w[2] = {0u, 0u};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float z = max_lo(acc[rf][q * 4 + e] + bs[e], 0.0f);
            if (e & 1) asm("v_fma_mixhi_f16 %0, %1, %2, %3" : "+v"(w[e >> 1]) : "v"(sc[e]), "v"(z), "v"(sh[e]));
            else asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "+v"(w[e >> 1]) : "v"(sc[e]), "v"(z), "v"(sh[e]));
          }
          pk.x = valid[rf] ? w[0] : 0u;
          pk.y = valid[rf] ? w[1] : 0u;
        } else {
          float y[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = tdnn_epilogue_fast(acc[rf][q * 4 + e], bs[e], 0.0f, sc[e], sh[e], valid[rf]);     // the per-layer kernels' own expression
          pk.x = pack_h16x2<ET>(y[0], y[1]);
          pk.y = pack_h16x2<ET>(y[2], y[3]);
        }
        if (rw >= NMARGIN && rw < NMARGIN + NM && inside[rf])
          *reinterpret_cast<uint2 *>(yg + (size_t)grow * y_pitch + (size_t)g * NROWB + (size_t)(cbase + 8 * q) * 2) = pk;
        if (more) {
          float p0, p1, p2, p3, x0, x1, x2, x3;
          unpack_h16x2<ET>(pk.x, p0, p1); unpack_h16x2<ET>(pk.y, p2, p3);
          unpack_h16x2<ET>(xn[rf][q].x, x0, x1); unpack_h16x2<ET>(xn[rf][q].y, x2, x3);
          uint2 sv;
          sv.x = pack_h16x2<ET>(p0 + x0, p1 + x1);
          sv.y = pack_h16x2<ET>(p2 + x2, p3 + x3);
          *reinterpret_cast<uint2 *>(lds + img_off(NPAD + rw, nf * 4 + q) + lh * 8) = sv;
        }
      }
    }
    __syncthreads();                                         // the image of the next branch is complete
  }
}

}  // namespace

int launch_res2n_chain(const Res2nKernelParams &p, hipStream_t s) {
  ASV_REQUIRE(p.rows >= 1, "res2n: %d rows", p.rows);
  ASV_REQUIRE(p.branches >= 1 && p.branches <= 7 && p.dilation >= 1 && p.dilation <= kHalo && p.pass_group >= 0 && p.pass_group <= p.branches,
              "res2n: %d branches, pass group %d, dilation %d", p.branches, p.pass_group, p.dilation);
  ASV_REQUIRE(p.x && p.y && p.wfrag && p.scale && p.shift && p.row_valid, "res2n: null argument");
  ASV_REQUIRE(p.et == ET_BF16 || p.et == ET_F16, "res2n: 16-bit element types only");
  const dim3 grid((p.rows + NM - 1) / NM);                   // the last tile may overhang the matrix: its loads and stores are guarded
  if (p.et == ET_F16) hipLaunchKernelGGL((res2n_chain_kernel<ET_F16>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((res2n_chain_kernel<ET_BF16>), grid, dim3(256), 0, s, p);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

}  // namespace asv
