// Stride-1 grid convolution with a RUNTIME tap table (asv_net_add_grid_conv): the folded 5 x 5 kernels of the RepSPK blocks
// (libs/nnet/repvgg.py: 17 live taps - the 3 x 3 at the centre, the 3 x 3 at dilation 2 and their shared centre), or any set of up
// to 25 (time, frequency) offsets within +-2 on a reach-2 grid (runtime.hip Domain: pitch >= width + 2, so a frequency offset of
// +-2 lands in the zero columns, and 2 pitch + 3 gap rows between utterances, so a time offset of +-2 lands in a gap).
//
//   y[row][co] = act( bias[co] + sum_chunk sum_tap sum_k  w[co][chunk k][tap] * x[row + off[tap]][chunk k] ),   0 on rows that are not valid
//
// One workgroup = 128 output rows x up to 128 output channels, four waves of 32 rows each.  Per 128-byte channel chunk (32 f32 /
// 64 16-bit channels) the activation window - 128 rows + the layer's halo on either side, at most 2 x 168 - is staged in LDS ONCE
// through the LDS-DMA (lds_dma.h glds16) and every tap reads it shifted: 16-byte slot s of window row w sits at lds_swz(w, s), so
// the 32 consecutive rows a fragment read touches spread over all banks whatever the shift.  The weights come from global memory
// (L2) in matrix-fragment order, packed by pack_grid_conv_taps (weight_pack.cpp) at add time.
//
// Accumulation order (fixed, a property of the kernel and never of the batch): chunk outermost, taps in table order, the four
// slot pairs of the chunk, and inside the matrix instruction.  Element types: bf16 / f16 rows on mfma_f32_32x32x16_*; f32 rows on
// mfma_f32_32x32x2f32 - the exact f32-input instruction, as tdnn_gemm_kernel<ET_F32>: the `f32`, `f32x` and `f32m` precision modes
// all run that instantiation (plain f32 rows in and out; a split-product form of this kernel is future work).
// The window of chunk c + 1 is not fetched under the matrix work of chunk c (one buffer): also future work.

#include <cstdlib>

#include "lds_dma.h"

namespace asv {
namespace {

constexpr int TBM = kConvTapsTileRows;                     // output rows per workgroup
constexpr int TWIN_MAX = TBM + 2 * kConvTapsMaxHalo;       // 464 window rows of 128 bytes: 59392 bytes, two workgroups per CU

template <int ET, int NF>
__global__ __launch_bounds__(256, 2) void grid_conv_taps_kernel(const ConvTapsParams p) {
  constexpr int ESIZE = ET == ET_F32 ? 4 : 2;
  constexpr int CHUNK_CH = 128 / ESIZE;                    // channels per 128-byte chunk: 32 | 64
  __shared__ __attribute__((aligned(16))) unsigned char win[TWIN_MAX * 128];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * TBM;
  const int nf0 = blockIdx.y * NF;                          // first 32-channel output fragment of this workgroup
  const int hp = p.halo_pad;                                // a multiple of 8, <= kConvTapsMaxHalo
  const int pieces = (TBM + 2 * hp) / 8;                    // 1 KiB pieces of 8 window rows
  const int row_bytes = p.cin_pad * ESIZE;                  // bytes of a row that belong to the input view
  const int chunks = (p.cin_pad + CHUNK_CH - 1) / CHUNK_CH;

  const unsigned char *xg = reinterpret_cast<const unsigned char *>(p.x);
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_byte *)win);
  const uint4 *wf = reinterpret_cast<const uint4 *>(p.w) + lane;      // fragment f at wf[f * 64]

  f32x16_t acc[NF];
#pragma unroll
  for (int n = 0; n < NF; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.0f;

  for (int c = 0; c < chunks; ++c) {
    // ---- window of this chunk: rows clamped onto the matrix (its first and last rows are gap rows: zeros), slots beyond the
    // view's channels fetched from the zero page (the weights there are zero, but 0 x garbage may be NaN)
    const int live_bytes = min(128, row_bytes - c * 128);   // a multiple of 32 (channel pitch granularity 16)
    if (c > 0) __builtin_amdgcn_s_barrier();                // every wave has read the previous chunk's window
    for (int piece = wave; piece < pieces; piece += 4) {
      const int w = piece * 8 + lane / 8;
      const int row = min(max(m0 - hp + w, 0), p.rows - 1);
      const int src_slot = lds_swz(w, lane % 8);
      const void *src = src_slot * 16 < live_bytes ? (const void *)(xg + (size_t)row * ((size_t)p.ldx * ESIZE) + (size_t)c * 128 + src_slot * 16) : p.zero16;
      glds16(src, __builtin_amdgcn_readfirstlane(lds_base + piece * 1024));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int pairs = (live_bytes + 31) / 32;               // slot pairs that hold channels: 1 .. 4
    for (int t = 0; t < p.n_taps; ++t) {
      const int wrow = hp + wave * 32 + lr + p.off[t];
      const uint4 *wt = wf + (size_t)((c * p.n_taps + t) * 4) * p.nf_total * 64;
      for (int q = 0; q < pairs; ++q) {
        const uint4 x = *reinterpret_cast<const uint4 *>(win + wrow * 128 + lds_swz(wrow, q * 2 + lh) * 16);
        uint4 wv[NF];
#pragma unroll
        for (int n = 0; n < NF; ++n) wv[n] = wt[(size_t)(q * p.nf_total + nf0 + n) * 64];
#pragma unroll
        for (int n = 0; n < NF; ++n) {
          if constexpr (ET == ET_F32) {
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wv[n].x), __uint_as_float(x.x), acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wv[n].y), __uint_as_float(x.y), acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wv[n].z), __uint_as_float(x.z), acc[n], 0, 0, 0);
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wv[n].w), __uint_as_float(x.w), acc[n], 0, 0, 0);
          } else {
            acc[n] = mfma16<ET>(wv[n], x, acc[n]);
          }
        }
      }
    }
  }

  // ---- epilogue: acc[n][r] = row m0 + wave * 32 + lr, channel (nf0 + n) * 32 + 8 * (r >> 2) + 4 * lh + (r & 3): bias, ReLU, and
  // zeros on the rows that are not valid (pad columns, gap rows), four channels per store
  const float act_lo = p.relu ? 0.0f : -INFINITY;
  const int row = m0 + wave * 32 + lr;
  const bool valid = (p.row_valid[row >> 5] >> (row & 31)) & 1u;
#pragma unroll
  for (int n = 0; n < NF; ++n)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ch = (nf0 + n) * 32 + 8 * q + 4 * lh;
      if (ch >= p.cout_store) continue;
      const float4 b4 = *reinterpret_cast<const float4 *>(p.bias + ch);
      const float b[4] = {b4.x, b4.y, b4.z, b4.w};
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = valid ? fmaxf(acc[n][q * 4 + e] + b[e], act_lo) : 0.0f;
      if constexpr (ET == ET_F32) {
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.y) + (size_t)row * p.ldy + ch) = make_float4(y[0], y[1], y[2], y[3]);
      } else {
        uint2 pk;
        pk.x = pack_h16x2<ET>(y[0], y[1]);
        pk.y = pack_h16x2<ET>(y[2], y[3]);
        *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(p.y) + (size_t)row * p.ldy + ch) = pk;
      }
    }
}

template <int ET>
int launch_et(const ConvTapsParams &p, hipStream_t s) {
  // the most fragments per workgroup (1 .. 4) that divide the layer's: every workgroup of a launch runs the same instantiation
  const int nf = p.nf_total % 4 == 0 ? 4 : (p.nf_total % 3 == 0 ? 3 : (p.nf_total % 2 == 0 ? 2 : 1));
  const dim3 grid((unsigned)(p.rows / TBM), (unsigned)(p.nf_total / nf));
  switch (nf) {
    case 4: hipLaunchKernelGGL((grid_conv_taps_kernel<ET, 4>), grid, dim3(256), 0, s, p); break;
    case 3: hipLaunchKernelGGL((grid_conv_taps_kernel<ET, 3>), grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL((grid_conv_taps_kernel<ET, 2>), grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((grid_conv_taps_kernel<ET, 1>), grid, dim3(256), 0, s, p); break;
  }
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

}  // namespace

int launch_grid_conv_taps(const ConvTapsParams &p, int et, hipStream_t s) {
  ASV_REQUIRE(p.rows % TBM == 0 && p.halo_pad % 8 == 0 && p.halo_pad >= 0 && p.halo_pad <= kConvTapsMaxHalo, "grid_conv_taps: rows %d / window halo %d", p.rows, p.halo_pad);
  ASV_REQUIRE(p.n_taps >= 1 && p.n_taps <= ASV_GRID_CONV_MAX_TAPS && p.nf_total >= 1 && p.cout_store <= p.nf_total * 32 && p.cin_pad % kChanAlign == 0, "grid_conv_taps: bad shape");
  for (int t = 0; t < p.n_taps; ++t) ASV_REQUIRE(std::abs(p.off[t]) <= p.halo_pad, "grid_conv_taps: tap offset %d beyond the window halo %d", p.off[t], p.halo_pad);
  switch (et) {
    case ET_BF16: return launch_et<ET_BF16>(p, s);
    case ET_F16: return launch_et<ET_F16>(p, s);
    default: return launch_et<ET_F32>(p, s);
  }
}

}  // namespace asv
