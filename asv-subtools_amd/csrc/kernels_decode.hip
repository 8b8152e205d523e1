// Kaldi compressed feature matrices ('CM ', 'CM2', 'CM3': compressed-matrix.cc; what make_fbank.sh / make_mfcc.sh write with their
// default compress=true) decoded on the MI355X (gfx950) into the packed float32 rows asv_ingest_frames and the engine read.  The host
// reads the bodies as they lie on disk - 1 byte per value ('CM ', 'CM3') or 2 ('CM2') instead of 4 - and this kernel runs on the stream
// in front of whatever consumes the rows.
//
// A body starts at the 16-byte global header {float min, float range, int32 rows, int32 cols}:
//   'CM ' (1)  cols x {uint16 p0, p25, p75, p100}, then cols x rows bytes COLUMN-major
//   'CM2' (2)  rows x cols uint16 row-major
//   'CM3' (3)  rows x cols uint8 row-major
// min and range are read from the body; rows and cols come from the caller's offsets and dim alone - the header's counts never address
// anything (libs.amd.frontend.decode_compressed compares them with the header before the bytes are copied).
//
// Arithmetic: that of libs/support/kaldi_io._read_compressed_mat (pinned to the reference's reader by fixtures), operation for
// operation in float32 - every multiply, add, subtract and divide rounded on its own.  hipcc contracts a * b + c into an FMA in device
// code by default, which changes 54 % of the decoded values in their last bit; this unit is therefore built with -ffp-contract=off
// (Makefile) and says so again below, and the divisions are correctly rounded ones (a multiplication by a rounded 1 / 63 changes 6.6 %).
//
// 'CM ' is a transposing decode.  One workgroup = one tile of 64 frames x 64 columns of one utterance: a wave reads 16 columns, lane =
// frame (64 consecutive bytes of a column per load; a column starts at 16 + 8 cols + c rows, any residue mod 4: byte loads), the bytes
// go through an LDS tile of 64 x 65 dwords (odd stride: the column-wise write and the row-wise read are both free of bank conflicts),
// then a wave writes 16 frames, lane = column: row segments of 4 * min(dim, 64) contiguous bytes, as ingest_frames_kernel writes them.
// A column's percentiles and slopes are computed once per tile (the first wave, through LDS) and sit in registers while the rows are
// written.  'CM2' / 'CM3' are row-major: the same grid streams them, lane = column, without the tile.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "asv_internal.h"
#include "offset_ring.h"

#pragma clang fp contract(off)

namespace asv {
namespace {

constexpr int kDecodeTile = 64;             // frames and columns per workgroup
constexpr int kDecodeStride = kDecodeTile + 1;

// one percentile of a column header: ((float(u16) * range) * (1 / 65535 rounded to float)) + min
__device__ __forceinline__ float decode_percentile(unsigned short q, float gmin, float grange) {
  return __fadd_rn(__fmul_rn(__fmul_rn((float)q, grange), 1.52590218966964e-05f), gmin);
}

// off: [frame_off (n_utts + 1) | body (n_utts + 1)], body[u] = byte offset of utterance u's body in `bytes` (a multiple of 16) | format.
__global__ __launch_bounds__(256) void decode_compressed_kernel(const unsigned char *__restrict__ bytes, const long long *__restrict__ off, int n_utts, int dim,
                                                                float *__restrict__ out) {
  __shared__ unsigned tile[kDecodeTile * kDecodeStride];                     // [column][frame]: the byte values of a 'CM ' tile
  __shared__ float head[6][kDecodeTile];                                     // p0, p25, p75 and the three slopes of the tile's columns
  const int u = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long f0 = off[u];
  const int n = (int)(off[u + 1] - f0);
  const int t0 = blockIdx.y * kDecodeTile, c0 = blockIdx.z * kDecodeTile;
  if (t0 >= n) return;                                                       // (uniform over the workgroup: before any barrier)
  const long long packed = off[n_utts + 1 + u];
  const int format = (int)(packed & 15);
  const unsigned char *body = bytes + (packed & ~15ll);
  const float gmin = reinterpret_cast<const float *>(body)[0], grange = reinterpret_cast<const float *>(body)[1];     // (16-byte aligned)
  const int c = c0 + lane;
  float *y = out + (size_t)f0 * dim + c;
  if (format != 1) {
    // row-major: wave = 16 frames, lane = column
    if (c >= dim) return;
    const float inc = format == 2 ? (float)((double)grange * (1.0 / 65535.0)) : (float)((double)grange * (1.0 / 255.0));
    const int ta = t0 + wave * 16, tb = min(ta + 16, n);
    if (format == 2) {
      const unsigned short *q = reinterpret_cast<const unsigned short *>(body + 16) + c;      // (body + 16: 2-byte aligned)
#pragma unroll 4
      for (int t = ta; t < tb; ++t) y[(size_t)t * dim] = __fadd_rn(gmin, __fmul_rn((float)q[(size_t)t * dim], inc));
    } else {
      const unsigned char *q = body + 16 + c;
#pragma unroll 4
      for (int t = ta; t < tb; ++t) y[(size_t)t * dim] = __fadd_rn(gmin, __fmul_rn((float)q[(size_t)t * dim], inc));
    }
    return;
  }
  // 'CM ': the column headers of the tile, once
  if (wave == 0 && c < dim) {
    const unsigned short *h = reinterpret_cast<const unsigned short *>(body + 16) + 4 * (size_t)c;
    const float p0 = decode_percentile(h[0], gmin, grange), p25 = decode_percentile(h[1], gmin, grange), p75 = decode_percentile(h[2], gmin, grange),
                p100 = decode_percentile(h[3], gmin, grange);
    head[0][lane] = p0;
    head[1][lane] = p25;
    head[2][lane] = p75;
    head[3][lane] = __fdiv_rn(__fsub_rn(p25, p0), 64.0f);
    head[4][lane] = __fdiv_rn(__fsub_rn(p75, p25), 128.0f);
    head[5][lane] = __fdiv_rn(__fsub_rn(p100, p75), 63.0f);
  }
  // bytes in: wave = 16 columns, lane = frame - all loads of a wave issued before the first is stored
  {
    const int t = t0 + lane;
    const unsigned char *data = body + 16 + 8 * (size_t)dim;
    unsigned char d[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int cc = c0 + wave * 16 + j;
      d[j] = (t < n && cc < dim) ? data[(size_t)cc * n + t] : (unsigned char)0;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) tile[(wave * 16 + j) * kDecodeStride + lane] = d[j];
  }
  __syncthreads();
  if (c >= dim) return;
  const float p0 = head[0][lane], p25 = head[1][lane], p75 = head[2][lane], s0 = head[3][lane], s1 = head[4][lane], s2 = head[5][lane];
  const int ta = wave * 16, tb = min(ta + 16, n - t0);
#pragma unroll 4
  for (int r = ta; r < tb; ++r) {
    const unsigned d = tile[lane * kDecodeStride + r];
    float v;
    if (d <= 64u) v = __fadd_rn(p0, __fmul_rn(s0, (float)d));
    else if (d > 192u) v = __fadd_rn(p75, __fmul_rn(s2, (float)(d - 192u)));
    else v = __fadd_rn(p25, __fmul_rn(s1, (float)(d - 64u)));
    y[(size_t)(t0 + r) * dim] = v;
  }
}

thread_local OffsetRing g_decode_offs;                                        // (offset_ring.h: this entry point's own ring, per calling thread)
thread_local std::vector<long long> g_decode_packed;

}  // namespace
}  // namespace asv

using namespace asv;

extern "C" int asv_decode_compressed(const unsigned char *bytes, const long long *byte_offsets, const long long *frame_offsets, const unsigned char *formats,
                                     int n_utts, int dim, float *out, void *stream) {
  ASV_REQUIRE(bytes && byte_offsets && frame_offsets && formats && out, "asv_decode_compressed: null pointer");
  ASV_REQUIRE(n_utts >= 1, "asv_decode_compressed: n_utts %d", n_utts);
  ASV_REQUIRE(dim >= 1, "asv_decode_compressed: dim %d", dim);
  ASV_REQUIRE(frame_offsets[0] == 0, "asv_decode_compressed: frame_offsets must start at 0");
  long long longest = 0, end = 0;
  std::vector<long long> &packed = g_decode_packed;
  packed.assign((size_t)n_utts + 1, 0);
  for (int u = 0; u < n_utts; ++u) {
    const long long frames = frame_offsets[u + 1] - frame_offsets[u], at = byte_offsets[u];
    const int format = formats[u];
    ASV_REQUIRE(frames >= 0, "asv_decode_compressed: frame_offsets decrease at utterance %d", u);
    ASV_REQUIRE(format >= 1 && format <= 3, "asv_decode_compressed: utterance %d has format %d (1 = 'CM ', 2 = 'CM2', 3 = 'CM3')", u, format);
    ASV_REQUIRE(at >= 0 && at % 16 == 0, "asv_decode_compressed: byte_offsets[%d] = %lld is not a multiple of 16", u, at);
    ASV_REQUIRE(at >= end, "asv_decode_compressed: the body of utterance %d starts at byte %lld, inside the one before it (ends at %lld)", u, at, end);
    end = at + 16 + (format == 1 ? 8ll * dim + frames * dim : format == 2 ? 2 * frames * dim : frames * dim);
    packed[u] = at | format;
    longest = std::max(longest, frames);
  }
  if (frame_offsets[n_utts] == 0) return ASV_OK;                             // no rows: nothing is written
  const long long blocks_y = (longest + kDecodeTile - 1) / kDecodeTile;
  ASV_REQUIRE(blocks_y <= 65535 && (dim + kDecodeTile - 1) / kDecodeTile <= 65535, "asv_decode_compressed: utterance of %lld frames / dim %d too large", longest,
              dim);
  ASV_ON_OWNER(out, "asv_decode_compressed");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long *d = nullptr;
  { const int rc = g_decode_offs.get(frame_offsets, packed.data(), (size_t)n_utts + 1, s, &d); if (rc) return rc; }
  hipLaunchKernelGGL(decode_compressed_kernel, dim3((unsigned)n_utts, (unsigned)blocks_y, (unsigned)((dim + kDecodeTile - 1) / kDecodeTile)), dim3(256), 0, s,
                     bytes, d, n_utts, dim, out);
  ASV_HIP_CHECK(hipGetLastError());
  return g_decode_offs.launched(s);
}
