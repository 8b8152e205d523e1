// Kaldi compressed feature matrices ('CM ', 'CM2': compressed-matrix.cc, the automatic method of copy-feats --compress=true) WRITTEN on
// the MI355X (gfx950) from packed float32 rows: the mirror of kernels_decode.hip.  Features leave the device at 1 byte per value ('CM ')
// instead of 4, in the bytes that lie behind the token on disk.
//
// A body starts at the 16-byte global header {float min, float range, int32 rows, int32 cols}:
//   'CM ' (1)  cols x {uint16 p0, p25, p75, p100}, then cols x rows bytes COLUMN-major
//   'CM2' (2)  rows x cols uint16 row-major
// The quantiser is a restatement of compressed-matrix.cc (tests/compress_cases.py holds the same rule in NumPy and the tests
// compare bytes): sequential float32, every operation rounded on its own (-ffp-contract=off, and the pragma below), correctly rounded
// divisions, float -> int conversions that truncate (and give INT_MIN for a NaN or a value outside int32, as cvttss2si does: what NumPy's
// astype gives on the host, so that the two agree on degenerate input too).
//
// Three launches on the caller's stream, 2 + 4 reads of the input in all (6 x 4 B in, 1 B out per value):
//   1. encode_minmax_kernel   min / max of every utterance as order-preserving uint32 keys, merged with INTEGER atomicMax into a per-call
//                             scratch {~min key, max key, non-finite flag}; no float atomics, the result does not depend on the order.
//   2. encode_select_kernel   one workgroup per (utterance, 32 columns): writes the global header and the status word, and for 'CM ' the
//                             exact order statistics s[n/4], s[3 (n/4)] of each column by a radix select on the keys - four passes of
//                             8 bits with per-column LDS histograms [rank][bin][column] (64 KiB) -, s[0] and s[n-1] as the column's min / max
//                             in the first pass.  Lanes run across columns (two rows of 32 columns per wave: 128-byte row segments), so
//                             the row-major reads coalesce and every lane's LDS atomic goes to its own bank.  Any row count an int32
//                             holds: nothing depends on a column fitting in LDS.
//   3. encode_compressed_kernel  a transposing write, the decode kernel backwards: a tile of 64 frames x 64 columns, wave = 16 frames, lane =
//                             column reads the rows and quantises; the bytes go through an LDS tile of 64 x 65 dwords (odd stride); then wave
//                             = 16 columns, lane = frame stores 64 consecutive bytes of one column per instruction.  A column starts at
//                             16 + 8 cols + c rows, any residue mod 4: byte stores throughout, nothing outside the body is ever touched.
//                             'CM2' is row-major: the same grid streams it, lane = column.

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "asv_internal.h"
#include "offset_ring.h"

#pragma clang fp contract(off)

namespace asv {
namespace {

constexpr int kEncodeTile = 64;               // frames and columns per tile of the transposing write
constexpr int kEncodeStride = kEncodeTile + 1;
constexpr int kSelectCols = 32;               // columns per workgroup of the select kernel
constexpr int kSelectSlots = 256 / kSelectCols;   // rows a workgroup reads per step
constexpr int kScratchWords = 4;              // per utterance: ~min key, max key, non-finite flag, (pad)

// float -> uint32 whose unsigned order is the floats' order (-0.0 in front of +0.0), and back
__device__ __forceinline__ unsigned to_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_key(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// (int)x, truncating; INT_MIN for a NaN and for anything outside int32
__device__ __forceinline__ int trunc_i32(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN; }

// one percentile of a column header as the reader sees it (kernels_decode.hip decode_percentile)
__device__ __forceinline__ float percentile_value(int q, float gmin, float grange) {
  return __fadd_rn(__fmul_rn(__fmul_rn((float)q, grange), 1.52590218966964e-05f), gmin);
}

// (int)(clamp((v - min) / range, 0, 1) * 65535 + 0.499f)
__device__ __forceinline__ int quant16(float v, float gmin, float grange) {
  float f = __fdiv_rn(__fsub_rn(v, gmin), grange);
  if (f > 1.0f) f = 1.0f;
  if (f < 0.0f) f = 0.0f;
  return trunc_i32(__fadd_rn(__fmul_rn(f, 65535.0f), 0.499f));
}
__device__ __forceinline__ unsigned short as_u16(int q) { return (unsigned short)min(max(q, 0), 65535); }

__device__ __forceinline__ int segment_code(float v, float lo, float width, float codes, int top) {
  const int i = trunc_i32(__fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(v, lo), width), codes), 0.5f));
  return min(max(i, 0), top);
}

__device__ __forceinline__ void header_of(const unsigned *scr, int u, float *gmin, float *grange) {
  const float mn = from_key(~scr[kScratchWords * (size_t)u]);
  float mx = from_key(scr[kScratchWords * (size_t)u + 1]);
  if (mx == mn) mx = __fadd_rn(mn, __fadd_rn(1.0f, fabsf(mn)));
  *gmin = mn;
  *grange = __fsub_rn(mx, mn);
}

// off: [frame_off (n_utts + 1) | body (n_utts + 1)], body[u] = byte offset of utterance u's body (a multiple of 16) | format
__global__ __launch_bounds__(256) void encode_minmax_kernel(const float *__restrict__ x, const long long *__restrict__ off, int dim, int rows_per_block,
                                                            unsigned *__restrict__ scr) {
  __shared__ unsigned red[3][4];
  const int u = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long f0 = off[u], n = off[u + 1] - f0;
  const long long t0 = (long long)blockIdx.y * rows_per_block;
  if (t0 >= n) return;                                                       // (uniform over the workgroup: before any barrier)
  const long long t1 = min(t0 + (long long)rows_per_block, n);
  const float *p = x + (size_t)(f0 + t0) * dim;                              // rows t0 .. t1 of an utterance are one run of floats
  const size_t count = (size_t)(t1 - t0) * dim;
  unsigned kmin = 0xffffffffu, kmax = 0u, bad = 0u;
#pragma unroll 4
  for (size_t i = threadIdx.x; i < count; i += 256) {
    const float v = p[i];
    const unsigned k = to_key(v);
    bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    kmin = min(kmin, k);
    kmax = max(kmax, k);
  }
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
    bad |= (unsigned)__shfl_xor((int)bad, o);
  }
  if (lane == 0) { red[0][wave] = kmin; red[1][wave] = kmax; red[2][wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { kmin = min(kmin, red[0][w]); kmax = max(kmax, red[1][w]); bad |= red[2][w]; }
    unsigned *s = scr + kScratchWords * (size_t)u;
    atomicMax(s, ~kmin);
    atomicMax(s + 1, kmax);
    if (bad) atomicOr(s + 2, 1u);
  }
}

// the chain of compressed-matrix.cc over the (up to) four order statistics of a column: strictly increasing uint16
__device__ __forceinline__ void write_percentiles(unsigned short *h, int have, float s0, float s1, float s2, float s3, float gmin, float grange) {
  const int p0 = min(quant16(s0, gmin, grange), 65532);
  const int p25 = have > 1 ? min(max(quant16(s1, gmin, grange), p0 + 1), 65533) : p0 + 1;
  const int p75 = have > 2 ? min(max(quant16(s2, gmin, grange), p25 + 1), 65534) : p25 + 1;
  const int p100 = have > 3 ? max(quant16(s3, gmin, grange), p75 + 1) : p75 + 1;
  h[0] = as_u16(p0);
  h[1] = as_u16(p25);
  h[2] = as_u16(p75);
  h[3] = as_u16(p100);
}

__global__ __launch_bounds__(256) void encode_select_kernel(const float *__restrict__ x, const long long *__restrict__ off, int n_utts, int dim,
                                                            const unsigned *__restrict__ scr, unsigned char *__restrict__ bytes, int *__restrict__ status) {
  __shared__ __align__(16) unsigned hist[2 * 256 * kSelectCols];             // [rank][bin][column]
  __shared__ unsigned part[4][2 * kSelectCols];                              // counts of a quarter of the bins, per (rank, column)
  __shared__ unsigned prefix[2 * kSelectCols], want[2 * kSelectCols];        // the digits found so far / the rank that is left, per (rank, column)
  __shared__ unsigned cmin[kSelectSlots][kSelectCols], cmax[kSelectSlots][kSelectCols];
  const int u = blockIdx.x, tid = threadIdx.x, col = tid & (kSelectCols - 1), slot = tid / kSelectCols;
  const long long f0 = off[u];
  const int n = (int)(off[u + 1] - f0);
  const long long packed = off[n_utts + 1 + u];
  const int format = (int)(packed & 15);
  unsigned char *body = bytes + (packed & ~15ll);
  float gmin, grange;
  header_of(scr, u, &gmin, &grange);
  if (blockIdx.y == 0 && tid == 0) {
    reinterpret_cast<float *>(body)[0] = gmin;                               // (16-byte aligned)
    reinterpret_cast<float *>(body)[1] = grange;
    reinterpret_cast<int *>(body)[2] = n;
    reinterpret_cast<int *>(body)[3] = dim;
    status[u] = scr[kScratchWords * (size_t)u + 2] ? 1 : 0;
  }
  if (format != 1) return;                                                   // (uniform)
  const int c = blockIdx.y * kSelectCols + col;
  const float *xc = x + (size_t)f0 * dim + c;
  unsigned short *h = reinterpret_cast<unsigned short *>(body + 16) + 4 * (size_t)c;
  if (n < 5) {                                                               // the whole column, sorted in registers
    if (slot == 0 && c < dim) {
      float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int t = 0; t < n; ++t) {
        float v = xc[(size_t)t * dim];
        int i = t;
        while (i > 0 && to_key(s[i - 1]) > to_key(v)) { s[i] = s[i - 1]; --i; }
        s[i] = v;
      }
      write_percentiles(h, n, s[0], s[1], s[2], s[3], gmin, grange);
    }
    return;
  }
  const int pair = tid & (2 * kSelectCols - 1), quarter = tid / (2 * kSelectCols);      // the scan's work split: (rank, column) x 64 bins
  if (tid < 2 * kSelectCols) {
    prefix[tid] = 0u;
    want[tid] = tid < kSelectCols ? (unsigned)(n / 4) : (unsigned)(3 * (n / 4));
  }
  unsigned kmin = 0xffffffffu, kmax = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < (pass == 0 ? 1 : 2) * 64 * kSelectCols; i += 256) reinterpret_cast<uint4 *>(hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (c < dim) {
      if (pass == 0) {                                                       // both ranks read the one histogram of the top digits
#pragma unroll 8
        for (int t = slot; t < n; t += kSelectSlots) {
          const unsigned k = to_key(xc[(size_t)t * dim]);
          kmin = min(kmin, k);
          kmax = max(kmax, k);
          atomicAdd(&hist[(k >> 24) * kSelectCols + col], 1u);
        }
      } else {
        const unsigned pre0 = prefix[col], pre1 = prefix[kSelectCols + col];
#pragma unroll 8
        for (int t = slot; t < n; t += kSelectSlots) {
          const unsigned k = to_key(xc[(size_t)t * dim]);
          const unsigned top = k >> (shift + 8), bin = (k >> shift) & 255u;
          if (top == pre0) atomicAdd(&hist[bin * kSelectCols + col], 1u);
          if (top == pre1) atomicAdd(&hist[(256 + bin) * kSelectCols + col], 1u);
        }
      }
    }
    __syncthreads();
    // the bin that holds rank want[pair]: four threads per (rank, column), 64 bins each
    const unsigned *hp = hist + ((pass == 0 ? 0 : (pair / kSelectCols) * 256) + quarter * 64) * kSelectCols + (pair & (kSelectCols - 1));
    unsigned cnt[64], sum = 0u;                                                // (in registers: the search below does not wait for LDS bin by bin)
#pragma unroll
    for (int b = 0; b < 64; ++b) cnt[b] = hp[b * kSelectCols];
#pragma unroll
    for (int b = 0; b < 64; ++b) sum += cnt[b];
    part[quarter][pair] = sum;
    const unsigned k_left = want[pair], pre = prefix[pair];
    __syncthreads();
    unsigned before = 0u;
    for (int q = 0; q < quarter; ++q) before += part[q][pair];
    if (k_left >= before && k_left < before + sum) {
      unsigned cum = before;
      int b = 63;
      bool found = false;
#pragma unroll
      for (int i = 0; i < 63; ++i) {
        if (!found && k_left < cum + cnt[i]) { b = i; found = true; }
        if (!found) cum += cnt[i];
      }
      prefix[pair] = (pre << 8) | (unsigned)(quarter * 64 + b);
      want[pair] = k_left - cum;
    }
    __syncthreads();
  }
  cmin[slot][col] = kmin;
  cmax[slot][col] = kmax;
  __syncthreads();
  if (slot == 0 && c < dim) {
    for (int s = 1; s < kSelectSlots; ++s) { kmin = min(kmin, cmin[s][col]); kmax = max(kmax, cmax[s][col]); }
    write_percentiles(h, 4, from_key(kmin), from_key(prefix[col]), from_key(prefix[kSelectCols + col]), from_key(kmax), gmin, grange);
  }
}

__global__ __launch_bounds__(256) void encode_compressed_kernel(const float *__restrict__ x, const long long *__restrict__ off, int n_utts, int dim,
                                                                unsigned char *__restrict__ bytes) {
  __shared__ unsigned tile[kEncodeTile * kEncodeStride];                     // [column][frame]: the byte values of a 'CM ' tile
  const int u = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long f0 = off[u];
  const int n = (int)(off[u + 1] - f0);
  const long long packed = off[n_utts + 1 + u];
  const int format = (int)(packed & 15);
  unsigned char *body = bytes + (packed & ~15ll);
  const float gmin = reinterpret_cast<const float *>(body)[0], grange = reinterpret_cast<const float *>(body)[1];     // (the select kernel wrote them)
  const int c0 = blockIdx.z * kEncodeTile, c = c0 + lane;
  const float *xc = x + (size_t)f0 * dim + c;
  const long long t_step = (long long)kEncodeTile * gridDim.y;
  if (format != 1) {
    // row-major uint16: wave = 16 frames, lane = column
    if (c >= dim) return;
    unsigned short *q = reinterpret_cast<unsigned short *>(body + 16) + c;   // (body + 16: 2-byte aligned)
    for (long long t0 = (long long)blockIdx.y * kEncodeTile; t0 < n; t0 += t_step) {
      const long long ta = t0 + wave * 16, tb = min(ta + 16, (long long)n);
#pragma unroll 4
      for (long long t = ta; t < tb; ++t) q[(size_t)t * dim] = as_u16(quant16(xc[(size_t)t * dim], gmin, grange));
    }
    return;
  }
  float p0 = 0.0f, p25 = 0.0f, p75 = 0.0f, w0 = 1.0f, w1 = 1.0f, w2 = 1.0f;
  if (c < dim) {
    const unsigned short *h = reinterpret_cast<const unsigned short *>(body + 16) + 4 * (size_t)c;
    p0 = percentile_value(h[0], gmin, grange);
    p25 = percentile_value(h[1], gmin, grange);
    p75 = percentile_value(h[2], gmin, grange);
    const float p100 = percentile_value(h[3], gmin, grange);
    w0 = __fsub_rn(p25, p0);
    w1 = __fsub_rn(p75, p25);
    w2 = __fsub_rn(p100, p75);
  }
  unsigned char *data = body + 16 + 8 * (size_t)dim;
  for (long long t0 = (long long)blockIdx.y * kEncodeTile; t0 < n; t0 += t_step) {       // (uniform over the workgroup)
    // rows in: wave = 16 frames, lane = column
    if (c < dim) {
      const int ra = wave * 16, rb = (int)min((long long)ra + 16, n - t0);
#pragma unroll 4
      for (int r = ra; r < rb; ++r) {
        const float v = xc[(size_t)(t0 + r) * dim];
        int code;
        if (v < p25) code = segment_code(v, p0, w0, 64.0f, 64);
        else if (v < p75) code = 64 + segment_code(v, p25, w1, 128.0f, 128);
        else code = 192 + segment_code(v, p75, w2, 63.0f, 63);
        tile[lane * kEncodeStride + r] = (unsigned)code;
      }
    }
    __syncthreads();
    // bytes out: wave = 16 columns, lane = frame - 64 consecutive bytes of one column per store
    const long long t = t0 + lane;
    if (t < n) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int cc = c0 + wave * 16 + j;
        if (cc < dim) data[(size_t)cc * n + t] = (unsigned char)tile[(wave * 16 + j) * kEncodeStride + lane];
      }
    }
    __syncthreads();
  }
}

thread_local OffsetRing g_encode_offs;                                        // (offset_ring.h: this entry point's own ring, per calling thread)
thread_local std::vector<long long> g_encode_packed;

}  // namespace
}  // namespace asv

using namespace asv;

extern "C" int asv_encode_compressed(const float *feats, const long long *frame_offsets, const long long *byte_offsets, const unsigned char *formats, int n_utts,
                                     int dim, unsigned char *bytes, int *status, void *stream) {
  ASV_REQUIRE(feats && frame_offsets && byte_offsets && formats && bytes && status, "asv_encode_compressed: null pointer");
  ASV_REQUIRE(n_utts >= 1, "asv_encode_compressed: n_utts %d", n_utts);
  ASV_REQUIRE(dim >= 1, "asv_encode_compressed: dim %d", dim);
  ASV_REQUIRE(frame_offsets[0] == 0, "asv_encode_compressed: frame_offsets must start at 0");
  long long longest = 0, end = 0;
  std::vector<long long> &packed = g_encode_packed;
  packed.assign((size_t)n_utts + 1, 0);
  for (int u = 0; u < n_utts; ++u) {
    const long long frames = frame_offsets[u + 1] - frame_offsets[u], at = byte_offsets[u];
    const int format = formats[u];
    ASV_REQUIRE(frames >= 1, "asv_encode_compressed: frame_offsets do not increase at utterance %d (an empty matrix has no compressed form)", u);
    ASV_REQUIRE(frames <= INT_MAX, "asv_encode_compressed: utterance %d has %lld rows", u, frames);
    ASV_REQUIRE(format == 1 || format == 2, "asv_encode_compressed: utterance %d has format %d (1 = 'CM ', 2 = 'CM2'; 'CM3' is never written)", u, format);
    ASV_REQUIRE(at >= 0 && at % 16 == 0, "asv_encode_compressed: byte_offsets[%d] = %lld is not a multiple of 16", u, at);
    ASV_REQUIRE(at >= end, "asv_encode_compressed: the body of utterance %d starts at byte %lld, inside the one before it (ends at %lld)", u, at, end);
    end = at + 16 + (format == 1 ? 8ll * dim + frames * dim : 2 * frames * dim);
    packed[u] = at | format;
    longest = std::max(longest, frames);
  }
  ASV_REQUIRE((dim + kSelectCols - 1) / kSelectCols <= 65535, "asv_encode_compressed: dim %d too large", dim);
  ASV_ON_OWNER(bytes, "asv_encode_compressed");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long *d = nullptr;
  { const int rc = g_encode_offs.get(frame_offsets, packed.data(), (size_t)n_utts + 1, s, &d); if (rc) return rc; }
  // per-utterance {~min key, max key, non-finite flag}: stream-ordered scratch, zeroed (both keys merge with atomicMax)
  unsigned *scr = nullptr;
  const size_t scr_bytes = (size_t)n_utts * kScratchWords * sizeof(unsigned);
  ASV_HIP_CHECK(hipMallocAsync(reinterpret_cast<void **>(&scr), scr_bytes, s));
  ASV_HIP_CHECK(hipMemsetAsync(scr, 0, scr_bytes, s));
  const int rows_per_block = (int)std::max<long long>(64, (longest + 65534) / 65535);
  hipLaunchKernelGGL(encode_minmax_kernel, dim3((unsigned)n_utts, (unsigned)((longest + rows_per_block - 1) / rows_per_block)), dim3(256), 0, s, feats, d, dim,
                     rows_per_block, scr);
  hipLaunchKernelGGL(encode_select_kernel, dim3((unsigned)n_utts, (unsigned)((dim + kSelectCols - 1) / kSelectCols)), dim3(256), 0, s, feats, d, n_utts, dim, scr,
                     bytes, status);
  const long long tiles = (longest + kEncodeTile - 1) / kEncodeTile;
  hipLaunchKernelGGL(encode_compressed_kernel, dim3((unsigned)n_utts, (unsigned)std::min<long long>(tiles, 65535), (unsigned)((dim + kEncodeTile - 1) / kEncodeTile)),
                     dim3(256), 0, s, feats, d, n_utts, dim, bytes);
  ASV_HIP_CHECK(hipGetLastError());
  ASV_HIP_CHECK(hipFreeAsync(scr, s));
  return g_encode_offs.launched(s);
}
