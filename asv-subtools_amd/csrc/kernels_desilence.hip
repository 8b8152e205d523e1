// De-silence of 16-bit PCM in HBM (asv_desilence_pcm16), in front of asv_fbank_pcm16: the waveform trimming the reference's online
// extraction applies with --de-silence true (pytorch/libs/egs/processor.py:149-175 de_sil -> signal_processing.py:13-55 de_silence).
//
// The rule, per utterance of L samples and n = win_samples: L / n full blocks and, if L % n > 0, one tail block of L % n samples; a block
// of m samples is kept iff mean(|x|) > min_eng / 32768 with x = s / 32768 - for 16-bit samples iff S > min_eng * m with the INTEGER
// S = sum |s_i| (the reference's float32 mean cannot land on the other side of the threshold while min_eng * m stays well
// below 2^24).  Kept blocks are concatenated in order; an utterance in which no block survives is kept whole (processor.py:170-171).
// |-32768| = 32768: the absolute value is taken in 32 bits.
//
// Four small launches on the caller's stream, all bandwidth (2 B read twice, <= 2 B written per sample):
//   block_sums_kernel     one wavefront per block: 16-byte loads between a scalar head and tail (a block starts at any 2-byte address: an
//                         odd-length utterance moves every later one to an odd sample), per-lane integer sums, a wavefront reduction,
//                         kept length (m or 0) per block
//   utt_scan_kernel       one workgroup per utterance: exclusive scan of its blocks' kept lengths (in chunks of 256 with a carry) = where each
//                         block goes inside the trimmed utterance; the total, or - nothing kept - every block kept again and the total L
//   offset_scan_kernel    one workgroup: exclusive scan of the utterances' totals (chunks of 256 with a carry) = out_offsets
//   compact_kernel        one wavefront per kept block: 16-byte stores aligned on the DESTINATION between a scalar head and tail; the source
//                         shares its alignment only by chance - dword loads where it is 4-byte aligned there, else dword loads one sample
//                         early and a 16-bit funnel shift.  Only [dst, dst + m) of a block is written: nothing behind out_offsets[n_utts].
// Every quantity of an utterance is a function of its own samples: its output does not depend on its batch neighbours.  Plain C++ and
// vector stores only.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "asv_internal.h"
#include "offset_ring.h"

namespace asv {
namespace {

constexpr int kScanThreads = 256;

__device__ __forceinline__ unsigned abs16(int s) { return (unsigned)(s < 0 ? -s : s); }
// |low half| + |high half| of a dword of two samples
__device__ __forceinline__ unsigned abs_pair(unsigned w) { return abs16((int)(short)(w & 0xffffu)) + abs16((int)w >> 16); }

// off: [sample_off (n_utts + 1) | block_off (n_utts + 1)]: utterance u owns blocks [block_off[u], block_off[u + 1])
__device__ __forceinline__ int utt_of_block(const long long *__restrict__ block_off, int n_utts, long long g) {
  int lo = 0, hi = n_utts - 1;                                                // the last u with block_off[u] <= g (empty utterances own no block)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void block_sums_kernel(const short *__restrict__ wave, const long long *__restrict__ off, int n_utts, long long n_blocks,
                                                         int win, double min_eng, int *__restrict__ kept_len) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_blocks) return;                                                  // (uniform over the wavefront)
  const long long *block_off = off + n_utts + 1;
  const int u = utt_of_block(block_off, n_utts, g);
  const long long j = g - block_off[u], s0 = off[u] + j * win;
  const int m = (int)min((long long)win, off[u + 1] - s0);
  const short *p = wave + s0;
  const int head = min(m, (int)(((16u - ((uintptr_t)p & 15u)) & 15u) >> 1));
  unsigned long long sum = 0;
  if (lane < head) sum += abs16(p[lane]);
  const short *body = p + head;
  const int nvec = (m - head) >> 3;
  const uint4 *bv = reinterpret_cast<const uint4 *>(body);                    // (16-byte aligned)
  for (int v = lane; v < nvec; v += 64) {
    const uint4 q = bv[v];
    sum += abs_pair(q.x) + abs_pair(q.y) + abs_pair(q.z) + abs_pair(q.w);     // <= 8 * 32768: fits 32 bits
  }
  const int tail0 = head + 8 * nvec;
  if (lane < m - tail0) sum += abs16(p[tail0 + lane]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if (lane == 0) kept_len[g] = ((double)sum > min_eng * (double)m) ? m : 0;
}

// exclusive prefix of v over the 256 threads of the workgroup (`ex`) and the sum of all 256 (returned); `wsum`: 4 shared slots
__device__ __forceinline__ long long workgroup_scan(long long v, long long *wsum, long long &ex) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanThreads / 64; ++k) {
    const long long t = wsum[k];
    if (k < wv) before += t;
    all += t;
  }
  __syncthreads();                                                            // (wsum is written again by the next chunk)
  ex = before + x - v;
  return all;
}

__global__ __launch_bounds__(kScanThreads) void utt_scan_kernel(const long long *__restrict__ off, int n_utts, int win, int *__restrict__ kept_len,
                                                               long long *__restrict__ rel, long long *__restrict__ utt_len) {
  __shared__ long long wsum[kScanThreads / 64];
  const int u = blockIdx.x;
  const long long b0 = off[n_utts + 1 + u], nb = off[n_utts + 2 + u] - b0, len = off[u + 1] - off[u];
  long long carry = 0;
  for (long long base = 0; base < nb; base += kScanThreads) {                 // (uniform trip count: the barriers inside are reached by all)
    const long long i = base + threadIdx.x;
    const long long v = i < nb ? kept_len[b0 + i] : 0;
    long long ex;
    const long long all = workgroup_scan(v, wsum, ex);
    if (i < nb) rel[b0 + i] = carry + ex;
    carry += all;
  }
  if (carry == 0) {                                                           // no block survives (or no sample at all): the utterance is kept whole
    for (long long i = threadIdx.x; i < nb; i += kScanThreads) {
      kept_len[b0 + i] = (int)min((long long)win, len - i * win);
      rel[b0 + i] = i * win;
    }
    carry = len;
  }
  if (threadIdx.x == 0) utt_len[u] = carry;
}

__global__ __launch_bounds__(kScanThreads) void offset_scan_kernel(const long long *__restrict__ utt_len, int n_utts, long long *__restrict__ out_off) {
  __shared__ long long wsum[kScanThreads / 64];
  long long carry = 0;
  for (int base = 0; base < n_utts; base += kScanThreads) {
    const int u = base + threadIdx.x;
    const long long v = u < n_utts ? utt_len[u] : 0;
    long long ex;
    const long long all = workgroup_scan(v, wsum, ex);
    if (u < n_utts) out_off[u] = carry + ex;
    carry += all;
  }
  if (threadIdx.x == 0) out_off[n_utts] = carry;
}

__global__ __launch_bounds__(256) void compact_kernel(const short *__restrict__ wave, const long long *__restrict__ off, int n_utts, long long n_blocks, int win,
                                                      const int *__restrict__ kept_len, const long long *__restrict__ rel,
                                                      const long long *__restrict__ out_off, short *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_blocks) return;
  const int m = kept_len[g];
  if (m == 0) return;
  const long long *block_off = off + n_utts + 1;
  const int u = utt_of_block(block_off, n_utts, g);
  const short *src = wave + off[u] + (g - block_off[u]) * win;
  short *dst = out + out_off[u] + rel[g];
  const int head = min(m, (int)(((16u - ((uintptr_t)dst & 15u)) & 15u) >> 1));
  if (lane < head) dst[lane] = src[lane];
  const short *sb = src + head;
  short *db = dst + head;
  const int nvec = (m - head) >> 3;
  uint4 *dv = reinterpret_cast<uint4 *>(db);                                  // (16-byte aligned)
  if (((uintptr_t)sb & 3u) == 0) {
    const unsigned *sw = reinterpret_cast<const unsigned *>(sb);              // the source is dword aligned here
    for (int v = lane; v < nvec; v += 64) {
      const unsigned *q = sw + 4 * (size_t)v;
      dv[v] = make_uint4(q[0], q[1], q[2], q[3]);
    }
  } else if (nvec > 0) {
    // the source is one sample off a dword: every aligned dword read holds at least one sample of this block (the first one's high
    // half is sample 0, the last one's low half sample 8 nvec - 1), so no load leaves the 4-byte words the block itself occupies
    const unsigned *sw = reinterpret_cast<const unsigned *>(sb - 1);
    for (int v = lane; v < nvec; v += 64) {
      const unsigned *q = sw + 4 * (size_t)v;
      const unsigned w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
      dv[v] = make_uint4((w0 >> 16) | (w1 << 16), (w1 >> 16) | (w2 << 16), (w2 >> 16) | (w3 << 16), (w3 >> 16) | (w4 << 16));
    }
  }
  const int tail0 = head + 8 * nvec;
  if (lane < m - tail0) dst[tail0 + lane] = src[tail0 + lane];
}

thread_local OffsetRing g_desilence_offs;                                      // (offset_ring.h: this entry point's own ring, per calling thread)
thread_local std::vector<long long> g_desilence_blocks;

}  // namespace
}  // namespace asv

using namespace asv;

extern "C" int asv_desilence_pcm16(const short *wave, const long long *sample_offsets, int n_utts, int win_samples, double min_eng, short *out,
                                   long long *out_offsets, void *stream) {
  ASV_REQUIRE(wave && sample_offsets && out && out_offsets, "asv_desilence_pcm16: null pointer");
  ASV_REQUIRE(n_utts >= 1, "asv_desilence_pcm16: n_utts %d", n_utts);
  ASV_REQUIRE(win_samples >= 1, "asv_desilence_pcm16: win_samples %d", win_samples);
  ASV_REQUIRE(isfinite(min_eng) && min_eng >= 0.0, "asv_desilence_pcm16: min_eng %g", min_eng);
  ASV_REQUIRE(sample_offsets[0] == 0, "asv_desilence_pcm16: sample_offsets must start at 0");
  std::vector<long long> &blocks = g_desilence_blocks;
  blocks.assign((size_t)n_utts + 1, 0);
  for (int u = 0; u < n_utts; ++u) {
    const long long len = sample_offsets[u + 1] - sample_offsets[u];
    ASV_REQUIRE(len >= 0, "asv_desilence_pcm16: sample_offsets decrease at utterance %d", u);
    blocks[(size_t)u + 1] = blocks[(size_t)u] + (len + win_samples - 1) / win_samples;
  }
  const long long total = sample_offsets[n_utts], n_blocks = blocks[(size_t)n_utts];
  const uintptr_t in_at = reinterpret_cast<uintptr_t>(wave), out_at = reinterpret_cast<uintptr_t>(out);
  ASV_REQUIRE(wave != out && (out_at + (size_t)total * 2 <= in_at || in_at + (size_t)total * 2 <= out_at),
              "asv_desilence_pcm16: out overlaps wave (in-place is not supported)");
  ASV_REQUIRE(n_blocks <= 0x7fffffffLL * 4, "asv_desilence_pcm16: %lld blocks of %d samples are too many for one launch", n_blocks, win_samples);
  if (total == 0) {                                                           // no sample: nothing is launched, nothing is written
    for (int u = 0; u <= n_utts; ++u) out_offsets[u] = 0;
    return ASV_OK;
  }
  ASV_ON_OWNER(wave, "asv_desilence_pcm16");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long *d = nullptr;
  { const int rc = g_desilence_offs.get(sample_offsets, blocks.data(), (size_t)n_utts + 1, s, &d); if (rc) return rc; }
  // scratch of the call: [rel (n_blocks) | utt_len (n_utts) | out_off (n_utts + 1) | kept_len (n_blocks, 32-bit)]
  const size_t words = (size_t)n_blocks + (size_t)n_utts + (size_t)n_utts + 1 + ((size_t)n_blocks + 1) / 2;
  long long *scratch = nullptr;
  ASV_HIP_CHECK(hipMallocAsync(reinterpret_cast<void **>(&scratch), words * 8, s));
  long long *rel = scratch, *utt_len = rel + n_blocks, *out_off = utt_len + n_utts;
  int *kept_len = reinterpret_cast<int *>(out_off + n_utts + 1);
  const unsigned waves4 = (unsigned)((n_blocks + 3) / 4);
  hipLaunchKernelGGL(block_sums_kernel, dim3(waves4), dim3(256), 0, s, wave, d, n_utts, n_blocks, win_samples, min_eng, kept_len);
  hipLaunchKernelGGL(utt_scan_kernel, dim3((unsigned)n_utts), dim3(kScanThreads), 0, s, d, n_utts, win_samples, kept_len, rel, utt_len);
  hipLaunchKernelGGL(offset_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, utt_len, n_utts, out_off);
  hipLaunchKernelGGL(compact_kernel, dim3(waves4), dim3(256), 0, s, wave, d, n_utts, n_blocks, win_samples, kept_len, rel, out_off, out);
  ASV_HIP_CHECK(hipGetLastError());
  { const int rc = g_desilence_offs.launched(s); if (rc) return rc; }
#ifdef ASV_WITH_ABLATION
  // developer build only (tools/bench_desilence.py): the launches without the copy of the offsets and the wait for it - out_offsets is NOT filled
  static const bool no_wait = getenv("ASV_AMD_DESILENCE_NOWAIT") != nullptr;
  if (no_wait) {
    ASV_HIP_CHECK(hipFreeAsync(scratch, s));
    return ASV_OK;
  }
#endif
  ASV_HIP_CHECK(hipMemcpyAsync(out_offsets, out_off, ((size_t)n_utts + 1) * 8, hipMemcpyDeviceToHost, s));
  ASV_HIP_CHECK(hipStreamSynchronize(s));                                     // the one wait of the call: the host needs the kept counts
  ASV_HIP_CHECK(hipFreeAsync(scratch, s));
  return ASV_OK;
}
