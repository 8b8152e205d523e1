// Fused ingest of raw Kaldi features on the MI355X (gfx950): sliding-window mean (/ variance) normalisation AND voiced-frame
// selection in ONE pass - the `apply-cmvn-sliding ... | select-voiced-frames ...` pipe the reference puts in front of its extractor
// (pytorch/pipeline/extract_xvectors_for_pytorch.sh:105-118), in that order: every raw frame is normalised over its window of RAW
// frames, then only the voiced ones are kept.
//
//     out[out_off[u] + rank_u(t)] = x[t] - mean(window_u(t))      (/ sqrt(max(var, 1e-10)) with norm_vars)      for voiced t
//
// asv_cmvn_sliding -> asv_select_frames (frontend.hip) compute the same in three launches: the normalised copy of the whole batch goes
// to HBM and is read back, and a source-row index of every kept row goes through HBM too.  Here a raw element is read once per window
// pass, only kept rows are written, and the rank of a frame is a ballot + popcount over the flag bytes.
//
// One wave per (utterance, segment of 32 frames, block of 64 columns); lane = column, so the 64 lanes read / write one row segment
// of 4 * min(dim, 64) contiguous bytes.  The window rule and the accumulation order are those of cmvn_sliding_kernel (segments from
// the utterance start, the first window summed directly in ascending order, then slide; f64 sums): without flags the output equals
// asv_cmvn_sliding's bit for bit, whichever entry point prepared the features.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "asv_internal.h"
#include "offset_ring.h"

namespace asv {
namespace {

// Kaldi's SlidingWindowCmnInternal window of frame t (feat/feature-functions.cc): the rule of cmn_window_of in frontend.hip.
__device__ __forceinline__ void ingest_window_of(int t, int n, int window, int min_window, int center, int *ws, int *we) {
  int a, b;
  if (center) { a = t - window / 2; b = a + window; } else { a = t - window; b = t + 1; }
  if (a < 0) { b -= a; a = 0; }
  if (!center && b > t) b = max(t + 1, min_window);
  if (b > n) { a -= b - n; b = n; if (a < 0) a = 0; }
  *ws = a; *we = b;
}

constexpr int kIngestSeg = 32;              // frames per wave: cmvn_sliding_kernel's kSlideSeg (part of the bit-for-bit contract)
constexpr int kIngestSegsPerBlock = 4;      // waves per workgroup
constexpr int kIngestAhead = 16;            // loads of the first window issued together

// The rows of ONE segment of one utterance, one column per lane: frames [t0, t1) of the n frames at x (the utterance's first frame, this
// lane's column) -> rows `row`, `row` + 1, ... of y (this lane's column of `out`) for the frames whose bit of `keep` is set; a row at or
// beyond o1 is never written.  Shared by ingest_frames_kernel and ingest_windows_kernel: one body, so both write the same bits for the
// same frames (the window rule, the ascending f64 summation of the first window, the slide order).
__device__ __forceinline__ void ingest_segment_rows(const float *__restrict__ x, float *__restrict__ y, int n, int t0, int t1, unsigned keep, long long row,
                                                    long long o1, int dim, int window, int min_window, int center, int norm_vars) {
  if (window <= 0) {
    for (int t = t0; t < t1; ++t)
      if ((keep >> (t - t0)) & 1u) {
        if (row < o1) y[(size_t)row * dim] = x[(size_t)t * dim];            // (row >= o1: the flags hold more than the caller counted - never written)
        ++row;
      }
    return;
  }
  int ws, we;
  ingest_window_of(t0, n, window, min_window, center, &ws, &we);
  double sum = 0.0, sumsq = 0.0;
  // the first window, summed in ascending order - kIngestAhead independent loads in flight, the additions in the same order as one by one
  int k = ws;
  for (; k + kIngestAhead <= we; k += kIngestAhead) {
    float ahead[kIngestAhead];
#pragma unroll
    for (int j = 0; j < kIngestAhead; ++j) ahead[j] = x[(size_t)(k + j) * dim];
#pragma unroll
    for (int j = 0; j < kIngestAhead; ++j) { const double v = ahead[j]; sum += v; sumsq += v * v; }
  }
  for (; k < we; ++k) { const double v = x[(size_t)k * dim]; sum += v; sumsq += v * v; }
  for (int t = t0; t < t1; ++t) {
    int a, b;
    ingest_window_of(t, n, window, min_window, center, &a, &b);
    // a window moves by at most one frame per step at either end: the (up to) three loads of a step are issued together, the
    // arithmetic keeps its order - removals, then additions
    const bool drop = ws < a, take = we < b;
    const float x_drop = drop ? x[(size_t)ws * dim] : 0.0f, x_take = take ? x[(size_t)we * dim] : 0.0f, x_t = x[(size_t)t * dim];
    if (drop) { const double v = x_drop; sum -= v; sumsq -= v * v; ++ws; }
    while (ws < a) { const double v = x[(size_t)ws * dim]; sum -= v; sumsq -= v * v; ++ws; }
    if (take) { const double v = x_take; sum += v; sumsq += v * v; ++we; }
    while (we < b) { const double v = x[(size_t)we * dim]; sum += v; sumsq += v * v; ++we; }
    if (!((keep >> (t - t0)) & 1u)) continue;                                 // the sums slide over unvoiced frames too
    const double frames = (double)(we - ws);
    double v = (double)x_t - sum / frames;
    if (norm_vars) {
      if (we - ws == 1) v = 0.0;
      else {
        double var = sumsq / frames - (sum / frames) * (sum / frames);
        var = fmax(var, 1.0e-10);
        v *= 1.0 / sqrt(var);
      }
    }
    if (row < o1) y[(size_t)row * dim] = (float)v;
    ++row;
  }
}

// off: [frame_off (n_utts + 1) | out_off (n_utts + 1)].  voiced: one byte per raw frame, or nullptr (every frame is kept).
// window <= 0: selection only (rows are copied as they are).
__global__ __launch_bounds__(256) void ingest_frames_kernel(const float *__restrict__ in, const unsigned char *__restrict__ voiced, float *__restrict__ out,
                                                            const long long *__restrict__ off, int n_utts, int dim, int window, int min_window,
                                                            int center, int norm_vars) {
  const int u = blockIdx.x, lane = threadIdx.x & 63, c = blockIdx.z * 64 + lane;
  const long long f0 = off[u];
  const int n = (int)(off[u + 1] - f0);
  const int seg = blockIdx.y * kIngestSegsPerBlock + (threadIdx.x >> 6);
  const int t0 = seg * kIngestSeg;
  if (t0 >= n) return;                                                       // (wave-uniform: a wave is one segment)
  const long long o0 = off[n_utts + 1 + u], o1 = off[n_utts + 2 + u];         // this utterance's rows of `out`
  // which frames of the segment are kept, and how many voiced frames of the utterance lie in front of it
  unsigned keep = 0xffffffffu;
  long long row = o0 + t0;
  if (voiced) {
    // (all flag bytes of a step are loaded before the first ballot waits for one: a wave's time here is load latency)
    const unsigned char *flag = voiced + f0;
    const unsigned char mine = lane < kIngestSeg && t0 + lane < n ? flag[t0 + lane] : 0;
    int before = 0;
    for (int b = 0; b < t0; b += 256) {
      unsigned char f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = b + j * 64 + lane < t0 ? flag[b + j * 64 + lane] : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) before += __popcll(__ballot(f[j] != 0));
    }
    keep = (unsigned)__ballot(mine != 0);
    row = o0 + before;
  }
  const int last = min(n - t0, kIngestSeg);
  if (last < kIngestSeg) keep &= (1u << last) - 1u;
  if (keep == 0 || c >= dim) return;
  const int t1 = t0 + 32 - __clz(keep);                                       // one behind the last kept frame
  ingest_segment_rows(in + (size_t)f0 * dim + c, out + c, n, t0, t1, keep, row, o1, dim, window, min_window, center, norm_vars);
}

// Windows of resident rows (asv_ingest_windows): window w is rows [start[w], start[w] + len[w]) of `in` and an utterance of its own -
// windows overlap, repeat and come in any order, which CSR offsets cannot say.  off: [start (n_windows) | len (n_windows) | first row
// of `out` (n_windows)].  Grid and mapping as ingest_frames_kernel; there are no flags, so a wave writes every frame of its segment.
__global__ __launch_bounds__(256) void ingest_windows_kernel(const float *__restrict__ in, float *__restrict__ out, const long long *__restrict__ off,
                                                             int n_windows, int dim, int window, int min_window, int center, int norm_vars) {
  const int w = blockIdx.x, lane = threadIdx.x & 63, c = blockIdx.z * 64 + lane;
  const int n = (int)off[n_windows + w];
  const int t0 = (blockIdx.y * kIngestSegsPerBlock + (threadIdx.x >> 6)) * kIngestSeg;
  if (t0 >= n || c >= dim) return;
  const long long f0 = off[w], o0 = off[2 * n_windows + w];
  const int t1 = min(n, t0 + kIngestSeg);
  const unsigned keep = t1 - t0 < kIngestSeg ? (1u << (t1 - t0)) - 1u : 0xffffffffu;
  ingest_segment_rows(in + (size_t)f0 * dim + c, out + c, n, t0, t1, keep, o0 + t0, o0 + n, dim, window, min_window, center, norm_vars);
}

// the two host offset arrays of a call, on the device (offset_ring.h): this entry point's ring, per calling thread
thread_local OffsetRing g_ingest_offs;
thread_local OffsetRing g_window_offs;                                        // (asv_ingest_windows: its own, so neither evicts the other's)

}  // namespace
}  // namespace asv

using namespace asv;

extern "C" int asv_ingest_frames(const float *feats, const unsigned char *voiced, const long long *frame_offsets, const long long *out_offsets, int n_utts,
                                 int dim, int cmn_window, int min_window, int center, int norm_vars, float *out, void *stream) {
  ASV_REQUIRE(feats && out && feats != out && frame_offsets && out_offsets && n_utts >= 1, "asv_ingest_frames: bad argument (in-place is not supported)");
  ASV_REQUIRE(dim >= 1, "asv_ingest_frames: dim %d", dim);
  ASV_REQUIRE(cmn_window <= 0 || center || (min_window > 0 && min_window <= cmn_window), "asv_ingest_frames: cmn_window %d / min_window %d", cmn_window,
              min_window);
  ASV_REQUIRE(frame_offsets[0] == 0 && out_offsets[0] == 0, "asv_ingest_frames: offsets must start at 0");
  long long longest = 0;
  for (int u = 0; u < n_utts; ++u) {
    const long long frames = frame_offsets[u + 1] - frame_offsets[u], kept = out_offsets[u + 1] - out_offsets[u];
    ASV_REQUIRE(frames >= 0 && kept >= 0, "asv_ingest_frames: offsets decrease at utterance %d", u);
    ASV_REQUIRE(kept <= frames, "asv_ingest_frames: utterance %d keeps %lld of %lld frames", u, kept, frames);
    ASV_REQUIRE(voiced || kept == frames, "asv_ingest_frames: utterance %d: without flags every frame is kept (%lld of %lld)", u, kept, frames);
    longest = std::max(longest, frames);
  }
  if (out_offsets[n_utts] == 0) return ASV_OK;                               // nothing is kept: nothing is written
  const long long blocks_y = (longest + kIngestSegsPerBlock * kIngestSeg - 1) / (kIngestSegsPerBlock * kIngestSeg);
  ASV_REQUIRE(blocks_y <= 65535 && (dim + 63) / 64 <= 65535, "asv_ingest_frames: utterance of %lld frames / dim %d too large", longest, dim);
  ASV_ON_OWNER(feats, "asv_ingest_frames");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long *d = nullptr;
  { const int rc = g_ingest_offs.get(frame_offsets, out_offsets, (size_t)n_utts + 1, s, &d); if (rc) return rc; }
  hipLaunchKernelGGL(ingest_frames_kernel, dim3((unsigned)n_utts, (unsigned)blocks_y, (unsigned)((dim + 63) / 64)), dim3(256), 0, s, feats, voiced, out, d,
                     n_utts, dim, cmn_window, min_window, center, norm_vars);
  ASV_HIP_CHECK(hipGetLastError());
  return g_ingest_offs.launched(s);
}

extern "C" int asv_ingest_windows(const float *feats, long long n_rows, const long long *win_start, const long long *win_len, int n_windows, int dim,
                                  int cmn_window, int min_window, int center, int norm_vars, float *out, void *stream) {
  ASV_REQUIRE(feats && out && win_start && win_len, "asv_ingest_windows: null pointer");
  ASV_REQUIRE(feats != out, "asv_ingest_windows: out is feats (in-place is not supported)");
  ASV_REQUIRE(n_windows >= 1 && n_rows >= 0, "asv_ingest_windows: %d windows of %lld rows", n_windows, n_rows);
  ASV_REQUIRE(dim >= 1, "asv_ingest_windows: dim %d", dim);
  ASV_REQUIRE(cmn_window <= 0 || center || (min_window > 0 && min_window <= cmn_window), "asv_ingest_windows: cmn_window %d / min_window %d", cmn_window,
              min_window);
  thread_local std::vector<long long> first;                                 // first row of `out` per window: the running sum of the lengths
  first.resize((size_t)n_windows);
  long long longest = 0, total = 0;
  for (int w = 0; w < n_windows; ++w) {
    const long long a = win_start[w], n = win_len[w];
    ASV_REQUIRE(a >= 0 && n >= 0, "asv_ingest_windows: window %d starts at %lld and has %lld rows", w, a, n);
    ASV_REQUIRE(a <= n_rows && n <= n_rows - a, "asv_ingest_windows: window %d (rows %lld + %lld) reaches beyond the %lld rows handed over", w, a, n, n_rows);
    first[(size_t)w] = total;
    total += n;
    longest = std::max(longest, n);
  }
  if (total == 0) return ASV_OK;                                             // nothing but empty windows: nothing is written
  // (windows read rows other windows of the same launch write next to: no part of `out` may lie inside `feats`)
  const uintptr_t in_at = reinterpret_cast<uintptr_t>(feats), out_at = reinterpret_cast<uintptr_t>(out);
  ASV_REQUIRE(out_at + (size_t)total * dim * 4 <= in_at || in_at + (size_t)n_rows * dim * 4 <= out_at,
              "asv_ingest_windows: out overlaps feats (in-place is not supported)");
  const long long blocks_y = (longest + kIngestSegsPerBlock * kIngestSeg - 1) / (kIngestSegsPerBlock * kIngestSeg);
  ASV_REQUIRE(blocks_y <= 65535 && (dim + 63) / 64 <= 65535, "asv_ingest_windows: window of %lld rows / dim %d too large", longest, dim);
  ASV_ON_OWNER(feats, "asv_ingest_windows");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long *d = nullptr;
  { const int rc = g_window_offs.get(win_start, win_len, (size_t)n_windows, s, &d, first.data()); if (rc) return rc; }
  hipLaunchKernelGGL(ingest_windows_kernel, dim3((unsigned)n_windows, (unsigned)blocks_y, (unsigned)((dim + 63) / 64)), dim3(256), 0, s, feats, out, d,
                     n_windows, dim, cmn_window, min_window, center, norm_vars);
  ASV_HIP_CHECK(hipGetLastError());
  return g_window_offs.launched(s);
}
