// Developer stamp reports of libasv_amd.so (net.h): the phase stamps a kernel wrote under ASV_AMD_CHAIN_DBG / ASV_AMD_RES2_DBG, summarised
// on stderr.  tools/chain_dbg.py and tools/res2_dbg.py parse the text.  Nothing here runs unless one of the two variables is set.
#include <algorithm>
#include <vector>

#include "net.h"

namespace asv {

int report_chain_stamps(void *dbg, size_t nwg, int chain_dbg, bool chain_mx, hipStream_t s) {
  std::vector<unsigned long long> h(nwg * 8 * 32);
  ASV_HIP_CHECK(hipStreamSynchronize(s));
  ASV_HIP_CHECK(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
  ASV_HIP_CHECK(hipFree(dbg));
  double sum[32] = {0}; size_t cnt = 0; double cyc = 0, rt = 0;
  for (size_t w = 0; w < nwg * 8; ++w) {
    const unsigned long long *t = &h[w * 32];
    if (t[0] == 0) continue;
    for (int k = 1; k < 14; ++k) if (t[k] > t[k - 1]) sum[k] += (double)(t[k] - t[k - 1]);      // 13: the 4-wave kernel's drain
    if (chain_dbg >= 3) {
      if (t[16] > t[7]) sum[16] += (double)(t[16] - t[7]);                                   // unit's K loop end -> epilogue body
      for (int k = 17; k < 22; ++k) if (t[k] > t[k - 1]) sum[k] += (double)(t[k] - t[k - 1]);
    }
    const unsigned long long t_end = t[13] > t[12] ? t[13] : t[12];
    if (t_end > t[0] && t[15] > t[14]) { cyc += (double)(t_end - t[0]); rt += (double)(t[15] - t[14]); }
    ++cnt;
  }
  fprintf(stderr, "[chain dbg] %zu waves, mean cycles per phase:", cnt);
  fprintf(stderr, " [shader clock %.0f MHz, %.1f us per workgroup]", rt > 0 ? 100.0 * cyc / rt : 0.0, cnt ? rt / 100.0 / (double)cnt : 0.0);
  for (int k = 1; k < 14; ++k) if (k < 13 || sum[k] > 0) fprintf(stderr, " %d:%.0f", k, sum[k] / (double)std::max<size_t>(cnt, 1));
  if (chain_dbg >= 3) {
    fprintf(stderr, " | first epilogue: entry %.0f, fragments", sum[16] / (double)std::max<size_t>(cnt, 1));
    for (int k = 17; k < 21; ++k) fprintf(stderr, " %.0f", sum[k] / (double)std::max<size_t>(cnt, 1));
    fprintf(stderr, ", publish %.0f", sum[21] / (double)std::max<size_t>(cnt, 1));
  }
  fprintf(stderr, "\n");
  if (chain_mx && chain_dbg >= 3) {                      // layer A, steps 0 .. 14: mean cycles per step, by wave
    for (int wv = 0; wv < 8; ++wv) {
      double d[15] = {0}; size_t cn = 0;
      for (size_t wg = 0; wg < nwg; ++wg) {
        const unsigned long long *t = &h[(wg * 8 + wv) * 32];
        if (t[16] == 0 || t[31] <= t[16]) continue;
        for (int k = 0; k < 15; ++k) d[k] += (double)(t[17 + k] - t[16 + k]);
        ++cn;
      }
      fprintf(stderr, "[chainm dbg] wave %d, cycles of layer A's steps 0..14:", wv);
      for (int k = 0; k < 15; ++k) fprintf(stderr, " %.0f", d[k] / (double)std::max<size_t>(cn, 1));
      fprintf(stderr, "\n");
    }
  }
  {                                                       // 4-wave kernel, ablation 8: fine stamps of wave 0's third unit (slots of wave 4..7)
    double fs[25] = {0}; size_t fc = 0;
    for (size_t wg = 0; wg < nwg; ++wg) {
      const unsigned long long *t = &h[(wg * 8 + 4) * 32];
      if (t[0] == 0 || t[24] <= t[0]) continue;
      for (int k = 1; k < 25; ++k) fs[k] += (double)(t[k] - t[k - 1]);
      ++fc;
    }
    if (fc) {
      fprintf(stderr, "[chain dbg] third unit of wave 0, %zu workgroups, per chunk: pre | 32 matrix instructions | post:", fc);
      for (int c = 0; c < 8; ++c) fprintf(stderr, "  %.0f | %.0f | %.0f", fs[3 * c + 1] / fc, fs[3 * c + 2] / fc, fs[3 * c + 3] / fc);
      fprintf(stderr, "\n");
    }
  }
  if (chain_dbg == 2 || chain_dbg >= 4) {                 // raw timelines of two workgroups: waves w and w + 4 share a SIMD
    const size_t picks[2] = {nwg / 4, nwg / 2 + 1};
    for (size_t wg : picks) {
      if (wg >= nwg) continue;
      unsigned long long t0 = ~0ull;
      for (int w = 0; w < 8; ++w) if (h[(wg * 8 + w) * 32] != 0) t0 = std::min(t0, h[(wg * 8 + w) * 32]);
      for (int w = 0; w < 8; ++w) {
        fprintf(stderr, "[chain dbg] workgroup %zu wave %d stamps (cycles since the first wave's stamp 0):", wg, w);
        for (int k = 0; k < 13; ++k) fprintf(stderr, " %lld", (long long)(h[(wg * 8 + w) * 32 + k] - t0));
        if (chain_dbg >= 4) { fprintf(stderr, " |"); for (int k = 16; k < 22; ++k) fprintf(stderr, " %lld", (long long)(h[(wg * 8 + w) * 32 + k] - t0)); }
        fprintf(stderr, "\n");
      }
    }
  }
  return ASV_OK;
}

int report_res2_stamps(void *dbg, size_t nwg, hipStream_t s) {
  std::vector<unsigned long long> h(nwg * 8 * 16);
  ASV_HIP_CHECK(hipStreamSynchronize(s));
  ASV_HIP_CHECK(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
  ASV_HIP_CHECK(hipFree(dbg));
  double sum[16] = {0}; size_t cnt = 0; double cyc = 0, rt = 0;
  for (size_t w = 0; w < nwg * 8; ++w) {
    const unsigned long long *t = &h[w * 16];
    if (t[0] == 0) continue;
    for (int k = 1; k < 14; ++k) if (t[k] > t[k - 1]) sum[k] += (double)(t[k] - t[k - 1]);
    if (t[13] > t[0] && t[15] > t[14]) { cyc += (double)(t[13] - t[0]); rt += (double)(t[15] - t[14]); }
    ++cnt;
  }
  fprintf(stderr, "[res2 dbg] %zu waves [shader clock %.0f MHz, %.1f us per workgroup] 1 = first windows; per branch (1..3): K loop, wait + barrier, epilogue, "
          "barrier; 13 = branches 4.. + end:", cnt, rt > 0 ? 100.0 * cyc / rt : 0.0, cnt ? rt / 100.0 / (double)cnt : 0.0);
  for (int k = 1; k < 14; ++k) fprintf(stderr, " %d:%.0f", k, sum[k] / (double)std::max<size_t>(cnt, 1));
  fprintf(stderr, "\n");
  return ASV_OK;
}

}  // namespace asv
