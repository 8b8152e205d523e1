// The per-batch planner (batch_plan.h): the chunk loop of `for_extract_embedding` (libs/nnet/framework.py:12-55) for a whole batch.
#include "batch_plan.h"

namespace asv {

int make_plan(const std::vector<Domain> &domains, const int32_t *offsets, int n_utts, int max_chunk, BatchPlan &bp) {
  ASV_REQUIRE(offsets != nullptr && n_utts >= 1, "extract: need at least one utterance");
  ASV_REQUIRE(offsets[0] == 0, "extract: offsets[0] must be 0");
  if (max_chunk <= 0) max_chunk = 10000;
  bp.n_utts = n_utts;
  bp.utt_seg0.resize(n_utts); bp.utt_nseg.resize(n_utts);
  for (int u = 0; u < n_utts; ++u) {
    const long long T = (long long)offsets[u + 1] - offsets[u];
    ASV_REQUIRE(T >= 1, "extract: utterance %d has %lld frames (the reference asserts T >= tot_context, components.py:119)", u, T);
    // framework.py:34-47
    const int num_split = (int)((T + max_chunk - 1) / max_chunk);
    const int split = (int)(T / num_split);
    bp.utt_seg0[u] = (int32_t)bp.seg_frames.size();
    bp.utt_nseg[u] = num_split;
    for (int i = 0; i < num_split; ++i) {
      const int off = i * split;
      const int len = (i == num_split - 1) ? (int)(T - off) : split;
      bp.seg_src0.push_back(offsets[u] + off);
      bp.seg_frames.push_back(len);
    }
    bp.frames += T;
  }
  bp.segments = (int)bp.seg_frames.size();
  bp.seg_pad = round_up(bp.segments, kRowTile);
  bp.dom.resize(domains.size());
  for (size_t di = 0; di < domains.size(); ++di) {
    const Domain &dm = domains[di];
    DomainPlan &dp = bp.dom[di];
    if (dm.kind == ASV_DOMAIN_UTTS) {
      dp.rows = bp.segments; dp.rows_pad = bp.seg_pad;
      dp.seg_row0 = {0}; dp.seg_len = {bp.segments};          // one pseudo segment covering the valid rows
      continue;
    }
    long long row = dm.gap();
    dp.seg_row0.reserve(bp.segments); dp.seg_len.reserve(bp.segments);
    for (int sidx = 0; sidx < bp.segments; ++sidx) {
      long long fr = bp.seg_frames[sidx];
      for (int k = 0; k < dm.shift; ++k) fr = dm.valid ? (fr - 1) / 2 : (fr + 1) / 2;       // stride-2 stages: ceil(T/2) each; unpadded ones: (T - 1) / 2
      ASV_REQUIRE(fr >= 1, "extract: a chunk of %d frames is too short for the unpadded subsampling front (%d stride-2 stages of kernel 3: at least %d frames)",
                  (int)bp.seg_frames[sidx], dm.shift, (1 << (dm.shift + 1)) - 1);
      const long long len = fr * dm.pitch;
      dp.seg_row0.push_back((int32_t)row);
      dp.seg_len.push_back((int32_t)len);
      row += len + dm.gap();
      ASV_REQUIRE(row < (1ll << 30), "extract: batch too large (%lld rows in domain %zu)", row, di);
    }
    dp.rows = (int)row;
    dp.rows_pad = round_up(dp.rows, kRowTile);
  }
  return ASV_OK;
}

}  // namespace asv
