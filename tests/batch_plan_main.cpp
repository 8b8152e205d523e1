// Stand-alone driver of csrc/batch_plan.cpp for tests/test_batch_plan_host.py (plain C++, no GPU).
// stdin (text): n_domains, then per domain `kind shift width pitch reach valid`; max_chunk; n_utts; offsets[n_utts + 1]; block_rows.
// stdout: `rc <code>`; after a failure `error <message>`; else every field of the BatchPlan, one `name: values` line each (per domain
//         `dom <i> rows`, `rows_pad`, `seg_row0`, `seg_len`), and with block_rows > 0 `max_segments_per_block` of the frames plan over
//         blocks of that many rows.
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "batch_plan.h"

static std::string g_error;

namespace asv {
void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace asv

using namespace asv;

static void print(const char *name, const std::vector<int32_t> &v) {
  printf("%s:", name);
  for (int32_t x : v) printf(" %d", (int)x);
  printf("\n");
}

int main() {
  int n_domains = 0, max_chunk = 0, n_utts = 0, block_rows = 0;
  if (scanf("%d", &n_domains) != 1 || n_domains < 0 || n_domains > 64) return 2;
  std::vector<Domain> domains;
  for (int i = 0; i < n_domains; ++i) {
    int kind, shift, width, pitch, reach, valid;
    if (scanf("%d %d %d %d %d %d", &kind, &shift, &width, &pitch, &reach, &valid) != 6) return 2;
    Domain d{kind};
    d.shift = shift; d.width = width; d.pitch = pitch; d.reach = reach; d.valid = valid != 0;
    domains.push_back(d);
  }
  if (scanf("%d %d", &max_chunk, &n_utts) != 2 || n_utts < 0 || n_utts > (1 << 20)) return 2;
  std::vector<int32_t> offsets((size_t)n_utts + 1);
  for (int32_t &o : offsets)
    if (scanf("%d", &o) != 1) return 2;
  if (scanf("%d", &block_rows) != 1 || block_rows < 0) return 2;

  BatchPlan bp;
  const int rc = make_plan(domains, offsets.data(), n_utts, max_chunk, bp);
  printf("rc %d\n", rc);
  if (rc != ASV_OK) {
    printf("error %s\n", g_error.c_str());
    return 0;
  }
  printf("n_utts: %d\nsegments: %d\nseg_pad: %d\nframes: %lld\n", bp.n_utts, bp.segments, bp.seg_pad, bp.frames);
  print("seg_src0", bp.seg_src0);
  print("seg_frames", bp.seg_frames);
  print("utt_seg0", bp.utt_seg0);
  print("utt_nseg", bp.utt_nseg);
  printf("n_dom: %zu\n", bp.dom.size());
  for (size_t i = 0; i < bp.dom.size(); ++i) {
    char name[64];
    printf("dom %zu rows: %d\ndom %zu rows_pad: %d\n", i, bp.dom[i].rows, i, bp.dom[i].rows_pad);
    snprintf(name, sizeof(name), "dom %zu seg_row0", i);
    print(name, bp.dom[i].seg_row0);
    snprintf(name, sizeof(name), "dom %zu seg_len", i);
    print(name, bp.dom[i].seg_len);
  }
  if (block_rows > 0) {
    const DomainPlan &fp = bp.dom[ASV_DOMAIN_FRAMES];
    printf("max_segments_per_block: %d\n", max_segments_per_block(fp, fp.rows_pad / block_rows, [&](int row) { return row / block_rows; }));
  }
  return 0;
}
