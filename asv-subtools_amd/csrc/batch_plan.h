// The per-batch segment / row planner of libasv_amd.so: utterance lengths -> chunks (framework.py:34-47) -> the rows every chunk owns
// in every row domain.  Plain C++ with no HIP in it (tests/test_batch_plan_host.py compiles it with g++ and restates its results).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/asv_amd.h"
#include "host_convert.h"

namespace asv {

// error plumbing: nothing throws across the C ABI
void set_error(const char *fmt, ...);

#define ASV_REQUIRE(cond, ...) do { if (!(cond)) { ::asv::set_error(__VA_ARGS__); return ASV_EINVAL; } } while (0)

// Row layout of the frames domain (see DESIGN.md "Data layout in HBM").
//
// A batch of S utterance segments is laid out as
//     [HALO zero rows][seg 0][HALO zero rows][seg 1] ... [seg S-1][HALO zero rows][zero fill to R_pad]
// so a tap that reaches up to HALO frames across a segment edge reads zeros: exactly the
// per-layer zero padding of TdnnAffine (components.py:116-117), with no masks in the GEMM
// main loop.  Every producer writes zeros into gap rows (row_valid bit clear).
constexpr int kHalo = 4;           // max |tap offset| supported (ECAPA dilation 4)
constexpr int kRowTile = 256;      // rows are padded to a multiple of the largest GEMM M tile

// Row domains.  0 = frames (1 row per frame, HALO-row gaps), 1 = utts (1 row per segment),
// >= 2 = grids for the 2-D ResNet trunk: a segment of T frames owns ceil(T / 2^shift) x pitch rows
// ((time, frequency), frequency fastest, `width` valid rows per frame) with pitch+2 gap rows around it.
struct Domain {
  int kind;                // ASV_DOMAIN_FRAMES / ASV_DOMAIN_UTTS / 2 (grid)
  int shift = 0, width = 1, pitch = 1;
  int reach = 1;           // grids: 2 = pitch >= width + 2 and gaps that cover +-(2 pitch + 2) rows (asv_net_define_grid_reach)
  bool valid = false;      // grids: a segment owns L(T) frames, L the chain n -> (n - 1) / 2 per shift (asv_net_define_grid_valid); else ceil(T / 2^shift)
  int halo() const { return kind == ASV_DOMAIN_FRAMES ? kHalo : (kind == ASV_DOMAIN_UTTS ? 0 : pitch + 1); }      // what a TDNN layer may reach
  int conv_halo() const { return kind == 2 ? reach * pitch + reach : 0; }                                          // what asv_net_add_grid_conv may reach
  int gap() const { return kind == ASV_DOMAIN_FRAMES ? kHalo : (reach == 2 ? 2 * pitch + 3 : pitch + 2); }
};

// Per-call plan of segments and rows.
struct DomainPlan {
  int rows = 0, rows_pad = 0;
  std::vector<int32_t> seg_row0, seg_len;      // first row / number of rows of each segment in this domain
};
struct BatchPlan {
  int n_utts = 0, segments = 0, seg_pad = 0;
  long long frames = 0;
  std::vector<int32_t> seg_src0, seg_frames, utt_seg0, utt_nseg;
  std::vector<DomainPlan> dom;                 // indexed like `domains`
};

int make_plan(const std::vector<Domain> &domains, const int32_t *offsets, int n_utts, int max_chunk, BatchPlan &bp);

// the most segments of the frames domain that any one block of rows holds (block_of: row -> block, at most n_blocks)
template <class BlockOf> int max_segments_per_block(const DomainPlan &fp, int n_blocks, BlockOf block_of) {
  std::vector<int> per_block((size_t)n_blocks + 1, 0);
  int slots = 1;
  for (size_t s = 0; s < fp.seg_row0.size(); ++s)
    for (int h = block_of(fp.seg_row0[s]); h <= block_of(fp.seg_row0[s] + fp.seg_len[s] - 1); ++h) slots = std::max(slots, ++per_block[h]);
  return slots;
}

}  // namespace asv
