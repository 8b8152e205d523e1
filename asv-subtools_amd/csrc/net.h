// The layer program behind asv_net_t, shared by the host units of libasv_amd.so: net_build.hip (the builder, asv_net_*), net_run.hip (the
// launch sequence of a batch behind asv_net_extract) and stamp_report.hip (developer reports).  The batch planner: batch_plan.h.
#pragma once
#include <atomic>
#include <vector>

#include "asv_internal.h"

namespace asv {

struct Buffer { int domain, channels, ld; };

enum OpKind { OP_TDNN = 0, OP_POOL = 1, OP_ATTPOOL = 2, OP_ELTWISE = 3, OP_GRID_INPUT = 4, OP_IM2COL = 5, OP_LDE = 6, OP_RES2 = 7, OP_FLATTEN = 8, OP_MQ_ATTPOOL = 9, OP_RES2N = 10, OP_ROWOP = 11, OP_GRID_CONV = 12, OP_ATTENTION = 13, OP_POSENC = 14, OP_FRONT_CONV = 15 };

struct Op {
  OpKind kind;
  // common views
  asv_tdnn_desc_t tdnn;          // host pointers nulled after packing
  asv_pool_desc_t pool;
  asv_attpool_desc_t att;
  asv_eltwise_desc_t elt;
  asv_grid_input_desc_t gin;
  asv_im2col_desc_t i2c;
  asv_grid_flatten_desc_t flat;
  asv_lde_desc_t lde;            // mu / beta live in `scale` / `shift` on the device
  asv_mq_attpool_desc_t mq;
  asv_res2n_desc_t res2n;        // likewise (bias stays nullptr when the op has none)
  asv_res2_desc_t res2;          // fragments in `wfrag`, per-branch constants in bias / scale / shift
  asv_rowop_desc_t rop;          // host pointers nulled; the per-channel tables live in `rop_tab`
  asv_grid_conv_desc_t gconv;    // host pointers nulled; fragments of pack_grid_conv_taps in `wconv`, bias in `bias`
  asv_self_attention_desc_t sa;
  asv_posenc_desc_t pos;         // host pointer nulled; the table [pe_rows][round_up(channels, 16)] in `scale`
  asv_front_conv_desc_t front;   // host pointers nulled; [out_ch][9] in `scale`, the bias in `bias`
  // device parameters
  void *w = nullptr;
  void *wfrag = nullptr;         // fragment-ordered copy for the variant-3 kernel (bf16 frame layers); pooled layers: bf16 hi halves
  void *wconv = nullptr;         // 3x3 trunk convolutions with 32 / 64 / 128 / 256 channels: fragment order of kernels_conv2d.hip
  void *wlo = nullptr;           // pooled layers in bf16 precision mode: bf16 lo halves (kernels_utts.hip)
  void *wx3p = nullptr;          // f32x mode, wide frame layers with the plain epilogue: [hi | lo] rows for kernels_tdnn_p8x.hip
  void *w8 = nullptr, *w8_fold = nullptr;      // f32m form (ASV_FLAG_X3_MX8): 8-bit fragments of the layer / of its folded weights (pack_tdnn_weight_mx8)
  float *bias = nullptr, *scale = nullptr, *shift = nullptr;
  float *rop_tab[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // row op: scale0, shift0, gamma, beta, scale1, shift1
  int cin_pad = 0, cout_pad = 0, cout_store = 0;
  // chain candidates (16-bit modes, 1-tap layers reading a 512-channel buffer): host copies kept until asv_net_finalize, which
  // folds the eval BatchNorm of the PREVIOUS chain layer into this layer's weights and bias (see the chain pass there)
  std::vector<float> host_w, host_bias, host_scale, host_shift;
  void *wfrag_fold = nullptr;    // fragment-ordered W diag(s_prev) ... (f32x: its hi halves, wlo_fold the lo halves, w_scale_fold their power of two)
  void *wlo_fold = nullptr;
  float w_scale_fold = 1.0f;
  float *bias_fold = nullptr;    // ... and b + W t_prev
  float w_scale = 1.0f;          // f32x mode, half-precision split: the power of two the fragment weights were multiplied by
  bool utts = false;             // op runs in the utts domain (always f32)
  bool has_affine = false;
  int fused_pool = -1;           // TDNN op: index of the statistics-pooling op folded into its epilogue
  int chain_last = -1;           // TDNN op heading a chain (kernels_tdnn_chain.hip): index of the chain's last layer
  int image_reader = -1;         // f32m: the ONE op that reads this TDNN op's whole output buffer, as its input rows - the buffer may hold images
                                 // (TdnnKernelParams::y_image) in a run where both ops go to image-capable kernels (run_tdnn_layer)
  bool skipped = false;          // pool op executed by its producer
  std::string desc;              // the op's line of asv_net_describe
};

struct DevMem { void *ptr = nullptr; size_t cap = 0; };

// kernel classes of the profile (asv_net_get_profile)
constexpr const char *kKernelNames[] = {"tdnn_gemm", "stats_pool", "attentive_pool", "eltwise", "rowmap", "pack_input", "combine", "grid_gather", "utts_gemm", "res2n_chain", "rowop", "grid_conv_taps", "self_attention", "posenc", "front_conv"};
enum { K_TDNN = 0, K_POOL, K_ATT, K_ELT, K_ROWMAP, K_PACK, K_COMBINE, K_GATHER, K_UTTS, K_RES2N, K_ROWOP, K_CONV_TAPS, K_ATTENTION, K_POSENC, K_FRONT_CONV, K_COUNT };   // K_UTTS: affine layers of the pooled domain; K_RES2N: res2n_chain_kernel (its own row: tools/res2n_profile_workload.py)

// a planned batch on the device: what prepare() hands a run, and leaves behind for the next call with identical offsets
struct DomainRun {
  int rows_pad = 0;
  int32_t *seg_row0 = nullptr, *seg_len = nullptr, *row_seg = nullptr;
  uint32_t *row_valid = nullptr;
};
struct PlannedBatch {
  BatchPlan bp;
  int32_t *seg_src0 = nullptr, *seg_frames = nullptr, *utt_seg0 = nullptr, *utt_nseg = nullptr;     // device metadata
  std::vector<DomainRun> dom;
};

}  // namespace asv

struct asv_net {
  int device = 0, precision = 0, feat_dim = 0;
  unsigned flags = 0;
  bool finalized = false;
  int out_buf = -1, embed_dim = 0;
  std::vector<asv::Buffer> bufs;
  std::vector<asv::Domain> domains;
  std::vector<asv::Op> ops;
  std::vector<void *> weight_allocs;
  size_t weight_bytes = 0;
  // per-call state
  std::vector<asv::DevMem> arena;        // one region per buffer
  asv::DevMem meta_dev;                  // int32 metadata (segments etc.)
  asv::DevMem rowmeta_dev;               // row_seg / row_valid for both domains
  asv::DevMem poolpart_dev;              // fused-pooling partial moments
  asv::DevMem lde_dev;                   // LDE pooling: per-row centre weights [rows][64]
  void *zero_page = nullptr;             // 256 zero bytes (masked direct-to-LDS loads); bytes 128..131: the status word (asv_net_status)
  void *meta_host = nullptr;             // pinned staging
  size_t meta_host_cap = 0;
  hipEvent_t meta_copied = nullptr;      // H2D of meta_host finished
  bool meta_inflight = false;
  // plan cache: a batch with the same utterance lengths as the previous one reuses the uploaded segment
  // tables and row maps (steady-state extraction loops over equally shaped batches)
  std::vector<int32_t> cached_offsets;
  int cached_max_chunk = -1;
  bool cache_valid = false;
  asv::PlannedBatch plan_cache;
  // profiling
  int profiling = 0;               // 0 off, 1 per kernel class, 2 per op, 3 frame-level GEMM launches only, 4 = 3 with ONE event
                                   // pair around every run of consecutive frame-level GEMM launches
  struct Stamp { int kclass; int op; double flops; hipEvent_t a, b; int launches = 1; bool open = false; };
  std::vector<Stamp> stamps;
  std::vector<hipEvent_t> event_pool;

  bool frames_h16() const { return precision == ASV_PREC_BF16 || precision == ASV_PREC_F16; }     // 16-bit frames-domain storage
  int frames_et() const { return precision == ASV_PREC_BF16 ? asv::ET_BF16 : (precision == ASV_PREC_F16 ? asv::ET_F16 : asv::ET_F32); }
  int x3_et() const { return (flags & ASV_FLAG_X3_SPLIT_BF16) ? asv::ET_BF16 : asv::ET_F16; }        // f32x: type of the operand halves
  int x3_terms() const { return 1 | ((flags & ASV_FLAG_X3_NO_XLO) ? 0 : 2) | ((flags & ASV_FLAG_X3_NO_WLO) ? 0 : 4); }
  bool x3() const { return precision == ASV_PREC_F32X; }        // f32 storage, split-bf16 matrix products
  bool x3_mx() const { return x3() && (flags & ASV_FLAG_X3_MX8) != 0 && x3_et() == asv::ET_F16 && x3_terms() == 7; }      // "f32m": corrections on the scaled 8-bit instruction
  bool is_utts(int domain) const { return domains[domain].kind == ASV_DOMAIN_UTTS; }
  // one row per frame: the frames domain, or a width-1 / pitch-1 grid (the 2-D trunk's output flattened, asv_net_add_grid_flatten)
  bool is_sequence(int domain) const { return domains[domain].kind == ASV_DOMAIN_FRAMES || (domains[domain].kind == 2 && domains[domain].width == 1 && domains[domain].pitch == 1); }
  int dom_et(int domain) const { return is_utts(domain) ? asv::ET_F32 : frames_et(); }               // element type of a domain's rows
  size_t elem_size(int domain) const { return dom_et(domain) != asv::ET_F32 ? 2 : 4; }
};

namespace asv {

// the range-status word of the f32x kernels lives behind the zero page's zeros (own 64-byte line; kernels only ever OR into it)
inline uint32_t *status_word(asv_net *net) { return reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(net->zero_page) + 128); }

extern std::atomic<unsigned long long> g_kernel_launches[ASV_KERNEL_FRONT_CONV + 1];       // asv_kernel_launch_count (ids start at 1; net_run.hip)

// developer aids (stamp_report.hip): a kernel's phase stamps summarised on stderr; both free the stamp buffer
int report_chain_stamps(void *dbg, size_t nwg, int chain_dbg, bool chain_mx, hipStream_t s);
int report_res2_stamps(void *dbg, size_t nwg, hipStream_t s);

}  // namespace asv
