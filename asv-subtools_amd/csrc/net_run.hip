// The launch sequence of one batch behind asv_net_extract(): prepare() (plan, metadata, row maps, arena), the kernel choice of the TDNN
// layers (choose_tdnn), one run function per op kind, and the one-op forwards on a one-off net.
//
// Replaces, for the batched device path, what `for_extract_embedding` +
// `<Model>.extract_embedding` do one utterance at a time in the reference
// (libs/nnet/framework.py:12-55, model/xvector.py:77-98, model/ecapa_tdnn_xvector.py:403-426).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "net.h"

namespace asv {

std::atomic<unsigned long long> g_kernel_launches[ASV_KERNEL_FRONT_CONV + 1];

namespace {

int ensure(DevMem &m, size_t bytes, hipStream_t s, bool zero) {
  if (bytes <= m.cap) return ASV_OK;
  if (m.ptr) {
    ASV_HIP_CHECK(hipStreamSynchronize(s));
    ASV_HIP_CHECK(hipFree(m.ptr));
    m.ptr = nullptr; m.cap = 0;
  }
  const size_t cap = bytes + bytes / 8 + 4096;
  ASV_HIP_CHECK(hipMalloc(&m.ptr, cap));
  m.cap = cap;
  if (zero) ASV_HIP_CHECK(hipMemsetAsync(m.ptr, 0, cap, s));
  return ASV_OK;
}

struct Prof {
  asv_net *net; hipStream_t s; bool active = false;
  // mode 4: a run of back-to-back frame-level GEMM launches shares one event pair (every recorded event is a barrier
  // packet between two kernels; ten of them per step slowed the sampled steps by up to 2x)
  int close_span() {
    if (net->profiling == 4 && !net->stamps.empty() && net->stamps.back().open) {
      net->stamps.back().open = false;
      ASV_HIP_CHECK(hipEventRecord(net->stamps.back().b, s));
    }
    return ASV_OK;
  }
  // a new stamp with its event pair (from the pool, or created), the first event recorded
  int open_stamp(int kclass, double flops, int op, bool open) {
    asv_net::Stamp st; st.kclass = kclass; st.flops = flops; st.op = op; st.open = open;
    for (hipEvent_t *e : {&st.a, &st.b}) {
      if (!net->event_pool.empty()) { *e = net->event_pool.back(); net->event_pool.pop_back(); }
      else ASV_HIP_CHECK(hipEventCreate(e));
    }
    ASV_HIP_CHECK(hipEventRecord(st.a, s));
    net->stamps.push_back(st);
    return ASV_OK;
  }
  int begin(int kclass, double flops, int op = -1) {
    if (net->profiling == 4) {
      active = false;
      if (kclass != K_TDNN) return close_span();
      if (net->stamps.empty() || !net->stamps.back().open) return open_stamp(kclass, flops, -1, true);
      net->stamps.back().flops += flops;
      net->stamps.back().launches += 1;
      return ASV_OK;
    }
    active = net->profiling != 0 && (net->profiling != 3 || kclass == K_TDNN);
    return active ? open_stamp(kclass, flops, op, false) : ASV_OK;
  }
  int end() {
    if (!active) return ASV_OK;
    ASV_HIP_CHECK(hipEventRecord(net->stamps.back().b, s));
    return ASV_OK;
  }
};

// One launch inside its profile stamp: begin / launch / count / end (count_id: the launch's asv_kernel_launch_count id, 0 = it has none).  A
// template on the callable: a step is a dozen launches in 0.27 ms, so nothing here may allocate or go through a function object.
template <class Launch> int timed(Prof &prof, int kclass, double flops, int op, int count_id, Launch launch) {
  int rc;
  if ((rc = prof.begin(kclass, flops, op)) || (rc = launch())) return rc;
  if (count_id > 0) ++g_kernel_launches[count_id];
  return prof.end();
}

// Kernel-selection switches of the TDNN layers (developer A/B aids, result-preserving), read once per process unless ASV_AMD_LIVE_TUNE is set -
// the in-process A/B tests switch that on after the library's first launch, so THAT lookup cannot be cached: one getenv per run
struct TdnnRules {
  int p8 = 1, p8x = 1, x3m = 1, x3m_image = 1;   // ASV_AMD_P8 / _P8X / _X3M / _X3M_IMAGE: 0 off, 1 the production rule, N > 1 a lowered tile count
  long long cus = 256;                           // "one round of tiles" = one 256 x 256 tile per CU of THIS device (the kernels size their persistent grids from the same count)
  int chain_dbg = 0;                             // ASV_AMD_CHAIN_DBG (read once): the chain kernels' phase stamps on stderr, levels 1 - 4
  void read_switches() {
    auto env = [](const char *name) { const char *v = getenv(name); return v != nullptr ? atoi(v) : 1; };
    p8 = env("ASV_AMD_P8"); p8x = env("ASV_AMD_P8X"); x3m = env("ASV_AMD_X3M"); x3m_image = env("ASV_AMD_X3M_IMAGE");
  }
};
TdnnRules tdnn_rules() {
  static const TdnnRules once = [] {
    TdnnRules r;
    r.read_switches();
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    r.cus = n > 0 ? n : 256;
    const char *dbg = getenv("ASV_AMD_CHAIN_DBG");
    r.chain_dbg = dbg != nullptr ? std::max(1, atoi(dbg)) : 0;
    return r;
  }();
  TdnnRules r = once;
  if (getenv("ASV_AMD_LIVE_TUNE") != nullptr) r.read_switches();
  return r;
}

struct RunCtx : PlannedBatch {
  asv_net *net; hipStream_t s;
  size_t n_ops = 0;                // run_ops: the ops of this run (a one-off net may run fewer than it holds)
  float *final_out = nullptr;      // asv_net_extract: the caller's result matrix (lets the last layer write it directly)
  bool final_written = false;
  std::vector<char> buf_image;     // per run: buffer holds images (TdnnKernelParams::y_image of its producer)
  TdnnRules rules;                 // per run (run_ops)
};

int prepare(RunCtx &c, const int32_t *offsets, int n_utts, int max_chunk) {
  asv_net *net = c.net;
  int rc;
  ASV_REQUIRE(offsets != nullptr && n_utts >= 1, "extract: need at least one utterance");
  if (net->cache_valid && net->cached_max_chunk == max_chunk && (int)net->cached_offsets.size() == n_utts + 1 &&
      memcmp(net->cached_offsets.data(), offsets, (size_t)(n_utts + 1) * 4) == 0) {
    static_cast<PlannedBatch &>(c) = net->plan_cache;
    return ASV_OK;                                   // device tables, row maps and arena are still valid
  }
  net->cache_valid = false;
  if ((rc = make_plan(net->domains, offsets, n_utts, max_chunk, c.bp))) return rc;
  const BatchPlan &bp = c.bp;
  const int S = bp.segments, B = bp.n_utts;
  const size_t ndom = net->domains.size();
  // ---- int32 metadata: one pinned staging buffer, one H2D copy
  size_t n_meta = (size_t)2 * S + 2 * B;
  for (auto &dp : bp.dom) n_meta += dp.seg_row0.size() + dp.seg_len.size();
  const size_t meta_bytes = n_meta * sizeof(int32_t);
  if (net->meta_inflight) { ASV_HIP_CHECK(hipEventSynchronize(net->meta_copied)); net->meta_inflight = false; }
  if (meta_bytes > net->meta_host_cap) {
    if (net->meta_host) ASV_HIP_CHECK(hipHostFree(net->meta_host));
    net->meta_host = nullptr;
    net->meta_host_cap = meta_bytes * 2 + 4096;
    ASV_HIP_CHECK(hipHostMalloc(&net->meta_host, net->meta_host_cap, hipHostMallocDefault));
  }
  if (!net->meta_copied) ASV_HIP_CHECK(hipEventCreateWithFlags(&net->meta_copied, hipEventDisableTiming));
  if ((rc = ensure(net->meta_dev, meta_bytes, c.s, false))) return rc;
  int32_t *h = reinterpret_cast<int32_t *>(net->meta_host);
  int32_t *d = reinterpret_cast<int32_t *>(net->meta_dev.ptr);
  size_t o = 0;
  auto put = [&](const std::vector<int32_t> &v, int32_t **dev) { memcpy(h + o, v.data(), v.size() * 4); *dev = d + o; o += v.size(); };
  put(bp.seg_src0, &c.seg_src0); put(bp.seg_frames, &c.seg_frames);
  put(bp.utt_seg0, &c.utt_seg0); put(bp.utt_nseg, &c.utt_nseg);
  c.dom.resize(ndom);
  size_t rm_words = 0;
  for (size_t i = 0; i < ndom; ++i) {
    put(bp.dom[i].seg_row0, &c.dom[i].seg_row0);
    put(bp.dom[i].seg_len, &c.dom[i].seg_len);
    c.dom[i].rows_pad = bp.dom[i].rows_pad;
    rm_words += (size_t)bp.dom[i].rows_pad + bp.dom[i].rows_pad / 32;
  }
  ASV_HIP_CHECK(hipMemcpyAsync(d, h, meta_bytes, hipMemcpyHostToDevice, c.s));
  ASV_HIP_CHECK(hipEventRecord(net->meta_copied, c.s));
  net->meta_inflight = true;
  // ---- row maps of every domain
  if ((rc = ensure(net->rowmeta_dev, rm_words * 4, c.s, false))) return rc;
  int32_t *r = reinterpret_cast<int32_t *>(net->rowmeta_dev.ptr);
  Prof prof{net, c.s};
  if ((rc = prof.begin(K_ROWMAP, 0))) return rc;
  for (size_t i = 0; i < ndom; ++i) {
    const Domain &dm = net->domains[i];
    c.dom[i].row_seg = r; r += c.dom[i].rows_pad;
    c.dom[i].row_valid = reinterpret_cast<uint32_t *>(r); r += c.dom[i].rows_pad / 32;
    const int nseg = (int)bp.dom[i].seg_row0.size();
    if ((rc = launch_rowmap(c.dom[i].seg_row0, c.dom[i].seg_len, nseg, c.dom[i].rows_pad, dm.kind == 2 ? dm.pitch : 1, dm.kind == 2 ? dm.width : 1,
                            c.dom[i].row_seg, c.dom[i].row_valid, c.s))) return rc;
  }
  if ((rc = prof.end())) return rc;
  // ---- activation arena
  for (size_t i = 0; i < net->bufs.size(); ++i) {
    const Buffer &b = net->bufs[i];
    if ((rc = ensure(net->arena[i], (size_t)c.dom[b.domain].rows_pad * b.ld * net->elem_size(b.domain), c.s, true))) return rc;
  }
  net->plan_cache = c;
  net->cached_offsets.assign(offsets, offsets + n_utts + 1);
  net->cached_max_chunk = max_chunk;
  net->cache_valid = true;
  return ASV_OK;
}

// channels [ch_off, ..) of a buffer's rows in the arena: the pointer and the row pitch a kernel's parameters take, bound in one go
struct View {
  unsigned char *p; int ld;
  template <class P> void to(P &ptr, int &pitch) const { ptr = reinterpret_cast<P>(p); pitch = ld; }
};
View view(RunCtx &c, int buf, int ch_off = 0) {
  const Buffer &b = c.net->bufs[buf];
  return {reinterpret_cast<unsigned char *>(c.net->arena[buf].ptr) + (size_t)ch_off * c.net->elem_size(b.domain), b.ld};
}

// The valid positions of the batch in a domain: frames, segments (the utts domain's one pseudo segment), or the (time, frequency) positions
// of a grid - `width` of every `pitch` rows.  A segment's rows are always a multiple of the pitch (make_plan), so the integer quotient
// is exact, and equal to the double-precision form two of the three former copies of this loop used.
double valid_positions(const RunCtx &c, int domid) {
  const Domain &dm = c.net->domains[domid];
  double n = 0;
  for (int32_t len : c.bp.dom[domid].seg_len) n += (double)(len / dm.pitch) * dm.width;
  return n;
}

// ---- TDNN layers: which kernel runs an op (choose_tdnn), and the pieces of its launch

// The kernel of a TDNN op: the head of a layer chain (the op, its 1-tap followers and the fused statistics pooling in one kernel),
// or one per-layer kernel.
enum class TdnnPath {
  Chain16, ChainX, ChainM,                        // kernels_tdnn_chain.hip (16-bit modes) / kernels_tdnn_chainx.hip (f32x) / kernels_tdnn_chainm.hip (f32m)
  Ref, Utts,                                      // plain-VALU self-check kernels / the pooled-domain GEMM (kernels_utts.hip)
  ConvNarrow, ConvWide, ConvS2d, ConvC1, ConvX3,  // grid convolutions of the 2-D trunk (kernels_conv2d.hip, kernels_conv2d_x3.hip)
  X3m, P8x, X3, P8, Big3, Mfma                    // frame layers
};
struct TdnnChoice {
  TdnnPath path = TdnnPath::Mfma;
  ChainTilePlan plan;          // Chain16: the launch's tile plan
  int n_blocks = 0;            // chains: partial-moment blocks
  int pool_slots = 0;          // > 0: the fused statistics pooling is taken (chains: always), at most this many segments per block
  int min_len = 0;             // chains: the batch's shortest segment in frames
  bool chain() const { return path == TdnnPath::Chain16 || path == TdnnPath::ChainX || path == TdnnPath::ChainM; }
};

// The kernel of TDNN op k (p: its kernel parameters, fill_tdnn_params).  run_tdnn launches by it, and asks it in advance about the
// op that will read a layer's output (reader_takes_image), so the two always agree.
TdnnChoice choose_tdnn(const RunCtx &c, size_t k, const TdnnKernelParams &p) {
  const asv_net *net = c.net;
  const Op &op = net->ops[k];
  const TdnnRules &r = c.rules;
  const DomainPlan &fp = c.bp.dom[ASV_DOMAIN_FRAMES];
  const bool use_ref = (net->flags & ASV_FLAG_REF_KERNELS) != 0, small = (net->flags & ASV_FLAG_SMALL_TILES) != 0;
  const bool h16 = p.et != ET_F32;              // 16-bit rows (bf16 or half)
  TdnnChoice ch;
  // tdnn -> [1-tap]* -> 1-tap + pooling in one kernel, if the batch allows the fused pooling: at most 16 segments per block (a crowd of
  // tiny utterances takes the per-layer kernels and the separate pooling kernel)
  if (op.chain_last >= 0 && !use_ref && (h16 || net->x3()) && p.halo <= kHalo && !small &&
      (net->x3() || (unsigned long long)p.rows * (unsigned long long)p.ldx * 2ull < (1ull << 32))) {
    if (net->x3()) {
      // f32x: the split-product chain on 64-row tiles; f32m: the chain with its correction products on the scaled 8-bit instruction, when
      // every layer of it has 8-bit fragments - in 64-frame tiles too
      bool mx = net->x3_mx();
      for (size_t j = k; j <= (size_t)op.chain_last && mx; ++j) mx = (net->ops[j].wfrag_fold != nullptr ? net->ops[j].w8_fold : net->ops[j].w8) != nullptr;
      ch.path = mx ? TdnnPath::ChainM : TdnnPath::ChainX;
      ch.n_blocks = p.rows >> 6;
      ch.pool_slots = max_segments_per_block(fp, ch.n_blocks, [](int row) { return row >> 6; });
    } else {
      // the 16-bit chain runs batches of less than one round of workgroups in 96- / 64-frame tiles (ChainTilePlan); developer runs with
      // phase stamps keep 128-frame tiles throughout
      ch.path = TdnnPath::Chain16;
      ch.plan = chain_tile_plan(p.rows, r.chain_dbg == 0);
      ch.n_blocks = ch.plan.tiles();
      ch.pool_slots = max_segments_per_block(fp, ch.n_blocks, [&](int row) { return ch.plan.tile_of(row); });
    }
    if (ch.pool_slots <= 16) {
      ch.min_len = 1 << 30;
      for (int32_t len : fp.seg_len) ch.min_len = std::min(ch.min_len, (int)len);
      return ch;
    }
    ch = TdnnChoice();
  }
  // fused statistics pooling: needs few enough segments per 128-row half-tile (i.e. no tiny utterances)
  int slots = 0;
  if (op.fused_pool >= 0 && !use_ref && !small) {
    slots = max_segments_per_block(fp, fp.rows_pad / 128, [](int row) { return row >> 7; });
    if (slots > 16) slots = 0;                  // many tiny utterances: use the separate pooling kernel
  }
  const bool big3 = !use_ref && p.halo <= kHalo && !small && tdnn_big3_supported(p, p.et, !h16);
  const bool x3 = !use_ref && !op.utts && net->x3() && !small && tdnn_x3_supported(p);
  const bool fuse = slots > 0 && (big3 || (x3 && tdnn_x3_pool_supported(p)));
  if (fuse) ch.pool_slots = slots;
  const long long tiles256 = (long long)(p.rows / 256) * (round_up(p.cout_store, 256) / 256);
  // Round 5: the layers of the variant-3 kernel with the plain epilogue, whole 64-channel chunks and at least one round of 256 x 256
  // tiles on the chip's CUs go to the 8-phase kernel (kernels_tdnn_p8.hip: both operands through LDS-DMA, staggered wave rows;
  // bit-identical outputs, 1.03 - 1.15 x the rate: profiles/r5e_p8_shapes.txt).  ASV_AMD_P8=0: the variant-3 kernel everywhere.
  const bool p8 = big3 && !fuse && r.p8 != 0 && tdnn_p8_supported(p, p.et, !h16) && tiles256 >= (r.p8 > 1 ? r.p8 : r.cus);
  // f32x: the 8-phase three-product kernel takes the wide plain layers that fill whole rounds of 256 x 256 tiles (kernels_tdnn_p8x.hip; the
  // bits of tdnn_gemm_x3_kernel; ASV_AMD_P8X=0: off).  Production rule: at least one round of tiles AND a last round that is >= 85 % full -
  // the x-vector's tdnn2 at 256 utterances is 408 tiles = 1.6 rounds, where the finer 128-row tiles of tdnn_gemm_x3_kernel are as fast and
  // leave CUs to the other stream: -0.9 % on two streams, profiles/r5s_p8x_model_ab.txt; ECAPA's layers are 4.75 and 7.1 rounds
  const bool p8x = x3 && !fuse && r.p8x != 0 && tdnn_p8x_supported(p) &&
                   (r.p8x > 1 ? tiles256 >= r.p8x : (tiles256 >= r.cus && tiles256 * 100 >= ((tiles256 + r.cus - 1) / r.cus) * r.cus * 85));
  // f32m: the 128-row kernel with its correction products on the scaled 8-bit instruction, where the three-product kernel would take its
  // 128-row tiles (ASV_AMD_X3M=0: off) and the 8-phase kernel does not (its fill rule: the x-vector's tdnn1 / tdnn2 - 163 us here against
  // 227 on the three-product kernel, profiles/r6f_*).  ECAPA's wide 1-tap layers stay on the 8-phase kernel: a new window (barrier +
  // conversion) per 32 channels makes this kernel only 4 - 12 % faster there on one stream and 8 % slower in the two-stream pipeline
  // (35.1 k against 38.2 k utterances/s, profiles/r6q_bench_line.json)
  const bool x3m = x3 && !fuse && !p8x && r.x3m != 0 && net->x3_mx() && tdnn_x3m_supported(p) &&
                   (long long)(p.rows / 128) * (round_up(p.cout_store, 256) / 256) >= (r.x3m > 1 ? r.x3m : 384);      // (384: where the three-product kernel takes its 128-row tiles)
  const bool grid = !use_ref && net->domains[net->bufs[op.tdnn.in_buf].domain].kind == 2 && !small;
  if (use_ref) ch.path = TdnnPath::Ref;
  else if (op.utts) ch.path = TdnnPath::Utts;
  else if (grid && grid_conv_narrow_supported(p, p.et)) ch.path = TdnnPath::ConvNarrow;
  else if (grid && grid_conv_wide_supported(p, p.et)) ch.path = TdnnPath::ConvWide;
  else if (grid && grid_conv_s2d_supported(p, p.et)) ch.path = TdnnPath::ConvS2d;
  else if (grid && grid_conv_c1_supported(p, p.et, op.tdnn.in_ch)) ch.path = TdnnPath::ConvC1;
  else if (x3m) ch.path = TdnnPath::X3m;
  else if (p8x) ch.path = TdnnPath::P8x;
  else if (x3) ch.path = TdnnPath::X3;
  else if (net->x3() && !small && grid_conv_x3_supported(p)) ch.path = TdnnPath::ConvX3;
  else if (p8) ch.path = TdnnPath::P8;
  else if (big3) ch.path = TdnnPath::Big3;
  return ch;
}

// the kernel parameters of TDNN op k (views, weights, taps)
void fill_tdnn_params(RunCtx &c, size_t k, TdnnKernelParams &p) {
  asv_net *net = c.net;
  const Op &op = net->ops[k];
  const auto &d = op.tdnn;
  const int domid = net->bufs[d.in_buf].domain;
  const DomainRun &dr = c.dom[domid];
  memset(&p, 0, sizeof(p));
  p.et = net->dom_et(domid); p.x3_et = net->x3_et(); p.x3_terms = net->x3_terms(); p.w_unscale = 1.0f / op.w_scale;
  p.x3_tile = (net->flags & ASV_FLAG_X3_TILE128) ? 128 : 0;
  p.status = status_word(net);
  view(c, d.in_buf, d.in_ch_off).to(p.x, p.ldx);
  if (d.in2_buf >= 0) view(c, d.in2_buf, d.in2_ch_off).to(p.x2, p.ldx2);
  p.w = op.w; p.bias = op.bias; p.scale = op.scale; p.shift = op.shift;
  if (d.seg_bias_buf >= 0) view(c, d.seg_bias_buf).to(p.seg_bias, p.ld_segbias);
  if (d.seg_scale_buf >= 0) view(c, d.seg_scale_buf).to(p.seg_scale, p.ld_segscale);
  if (d.res_buf >= 0) view(c, d.res_buf, d.res_ch_off).to(p.res, p.ldres);
  view(c, d.out_buf, d.out_ch_off).to(p.y, p.ldy);
  p.row_seg = dr.row_seg; p.row_valid = dr.row_valid; p.rows = dr.rows_pad;
  p.cin_pad = op.cin_pad; p.cout_store = op.cout_store;
  p.n_taps = d.n_taps;
  for (int t = 0; t < d.n_taps; ++t) { p.taps[t] = d.taps[t]; p.halo = std::max(p.halo, std::abs(d.taps[t])); }
  p.act1 = d.act1; p.act2 = d.act2; p.affine_first = d.affine_first;
  p.zero16 = net->zero_page;
  p.wfrag = op.wfrag; p.wlo = op.wlo; p.wconv = op.wconv; p.wx3p = op.wx3p; p.w8 = op.w8;
}

// f32m, op j reads ONE buffer as its input rows (Op::image_reader of the producer): will it, in THIS run, go to a kernel that reads images?
bool reader_takes_image(RunCtx &c, size_t j) {
  TdnnKernelParams q;
  fill_tdnn_params(c, j, q);
  const TdnnChoice r = choose_tdnn(c, j, q);
  return (r.path == TdnnPath::ChainM && q.cin_pad % 32 == 0) ||
         (r.path == TdnnPath::X3m && c.net->ops[j].fused_pool < 0 && tdnn_x3m_image_in_supported(q));
}

// The second half of a fused statistics pooling (pool op `pool_op`): adds each segment's partial moments in row order, adds the BN
// shift back to the mean and writes mean || std.  Chain kernels: partials [block][slot][lh][3][ld] (lh_split 1) in 2^tile_shift-row blocks,
// then the tail blocks of `plan`; per-layer kernels: [128-row tile][slot][3][ld] (lh_split 0, tile_shift 7, an empty plan).
int finish_fused_pool(RunCtx &c, Prof &prof, int pool_op, const DomainRun &dr, const float *partial, int ld_partial, int slots, int lh_split,
                      int tile_shift, const ChainTilePlan &plan, const float *shift) {
  const auto &q = c.net->ops[pool_op].pool;
  PoolFinishParams f;
  f.partial = partial; f.ld_partial = ld_partial; f.pool_slots = slots; f.lh_split = lh_split; f.tile_shift = tile_shift;
  f.rows_shift = plan.rows128(); f.tail_rows = plan.n_tail > 0 ? plan.tail_rows : 0; f.n_shift = plan.n128;
  f.row_seg = dr.row_seg; f.rows = dr.rows_pad; f.seg_row0 = dr.seg_row0; f.seg_len = dr.seg_len; f.shift = shift;
  view(c, q.out_buf, q.out_ch_off).to(f.out, f.ld_out); f.channels = q.channels;
  f.stddev = q.stddev; f.unbiased = q.unbiased; f.var_mode = q.var_mode; f.eps = q.eps;
  return timed(prof, K_POOL, 0, pool_op, 0, [&] { return launch_pool_finish(f, c.bp.segments, c.s); });
}

// one layer of a chain, as its kernel takes it: a layer whose consumer holds folded weights (wfrag_fold) stores ReLU(acc) only - its
// scale / shift are not passed
TdnnChainLayer chain_layer(const asv_net *net, size_t k, size_t last) {
  const Op &o = net->ops[k];
  const bool folded_in = o.wfrag_fold != nullptr;                                  // the previous layer's BN sits in these weights
  const bool folded_out = k < last && net->ops[k + 1].wfrag_fold != nullptr;       // this layer's BN sits in the next layer's
  TdnnChainLayer L;
  L.wfrag = folded_in ? o.wfrag_fold : o.wfrag; L.bias = folded_in ? o.bias_fold : o.bias;
  L.wlo = folded_in ? o.wlo_fold : o.wlo; L.w_scale = folded_in ? o.w_scale_fold : o.w_scale;
  L.w8 = folded_in ? o.w8_fold : o.w8;
  L.scale = folded_out ? nullptr : o.scale; L.shift = folded_out ? nullptr : o.shift;
  L.relu = o.tdnn.act1 == ASV_ACT_RELU; L.cout_pad = o.cout_pad;
  return L;
}

// ops i .. chain_last and the statistics pooling behind them as one chain kernel (p: op i's parameters) + the pooling's second half
int run_tdnn_chain(RunCtx &c, Prof &prof, size_t i, const TdnnKernelParams &p, const TdnnChoice &ch) {
  asv_net *net = c.net;
  ASV_REQUIRE(!p.x_image || ch.path == TdnnPath::ChainM, "tdnn(chain): image rows reached a chain kernel that cannot read them (internal)");
  const size_t l = (size_t)net->ops[i].chain_last;
  const Op &lo = net->ops[l];
  const DomainRun &dr = c.dom[ASV_DOMAIN_FRAMES];
  int rc;
  TdnnChainParams cp;
  memset(&cp, 0, sizeof(cp));
  cp.x = p.x; cp.ldx = p.ldx; cp.rows = p.rows; cp.cin_pad = p.cin_pad; cp.n_taps = p.n_taps;
  for (int t = 0; t < p.n_taps; ++t) cp.taps[t] = p.taps[t];
  cp.first = chain_layer(net, i, l);
  cp.n_mid = (int)(l - i - 1);
  for (size_t k = i + 1; k < l; ++k) cp.mid[k - i - 1] = chain_layer(net, k, l);
  cp.last = chain_layer(net, l, l);
  cp.pool_slots = ch.pool_slots; cp.ld_partial = lo.cout_pad; cp.row_seg = dr.row_seg;
  cp.et = ch.path == TdnnPath::Chain16 ? p.et : net->x3_et();
  cp.min_seg_len = ch.min_len;
  cp.status = status_word(net);
  cp.x_image = p.x_image ? 1 : 0;
#ifdef ASV_WITH_ABLATION
  // developer build only: ASV_AMD_CHAINM_GROUP=0 reads image rows under the per-chunk protocol of the f32 rows (a measuring aid,
  // same results); ASV_AMD_CHAINM_ABL sets the f32m chain's ablation bits (TdnnChainParams::abl), the garbage-result ones only under
  // ASV_AMD_CHAIN_DBG
  static const bool chainm_group_off = getenv("ASV_AMD_CHAINM_GROUP") != nullptr && atoi(getenv("ASV_AMD_CHAINM_GROUP")) == 0;
  if (cp.x_image && chainm_group_off) cp.x_image = 2;
  static const int chainm_abl = getenv("ASV_AMD_CHAINM_ABL") != nullptr ? atoi(getenv("ASV_AMD_CHAINM_ABL")) : 0;       // read once
  cp.abl = (chainm_abl & ~8) != 0 && getenv("ASV_AMD_CHAIN_DBG") == nullptr ? (chainm_abl & 8) : chainm_abl;
#endif
  cp.n128 = ch.plan.n128; cp.n_tail = ch.plan.n_tail; cp.tail_rows = ch.plan.tail_rows;
  if ((rc = ensure(net->poolpart_dev, (size_t)ch.n_blocks * ch.pool_slots * 2 * 3 * cp.ld_partial * 4, c.s, false))) return rc;
  cp.pool_partial = reinterpret_cast<float *>(net->poolpart_dev.ptr);
  double fl = 0.0;
  for (size_t k = i; k <= l; ++k) fl += 2.0 * (double)c.bp.frames * net->ops[k].tdnn.in_ch * net->ops[k].tdnn.out_ch * net->ops[k].tdnn.n_taps;
  // developer aid (ASV_AMD_CHAIN_DBG): phase stamps of the 16-bit and the f32m chain, one block of 8 x 32 per workgroup
  const bool stamps = c.rules.chain_dbg != 0 && ch.path != TdnnPath::ChainX;
  const size_t n_wgs = (size_t)(p.rows / (ch.path == TdnnPath::ChainM ? 64 : 128));
  DevMem dbg;
  if (stamps) {
    if ((rc = ensure(dbg, n_wgs * 8 * 32 * 8, c.s, true))) return rc;
    cp.dbg = reinterpret_cast<unsigned long long *>(dbg.ptr);
    cp.dbg_fine = c.rules.chain_dbg >= 3;
  }
  rc = timed(prof, K_TDNN, fl, (int)i, ch.path == TdnnPath::ChainM ? ASV_KERNEL_TDNN_CHAINM : 0, [&] {
    return ch.path == TdnnPath::ChainM ? launch_tdnn_chainm(cp, c.s) : (ch.path == TdnnPath::ChainX ? launch_tdnn_chainx(cp, c.s) : launch_tdnn_chain(cp, c.s));
  });
  if (rc) return rc;
  if (stamps && (rc = report_chain_stamps(dbg.ptr, n_wgs, c.rules.chain_dbg, ch.path == TdnnPath::ChainM, c.s))) return rc;
  net->ops[lo.fused_pool].skipped = true;
  return finish_fused_pool(c, prof, lo.fused_pool, dr, cp.pool_partial, cp.ld_partial, ch.pool_slots, 1, ch.path == TdnnPath::Chain16 ? 7 : 6, ch.plan, lo.shift);
}

// the per-layer kernel of `path`.  *count_id: its asv_kernel_launch_count id (stays 0 where the kernel has none)
int launch_tdnn_path(TdnnPath path, const TdnnKernelParams &p, int segments, bool utts_split, hipStream_t s, int *count_id) {
  switch (path) {
    case TdnnPath::Ref: return launch_tdnn_ref(p, p.et, p.et == ET_F32, s);
    // pooled-domain layers: split-bf16 products (f32-grade to ~2^-17, twice the rate of the f32-input MFMA) in the 16-bit
    // throughput modes; the exact f32-input MFMA in the parity modes - with IEEE-half operand halves in the frame layers
    // the bf16 split here would be the largest error left in the f32x mode (< 0.3 % of the FLOPs: +1 % of an f32x step)
    case TdnnPath::Utts: return launch_utts_gemm(p, segments, utts_split, s);
    case TdnnPath::ConvNarrow: {
      bool persistent = false;
      const int rc = launch_grid_conv_narrow(p, s, &persistent);
      *count_id = persistent ? ASV_KERNEL_CONV_NARROW_PERS : ASV_KERNEL_CONV_NARROW;
      return rc;
    }
    case TdnnPath::ConvWide: *count_id = ASV_KERNEL_CONV_WIDE; return launch_grid_conv_wide(p, s);
    case TdnnPath::ConvS2d: *count_id = ASV_KERNEL_CONV_S2D; return launch_grid_conv_s2d(p, s);
    case TdnnPath::ConvC1: *count_id = ASV_KERNEL_CONV_C1; return launch_grid_conv_c1(p, s);
    case TdnnPath::X3m: *count_id = ASV_KERNEL_TDNN_X3M; return launch_tdnn_x3m(p, s);
    case TdnnPath::P8x: *count_id = ASV_KERNEL_TDNN_P8X; return launch_tdnn_p8x(p, s);
    case TdnnPath::X3: return launch_tdnn_x3(p, s);
    case TdnnPath::ConvX3: return launch_grid_conv_x3(p, s);
    case TdnnPath::P8: *count_id = ASV_KERNEL_TDNN_P8; return launch_tdnn_p8(p, s);
    case TdnnPath::Big3: *count_id = ASV_KERNEL_TDNN_BIG3; return launch_tdnn_big3(p, s);
    default: return launch_tdnn_mfma(p, p.et, p.et == ET_F32, s);              // TdnnPath::Mfma (the chains: run_tdnn_chain)
  }
}

// op i as one per-layer kernel (p: its parameters), with the fused statistics pooling's second half where the choice took it
int run_tdnn_layer(RunCtx &c, Prof &prof, size_t i, TdnnKernelParams &p, const TdnnChoice &ch) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.tdnn;
  const int domid = net->bufs[d.in_buf].domain;
  int rc;
  const double flops = 2.0 * valid_positions(c, domid) * d.in_ch * d.out_ch * d.n_taps * (d.alg_fraction > 0.0f ? (double)d.alg_fraction : 1.0);
  if ((rc = prof.begin(op.utts ? K_UTTS : K_TDNN, flops, (int)i))) return rc;
  if (ch.pool_slots > 0) {
    p.pool_slots = ch.pool_slots;
    p.ld_partial = op.cout_pad;
    if ((rc = ensure(net->poolpart_dev, (size_t)(p.rows / 128) * ch.pool_slots * 3 * p.ld_partial * 4, c.s, false))) return rc;
    p.pool_partial = reinterpret_cast<float *>(net->poolpart_dev.ptr);
  }
  ASV_REQUIRE(!p.x_image || (ch.path == TdnnPath::X3m && tdnn_x3m_image_in_supported(p)), "tdnn: image rows reached a kernel that cannot read them (internal)");
  // f32m: the output rows as images, when their one reader will take them as such in this run (Op::image_reader; ASV_AMD_X3M_IMAGE=0: off)
  if (ch.path == TdnnPath::X3m && c.rules.x3m_image != 0 && op.image_reader >= 0 && (size_t)op.image_reader < c.n_ops && tdnn_x3m_image_out_supported(p) &&
      reader_takes_image(c, (size_t)op.image_reader)) {
    p.y_image = 1;
    c.buf_image[d.out_buf] = 1;
    ++g_kernel_launches[ASV_KERNEL_TDNN_X3M_IMAGE];
  }
  // last layer, every utterance a single chunk: the pooled-domain kernel also produces the caller's [utterance][embed_dim] result
  if (ch.path == TdnnPath::Utts && c.final_out != nullptr && i + 1 == net->ops.size() && d.out_buf == net->out_buf && d.out_ch_off == 0 &&
      d.out_ch == net->embed_dim && c.bp.segments == c.bp.n_utts) {
    p.final_out = c.final_out; p.final_ld = net->embed_dim; p.final_len = c.seg_frames;
    c.final_written = true;
  }
  int count_id = 0;
  rc = launch_tdnn_path(ch.path, p, c.bp.segments, net->frames_h16(), c.s, &count_id);
  if (count_id > 0) ++g_kernel_launches[count_id];
  if (rc || (rc = prof.end())) return rc;
  if (op.fused_pool >= 0) net->ops[op.fused_pool].skipped = ch.pool_slots > 0;
  if (ch.pool_slots == 0) return ASV_OK;
  return finish_fused_pool(c, prof, op.fused_pool, c.dom[domid], p.pool_partial, p.ld_partial, ch.pool_slots, 0, 7, ChainTilePlan(), op.shift);
}

// ---- one run function per op kind (run_ops dispatches)

// i: in, the op; out, the last op the launch covered (a chain runs its other layers inside the kernel)
int run_tdnn(RunCtx &c, Prof &prof, size_t &i) {
  const Op &op = c.net->ops[i];
  TdnnKernelParams p;
  fill_tdnn_params(c, i, p);
  p.x_image = c.buf_image[op.tdnn.in_buf];
  const TdnnChoice ch = choose_tdnn(c, i, p);
  if (!ch.chain()) return run_tdnn_layer(c, prof, i, p, ch);
  const size_t head = i;
  i = (size_t)op.chain_last;
  return run_tdnn_chain(c, prof, head, p, ch);
}

int run_pool(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  if (net->ops[i].skipped) return ASV_OK;      // folded into the producing layer's epilogue
  const auto &d = net->ops[i].pool;
  const int domid = net->bufs[d.in_buf].domain;
  const Domain &dm = net->domains[domid];
  PoolKernelParams p;
  view(c, d.in_buf, d.in_ch_off).to(p.x, p.ldx); p.channels = d.channels;
  p.seg_row0 = c.dom[domid].seg_row0; p.seg_len = c.dom[domid].seg_len;
  view(c, d.out_buf, d.out_ch_off).to(p.out, p.ld_out);
  p.stddev = d.stddev; p.unbiased = d.unbiased; p.var_mode = d.var_mode; p.eps = d.eps;
  p.row_stride = d.per_bin ? dm.pitch : 1;
  p.groups = d.per_bin ? dm.width : 1;
  p.chunk_partial = nullptr; p.chunks = 0; p.ld_chunk = 0;
  if (!d.stddev && !d.per_bin && dm.kind == 2 && dm.pitch >= 32 && (net->flags & ASV_FLAG_NO_FUSE) == 0) {      // (narrow maps: the second launch costs more than it saves)
    // mean over a 2-D map (SE squeeze): long segments, few of them - kPoolChunkRows rows per workgroup + a finish kernel
    int max_len = 0;
    for (int32_t len : c.bp.dom[domid].seg_len) max_len = std::max(max_len, (int)len);
    const int chunks = (max_len + kPoolChunkRows - 1) / kPoolChunkRows;
    if (chunks >= 1) {                                       // always this form for these ops: the arithmetic must not depend on the batch
      p.chunks = chunks; p.ld_chunk = round_up(d.channels, 64);
      if (int rc = ensure(net->poolpart_dev, (size_t)c.bp.segments * chunks * p.ld_chunk * 4, c.s, false)) return rc;
      p.chunk_partial = reinterpret_cast<float *>(net->poolpart_dev.ptr);
    }
  }
  return timed(prof, K_POOL, 0, (int)i, 0, [&] { return launch_stats_pool(p, c.bp.segments, net->dom_et(domid), c.s); });
}

int run_attpool(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.att;
  const DomainRun &dr = c.dom[net->bufs[d.x_buf].domain];          // the frames domain, or a sequence domain behind the 2-D trunk
  const int group = d.logit_group > 1 ? d.logit_group : (d.shared_logits ? d.channels : 1);
  const View x = view(c, d.x_buf, d.x_ch_off), logits = view(c, d.logit_buf, d.logit_ch_off), out = view(c, d.out_buf, d.out_ch_off);
  return timed(prof, K_ATT, 0, (int)i, 0, [&] {
    return launch_attentive_pool(x.p, x.ld, logits.p, logits.ld, d.channels, dr.seg_row0, dr.seg_len, c.bp.segments, d.eps, reinterpret_cast<float *>(out.p), out.ld,
                                 net->frames_et(), group, d.logit_softplus2 != 0, op.scale, op.shift, c.s);
  });
}

int run_mq_attpool(RunCtx &c, Prof &prof, size_t i) {
  const auto &d = c.net->ops[i].mq;
  const DomainRun &dr = c.dom[c.net->bufs[d.x_buf].domain];
  MqPoolKernelParams p;
  view(c, d.x_buf, d.x_ch_off).to(p.x, p.ldx);
  view(c, d.logit_buf, d.logit_ch_off).to(p.logits, p.ldl);
  p.channels = d.channels; p.head_ch = d.channels / d.heads;
  p.seg_row0 = dr.seg_row0; p.seg_len = dr.seg_len; p.eps = d.eps;
  view(c, d.out_buf, d.out_ch_off).to(p.out, p.ld_out);
  p.pair_stride = d.pair_stride; p.std_off = d.std_off;
  return timed(prof, K_ATT, 0, (int)i, ASV_KERNEL_MQ_ATTPOOL,
               [&] { return launch_mq_attentive_pool(p, d.queries, d.shared_logits != 0, c.bp.segments, c.net->frames_et(), c.s); });
}

int run_lde(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.lde;
  const DomainRun &dr = c.dom[net->bufs[d.x_buf].domain];
  if (int rc = ensure(net->lde_dev, (size_t)dr.rows_pad * 64 * 4, c.s, false)) return rc;
  const View x = view(c, d.x_buf, d.x_ch_off), out = view(c, d.out_buf, d.out_ch_off);
  return timed(prof, K_ATT, 0, (int)i, 0, [&] {
    return launch_lde_pool(x.p, x.ld, d.channels, dr.rows_pad, op.scale, op.shift, d.n_centres, reinterpret_cast<float *>(net->lde_dev.ptr), dr.seg_row0, dr.seg_len,
                           c.bp.segments, reinterpret_cast<float *>(out.p), out.ld, net->frames_et(), c.s);
  });
}

int run_eltwise(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.elt;
  const int domid = net->bufs[d.a_buf].domain;
  EltwiseKernelParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.a_buf, d.a_ch_off).to(p.a, p.lda);
  if (d.b_buf >= 0) view(c, d.b_buf, d.b_ch_off).to(p.b, p.ldb);
  if (d.c_buf >= 0) view(c, d.c_buf, d.c_ch_off).to(p.c, p.ldc);
  view(c, d.out_buf, d.out_ch_off).to(p.out, p.ldo);
  p.channels = d.channels; p.scale = op.scale; p.shift = op.shift; p.act = d.act;
  if (d.seg_scale_buf >= 0) view(c, d.seg_scale_buf).to(p.seg_scale, p.ld_segscale);
  if (d.seg_norm_buf >= 0) { view(c, d.seg_norm_buf).to(p.seg_norm, p.ld_segnorm); p.seg_norm_mode = d.seg_norm_mode; }
  if (d.out2_buf >= 0) {
    view(c, d.d_buf, d.d_ch_off).to(p.d, p.ldd);
    view(c, d.out2_buf, d.out2_ch_off).to(p.out2, p.ldo2);
  }
  if (op.utts) { p.rows = c.bp.segments; }
  else { p.rows = c.dom[domid].rows_pad; p.row_seg = c.dom[domid].row_seg; p.row_valid = c.dom[domid].row_valid; }
  return timed(prof, K_ELT, 0, (int)i, 0, [&] { return launch_eltwise(p, net->dom_et(domid), c.s); });
}

int run_rowop(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.rop;
  const int domid = net->bufs[d.in_buf].domain;
  ASV_REQUIRE(!c.buf_image[d.in_buf], "rowop: image rows reached the row op (internal)");
  RowopKernelParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf, d.in_ch_off).to(p.in, p.ldi);
  view(c, d.out_buf, d.out_ch_off).to(p.out, p.ldo);
  p.channels = d.channels; p.scale0 = op.rop_tab[0]; p.shift0 = op.rop_tab[1]; p.gamma = op.rop_tab[2]; p.beta = op.rop_tab[3]; p.scale1 = op.rop_tab[4]; p.shift1 = op.rop_tab[5];
  p.act0 = d.act0; p.act1 = d.act1; p.ln = d.ln; p.slope0 = d.slope0; p.slope1 = d.slope1; p.eps = d.eps;
  if (op.utts) { p.rows = c.bp.segments; }
  else { p.rows = c.dom[domid].rows_pad; p.row_valid = c.dom[domid].row_valid; }
  return timed(prof, K_ROWOP, 0, (int)i, ASV_KERNEL_ROWOP, [&] { return launch_rowop(p, net->dom_et(domid), c.s); });
}

int run_grid_conv(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.gconv;
  const int domid = net->bufs[d.in_buf].domain;
  const Domain &dm = net->domains[domid];
  const DomainRun &dr = c.dom[domid];
  ASV_REQUIRE(!c.buf_image[d.in_buf], "grid_conv: image rows reached the grid convolution (internal)");
  ConvTapsParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf, d.in_ch_off).to(p.x, p.ldx);
  view(c, d.out_buf, d.out_ch_off).to(p.y, p.ldy);
  p.w = op.wconv; p.bias = op.bias; p.row_valid = dr.row_valid; p.zero16 = net->zero_page;
  p.rows = dr.rows_pad; p.cin_pad = op.cin_pad; p.cout_store = op.cout_store; p.nf_total = op.cout_pad / 32;
  p.n_taps = d.n_taps; p.relu = d.act == ASV_ACT_RELU;
  int halo = 0;
  for (int t = 0; t < d.n_taps; ++t) { p.off[t] = d.dt[t] * dm.pitch + d.df[t]; halo = std::max(halo, std::abs(p.off[t])); }
  ASV_REQUIRE(halo <= dm.conv_halo() && halo <= dm.gap(), "grid_conv: tap offset %d beyond the grid's %d zero rows (internal)", halo, dm.conv_halo());
  p.halo_pad = round_up(halo, 8);
  return timed(prof, K_CONV_TAPS, 2.0 * valid_positions(c, domid) * d.in_ch * d.out_ch * d.n_taps, (int)i, ASV_KERNEL_CONV_TAPS,
               [&] { return launch_grid_conv_taps(p, net->dom_et(domid), c.s); });
}

int run_attention(RunCtx &c, Prof &prof, size_t i) {
  const auto &d = c.net->ops[i].sa;
  const int domid = c.net->bufs[d.q_buf].domain;
  const DomainRun &dr = c.dom[domid];
  ASV_REQUIRE(!c.buf_image[d.q_buf] && !c.buf_image[d.k_buf] && !c.buf_image[d.v_buf], "self_attention: image rows reached the attention op (internal)");
  AttentionKernelParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.q_buf, d.q_ch_off).to(p.q, p.ldq);
  view(c, d.k_buf, d.k_ch_off).to(p.k, p.ldk);
  view(c, d.v_buf, d.v_ch_off).to(p.v, p.ldv);
  view(c, d.out_buf, d.out_ch_off).to(p.out, p.ldo);
  p.heads = d.heads; p.d_k = d.d_k; p.scale = 1.0f / std::sqrt((float)d.d_k);
  p.seg_row0 = dr.seg_row0; p.seg_len = dr.seg_len; p.segments = c.bp.segments; p.rows = dr.rows_pad;
  double pairs = 0;                             // (query, key) pairs of the batch
  for (int32_t len : c.bp.dom[domid].seg_len) { p.max_len = std::max(p.max_len, (int)len); pairs += (double)len * len; }
  return timed(prof, K_ATTENTION, 4.0 * pairs * d.heads * d.d_k, (int)i, ASV_KERNEL_ATTENTION, [&] { return launch_self_attention(p, c.net->dom_et(domid), c.s); });
}

int run_posenc(RunCtx &c, Prof &prof, size_t i) {
  const Op &op = c.net->ops[i]; const auto &d = op.pos;
  const int domid = c.net->bufs[d.in_buf].domain;
  const DomainRun &dr = c.dom[domid];
  ASV_REQUIRE(!c.buf_image[d.in_buf], "posenc: image rows reached the positional encoding (internal)");
  for (int32_t len : c.bp.dom[domid].seg_len)
    ASV_REQUIRE(len < d.pe_rows, "extract: a chunk of %d positions reaches the end of the positional-encoding table (%d rows; the reference asserts rows < max_len)", (int)len,
                d.pe_rows);
  PosencKernelParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf, d.in_ch_off).to(p.in, p.ldi);
  view(c, d.out_buf, d.out_ch_off).to(p.out, p.ldo);
  p.channels = d.channels; p.rows = dr.rows_pad; p.scale = d.scale;
  p.pe = op.scale; p.ld_pe = round_up(d.channels, kChanAlign);
  p.row_seg = dr.row_seg; p.seg_row0 = dr.seg_row0; p.row_valid = dr.row_valid;
  return timed(prof, K_POSENC, 0, (int)i, ASV_KERNEL_POSENC, [&] { return launch_posenc(p, c.net->dom_et(domid), c.s); });
}

int run_front_conv(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const Op &op = net->ops[i]; const auto &d = op.front;
  const int domid = net->bufs[d.out_buf].domain;
  const DomainRun &dg = c.dom[domid];
  FrontConvParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf).to(p.x, p.ldx);
  view(c, d.out_buf).to(p.out, p.ldo);
  p.channels = d.out_ch; p.rows = dg.rows_pad; p.pitch = net->domains[domid].pitch;
  p.w = op.scale; p.bias = op.bias;
  p.fr_row0 = c.dom[ASV_DOMAIN_FRAMES].seg_row0; p.g_row0 = dg.seg_row0; p.row_seg = dg.row_seg; p.row_valid = dg.row_valid;
  return timed(prof, K_FRONT_CONV, 2.0 * valid_positions(c, domid) * 9 * d.out_ch, (int)i, ASV_KERNEL_FRONT_CONV,
               [&] { return launch_front_conv(p, net->frames_et(), c.s); });
}

int run_res2(RunCtx &c, Prof &prof, size_t i) {
  const Op &op = c.net->ops[i]; const auto &d = op.res2;
  const DomainRun &dr = c.dom[ASV_DOMAIN_FRAMES];
  Res2KernelParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf, d.in_ch_off).to(p.x, p.ldx);
  view(c, d.out_buf, d.out_ch_off).to(p.y, p.ldy);
  p.rows = dr.rows_pad; p.wfrag = op.wfrag; p.bias = op.bias; p.scale = op.scale; p.shift = op.shift; p.row_valid = dr.row_valid;
  p.branches = d.branches; p.dilation = d.dilation; p.et = c.net->frames_et();
  static const bool res2_dbg = getenv("ASV_AMD_RES2_DBG") != nullptr;          // developer aid: phase durations to stderr
  DevMem dbg;
  int rc;
  if (res2_dbg) {
    if ((rc = ensure(dbg, (size_t)(p.rows / 128) * 8 * 16 * 8, c.s, true))) return rc;
    p.dbg = reinterpret_cast<unsigned long long *>(dbg.ptr);
  }
  rc = timed(prof, K_TDNN, 2.0 * (double)c.bp.frames * kRes2Width * kRes2Width * 3 * d.branches, (int)i, 0, [&] { return launch_res2_chain(p, c.s); });
  return rc || !res2_dbg ? rc : report_res2_stamps(dbg.ptr, (size_t)(p.rows / 128), c.s);
}

int run_res2n(RunCtx &c, Prof &prof, size_t i) {
  const Op &op = c.net->ops[i]; const auto &d = op.res2n;
  const DomainRun &dr = c.dom[ASV_DOMAIN_FRAMES];
  Res2nKernelParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf, d.in_ch_off).to(p.x, p.ldx);
  view(c, d.out_buf, d.out_ch_off).to(p.y, p.ldy);
  p.rows = dr.rows_pad; p.wfrag = op.wfrag; p.bias = op.bias; p.scale = op.scale; p.shift = op.shift; p.row_valid = dr.row_valid;
  p.branches = d.groups - 1; p.pass_group = d.pass_group; p.dilation = d.dilation; p.et = c.net->frames_et();
  return timed(prof, K_RES2N, 2.0 * (double)c.bp.frames * d.width * d.width * 3 * (d.groups - 1), (int)i, ASV_KERNEL_RES2N, [&] { return launch_res2n_chain(p, c.s); });
}

int run_grid_input(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const auto &d = net->ops[i].gin;
  const int domid = net->bufs[d.out_buf].domain;
  const DomainRun &dg = c.dom[domid];
  const View in = view(c, d.in_buf), out = view(c, d.out_buf);
  return timed(prof, K_GATHER, 0, (int)i, 0, [&] {
    return launch_grid_from_frames(in.p, in.ld, net->feat_dim, c.dom[ASV_DOMAIN_FRAMES].seg_row0, dg.seg_row0, dg.row_seg, dg.row_valid, dg.rows_pad,
                                   net->domains[domid].pitch, out.p, out.ld, net->frames_et(), c.s);
  });
}

int run_flatten(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const auto &d = net->ops[i].flat;
  const int din = net->bufs[d.in_buf].domain, dout = net->bufs[d.out_buf].domain;
  const View in = view(c, d.in_buf), out = view(c, d.out_buf);
  return timed(prof, K_GATHER, 0, (int)i, 0, [&] {
    return launch_grid_flatten(in.p, in.ld, net->bufs[d.in_buf].channels, net->domains[din].width, net->domains[din].pitch, c.dom[din].seg_row0, c.dom[dout].seg_row0,
                               c.dom[dout].row_seg, c.dom[dout].row_valid, c.dom[dout].rows_pad, out.p, out.ld, net->frames_et(), c.s);
  });
}

int run_im2col(RunCtx &c, Prof &prof, size_t i) {
  asv_net *net = c.net;
  const auto &d = net->ops[i].i2c;
  const int din = net->bufs[d.in_buf].domain, dout = net->bufs[d.out_buf].domain;
  Im2colParams p;
  memset(&p, 0, sizeof(p));
  view(c, d.in_buf).to(p.in, p.ldi);
  view(c, d.out_buf).to(p.out, p.ldo);
  p.channels = d.channels; p.n_taps = d.n_taps; p.stride = d.stride;
  for (int t = 0; t < d.n_taps; ++t) { p.dt[t] = d.dt[t]; p.df[t] = d.df[t]; }
  p.in_row0 = c.dom[din].seg_row0; p.in_len = c.dom[din].seg_len;
  p.out_row0 = c.dom[dout].seg_row0; p.out_row_seg = c.dom[dout].row_seg; p.out_row_valid = c.dom[dout].row_valid;
  p.in_pitch = net->domains[din].pitch; p.in_width = net->domains[din].width;
  p.out_pitch = net->domains[dout].pitch; p.out_rows = c.dom[dout].rows_pad;
  if (d.b_buf >= 0) view(c, d.b_buf).to(p.b, p.ldb);
  if (d.seg_scale_buf >= 0) view(c, d.seg_scale_buf).to(p.seg_scale, p.ld_segscale);
  p.act = d.act;
  return timed(prof, K_GATHER, 0, (int)i, 0, [&] { return launch_im2col(p, net->frames_et(), c.s); });
}

int run_ops(RunCtx &c, size_t n_ops) {
  Prof prof{c.net, c.s};
  c.n_ops = n_ops;
  c.buf_image.assign(c.net->bufs.size(), 0);
  c.rules = tdnn_rules();
  for (size_t i = 0; i < n_ops; ++i) {
    int rc = ASV_OK;
    switch (c.net->ops[i].kind) {
      case OP_TDNN: rc = run_tdnn(c, prof, i); break;                  // (a chain moves i to its last layer)
      case OP_POOL: rc = run_pool(c, prof, i); break;
      case OP_ATTPOOL: rc = run_attpool(c, prof, i); break;
      case OP_MQ_ATTPOOL: rc = run_mq_attpool(c, prof, i); break;
      case OP_LDE: rc = run_lde(c, prof, i); break;
      case OP_ELTWISE: rc = run_eltwise(c, prof, i); break;
      case OP_ROWOP: rc = run_rowop(c, prof, i); break;
      case OP_GRID_CONV: rc = run_grid_conv(c, prof, i); break;
      case OP_ATTENTION: rc = run_attention(c, prof, i); break;
      case OP_POSENC: rc = run_posenc(c, prof, i); break;
      case OP_FRONT_CONV: rc = run_front_conv(c, prof, i); break;
      case OP_RES2: rc = run_res2(c, prof, i); break;
      case OP_RES2N: rc = run_res2n(c, prof, i); break;
      case OP_GRID_INPUT: rc = run_grid_input(c, prof, i); break;
      case OP_FLATTEN: rc = run_flatten(c, prof, i); break;
      case OP_IM2COL: rc = run_im2col(c, prof, i); break;
    }
    if (rc) return rc;
  }
  return prof.close_span();
}

int pack_features(RunCtx &c, const float *feats) {
  Prof prof{c.net, c.s};
  const DomainRun &dr = c.dom[ASV_DOMAIN_FRAMES];
  return timed(prof, K_PACK, 0, -1, 0, [&] {
    return launch_pack_input(feats, c.net->feat_dim, c.seg_src0, dr.seg_row0, dr.row_seg, dr.rows_pad, c.net->arena[0].ptr, c.net->bufs[0].ld, c.net->frames_et(), c.s);
  });
}

// ---- the one-op forwards: a one-off net (never finalized) around the caller's rows

struct OneOffNet {
  asv_net_t *net = nullptr;
  ~OneOffNet() { asv_net_destroy(net); }
  int create(int precision, unsigned flags, int feat_dim) {
    int dev = 0;
    ASV_HIP_CHECK(hipGetDevice(&dev));
    return asv_net_create(&net, dev, precision, flags, feat_dim);
  }
};

// Runs the first n_ops ops of a one-off net on the rows x, every utterance one chunk, and copies the first `width` channels of buffer `buf`
// to the caller's y: one row per utterance (utts domain) or per frame, in the caller's order
int run_one_off(asv_net *net, const float *x, const int32_t *offsets, int n_utts, size_t n_ops, void *stream, int buf, int width, bool utts, float *y) {
  net->arena.resize(net->bufs.size());
  RunCtx c;
  c.net = net; c.s = reinterpret_cast<hipStream_t>(stream);
  int rc;
  if ((rc = prepare(c, offsets, n_utts, 1 << 30)) || (rc = pack_features(c, x)) || (rc = run_ops(c, n_ops))) return rc;
  if (utts) {
    ASV_HIP_CHECK(hipMemcpy2DAsync(y, (size_t)width * 4, net->arena[buf].ptr, (size_t)net->bufs[buf].ld * 4, (size_t)width * 4, n_utts, hipMemcpyDeviceToDevice, c.s));
  } else {
    const DomainRun &dr = c.dom[ASV_DOMAIN_FRAMES];
    if ((rc = launch_unpack_rows(net->arena[buf].ptr, net->bufs[buf].ld, width, c.seg_src0, dr.seg_row0, dr.row_seg, dr.rows_pad, y, net->frames_et(), c.s))) return rc;
  }
  ASV_HIP_CHECK(hipStreamSynchronize(c.s));
  return ASV_OK;
}

}  // namespace
}  // namespace asv

using namespace asv;

extern "C" {

unsigned long long asv_kernel_launch_count(int which) {
  return (which >= ASV_KERNEL_TDNN_P8 && which <= ASV_KERNEL_FRONT_CONV) ? g_kernel_launches[which].load() : 0ull;
}

int asv_net_extract(asv_net_t *net, const float *feats, const int32_t *offsets, int n_utts, float *out, int max_chunk, void *stream) {
  ASV_REQUIRE(net && net->finalized, "asv_net_extract: net is null or not finalized");
  ASV_REQUIRE(feats && out, "asv_net_extract: null feature or output pointer");
  ASV_ON_DEVICE(net->device);
  RunCtx c;
  c.net = net; c.s = reinterpret_cast<hipStream_t>(stream);
  int rc;
  if ((rc = prepare(c, offsets, n_utts, max_chunk)) || (rc = pack_features(c, feats))) return rc;
  c.final_out = out;
  if ((rc = run_ops(c, net->ops.size()))) return rc;
  if (c.final_written) return ASV_OK;               // the last layer wrote `out` itself (single-chunk utterances)
  Prof prof{net, c.s};
  return timed(prof, K_COMBINE, 0, -1, 0, [&] {
    return launch_combine(reinterpret_cast<const float *>(net->arena[net->out_buf].ptr), net->bufs[net->out_buf].ld, c.utt_seg0, c.utt_nseg, c.seg_frames, n_utts,
                          net->embed_dim, out, c.s);
  });
}

int asv_tdnn_forward(const asv_tdnn_desc_t *d, int precision, unsigned flags, const float *x, const int32_t *offsets, int n_utts, float *y, void *stream) {
  ASV_REQUIRE(d && x && y && offsets, "asv_tdnn_forward: null argument");
  OneOffNet one;
  int rc = one.create(precision, flags, d->in_ch);
  if (rc) return rc;
  const int ob = asv_net_new_buffer(one.net, ASV_DOMAIN_FRAMES, d->out_ch);
  if (ob < 0) return ob;
  asv_tdnn_desc_t dd = *d;
  dd.in_buf = 0; dd.in_ch_off = 0; dd.in2_buf = -1; dd.out_buf = ob; dd.out_ch_off = 0;
  dd.seg_bias_buf = -1; dd.seg_scale_buf = -1; dd.res_buf = -1;
  if ((rc = asv_net_add_tdnn(one.net, &dd))) return rc;
  return run_one_off(one.net, x, offsets, n_utts, 1, stream, ob, d->out_ch, false, y);
}

int asv_stats_pool_forward(const float *x, int channels, const int32_t *offsets, int n_utts, int stddev, int unbiased, int var_mode, float eps, float *y,
                           void *stream) {
  ASV_REQUIRE(x && y && offsets && channels >= 1, "asv_stats_pool_forward: bad argument");
  OneOffNet one;
  int rc = one.create(ASV_PREC_F32, 0, channels);
  if (rc) return rc;
  const int out_ch = channels * (stddev ? 2 : 1);
  const int ob = asv_net_new_buffer(one.net, ASV_DOMAIN_UTTS, out_ch);
  if (ob < 0) return ob;
  asv_pool_desc_t pd;
  memset(&pd, 0, sizeof(pd));
  pd.struct_size = sizeof(pd); pd.in_buf = 0; pd.channels = channels; pd.out_buf = ob; pd.stddev = stddev; pd.unbiased = unbiased; pd.var_mode = var_mode; pd.eps = eps;
  if ((rc = asv_net_add_stats_pool(one.net, &pd))) return rc;
  return run_one_off(one.net, x, offsets, n_utts, 1, stream, ob, out_ch, true, y);
}

int asv_rowop_forward(const asv_rowop_desc_t *d, int precision, int domain, int width, const float *x, const int32_t *offsets, int n_utts, float *y,
                      void *stream) {
  ASV_REQUIRE(d && x && y && offsets && width >= 1 && n_utts >= 1, "asv_rowop_forward: bad argument");
  ASV_REQUIRE(domain == ASV_DOMAIN_FRAMES || domain == ASV_DOMAIN_UTTS, "asv_rowop_forward: domain %d (frames or utts)", domain);
  const bool utts = domain == ASV_DOMAIN_UTTS;
  if (utts)
    for (int u = 0; u < n_utts; ++u) ASV_REQUIRE(offsets[u + 1] - offsets[u] == 1, "asv_rowop_forward: utts domain: utterance %d must be one frame long", u);
  OneOffNet one;
  int rc = one.create(precision, 0, width);
  if (rc) return rc;
  asv_net_t *net = one.net;
  // buffer 1 (and 2, unless the op runs in place) = the rows themselves: a copy in the frames domain, the mean of each one-frame
  // utterance - the frame, exactly - in the utts domain
  const int n_bufs = d->out_buf == 1 ? 1 : 2;
  for (int b = 1; b <= n_bufs; ++b) {
    const int id = asv_net_new_buffer(net, domain, width);
    if (id < 0) return id;
    if (utts) {
      asv_pool_desc_t pd;
      memset(&pd, 0, sizeof(pd));
      pd.struct_size = sizeof(pd); pd.in_buf = 0; pd.channels = width; pd.out_buf = id; pd.eps = 1e-10f;
      if ((rc = asv_net_add_stats_pool(net, &pd))) return rc;
    } else {
      asv_eltwise_desc_t ed;
      memset(&ed, 0, sizeof(ed));
      ed.struct_size = sizeof(ed); ed.channels = width; ed.a_buf = 0; ed.b_buf = ed.c_buf = ed.seg_scale_buf = ed.seg_norm_buf = ed.d_buf = ed.out2_buf = -1; ed.out_buf = id;
      if ((rc = asv_net_add_eltwise(net, &ed))) return rc;
    }
  }
  asv_rowop_desc_t dd = *d;
  dd.in_buf = 1; dd.out_buf = n_bufs;
  if ((rc = asv_net_add_rowop(net, &dd))) return rc;
  return run_one_off(net, x, offsets, n_utts, net->ops.size(), stream, n_bufs, width, utts, y);
}

}  // extern "C"
