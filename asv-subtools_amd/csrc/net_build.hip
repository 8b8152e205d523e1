// The layer-program builder of libasv_amd.so (asv_net_*): create / destroy, grids and buffers, one add function per op kind with its line
// of asv_net_describe next to it, asv_net_finalize (which ops fuse), status, device bytes and the profile read-out.
// (The weight layouts: weight_pack.cpp; the launch sequence of a batch: net_run.hip.)
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <map>

#include "net.h"
#include "weight_pack.h"

namespace asv {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

namespace {

int dev_upload(asv_net *net, const void *host, size_t bytes, void **out) {
  void *d = nullptr;
  ASV_HIP_CHECK(hipMalloc(&d, bytes));
  hipError_t e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    set_error("hipMemcpy H2D failed: %s", hipGetErrorString(e));
    return ASV_EHIP;
  }
  net->weight_allocs.push_back(d);
  net->weight_bytes += bytes;
  *out = d;
  return ASV_OK;
}

template <class T>
int upload_vec(asv_net *net, const std::vector<T> &v, void **out) { return dev_upload(net, v.data(), v.size() * sizeof(T), out); }

int upload_padded(asv_net *net, const float *src, int n, int n_pad, float fill, float **out) {
  std::vector<float> tmp((size_t)n_pad, fill);
  if (src) memcpy(tmp.data(), src, (size_t)n * sizeof(float));
  void *d = nullptr;
  int rc = upload_vec(net, tmp, &d);
  *out = reinterpret_cast<float *>(d);
  return rc;
}

// A layer's weights in the fragment forms the wide frame kernels and the layer chains read (kernels_tdnn_v3.hip order): the 16-bit
// fragments alone, or - with_lo, the f32x mode - the hi / lo halves of w * s.scale, and - with_mx8, the f32m form - their 8-bit planes
struct FragForms { std::vector<uint16_t> hi, lo; std::vector<uint8_t> w8; };
FragForms pack_frag_forms(const TapWeights &s, int cout_pad, int cin_pad, int et, bool with_lo, bool with_mx8) {
  FragForms f;
  f.hi.resize(tdnn_weight_frag_elems(cout_pad, cin_pad, s.n_taps));
  f.lo.resize(with_lo ? f.hi.size() : 0);
  pack_tdnn_weight_frags(s.w, s.out_ch, s.in_ch, s.tot_ctx, s.left_ctx, s.taps, s.n_taps, cout_pad, cin_pad, f.hi.data(), with_lo ? f.lo.data() : nullptr, et, s.scale);
  if (with_mx8) f.w8 = pack_tdnn_weight_mx8(s, cout_pad, cin_pad);
  return f;
}

// Which weight layouts a TDNN layer gets, besides the plain order every layer has (asv_net_add_tdnn packs and uploads one per field).
struct TdnnPacks { bool frags16, x3_frags, mx8, x3p, conv2d, conv2d_x3, utts_split, chain_host_copies; };
TdnnPacks tdnn_packs_for(const asv_net *net, const asv_tdnn_desc_t &d, int dom, const Op &op) {
  const int kind = net->domains[dom].kind;
  const bool h16 = net->dom_et(dom) != ET_F32;     // 16-bit rows and weights (bf16 or half)
  TdnnPacks n;
  // the two fragment orders are mutually exclusive per layer: a 3x3 trunk convolution the conv2d kernels take never needs
  // the v3 order (grid_conv_* precede big3 in the dispatch and accept every such layer), and each family has its own pointer
  // (+ the 32 -> 64 stride-2 convolution in space-to-depth form: 4 x 32 input channels, 4 taps, 64 output channels)
  const bool s2d = h16 && kind == 2 && d.n_taps == 4 && op.cin_pad == 128 && d.in_ch == 128 && d.out_ch == 64;
  // 3x3 trunk convolutions with 32 / 64 / 128 / 256 channels: fragment order of kernels_conv2d.hip
  n.conv2d = s2d || (h16 && kind == 2 && d.n_taps == 9 && (op.cin_pad == 32 || op.cin_pad == 64 || op.cin_pad == 128 || op.cin_pad == 256) &&
                     d.in_ch == op.cin_pad && d.out_ch == d.in_ch);
  n.frags16 = h16 && !n.conv2d && op.cout_store > 96 && op.cin_pad >= 64;         // candidates of the 256- / 128-channel tiles (kernels_tdnn_v3.hip)
  // f32x mode: hi / lo halves of the weights in the same fragment order (kernels_tdnn_x3.hip)
  n.x3_frags = net->x3() && !op.utts && kind == ASV_DOMAIN_FRAMES && op.cout_store >= 192 && op.cin_pad >= 32;
  n.mx8 = n.x3_frags && net->x3_mx() && op.cout_pad % 32 == 0;
  // the candidates of the 8-phase form (256 x 256 tiles; the dispatch decides per batch): the plain epilogue, whole 32-channel chunks
  const bool plain = (d.act1 == ASV_ACT_NONE || d.act1 == ASV_ACT_RELU) && d.act2 == ASV_ACT_NONE && !d.affine_first;
  n.x3p = n.x3_frags && plain && op.cin_pad % 32 == 0 && d.in2_buf < 0 && d.seg_bias_buf < 0 && d.seg_scale_buf < 0 && d.res_buf < 0 && (long long)op.cin_pad * d.n_taps >= 512;
  // f32x mode, grid domain (the 2-D ResNet trunk) and the frames-domain layers the wide split kernel does not take (fewer than
  // 192 output channels, or a second input): hi / lo halves in the fragment order of kernels_conv2d_x3.hip, scaled by the
  // layer's power of two for the half-precision split
  n.conv2d_x3 = net->x3() && !op.utts && (kind == 2 || !(n.x3_frags && d.in2_buf < 0)) && grid_conv_x3_shape_ok(op.cin_pad, op.cout_store) &&
                (net->flags & ASV_FLAG_SMALL_TILES) == 0;
  // pooled-domain layers keep f32 activations; their GEMM runs on the bf16 matrix cores with every operand split into two bf16
  // halves, the weight halves in the fragment order kernels_utts.hip walks
  n.utts_split = op.utts && net->frames_h16();
  // possible member of a layer chain (it has fragments): its BatchNorm may be folded into the next member, or the previous member's into it
  n.chain_host_copies = (n.frags16 || n.x3_frags) && kind == ASV_DOMAIN_FRAMES && (net->flags & (ASV_FLAG_NO_FUSE | ASV_FLAG_NO_CHAIN)) == 0;
  return n;
}

// possible member of a layer chain: the host copies asv_net_finalize folds BatchNorms with (the previous member's into this layer, this one's into the next)
void keep_chain_host_copies(Op &op, const asv_tdnn_desc_t &d) {
  if (d.scale) { op.host_scale.assign(d.scale, d.scale + d.out_ch); op.host_shift.assign(d.shift, d.shift + d.out_ch); }
  if (d.n_taps == 1 && d.taps[0] == 0 && d.in_ch == kChainWidth) {
    const size_t tot = (size_t)d.w_tot_context, k = (size_t)(0 - d.w_left_context);
    op.host_w.resize((size_t)d.out_ch * d.in_ch);
    for (size_t i = 0; i < op.host_w.size(); ++i) op.host_w[i] = d.weight[i * tot + k];           // the one active tap, [out][in]
    op.host_bias.assign((size_t)d.out_ch, 0.0f);
    if (d.bias) op.host_bias.assign(d.bias, d.bias + d.out_ch);
  }
}

int check_view(const asv_net *net, int buf, int ch_off, int ch, const char *what) {
  ASV_REQUIRE(buf >= 0 && buf < (int)net->bufs.size(), "%s: buffer id %d out of range", what, buf);
  ASV_REQUIRE(ch_off >= 0 && ch_off % kChanAlign == 0, "%s: channel offset %d must be a non-negative multiple of %d", what, ch_off, kChanAlign);
  ASV_REQUIRE(ch >= 1 && ch_off + ch <= net->bufs[buf].channels, "%s: view [%d,%d) exceeds buffer %d (%d channels)", what, ch_off, ch_off + ch, buf, net->bufs[buf].channels);
  return ASV_OK;
}

// ---- what the asv_net_add_* functions share.  `fn` / `name`: the caller's, so that every message reads as the function's own

// null / finalized / struct_size.  both_sizes: the kinds whose message prints the two sizes
template <class Desc> int add_prologue(const asv_net *net, const Desc *d, const char *fn, bool both_sizes) {
  ASV_REQUIRE(net && d && !net->finalized, "%s: net is null or finalized", fn);
  if (both_sizes) ASV_REQUIRE(d->struct_size == sizeof(Desc), "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(Desc));
  ASV_REQUIRE(d->struct_size == sizeof(Desc), "%s: struct_size mismatch", fn);
  return ASV_OK;
}

struct Slice { int buf, off, ch; };      // channels [off, off + ch) of a buffer

// Two slices share no (padded) channel of one buffer.  A kernel whose tiles read rows of its input that other workgroups own (halo
// rows, the keys of other positions) while it stores its output rows may read and write one buffer only through disjoint slices.
bool disjoint(Slice a, Slice b) { return a.buf != b.buf || a.off + round_up(a.ch, kChanAlign) <= b.off || b.off + round_up(b.ch, kChanAlign) <= a.off; }

// row-local ops: the output is the input view itself (in place) or disjoint from it
int check_in_place_or_disjoint(const char *name, Slice in, Slice out) {
  ASV_REQUIRE((in.buf == out.buf && in.off == out.off) || disjoint(in, out), "%s: the output view overlaps the input view without being it (in place: the same offset)", name);
  return ASV_OK;
}

// The vector-wide kernels store whole vectors (8 x 16-bit / 4 x f32): the view rounded up to one must fit the buffer's pitch.  (A guard: check_view
// admits only offsets that are multiples of 16 and views inside the buffer's channels, and the pitch is the channels rounded up to 16.)
int check_padded_view(const asv_net *net, const char *name, const char *which, Slice v) {
  const int vec = net->dom_et(net->bufs[v.buf].domain) != ET_F32 ? 8 : 4;
  ASV_REQUIRE(v.off + round_up(v.ch, vec) <= net->bufs[v.buf].ld, "%s: padded %sview exceeds pitch", name, which);
  return ASV_OK;
}

// the op's line of asv_net_describe (behind "  op <index>: "), written where the op is added
void describe(Op &op, const char *fmt, ...) {
  char line[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(line, sizeof(line), fmt, ap);
  va_end(ap);
  op.desc = line;
}

// does op `o` read buffer `buf`?  The one list of every kind's input buffers (an unused one is -1), for both scans of asv_net_finalize.
// The fused-pool scan once had a list of its own, without tdnn.seg_bias_buf / seg_scale_buf, elt.seg_scale_buf / seg_norm_buf,
// i2c.seg_scale_buf and gin.in_buf.  Asking about them too cannot change which pools fuse: the per-segment buffers are utts-domain while a
// candidate's output is frames-domain, and a grid_input source has feat_dim <= 82 channels (a grid's pitch is at most 83), so
// cout_store <= 96, so its producing layer has no `wfrag` and is no candidate.
bool op_reads(const Op &o, int buf) {
  auto any = [buf](std::initializer_list<int> ids) { return std::find(ids.begin(), ids.end(), buf) != ids.end(); };
  switch (o.kind) {
    case OP_TDNN: return any({o.tdnn.in_buf, o.tdnn.in2_buf, o.tdnn.res_buf, o.tdnn.seg_bias_buf, o.tdnn.seg_scale_buf});
    case OP_POOL: return any({o.pool.in_buf});
    case OP_ATTPOOL: return any({o.att.x_buf, o.att.logit_buf});
    case OP_MQ_ATTPOOL: return any({o.mq.x_buf, o.mq.logit_buf});
    case OP_ELTWISE: return any({o.elt.a_buf, o.elt.b_buf, o.elt.c_buf, o.elt.seg_scale_buf, o.elt.seg_norm_buf, o.elt.d_buf});
    case OP_IM2COL: return any({o.i2c.in_buf, o.i2c.b_buf, o.i2c.seg_scale_buf});
    case OP_LDE: return any({o.lde.x_buf});
    case OP_GRID_INPUT: return any({o.gin.in_buf});
    case OP_RES2: return any({o.res2.in_buf});
    case OP_RES2N: return any({o.res2n.in_buf});
    case OP_FLATTEN: return any({o.flat.in_buf});
    case OP_ROWOP: return any({o.rop.in_buf});
    case OP_GRID_CONV: return any({o.gconv.in_buf});
    case OP_ATTENTION: return any({o.sa.q_buf, o.sa.k_buf, o.sa.v_buf});
    case OP_POSENC: return any({o.pos.in_buf});
    case OP_FRONT_CONV: return any({o.front.in_buf});
  }
  return false;
}

}  // namespace
}  // namespace asv

using namespace asv;

extern "C" {

int asv_version(void) { return ASV_AMD_VERSION; }
const char *asv_last_error(void) { return g_last_error.c_str(); }

int asv_device_count(int *count) {
  ASV_REQUIRE(count != nullptr, "asv_device_count: null argument");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { n = 0; (void)hipGetLastError(); }
  *count = n;
  return ASV_OK;
}

int asv_net_create(asv_net_t **out, int device, int precision, unsigned flags, int feat_dim) {
  ASV_REQUIRE(out != nullptr, "asv_net_create: null out pointer");
  ASV_REQUIRE(precision == ASV_PREC_F32 || precision == ASV_PREC_BF16 || precision == ASV_PREC_F32X || precision == ASV_PREC_F16, "asv_net_create: unknown precision %d", precision);
  ASV_REQUIRE((flags & ASV_FLAG_X3_SPLIT_BF16) == 0 || (flags & ASV_FLAG_X3_SPLIT_F16) == 0, "asv_net_create: both split types requested");
  ASV_REQUIRE(feat_dim >= 1, "asv_net_create: feat_dim %d", feat_dim);
  int ndev = 0;
  ASV_HIP_CHECK(hipGetDeviceCount(&ndev));
  ASV_REQUIRE(device >= 0 && device < ndev, "asv_net_create: device %d of %d", device, ndev);
  ASV_ON_DEVICE(device);
  asv_net *net = new (std::nothrow) asv_net();
  if (!net) { set_error("out of host memory"); return ASV_ENOMEM; }
  net->device = device; net->precision = precision; net->flags = flags; net->feat_dim = feat_dim;
  net->domains.push_back(Domain{ASV_DOMAIN_FRAMES});
  net->domains.push_back(Domain{ASV_DOMAIN_UTTS});
  net->bufs.push_back({ASV_DOMAIN_FRAMES, feat_dim, round_up(feat_dim, kChanAlign)});
  hipError_t ze = hipMalloc(&net->zero_page, 256);
  if (ze == hipSuccess) ze = hipMemset(net->zero_page, 0, 256);
  if (ze != hipSuccess) { set_error("zero page allocation failed: %s", hipGetErrorString(ze)); delete net; return ASV_EHIP; }
  *out = net;
  return ASV_OK;
}

void asv_net_destroy(asv_net_t *net) {
  if (!net) return;
  DeviceGuard guard;
  (void)guard.enter(net->device);
  (void)hipDeviceSynchronize();
  for (void *p : net->weight_allocs) (void)hipFree(p);
  for (auto &m : net->arena) if (m.ptr) (void)hipFree(m.ptr);
  if (net->meta_dev.ptr) (void)hipFree(net->meta_dev.ptr);
  if (net->rowmeta_dev.ptr) (void)hipFree(net->rowmeta_dev.ptr);
  if (net->poolpart_dev.ptr) (void)hipFree(net->poolpart_dev.ptr);
  if (net->lde_dev.ptr) (void)hipFree(net->lde_dev.ptr);
  if (net->zero_page) (void)hipFree(net->zero_page);
  if (net->meta_host) (void)hipHostFree(net->meta_host);
  if (net->meta_copied) (void)hipEventDestroy(net->meta_copied);
  for (auto &st : net->stamps) { (void)hipEventDestroy(st.a); (void)hipEventDestroy(st.b); }
  for (auto e : net->event_pool) (void)hipEventDestroy(e);
  delete net;
}

int asv_net_define_grid(asv_net_t *net, int time_shift, int width, int pitch) {
  ASV_REQUIRE(net && !net->finalized, "asv_net_define_grid: net is null or finalized");
  ASV_REQUIRE(time_shift >= 0 && time_shift <= 8, "asv_net_define_grid: time_shift %d", time_shift);
  // (width 1, pitch 1: a sequence at the grid's frame rate - no frequency neighbours, so no zero column between frames; asv_net_add_grid_flatten)
  ASV_REQUIRE(width >= 1 && (pitch >= width + 1 || (width == 1 && pitch == 1)) && pitch + 1 <= 84, "asv_net_define_grid: need 1 <= width < pitch <= 83, or width = pitch = 1 (got %d, %d)", width, pitch);
  Domain d{2};
  d.shift = time_shift; d.width = width; d.pitch = pitch;
  net->domains.push_back(d);
  return (int)net->domains.size() - 1;
}

int asv_net_define_grid_reach(asv_net_t *net, int time_shift, int width, int pitch, int reach) {
  ASV_REQUIRE(reach == 1 || reach == 2, "asv_net_define_grid_reach: reach %d (1 or 2)", reach);
  if (reach == 1) return asv_net_define_grid(net, time_shift, width, pitch);
  ASV_REQUIRE(net && !net->finalized, "asv_net_define_grid_reach: net is null or finalized");
  ASV_REQUIRE(time_shift >= 0 && time_shift <= 8, "asv_net_define_grid_reach: time_shift %d", time_shift);
  ASV_REQUIRE(width >= 1 && pitch >= width + 2 && 2 * pitch + 2 <= kConvTapsMaxHalo && pitch + 1 <= 84,
              "asv_net_define_grid_reach: reach 2 needs 1 <= width, width + 2 <= pitch <= 83 (got %d, %d)", width, pitch);
  Domain d{2};
  d.shift = time_shift; d.width = width; d.pitch = pitch; d.reach = 2;
  net->domains.push_back(d);
  return (int)net->domains.size() - 1;
}

int asv_net_define_grid_valid(asv_net_t *net, int time_shift, int width, int pitch) {
  ASV_REQUIRE(time_shift >= 1, "asv_net_define_grid_valid: time_shift %d (at least one unpadded stride-2 stage)", time_shift);
  const int id = asv_net_define_grid(net, time_shift, width, pitch);
  if (id >= 0) net->domains[id].valid = true;
  return id;
}

int asv_net_new_buffer(asv_net_t *net, int domain, int channels) {
  ASV_REQUIRE(net && !net->finalized, "asv_net_new_buffer: net is null or finalized");
  ASV_REQUIRE(domain >= 0 && domain < (int)net->domains.size(), "asv_net_new_buffer: domain %d", domain);
  ASV_REQUIRE(channels >= 1 && channels <= (1 << 20), "asv_net_new_buffer: channels %d", channels);
  net->bufs.push_back({domain, channels, round_up(channels, kChanAlign)});
  return (int)net->bufs.size() - 1;
}

int asv_net_add_tdnn(asv_net_t *net, const asv_tdnn_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_tdnn", true)) return rc;
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, d->in_ch, "tdnn input"))) return rc;
  if ((rc = check_view(net, d->out_buf, d->out_ch_off, d->out_ch, "tdnn output"))) return rc;
  const int dom = net->bufs[d->in_buf].domain;
  ASV_REQUIRE(net->bufs[d->out_buf].domain == dom, "tdnn: input and output domains differ");
  const Slice out{d->out_buf, d->out_ch_off, d->out_ch};
  ASV_REQUIRE(d->out_buf != 0, "tdnn: the input feature buffer cannot be an output");
  ASV_REQUIRE(disjoint({d->in_buf, d->in_ch_off, d->in_ch}, out), "tdnn: output slice overlaps the input slice of the same buffer");
  if (d->in2_buf >= 0) {
    if ((rc = check_view(net, d->in2_buf, d->in2_ch_off, d->in_ch, "tdnn second input"))) return rc;
    ASV_REQUIRE(net->bufs[d->in2_buf].domain == dom, "tdnn: second input domain differs");
    ASV_REQUIRE(disjoint({d->in2_buf, d->in2_ch_off, d->in_ch}, out), "tdnn: output slice overlaps the second input slice");
  }
  if (d->res_buf >= 0) {
    if ((rc = check_view(net, d->res_buf, d->res_ch_off, d->out_ch, "tdnn residual"))) return rc;
    ASV_REQUIRE(net->bufs[d->res_buf].domain == dom, "tdnn: residual domain differs");
    ASV_REQUIRE(disjoint({d->res_buf, d->res_ch_off, d->out_ch}, out), "tdnn: output slice overlaps the residual slice");
  }
  for (int sb : {d->seg_bias_buf, d->seg_scale_buf})
    if (sb >= 0) {
      ASV_REQUIRE(!net->is_utts(dom), "tdnn: per-segment bias/scale only applies to frame-level layers");
      ASV_REQUIRE(sb < (int)net->bufs.size() && net->is_utts(net->bufs[sb].domain) && net->bufs[sb].channels >= d->out_ch,
                  "tdnn: per-segment buffer %d must be an utts-domain buffer with >= %d channels", sb, d->out_ch);
    }
  ASV_REQUIRE(d->n_taps >= 1 && d->n_taps <= ASV_MAX_TAPS, "tdnn: n_taps %d", d->n_taps);
  for (int t = 0; t < d->n_taps; ++t) {
    ASV_REQUIRE(t == 0 || d->taps[t] > d->taps[t - 1], "tdnn: context must be strictly ascending (components.py:33-35)");
    ASV_REQUIRE(std::abs(d->taps[t]) <= net->domains[dom].halo() || (net->is_utts(dom) && d->taps[t] == 0),
                "tdnn: tap offset %d beyond the +-%d rows this domain keeps zero-padded", d->taps[t], net->domains[dom].halo());
    const int k = d->taps[t] - d->w_left_context;
    ASV_REQUIRE(k >= 0 && k < d->w_tot_context, "tdnn: tap %d outside the dense kernel [%d, %d)", d->taps[t], d->w_left_context, d->w_left_context + d->w_tot_context);
  }
  ASV_REQUIRE(!net->is_utts(dom) || (d->n_taps == 1 && d->taps[0] == 0), "tdnn: utts-domain layers have context [0] only");
  ASV_REQUIRE(d->weight != nullptr, "tdnn: null weight");
  ASV_REQUIRE((d->scale == nullptr) == (d->shift == nullptr), "tdnn: scale and shift come together");
  for (int a : {d->act1, d->act2}) ASV_REQUIRE(a >= ASV_ACT_NONE && a <= ASV_ACT_SIGMOID, "tdnn: unknown activation %d", a);

  Op op; op.kind = OP_TDNN; op.tdnn = *d; op.utts = net->is_utts(dom);
  const int et = net->dom_et(dom);
  op.cin_pad = round_up(d->in_ch, kChanAlign);
  op.cout_pad = round_up(d->out_ch, kBigTileN);
  op.cout_store = round_up(d->out_ch, kChanAlign);
  ASV_REQUIRE(d->out_ch_off + op.cout_store <= net->bufs[d->out_buf].ld, "tdnn: padded output view exceeds the buffer pitch");
  ASV_ON_DEVICE(net->device);
  const TdnnPacks need = tdnn_packs_for(net, *d, dom, op);
  // the half-precision split of the f32x mode scales the layer's weights by a power of two first (see x3_weight_scale)
  if ((need.x3_frags || need.conv2d_x3) && net->x3_et() == ET_F16) op.w_scale = x3_weight_scale(d->weight, (size_t)d->out_ch * d->in_ch * d->w_tot_context);
  const TapWeights tw{d->weight, d->out_ch, d->in_ch, d->w_tot_context, d->w_left_context, d->taps, d->n_taps};
  const TapWeights tws{tw.w, tw.out_ch, tw.in_ch, tw.tot_ctx, tw.left_ctx, tw.taps, tw.n_taps, op.w_scale};      // for the split layouts
  std::vector<unsigned char> packed(tdnn_weight_bytes(op.cout_pad, op.cin_pad, d->n_taps, et));
  pack_tdnn_weight(d->weight, d->out_ch, d->in_ch, d->w_tot_context, d->w_left_context, d->taps, d->n_taps, op.cout_pad, op.cin_pad, et, packed.data());
  if ((rc = upload_vec(net, packed, &op.w))) return rc;
  if (need.frags16 && (rc = upload_vec(net, pack_frag_forms(tw, op.cout_pad, op.cin_pad, et, false, false).hi, &op.wfrag))) return rc;
  if (need.x3_frags) {
    const FragForms f = pack_frag_forms(tws, op.cout_pad, op.cin_pad, net->x3_et(), true, need.mx8);
    if ((rc = upload_vec(net, f.hi, &op.wfrag)) || (rc = upload_vec(net, f.lo, &op.wlo))) return rc;
    if (need.mx8 && (rc = upload_vec(net, f.w8, &op.w8))) return rc;
  }
  if (need.x3p && (rc = upload_vec(net, pack_tdnn_weight_x3p(tws, op.cout_pad, op.cin_pad, net->x3_et()), &op.wx3p))) return rc;
  if (need.conv2d_x3 && (rc = upload_vec(net, pack_grid_conv_x3_frags(tws, op.cin_pad, op.cout_store, net->x3_et()), &op.wconv))) return rc;
  if (need.conv2d && (rc = upload_vec(net, pack_grid_conv_frags(tw, op.cin_pad, et), &op.wconv))) return rc;
  if (need.utts_split) {
    std::vector<uint16_t> hi(utts_weight_split_elems(op.cout_pad, op.cin_pad)), lo(hi.size());
    pack_utts_weight_split(tw, op.cout_pad, op.cin_pad, hi.data(), lo.data());
    if ((rc = upload_vec(net, hi, &op.wfrag)) || (rc = upload_vec(net, lo, &op.wlo))) return rc;
  }
  if ((rc = upload_padded(net, d->bias, d->out_ch, op.cout_pad, 0.0f, &op.bias))) return rc;
  op.has_affine = d->scale != nullptr;
  if (op.has_affine) {
    if ((rc = upload_padded(net, d->scale, d->out_ch, op.cout_pad, 0.0f, &op.scale))) return rc;
    if ((rc = upload_padded(net, d->shift, d->out_ch, op.cout_pad, 0.0f, &op.shift))) return rc;
  }
  if (need.chain_host_copies) keep_chain_host_copies(op, *d);
  op.tdnn.weight = nullptr; op.tdnn.bias = nullptr; op.tdnn.scale = nullptr; op.tdnn.shift = nullptr;
  std::string taps;
  for (int t = 0; t < d->n_taps; ++t) { taps += (t ? "," : ""); taps += std::to_string(d->taps[t]); }
  describe(op, "tdnn %d[%d:+%d]%s -> %d[%d:+%d] taps=[%s] act1=%d affine=%d first=%d act2=%d segbias=%d segscale=%d res=%d\n", d->in_buf, d->in_ch_off, d->in_ch,
           d->in2_buf >= 0 ? "+in2" : "", d->out_buf, d->out_ch_off, d->out_ch, taps.c_str(), d->act1, (int)op.has_affine, d->affine_first, d->act2, d->seg_bias_buf,
           d->seg_scale_buf, d->res_buf);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_stats_pool(asv_net_t *net, const asv_pool_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_stats_pool", false)) return rc;
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, d->channels, "pool input"))) return rc;
  int out_ch = d->channels * (d->stddev ? 2 : 1);
  ASV_REQUIRE(d->in_buf >= 0 && d->in_buf < (int)net->bufs.size(), "pool: input buffer id %d", d->in_buf);
  if (d->per_bin) out_ch *= net->domains[net->bufs[d->in_buf].domain].width;
  ASV_REQUIRE(d->out_buf > 0 && d->out_buf < (int)net->bufs.size(), "pool: output buffer id %d", d->out_buf);
  ASV_REQUIRE(d->out_ch_off >= 0 && d->out_ch_off + out_ch <= net->bufs[d->out_buf].channels, "pool: output view exceeds buffer");
  ASV_REQUIRE(!net->is_utts(net->bufs[d->in_buf].domain) && net->is_utts(net->bufs[d->out_buf].domain),
              "pool: goes from a frame-level domain to the utts domain");
  ASV_REQUIRE(d->per_bin == 0 || net->domains[net->bufs[d->in_buf].domain].kind == 2, "pool: per_bin needs a grid-domain input");
  ASV_REQUIRE(d->unbiased >= 0 && d->unbiased <= 2 && (d->var_mode == ASV_POOL_VAR_CLAMP || d->var_mode == ASV_POOL_VAR_ADD), "pool: bad mode");
  Op op; op.kind = OP_POOL; op.pool = *d;
  describe(op, "stats_pool %d[%d:+%d] -> %d[%d] stddev=%d unbiased=%d var_mode=%d eps=%g\n", op.pool.in_buf, op.pool.in_ch_off,
           op.pool.channels, op.pool.out_buf, op.pool.out_ch_off, op.pool.stddev, op.pool.unbiased, op.pool.var_mode, op.pool.eps);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_attentive_pool(asv_net_t *net, const asv_attpool_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_attentive_pool", false)) return rc;
  int rc;
  if ((rc = check_view(net, d->x_buf, d->x_ch_off, d->channels, "attentive pool x"))) return rc;
  ASV_REQUIRE(d->logit_group >= 0 && d->logit_group <= d->channels, "attentive pool: logit_group %d", d->logit_group);
  const int group = d->logit_group > 1 ? d->logit_group : (d->shared_logits ? d->channels : 1);
  if (group > 1) {                 // head logits are read one element at a time: any column offset (head h of the global poolings)
    ASV_REQUIRE(d->logit_buf >= 0 && d->logit_buf < (int)net->bufs.size() && d->logit_ch_off >= 0 &&
                d->logit_ch_off + (d->channels + group - 1) / group <= net->bufs[d->logit_buf].channels,
                "attentive pool logits: columns [%d,%d) exceed buffer %d", d->logit_ch_off, d->logit_ch_off + (d->channels + group - 1) / group, d->logit_buf);
  } else if ((rc = check_view(net, d->logit_buf, d->logit_ch_off, d->channels, "attentive pool logits"))) return rc;
  ASV_REQUIRE(d->out_buf > 0 && d->out_buf < (int)net->bufs.size(), "attentive pool: output buffer id %d", d->out_buf);
  ASV_REQUIRE(d->out_ch_off >= 0 && d->out_ch_off + 2 * d->channels <= net->bufs[d->out_buf].channels, "attentive pool: output view exceeds buffer");
  ASV_REQUIRE(net->is_sequence(net->bufs[d->x_buf].domain) && net->bufs[d->logit_buf].domain == net->bufs[d->x_buf].domain &&
              net->is_utts(net->bufs[d->out_buf].domain), "attentive pool: frames (or a sequence domain) -> utts");
  ASV_REQUIRE((d->prior_logit == nullptr) == (d->prior_value == nullptr), "attentive pool: prior logits and values come together");
  ASV_REQUIRE(!(d->logit_softplus2 || d->prior_logit) || group == 1, "attentive pool: the xi-vector options need per-channel logits");
  Op op; op.kind = OP_ATTPOOL; op.att = *d;
  if (d->prior_logit) {                                         // parked in the scale / shift slots of the op
    ASV_ON_DEVICE(net->device);
    if ((rc = upload_padded(net, d->prior_logit, d->channels, round_up(d->channels, kChanAlign), 0.0f, &op.scale))) return rc;
    if ((rc = upload_padded(net, d->prior_value, d->channels, round_up(d->channels, kChanAlign), 0.0f, &op.shift))) return rc;
  }
  op.att.prior_logit = nullptr; op.att.prior_value = nullptr;
  describe(op, "attentive_pool x=%d logits=%d channels=%d -> %d[%d] eps=%g\n", op.att.x_buf, op.att.logit_buf, op.att.channels,
           op.att.out_buf, op.att.out_ch_off, op.att.eps);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_mq_attentive_pool(asv_net_t *net, const asv_mq_attpool_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_mq_attentive_pool", false)) return rc;
  ASV_REQUIRE(d->heads >= 1 && d->queries >= 1 && d->queries <= 4, "mq attentive pool: %d heads, %d queries (1 .. 4 queries)", d->heads, d->queries);
  ASV_REQUIRE(d->channels >= 1 && d->channels % d->heads == 0 && (d->channels / d->heads) % kChanAlign == 0,
              "mq attentive pool: %d channels in %d heads: every head needs a multiple of %d channels", d->channels, d->heads, kChanAlign);
  const int head_ch = d->channels / d->heads, pairs = d->heads * d->queries;
  int rc;
  if ((rc = check_view(net, d->x_buf, d->x_ch_off, d->channels, "mq attentive pool x"))) return rc;
  if (d->shared_logits) {          // one element per (frame, pair): any column offset, like the head logits of asv_attpool_desc_t
    ASV_REQUIRE(d->logit_buf >= 0 && d->logit_buf < (int)net->bufs.size() && d->logit_ch_off >= 0 && d->logit_ch_off + pairs <= net->bufs[d->logit_buf].channels,
                "mq attentive pool logits: columns [%d,%d) exceed buffer %d", d->logit_ch_off, d->logit_ch_off + pairs, d->logit_buf);
  } else if ((rc = check_view(net, d->logit_buf, d->logit_ch_off, pairs * head_ch, "mq attentive pool logits"))) return rc;
  ASV_REQUIRE(d->out_buf > 0 && d->out_buf < (int)net->bufs.size(), "mq attentive pool: output buffer id %d", d->out_buf);
  // the two layouts without overlap: [mean | std] per pair, or all means in front of all stds
  ASV_REQUIRE((d->std_off >= head_ch && d->pair_stride >= d->std_off + head_ch) ||
              (d->pair_stride >= head_ch && d->std_off >= (pairs - 1) * d->pair_stride + head_ch),
              "mq attentive pool: pair_stride %d / std_off %d make means and stds of %d-channel heads overlap", d->pair_stride, d->std_off, head_ch);
  ASV_REQUIRE(d->out_ch_off >= 0 && (long long)d->out_ch_off + (long long)(pairs - 1) * d->pair_stride + d->std_off + head_ch <= net->bufs[d->out_buf].channels,
              "mq attentive pool: output view exceeds buffer");
  ASV_REQUIRE(net->is_sequence(net->bufs[d->x_buf].domain) && net->bufs[d->logit_buf].domain == net->bufs[d->x_buf].domain &&
              net->is_utts(net->bufs[d->out_buf].domain), "mq attentive pool: frames (or a sequence domain) -> utts");
  Op op; op.kind = OP_MQ_ATTPOOL; op.mq = *d;
  describe(op, "mq_attentive_pool x=%d logits=%d channels=%d heads=%d queries=%d shared=%d -> %d[%d] eps=%g\n", op.mq.x_buf, op.mq.logit_buf,
           op.mq.channels, op.mq.heads, op.mq.queries, op.mq.shared_logits, op.mq.out_buf, op.mq.out_ch_off, op.mq.eps);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_lde_pool(asv_net_t *net, const asv_lde_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_lde_pool", false)) return rc;
  ASV_REQUIRE(d->mu && d->beta && d->n_centres >= 1 && d->n_centres <= 64, "lde pool: mu / beta are required and 1 <= n_centres <= 64 (got %d)", d->n_centres);
  int rc;
  if ((rc = check_view(net, d->x_buf, d->x_ch_off, d->channels, "lde pool x"))) return rc;
  ASV_REQUIRE(d->out_buf > 0 && d->out_buf < (int)net->bufs.size(), "lde pool: output buffer id %d", d->out_buf);
  ASV_REQUIRE(d->out_ch_off >= 0 && d->out_ch_off + d->channels * d->n_centres <= net->bufs[d->out_buf].channels, "lde pool: output view exceeds buffer");
  ASV_REQUIRE(net->is_sequence(net->bufs[d->x_buf].domain) && net->is_utts(net->bufs[d->out_buf].domain), "lde pool: frames (or a sequence domain) -> utts");
  Op op; op.kind = OP_LDE; op.lde = *d;
  ASV_ON_DEVICE(net->device);
  const int n = d->channels * d->n_centres;
  if ((rc = upload_padded(net, d->mu, n, round_up(n, kChanAlign), 0.0f, &op.scale))) return rc;
  if ((rc = upload_padded(net, d->beta, d->n_centres, 64, 0.0f, &op.shift))) return rc;
  op.lde.mu = nullptr; op.lde.beta = nullptr;
  describe(op, "lde_pool x=%d channels=%d centres=%d -> %d[%d]\n", op.lde.x_buf, op.lde.channels, op.lde.n_centres, op.lde.out_buf,
           op.lde.out_ch_off);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_res2(asv_net_t *net, const asv_res2_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_res2", false)) return rc;
  ASV_REQUIRE(net->frames_h16(), "res2: the one-kernel Res2NetBlock exists for the 16-bit precision modes (bf16, f16) only");
  ASV_REQUIRE(d->branches >= 1 && d->branches <= 7 && d->dilation >= 1 && d->dilation <= kHalo, "res2: %d branches, dilation %d", d->branches, d->dilation);
  ASV_REQUIRE(d->weight && d->bias && d->scale && d->shift, "res2: weight / bias / scale / shift are required");
  const int ch = (d->branches + 1) * kRes2Width;
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, ch, "res2 input"))) return rc;
  if ((rc = check_view(net, d->out_buf, d->out_ch_off, ch, "res2 output"))) return rc;
  ASV_REQUIRE(net->bufs[d->in_buf].domain == ASV_DOMAIN_FRAMES && net->bufs[d->out_buf].domain == ASV_DOMAIN_FRAMES && d->out_buf != d->in_buf && d->out_buf != 0,
              "res2: frames-domain input and a different frames-domain output buffer");
  ASV_REQUIRE(d->in_ch_off % 8 == 0 && d->out_ch_off % 8 == 0, "res2: channel offsets must be multiples of 8 (16-byte rows pieces)");
  Op op; op.kind = OP_RES2; op.res2 = *d;
  ASV_ON_DEVICE(net->device);
  const int W = kRes2Width;
  if ((rc = upload_vec(net, pack_res2_branch_frags(d->weight, W, d->branches, d->dilation, net->frames_et()), &op.wfrag))) return rc;
  if ((rc = upload_padded(net, d->bias, d->branches * W, d->branches * W, 0.0f, &op.bias))) return rc;
  if ((rc = upload_padded(net, d->scale, d->branches * W, d->branches * W, 0.0f, &op.scale))) return rc;
  if ((rc = upload_padded(net, d->shift, d->branches * W, d->branches * W, 0.0f, &op.shift))) return rc;
  op.res2.weight = nullptr; op.res2.bias = nullptr; op.res2.scale = nullptr; op.res2.shift = nullptr;
  describe(op, "res2 %d[%d] -> %d[%d] branches=%d dilation=%d\n", op.res2.in_buf, op.res2.in_ch_off, op.res2.out_buf, op.res2.out_ch_off,
           op.res2.branches, op.res2.dilation);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_res2n(asv_net_t *net, const asv_res2n_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_res2n", false)) return rc;
  ASV_REQUIRE(net->frames_h16(), "res2n: the one-kernel Res2 chain exists for the 16-bit precision modes (bf16, f16) only");
  ASV_REQUIRE(d->width == kRes2nWidth, "res2n: width %d (the kernel is built for groups of %d channels)", d->width, kRes2nWidth);
  ASV_REQUIRE(d->groups >= 2 && d->groups <= 8 && d->pass_group >= 0 && d->pass_group < d->groups && d->dilation >= 1 && d->dilation <= kHalo,
              "res2n: %d groups, pass group %d, dilation %d", d->groups, d->pass_group, d->dilation);
  ASV_REQUIRE(d->weight && d->scale && d->shift, "res2n: weight / scale / shift are required");
  const int W = d->width, branches = d->groups - 1, ch = d->groups * W;
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, ch, "res2n input"))) return rc;
  if ((rc = check_view(net, d->out_buf, d->out_ch_off, ch, "res2n output"))) return rc;
  ASV_REQUIRE(net->bufs[d->in_buf].domain == ASV_DOMAIN_FRAMES && net->bufs[d->out_buf].domain == ASV_DOMAIN_FRAMES && d->out_buf != d->in_buf && d->out_buf != 0,
              "res2n: frames-domain input and a different frames-domain output buffer");
  ASV_REQUIRE(d->in_ch_off % 8 == 0 && d->out_ch_off % 8 == 0, "res2n: channel offsets must be multiples of 8 (16-byte row pieces)");
  Op op; op.kind = OP_RES2N; op.res2n = *d;
  ASV_ON_DEVICE(net->device);
  if ((rc = upload_vec(net, pack_res2_branch_frags(d->weight, W, branches, d->dilation, net->frames_et()), &op.wfrag))) return rc;
  if (d->bias != nullptr && (rc = upload_padded(net, d->bias, branches * W, branches * W, 0.0f, &op.bias))) return rc;
  if ((rc = upload_padded(net, d->scale, branches * W, branches * W, 0.0f, &op.scale))) return rc;
  if ((rc = upload_padded(net, d->shift, branches * W, branches * W, 0.0f, &op.shift))) return rc;
  op.res2n.weight = nullptr; op.res2n.bias = nullptr; op.res2n.scale = nullptr; op.res2n.shift = nullptr;
  describe(op, "res2n %d[%d] -> %d[%d] width=%d groups=%d pass_group=%d dilation=%d bias=%d\n", op.res2n.in_buf, op.res2n.in_ch_off,
           op.res2n.out_buf, op.res2n.out_ch_off, op.res2n.width, op.res2n.groups, op.res2n.pass_group, op.res2n.dilation, op.bias != nullptr);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_eltwise(asv_net_t *net, const asv_eltwise_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_eltwise", false)) return rc;
  int rc;
  if ((rc = check_view(net, d->a_buf, d->a_ch_off, d->channels, "eltwise a"))) return rc;
  if ((rc = check_view(net, d->out_buf, d->out_ch_off, d->channels, "eltwise out"))) return rc;
  const int dom = net->bufs[d->a_buf].domain;
  ASV_REQUIRE(net->bufs[d->out_buf].domain == dom && d->out_buf != 0, "eltwise: bad output buffer");
  if (d->b_buf >= 0) { if ((rc = check_view(net, d->b_buf, d->b_ch_off, d->channels, "eltwise b"))) return rc; ASV_REQUIRE(net->bufs[d->b_buf].domain == dom, "eltwise: b domain"); }
  if (d->c_buf >= 0) { if ((rc = check_view(net, d->c_buf, d->c_ch_off, d->channels, "eltwise c"))) return rc; ASV_REQUIRE(net->bufs[d->c_buf].domain == dom, "eltwise: c domain"); }
  if (d->seg_scale_buf >= 0)
    ASV_REQUIRE(!net->is_utts(dom) && d->seg_scale_buf < (int)net->bufs.size() && net->is_utts(net->bufs[d->seg_scale_buf].domain) &&
                net->bufs[d->seg_scale_buf].channels >= d->channels, "eltwise: bad per-segment scale buffer");
  ASV_REQUIRE((d->scale == nullptr) == (d->shift == nullptr), "eltwise: scale and shift come together");
  if (d->seg_norm_buf >= 0)
    ASV_REQUIRE(!net->is_utts(dom) && d->seg_norm_buf < (int)net->bufs.size() && net->is_utts(net->bufs[d->seg_norm_buf].domain) &&
                net->bufs[d->seg_norm_buf].channels >= 2 * d->channels && d->seg_norm_mode >= 1 && d->seg_norm_mode <= 3,
                "eltwise: bad per-segment normalisation buffer / mode");
  ASV_REQUIRE(d->act >= ASV_ACT_NONE && d->act <= ASV_ACT_SIGMOID, "eltwise: unknown activation %d", d->act);
  if ((rc = check_padded_view(net, "eltwise", "", {d->out_buf, d->out_ch_off, d->channels}))) return rc;
  ASV_REQUIRE((d->out2_buf >= 0) == (d->d_buf >= 0), "eltwise: the second output and its addend come together");
  if (d->out2_buf >= 0) {
    if ((rc = check_view(net, d->d_buf, d->d_ch_off, d->channels, "eltwise d"))) return rc;
    if ((rc = check_view(net, d->out2_buf, d->out2_ch_off, d->channels, "eltwise out2"))) return rc;
    ASV_REQUIRE(net->bufs[d->d_buf].domain == dom && net->bufs[d->out2_buf].domain == dom && d->out2_buf != 0 && d->out2_buf != d->out_buf,
                "eltwise: bad second output / addend buffer");
    if ((rc = check_padded_view(net, "eltwise", "second ", {d->out2_buf, d->out2_ch_off, d->channels}))) return rc;
  }
  Op op; op.kind = OP_ELTWISE; op.elt = *d; op.utts = net->is_utts(dom);
  ASV_ON_DEVICE(net->device);
  if (d->scale) {
    const int n_pad = round_up(d->channels, kChanAlign);
    if ((rc = upload_padded(net, d->scale, d->channels, n_pad, 0.0f, &op.scale))) return rc;
    if ((rc = upload_padded(net, d->shift, d->channels, n_pad, 0.0f, &op.shift))) return rc;
  }
  op.elt.scale = nullptr; op.elt.shift = nullptr;
  describe(op, "eltwise a=%d b=%d c=%d segscale=%d affine=%d channels=%d -> %d[%d]%s\n", op.elt.a_buf, op.elt.b_buf, op.elt.c_buf,
           op.elt.seg_scale_buf, op.scale != nullptr, op.elt.channels, op.elt.out_buf, op.elt.out_ch_off, op.elt.out2_buf >= 0 ? " (+ second output)" : "");
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_rowop(asv_net_t *net, const asv_rowop_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_rowop", true)) return rc;
  for (int a : {d->act0, d->act1}) ASV_REQUIRE(a >= ASV_ACT_NONE && a <= ASV_ACT_DOUBLE_SWISH, "rowop: unknown activation %d", a);
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, d->channels, "rowop input")) || (rc = check_view(net, d->out_buf, d->out_ch_off, d->channels, "rowop output"))) return rc;
  const int dom = net->bufs[d->in_buf].domain;
  ASV_REQUIRE(net->is_utts(dom) || net->is_sequence(dom), "rowop: grid domains are not supported (frames, sequence and utts domains only)");
  ASV_REQUIRE(net->bufs[d->out_buf].domain == dom && d->out_buf != 0, "rowop: bad output buffer (the input's domain, never the feature buffer)");
  ASV_REQUIRE(d->channels <= kRowopMaxChannels, "rowop: %d channels (at most %d: a row lives in one wave's registers)", d->channels, kRowopMaxChannels);
  const Slice in{d->in_buf, d->in_ch_off, d->channels}, out{d->out_buf, d->out_ch_off, d->channels};
  if ((rc = check_padded_view(net, "rowop", "", in)) || (rc = check_padded_view(net, "rowop", "", out)) || (rc = check_in_place_or_disjoint("rowop", in, out))) return rc;
  ASV_REQUIRE((d->scale0 == nullptr) == (d->shift0 == nullptr) && (d->scale1 == nullptr) == (d->shift1 == nullptr), "rowop: scale and shift come together");
  ASV_REQUIRE((d->gamma == nullptr) == (d->beta == nullptr), "rowop: gamma and beta come together");
  ASV_REQUIRE(d->gamma == nullptr || d->ln, "rowop: gamma / beta without ln");
  ASV_REQUIRE(!d->ln || (d->eps > 0.0f && std::isfinite(d->eps)), "rowop: ln needs a positive eps (got %g)", (double)d->eps);
  Op op; op.kind = OP_ROWOP; op.rop = *d; op.utts = net->is_utts(dom);
  ASV_ON_DEVICE(net->device);
  const float *tabs[6] = {d->scale0, d->shift0, d->gamma, d->beta, d->scale1, d->shift1};
  for (int k = 0; k < 6; ++k)
    if (tabs[k] != nullptr && (rc = upload_padded(net, tabs[k], d->channels, round_up(d->channels, kChanAlign), 0.0f, &op.rop_tab[k]))) return rc;
  op.rop.scale0 = op.rop.shift0 = op.rop.gamma = op.rop.beta = op.rop.scale1 = op.rop.shift1 = nullptr;
  describe(op, "rowop %d[%d:+%d] -> %d[%d] affine0=%d act0=%d ln=%d(affine=%d eps=%g) act1=%d affine1=%d\n", op.rop.in_buf, op.rop.in_ch_off,
           op.rop.channels, op.rop.out_buf, op.rop.out_ch_off, op.rop_tab[0] != nullptr, op.rop.act0, op.rop.ln, op.rop_tab[2] != nullptr, (double)op.rop.eps,
           op.rop.act1, op.rop_tab[4] != nullptr);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_grid_conv(asv_net_t *net, const asv_grid_conv_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_grid_conv", true)) return rc;
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, d->in_ch, "grid_conv input"))) return rc;
  if ((rc = check_view(net, d->out_buf, d->out_ch_off, d->out_ch, "grid_conv output"))) return rc;
  const int dom = net->bufs[d->in_buf].domain;
  const Domain &dm = net->domains[dom];
  ASV_REQUIRE(dm.kind == 2 && !net->is_sequence(dom), "grid_conv: the input must live on a (time, frequency) grid");
  ASV_REQUIRE(net->bufs[d->out_buf].domain == dom && d->out_buf != 0, "grid_conv: bad output buffer (the input's grid, never the feature buffer)");
  const int cin_pad = round_up(d->in_ch, kChanAlign), cout_store = round_up(d->out_ch, kChanAlign), nf_total = (d->out_ch + 31) / 32;
  ASV_REQUIRE(d->in_ch_off + cin_pad <= net->bufs[d->in_buf].ld && d->out_ch_off + cout_store <= net->bufs[d->out_buf].ld, "grid_conv: padded view exceeds the buffer pitch");
  ASV_REQUIRE(disjoint({d->in_buf, d->in_ch_off, d->in_ch}, {d->out_buf, d->out_ch_off, d->out_ch}), "grid_conv: the output slice overlaps the input slice of the same buffer");
  ASV_REQUIRE(d->n_taps >= 1 && d->n_taps <= ASV_GRID_CONV_MAX_TAPS, "grid_conv: n_taps %d (1 .. %d)", d->n_taps, ASV_GRID_CONV_MAX_TAPS);
  for (int t = 0; t < d->n_taps; ++t) {
    ASV_REQUIRE(std::abs(d->dt[t]) <= dm.reach && std::abs(d->df[t]) <= dm.reach, "grid_conv: tap (%d, %d) beyond the reach %d of this grid (asv_net_define_grid_reach)",
                d->dt[t], d->df[t], dm.reach);
    for (int u = 0; u < t; ++u) ASV_REQUIRE(d->dt[u] != d->dt[t] || d->df[u] != d->df[t], "grid_conv: tap (%d, %d) appears twice", d->dt[t], d->df[t]);
  }
  ASV_REQUIRE(d->weight != nullptr, "grid_conv: null weight");
  ASV_REQUIRE(d->act == ASV_ACT_NONE || d->act == ASV_ACT_RELU, "grid_conv: activation %d (none or ReLU)", d->act);
  Op op; op.kind = OP_GRID_CONV; op.gconv = *d;
  op.cin_pad = cin_pad; op.cout_store = cout_store; op.cout_pad = nf_total * 32;
  ASV_ON_DEVICE(net->device);
  const int et = net->dom_et(dom);
  std::vector<unsigned char> frags(grid_conv_taps_frag_bytes(cin_pad, nf_total, d->n_taps, et));
  pack_grid_conv_taps(d->weight, d->out_ch, d->in_ch, d->n_taps, cin_pad, nf_total, et, frags.data());
  if ((rc = upload_vec(net, frags, &op.wconv))) return rc;
  if ((rc = upload_padded(net, d->bias, d->bias ? d->out_ch : 0, op.cout_pad, 0.0f, &op.bias))) return rc;
  op.gconv.weight = nullptr; op.gconv.bias = nullptr;
  describe(op, "grid_conv %d[%d:+%d] -> %d[%d:+%d] taps=%d act=%d bias=%d\n", op.gconv.in_buf, op.gconv.in_ch_off, op.gconv.in_ch,
           op.gconv.out_buf, op.gconv.out_ch_off, op.gconv.out_ch, op.gconv.n_taps, op.gconv.act, op.bias != nullptr);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_grid_input(asv_net_t *net, const asv_grid_input_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_grid_input", false)) return rc;
  ASV_REQUIRE(d->out_buf > 0 && d->out_buf < (int)net->bufs.size(), "grid_input: output buffer id %d", d->out_buf);
  ASV_REQUIRE(d->in_buf >= 0 && d->in_buf < (int)net->bufs.size() && net->bufs[d->in_buf].domain == ASV_DOMAIN_FRAMES && net->bufs[d->in_buf].channels == net->feat_dim,
              "grid_input: input must be a frames-domain buffer with feat_dim channels");
  const Domain &dm = net->domains[net->bufs[d->out_buf].domain];
  ASV_REQUIRE(dm.kind == 2 && dm.shift == 0 && dm.width == net->feat_dim, "grid_input: output must be a full-resolution grid of width feat_dim (%d)", net->feat_dim);
  Op op; op.kind = OP_GRID_INPUT; op.gin = *d;
  describe(op, "grid_input %d -> %d\n", op.gin.in_buf, op.gin.out_buf);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_im2col(asv_net_t *net, const asv_im2col_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_im2col", false)) return rc;
  int rc;
  if ((rc = check_view(net, d->in_buf, 0, d->channels, "im2col input"))) return rc;
  ASV_REQUIRE(d->n_taps >= 1 && d->n_taps <= ASV_MAX_TAPS && (d->stride == 1 || d->stride == 2), "im2col: n_taps %d stride %d", d->n_taps, d->stride);
  ASV_REQUIRE(d->channels % kChanAlign == 0 && d->channels == net->bufs[d->in_buf].channels, "im2col: channels must be the whole input buffer and a multiple of %d", kChanAlign);
  if ((rc = check_view(net, d->out_buf, 0, d->channels * d->n_taps, "im2col output"))) return rc;
  const Domain &di = net->domains[net->bufs[d->in_buf].domain], &dq = net->domains[net->bufs[d->out_buf].domain];
  ASV_REQUIRE(di.kind == 2 && dq.kind == 2 && d->out_buf != d->in_buf && d->out_buf != 0, "im2col: grid -> grid");
  if (dq.valid) {
    // the unpadded stride-2 form: taps (0 .. 2, 0 .. 2) relative to (2 t', 2 f'), every one inside the input map by the domain rule
    ASV_REQUIRE(di.valid && d->stride == 2 && dq.shift == di.shift + 1 && dq.width == (di.width - 1) / 2,
                "im2col: unpadded output grid (shift %d, width %d) does not match stride 2 over the unpadded input grid (shift %d, width %d): width (W - 1) / 2", dq.shift, dq.width,
                di.shift, di.width);
    for (int t = 0; t < d->n_taps; ++t)
      ASV_REQUIRE(d->dt[t] >= 0 && d->dt[t] <= 2 && d->df[t] >= 0 && d->df[t] <= 2, "im2col: tap (%d, %d) of the unpadded form (0 .. 2 in both axes)", d->dt[t], d->df[t]);
  } else {
    ASV_REQUIRE(!di.valid, "im2col: a padded gather from an unpadded grid");
    ASV_REQUIRE(dq.shift == di.shift + (d->stride == 2 ? 1 : 0) && dq.width == (di.width + d->stride - 1) / d->stride,
                "im2col: output grid (T/%d x %d) does not match stride %d over input grid (T/%d x %d)", 1 << dq.shift, dq.width, d->stride, 1 << di.shift, di.width);
  }
  ASV_REQUIRE(d->act == ASV_ACT_NONE || d->act == ASV_ACT_RELU, "im2col: the elementwise prologue takes no activation or ReLU (got %d)", d->act);
  // optional buffers: -1 = none, and so is 0 - buffer 0 is the feature matrix (frames domain), which can be neither a grid addend nor a
  // per-segment scale, so a caller that zero-initialises the descriptor (memset + struct_size, the usual C pattern) gets what the
  // descriptor meant before these fields existed
  asv_im2col_desc_t norm = *d;
  if (norm.b_buf <= 0) norm.b_buf = -1;
  if (norm.seg_scale_buf <= 0) norm.seg_scale_buf = -1;
  d = &norm;
  if (d->b_buf >= 0) {
    if ((rc = check_view(net, d->b_buf, 0, d->channels, "im2col addend"))) return rc;
    ASV_REQUIRE(net->bufs[d->b_buf].domain == net->bufs[d->in_buf].domain && net->bufs[d->b_buf].channels == d->channels && d->b_buf != d->out_buf,
                "im2col: the addend must be a whole buffer of the input's grid and width");
  }
  if (d->seg_scale_buf >= 0)
    ASV_REQUIRE(d->seg_scale_buf < (int)net->bufs.size() && net->is_utts(net->bufs[d->seg_scale_buf].domain) && net->bufs[d->seg_scale_buf].channels >= d->channels,
                "im2col: bad per-segment scale buffer");
  Op op; op.kind = OP_IM2COL; op.i2c = *d;
  describe(op, "im2col %d -> %d taps=%d stride=%d channels=%d\n", op.i2c.in_buf, op.i2c.out_buf, op.i2c.n_taps, op.i2c.stride, op.i2c.channels);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_grid_flatten(asv_net_t *net, const asv_grid_flatten_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_grid_flatten", false)) return rc;
  ASV_REQUIRE(d->in_buf > 0 && d->in_buf < (int)net->bufs.size() && d->out_buf > 0 && d->out_buf < (int)net->bufs.size() && d->in_buf != d->out_buf,
              "grid_flatten: buffer ids %d -> %d", d->in_buf, d->out_buf);
  const Domain &di = net->domains[net->bufs[d->in_buf].domain], &dq = net->domains[net->bufs[d->out_buf].domain];
  ASV_REQUIRE(di.kind == 2 && dq.kind == 2 && dq.width == 1 && dq.pitch == 1 && dq.shift == di.shift && dq.valid == di.valid,
              "grid_flatten: the output must live on the sequence domain (width 1, pitch 1) of the input grid's time shift and row rule");
  ASV_REQUIRE(net->bufs[d->out_buf].channels == net->bufs[d->in_buf].channels * di.width, "grid_flatten: %d channels x %d bins do not give %d output channels",
              net->bufs[d->in_buf].channels, di.width, net->bufs[d->out_buf].channels);
  Op op; op.kind = OP_FLATTEN; op.flat = *d;
  describe(op, "grid_flatten %d -> %d\n", op.flat.in_buf, op.flat.out_buf);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_front_conv(asv_net_t *net, const asv_front_conv_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_front_conv", true)) return rc;
  ASV_REQUIRE(d->in_buf >= 0 && d->in_buf < (int)net->bufs.size() && net->bufs[d->in_buf].domain == ASV_DOMAIN_FRAMES && net->bufs[d->in_buf].channels == net->feat_dim,
              "front_conv: the input must be a frames-domain buffer with feat_dim channels");
  ASV_REQUIRE(d->out_buf > 0 && d->out_buf < (int)net->bufs.size() && d->out_buf != d->in_buf, "front_conv: output buffer id %d", d->out_buf);
  ASV_REQUIRE(d->out_ch >= 1 && d->out_ch == net->bufs[d->out_buf].channels, "front_conv: out_ch %d must be the whole output buffer (%d channels)", d->out_ch,
              net->bufs[d->out_buf].channels);
  const Domain &dm = net->domains[net->bufs[d->out_buf].domain];
  ASV_REQUIRE(dm.kind == 2 && dm.valid && dm.shift == 1 && dm.width == (net->feat_dim - 1) / 2 && dm.width >= 1 && dm.pitch > dm.width,
              "front_conv: the output must live on the unpadded grid of time shift 1 and width (feat_dim - 1) / 2 = %d (asv_net_define_grid_valid)", (net->feat_dim - 1) / 2);
  ASV_REQUIRE(d->weight != nullptr && d->bias != nullptr, "front_conv: null weight or bias");
  Op op; op.kind = OP_FRONT_CONV; op.front = *d;
  ASV_ON_DEVICE(net->device);
  int rc;
  if ((rc = upload_padded(net, d->weight, d->out_ch * 9, round_up(d->out_ch, kChanAlign) * 9, 0.0f, &op.scale))) return rc;
  if ((rc = upload_padded(net, d->bias, d->out_ch, round_up(d->out_ch, kChanAlign), 0.0f, &op.bias))) return rc;
  op.front.weight = nullptr; op.front.bias = nullptr;
  describe(op, "front_conv %d -> %d channels=%d\n", op.front.in_buf, op.front.out_buf, op.front.out_ch);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_posenc(asv_net_t *net, const asv_posenc_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_posenc", true)) return rc;
  int rc;
  if ((rc = check_view(net, d->in_buf, d->in_ch_off, d->channels, "posenc input")) || (rc = check_view(net, d->out_buf, d->out_ch_off, d->channels, "posenc output"))) return rc;
  const int dom = net->bufs[d->in_buf].domain;
  ASV_REQUIRE(net->is_sequence(dom), "posenc: frames and sequence domains only (one row per position)");
  ASV_REQUIRE(net->bufs[d->out_buf].domain == dom && d->out_buf != 0, "posenc: bad output buffer (the input's domain, never the feature buffer)");
  const Slice in{d->in_buf, d->in_ch_off, d->channels}, out{d->out_buf, d->out_ch_off, d->channels};
  if ((rc = check_padded_view(net, "posenc", "", in)) || (rc = check_padded_view(net, "posenc", "", out)) || (rc = check_in_place_or_disjoint("posenc", in, out))) return rc;
  ASV_REQUIRE(d->pe != nullptr && d->pe_rows >= 1 && d->pe_rows <= (1 << 20), "posenc: null table or pe_rows %d", d->pe_rows);
  ASV_REQUIRE(std::isfinite(d->scale), "posenc: scale %g", (double)d->scale);
  Op op; op.kind = OP_POSENC; op.pos = *d;
  ASV_ON_DEVICE(net->device);
  const int ld = round_up(d->channels, kChanAlign);
  std::vector<float> tab((size_t)d->pe_rows * ld, 0.0f);
  for (int r = 0; r < d->pe_rows; ++r) memcpy(&tab[(size_t)r * ld], d->pe + (size_t)r * d->channels, (size_t)d->channels * sizeof(float));
  void *dev = nullptr;
  if ((rc = upload_vec(net, tab, &dev))) return rc;
  op.scale = reinterpret_cast<float *>(dev);
  op.pos.pe = nullptr;
  describe(op, "posenc %d[%d:+%d] -> %d[%d] scale=%g positions=%d\n", op.pos.in_buf, op.pos.in_ch_off, op.pos.channels, op.pos.out_buf,
           op.pos.out_ch_off, (double)op.pos.scale, op.pos.pe_rows);
  net->ops.push_back(op);
  return ASV_OK;
}

int asv_net_add_self_attention(asv_net_t *net, const asv_self_attention_desc_t *d) {
  if (int rc = add_prologue(net, d, "asv_net_add_self_attention", true)) return rc;
  ASV_REQUIRE(d->heads >= 1 && d->heads <= 4096, "self_attention: %d heads (1 .. 4096)", d->heads);
  ASV_REQUIRE(d->d_k >= 16 && d->d_k <= kAttentionMaxDk && d->d_k % 16 == 0, "self_attention: d_k %d (a multiple of 16 up to %d)", d->d_k, kAttentionMaxDk);
  const int ch = d->heads * d->d_k;
  int rc;
  if ((rc = check_view(net, d->q_buf, d->q_ch_off, ch, "self_attention q"))) return rc;
  if ((rc = check_view(net, d->k_buf, d->k_ch_off, ch, "self_attention k"))) return rc;
  if ((rc = check_view(net, d->v_buf, d->v_ch_off, ch, "self_attention v"))) return rc;
  if ((rc = check_view(net, d->out_buf, d->out_ch_off, ch, "self_attention out"))) return rc;
  const int dom = net->bufs[d->q_buf].domain;
  ASV_REQUIRE(net->is_sequence(dom), "self_attention: frames and sequence domains only (one row per position)");
  ASV_REQUIRE(net->bufs[d->k_buf].domain == dom && net->bufs[d->v_buf].domain == dom && net->bufs[d->out_buf].domain == dom && d->out_buf != 0,
              "self_attention: q, k, v and out must share one domain, and out is never the feature buffer");
  const Slice ins[3] = {{d->q_buf, d->q_ch_off, ch}, {d->k_buf, d->k_ch_off, ch}, {d->v_buf, d->v_ch_off, ch}};
  for (int i = 0; i < 3; ++i)
    ASV_REQUIRE(disjoint(ins[i], {d->out_buf, d->out_ch_off, ch}), "self_attention: the out view overlaps the %s view", i == 0 ? "q" : (i == 1 ? "k" : "v"));
  Op op; op.kind = OP_ATTENTION; op.sa = *d;
  describe(op, "self_attention q=%d[%d] k=%d[%d] v=%d[%d] heads=%d d_k=%d -> %d[%d]\n", op.sa.q_buf, op.sa.q_ch_off, op.sa.k_buf, op.sa.k_ch_off,
           op.sa.v_buf, op.sa.v_ch_off, op.sa.heads, op.sa.d_k, op.sa.out_buf, op.sa.out_ch_off);
  net->ops.push_back(op);
  return ASV_OK;
}

// ---- asv_net_finalize: which ops fuse.  out_buf: the program's result buffer, which every pass leaves alone

// no op but `reader` reads buffer `buf`
static bool sole_reader(const asv_net *net, int out_buf, int buf, size_t reader) {
  if (buf == out_buf) return false;
  for (size_t k = 0; k < net->ops.size(); ++k)
    if (k != reader && op_reads(net->ops[k], buf)) return false;
  return true;
}

// a frame-level layer of the wide kernels with the plain epilogue: no second input, per-segment term or residual, at most a ReLU
// (x3_needs_lo: an f32x chain member also needs its lo halves)
static bool plain_frames_layer(const asv_net *net, const Op &o, bool x3_needs_lo) {
  const auto &d = o.tdnn;
  return o.kind == OP_TDNN && !o.utts && o.wfrag != nullptr && (!x3_needs_lo || !net->x3() || o.wlo != nullptr) && net->bufs[d.in_buf].domain == ASV_DOMAIN_FRAMES &&
         d.in2_buf < 0 && d.seg_bias_buf < 0 && d.seg_scale_buf < 0 && d.res_buf < 0 && !d.affine_first && d.act2 == ASV_ACT_NONE &&
         (d.act1 == ASV_ACT_NONE || d.act1 == ASV_ACT_RELU);
}

// fuse "layer -> StatisticsPooling" when the layer's output has no other reader: the 157 MB tensor
// (C2: 52k frames x 1500 channels) is then never written to or re-read from HBM
static void fuse_pools(asv_net *net, int out_buf) {
  if ((net->flags & ASV_FLAG_NO_FUSE) != 0 || !(net->frames_h16() || net->x3())) return;
  for (size_t i = 0; i + 1 < net->ops.size(); ++i) {
    Op &a = net->ops[i], &b = net->ops[i + 1];
    if (b.kind != OP_POOL || !plain_frames_layer(net, a, false)) continue;
    const auto &d = a.tdnn; const auto &q = b.pool;
    if (q.in_buf != d.out_buf || q.in_ch_off != d.out_ch_off || q.channels != d.out_ch || q.per_bin) continue;
    bool other_reader = false;
    for (size_t k = 0; k < net->ops.size(); ++k) other_reader |= k != i && k != i + 1 && op_reads(net->ops[k], d.out_buf);
    if (other_reader || d.out_buf == out_buf) continue;
    a.fused_pool = (int)(i + 1);
    b.skipped = true;
  }
}

// Fold the eval BatchNorm y = s u + t of every layer of the chain head .. l but the last into its (1-tap) consumer:
//   W (s u + t) + b = (W diag s) u + (W t + b)          - exact in real arithmetic; the products W s are rounded to the
// 16-bit element type once, here, instead of s u + t being rounded per value in the kernel.  The producing layer's
// epilogue inside the chain kernel is then ReLU + conversion alone (kernels_tdnn_chain.hip store_Y).  The per-layer
// path (ASV_FLAG_NO_CHAIN, batches the chain cannot take) keeps the unfolded weights: both are uploaded.
static int fold_chain_affines(asv_net *net, size_t head, size_t l) {
  static const bool no_fold = getenv("ASV_AMD_CHAIN_FOLD") != nullptr && atoi(getenv("ASV_AMD_CHAIN_FOLD")) == 0;
  for (size_t k = head + 1; k <= l && !no_fold; ++k) {
    Op &cur = net->ops[k];
    const Op &prev = net->ops[k - 1];
    if (!prev.has_affine || prev.host_scale.empty() || cur.host_w.empty()) continue;
    const int out_ch = cur.tdnn.out_ch, in_ch = cur.tdnn.in_ch;
    std::vector<float> wf((size_t)out_ch * in_ch), bf((size_t)cur.cout_pad, 0.0f);
    fold_affine_into(cur.host_w.data(), cur.host_bias.data(), prev.host_scale.data(), prev.host_shift.data(), out_ch, in_ch, wf.data(), bf.data());
    const int tap0 = 0;
    if (net->x3() && net->x3_et() == ET_F16) cur.w_scale_fold = x3_weight_scale(wf.data(), wf.size());
    const TapWeights tw{wf.data(), out_ch, in_ch, 1, 0, &tap0, 1, cur.w_scale_fold};
    const FragForms f = pack_frag_forms(tw, cur.cout_pad, cur.cin_pad, net->x3() ? net->x3_et() : net->frames_et(), net->x3(), net->x3_mx());
    ASV_ON_DEVICE(net->device);
    int rc;
    if (net->x3() && (rc = upload_vec(net, f.lo, &cur.wlo_fold))) return rc;
    if (net->x3_mx() && (rc = upload_vec(net, f.w8, &cur.w8_fold))) return rc;
    if ((rc = upload_vec(net, f.hi, &cur.wfrag_fold))) return rc;
    void *bdev = nullptr;
    if ((rc = upload_vec(net, bf, &bdev))) return rc;
    cur.bias_fold = reinterpret_cast<float *>(bdev);
  }
  return ASV_OK;
}

// chains "layer -> 512, [1-tap 512 -> 512]*, 1-tap + fused pooling" whose intermediate tensors nobody else reads run as
// ONE kernel with the 128 x 512 tiles resident in LDS (x-vector: tdnn3 -> tdnn4 -> tdnn5 -> pooling)
static int build_chains(asv_net *net, int out_buf) {
  if ((net->flags & (ASV_FLAG_NO_FUSE | ASV_FLAG_NO_CHAIN)) != 0 || !(net->frames_h16() || (net->x3() && net->x3_terms() == 7))) return ASV_OK;
  auto from_resident = [&](const Op &o) {            // 1-tap layer that consumes a whole 512-channel buffer
    const auto &d = o.tdnn;
    return d.n_taps == 1 && d.taps[0] == 0 && d.in_ch == kChainWidth && d.in_ch_off == 0 && net->bufs[d.in_buf].channels == kChainWidth;
  };
  for (size_t l = 1; l < net->ops.size(); ++l) {
    Op &last = net->ops[l];
    if (!plain_frames_layer(net, last, true) || last.fused_pool < 0 || !from_resident(last)) continue;
    size_t head = l;
    while (head > 0 && l - head < 3) {
      const Op &prev = net->ops[head - 1], &cur = net->ops[head];
      if (!plain_frames_layer(net, prev, true) || prev.fused_pool >= 0 || prev.tdnn.out_buf != cur.tdnn.in_buf || prev.tdnn.out_ch_off != 0 || prev.tdnn.out_ch != kChainWidth ||
          prev.cout_pad != kChainWidth || !sole_reader(net, out_buf, prev.tdnn.out_buf, head)) break;
      --head;
      if (!from_resident(prev)) break;               // any-tap layer: it can only be the chain's first
    }
    const Op &first = net->ops[head];
    if (head == l || first.cin_pad % 64 != 0 || first.cin_pad < 64) continue;
    bool mids_ok = true;
    for (size_t k = head + 1; k < l; ++k) mids_ok &= from_resident(net->ops[k]);
    if (!mids_ok) continue;
    net->ops[head].chain_last = (int)l;
    if (int rc = fold_chain_affines(net, head, l)) return rc;
  }
  return ASV_OK;
}

// f32m: a frame-level TDNN layer whose whole output buffer is read by exactly one other TDNN layer, as its input rows, may hand it over
// as IMAGES (the split [hi halves | x_lo8 | x_hi8] the reader would otherwise make of the f32 rows per workgroup and chunk): recorded
// here, decided per run (run_tdnn_layer: both kernels must be the image-capable ones for that batch)
static void mark_image_readers(asv_net *net, int out_buf) {
  if (!net->x3_mx()) return;
  for (size_t i = 0; i + 1 < net->ops.size(); ++i) {
    Op &o = net->ops[i];
    if (o.kind != OP_TDNN || o.utts || o.w8 == nullptr || o.fused_pool >= 0 || o.chain_last >= 0) continue;
    const auto &d = o.tdnn;
    const Buffer &b = net->bufs[d.out_buf];
    if (b.domain != ASV_DOMAIN_FRAMES || d.out_ch_off != 0 || d.out_ch != b.channels || b.channels % 32 != 0 || d.res_buf >= 0) continue;
    bool inside_chain = false;
    for (size_t h = 0; h < i; ++h) inside_chain |= net->ops[h].chain_last >= (int)i;
    if (inside_chain) continue;
    for (size_t j = i + 1; j < net->ops.size(); ++j) {
      const Op &r = net->ops[j];
      if (r.kind != OP_TDNN || r.tdnn.in_buf != d.out_buf) continue;
      const auto &rd = r.tdnn;
      const bool clean = rd.in_ch_off == 0 && rd.in_ch == b.channels && rd.in2_buf < 0 && rd.res_buf != d.out_buf && rd.seg_bias_buf != d.out_buf &&
                         rd.seg_scale_buf != d.out_buf && !r.utts && (r.chain_last >= 0 || (r.w8 != nullptr && r.fused_pool < 0));
      if (clean && sole_reader(net, out_buf, d.out_buf, j)) o.image_reader = (int)j;
      break;
    }
  }
}

int asv_net_finalize(asv_net_t *net, int out_buf, int embed_dim) {
  ASV_REQUIRE(net && !net->finalized, "asv_net_finalize: net is null or already finalized");
  ASV_REQUIRE(out_buf > 0 && out_buf < (int)net->bufs.size() && net->is_utts(net->bufs[out_buf].domain),
              "asv_net_finalize: output must be an utts-domain buffer");
  ASV_REQUIRE(embed_dim >= 1 && embed_dim <= net->bufs[out_buf].channels, "asv_net_finalize: embed_dim %d", embed_dim);
  ASV_REQUIRE(!net->ops.empty(), "asv_net_finalize: empty program");
  fuse_pools(net, out_buf);
  if (int rc = build_chains(net, out_buf)) return rc;
  mark_image_readers(net, out_buf);
  for (Op &o : net->ops) {                       // the host copies have served their purpose
    std::vector<float>().swap(o.host_w); std::vector<float>().swap(o.host_bias);
    std::vector<float>().swap(o.host_scale); std::vector<float>().swap(o.host_shift);
  }
  net->out_buf = out_buf; net->embed_dim = embed_dim; net->finalized = true;
  net->arena.resize(net->bufs.size());
  return ASV_OK;
}

int asv_net_embed_dim(const asv_net_t *net) { return net ? net->embed_dim : ASV_EINVAL; }

int asv_net_status_async(asv_net_t *net, unsigned *host_status, void *stream) {
  ASV_REQUIRE(net != nullptr && host_status != nullptr, "asv_net_status_async: null argument");
  ASV_ON_DEVICE(net->device);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ASV_HIP_CHECK(hipMemcpyAsync(host_status, status_word(net), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ASV_HIP_CHECK(hipMemsetAsync(status_word(net), 0, sizeof(uint32_t), s));
  return ASV_OK;
}

int asv_net_status(asv_net_t *net, unsigned *status, void *stream) {
  ASV_REQUIRE(net != nullptr && status != nullptr, "asv_net_status: null argument");
  ASV_ON_DEVICE(net->device);
  uint32_t word = 0;
  if (int rc = asv_net_status_async(net, &word, stream)) return rc;
  ASV_HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  *status = word;
  return ASV_OK;
}

size_t asv_net_device_bytes(const asv_net_t *net) {
  if (!net) return 0;
  size_t n = net->weight_bytes + net->meta_dev.cap + net->rowmeta_dev.cap;
  for (auto &m : net->arena) n += m.cap;
  return n;
}

int asv_net_describe(const asv_net_t *net, char *buf, size_t cap) {
  if (!net || !buf || cap == 0) return ASV_EINVAL;
  std::string s;
  char line[512];
  snprintf(line, sizeof(line), "asv_net precision=%s flags=%u feat_dim=%d buffers=%zu ops=%zu out=%d embed_dim=%d\n",
           net->precision == ASV_PREC_BF16 ? "bf16" : (net->precision == ASV_PREC_F16 ? "f16" : (net->precision == ASV_PREC_F32X ? "f32x" : "f32")), net->flags, net->feat_dim, net->bufs.size(), net->ops.size(), net->out_buf, net->embed_dim);
  s += line;
  for (size_t i = 0; i < net->bufs.size(); ++i) {
    const Domain &dm = net->domains[net->bufs[i].domain];
    char dname[64];
    if (dm.kind == 2 && dm.reach == 2) snprintf(dname, sizeof(dname), "grid(T/%d x %d, pitch %d, reach 2)", 1 << dm.shift, dm.width, dm.pitch);
    else if (dm.kind == 2 && dm.valid) snprintf(dname, sizeof(dname), "grid(%d unpadded stride-2 stages x %d, pitch %d)", dm.shift, dm.width, dm.pitch);
    else if (dm.kind == 2) snprintf(dname, sizeof(dname), "grid(T/%d x %d, pitch %d)", 1 << dm.shift, dm.width, dm.pitch);
    else snprintf(dname, sizeof(dname), "%s", dm.kind == ASV_DOMAIN_FRAMES ? "frames" : "utts");
    snprintf(line, sizeof(line), "  buf %zu: %s channels=%d ld=%d\n", i, dname, net->bufs[i].channels, net->bufs[i].ld);
    s += line;
  }
  for (size_t i = 0; i < net->ops.size(); ++i) {
    snprintf(line, sizeof(line), "  op %zu: %s", i, net->ops[i].desc.c_str());
    s += line;
  }
  const size_t n = std::min(cap - 1, s.size());
  memcpy(buf, s.data(), n);
  buf[n] = 0;
  return (int)n;
}

int asv_net_set_profiling(asv_net_t *net, int enable) {
  ASV_REQUIRE(net != nullptr, "asv_net_set_profiling: null net");
  net->profiling = enable;
  return ASV_OK;
}

int asv_net_get_profile(asv_net_t *net, asv_kernel_time_t *rows, int cap, int *n_rows) {
  ASV_REQUIRE(net && rows && n_rows && cap >= 1, "asv_net_get_profile: bad arguments");
  ASV_ON_DEVICE(net->device);
  std::map<std::pair<int, int>, asv_kernel_time_t> agg;      // (kernel class, op or -1)
  for (auto &st : net->stamps) {
    ASV_HIP_CHECK(hipEventSynchronize(st.b));
    float ms = 0.0f;
    ASV_HIP_CHECK(hipEventElapsedTime(&ms, st.a, st.b));
    const int op = net->profiling == 2 ? st.op : -1;
    auto it = agg.find({st.kclass, op});
    if (it == agg.end()) {
      asv_kernel_time_t row;
      memset(&row, 0, sizeof(row));
      snprintf(row.name, sizeof(row.name), "%s", kKernelNames[st.kclass]);
      row.op_index = op;
      it = agg.emplace(std::make_pair(st.kclass, op), row).first;
    }
    it->second.launches += st.launches;
    it->second.total_ms += ms;
    it->second.flops += st.flops;
    net->event_pool.push_back(st.a);
    net->event_pool.push_back(st.b);
  }
  net->stamps.clear();
  int n = 0;
  for (auto &kv : agg)
    if (n < cap) rows[n++] = kv.second;
  *n_rows = n;
  return ASV_OK;
}

}  // extern "C"
