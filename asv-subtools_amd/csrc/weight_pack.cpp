// Every host-side weight layout: one walk over the real weights (for_each_weight), one conversion (f32_to_h16_host / split_h16), and
// per layout a size function and an index function (co, t, ci) -> element offset under the comment that states the layout - the only
// documentation of what the kernels expect.  A new kernel adds its pair here (and a case to tests/test_weight_pack_host.py).
// Built with -ffp-contract=off: every operation rounded on its own, the same bytes under any compiler.
#include "weight_pack.h"

#include <algorithm>
#include <cmath>

namespace asv {

// Power of two that lifts the largest weight of a layer to [2^13, 2^14) (the half-precision split of the f32x mode): every
// weight down to 2^-15 of the largest keeps a normal lo half; the products grow by the same factor, far inside f32.
float x3_weight_scale(const float *w, size_t n) {
  float mx = 0.0f;
  for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(w[i]));
  if (!(mx > 0.0f) || !std::isfinite(mx)) return 1.0f;
  int e = 0;
  (void)std::frexp(mx, &e);                       // mx = m * 2^e, 0.5 <= m < 1
  return std::ldexp(1.0f, 14 - e);
}

// Plain order (kernels_tdnn.hip, kernels_tdnn_p8.hip, the f32 pooled-domain layers): [cout_pad][tap][cin_pad] in the element type
size_t tdnn_weight_bytes(int cout_pad, int cin_pad, int n_taps, int et) { return (size_t)cout_pad * n_taps * cin_pad * (et != ET_F32 ? 2 : 4); }
static size_t tdnn_weight_index(int n_taps, int cin_pad, int co, int t, int ci) { return ((size_t)co * n_taps + t) * cin_pad + ci; }
void pack_tdnn_weight(const float *w, int out_ch, int in_ch, int tot_ctx, int left_ctx, const int *taps, int n_taps, int cout_pad, int cin_pad, int et, void *dst) {
  memset(dst, 0, tdnn_weight_bytes(cout_pad, cin_pad, n_taps, et));
  for_each_weight(TapWeights{w, out_ch, in_ch, tot_ctx, left_ctx, taps, n_taps}, [&](int co, int t, int ci, float v) {
    const size_t idx = tdnn_weight_index(n_taps, cin_pad, co, t, ci);
    if (et != ET_F32) static_cast<uint16_t *>(dst)[idx] = f32_to_h16_host(v, et);
    else static_cast<float *>(dst)[idx] = v;
  });
}

// MFMA-fragment order for kernels_tdnn_v3.hip: [n_frag32][tap][chunk64][k_group16][lane][8];
// lane = (k half lh, channel lr): channel n_frag*32 + lr, k = chunk*64 + k_group*16 + lh*8 + e.
// et: ET_BF16 / ET_F16 = the 16-bit type of the fragments.  dst_lo (the f32x mode): the second halves w * scale - hi;
// `scale` (a power of two, exact) multiplies every weight first - the half-precision split uses it to lift the weights of a
// layer into the upper part of the half range, where hi AND lo are normal numbers (22 significant bits together); the
// kernel's epilogue multiplies the accumulator by 1 / scale (exact).
size_t tdnn_weight_frag_elems(int cout_pad, int cin_pad, int n_taps) { return (size_t)cout_pad * n_taps * round_up(cin_pad, 64); }
static size_t tdnn_weight_frag_index(int n_taps, int cin_pad, int co, int t, int ci) {
  const int nchunks = round_up(cin_pad, 64) / 64, nf = co / 32, lr = co % 32, c = ci / 64, kg = (ci % 64) / 16, lh = (ci % 16) / 8, e = ci % 8;
  return ((((size_t)nf * n_taps + t) * nchunks + c) * 4 + kg) * 512 + (size_t)(lh * 32 + lr) * 8 + e;
}
void pack_tdnn_weight_frags(const float *w, int out_ch, int in_ch, int tot_ctx, int left_ctx, const int *taps, int n_taps,
                            int cout_pad, int cin_pad, uint16_t *dst, uint16_t *dst_lo, int et, float scale) {
  memset(dst, 0, tdnn_weight_frag_elems(cout_pad, cin_pad, n_taps) * 2);
  if (dst_lo) memset(dst_lo, 0, tdnn_weight_frag_elems(cout_pad, cin_pad, n_taps) * 2);
  for_each_weight(TapWeights{w, out_ch, in_ch, tot_ctx, left_ctx, taps, n_taps, scale}, [&](int co, int t, int ci, float v) {
    const size_t idx = tdnn_weight_frag_index(n_taps, cin_pad, co, t, ci);
    const HiLo h = split_h16(v, et);
    dst[idx] = h.hi;
    if (dst_lo) dst_lo[idx] = h.lo;                 // f32x mode: w = hi + lo
  });
}

// Plain order for kernels_tdnn_p8x.hip (the weight half-tiles arrive by LDS-DMA, 128-byte rows): [cout_pad][tap][chunk32][hi 32 | lo 32],
// the same halves of w * scale as pack_tdnn_weight_frags writes (the two kernels give the same bits)
size_t tdnn_weight_x3p_elems(int cout_pad, int cin_pad, int n_taps) { return (size_t)cout_pad * n_taps * (cin_pad / 32) * 64; }
static size_t tdnn_weight_x3p_index(int n_taps, int cin_pad, int co, int t, int ci) {           // of the hi half; the lo half 32 behind it
  return (((size_t)co * n_taps + t) * (cin_pad / 32) + ci / 32) * 64 + ci % 32;
}
std::vector<uint16_t> pack_tdnn_weight_x3p(const TapWeights &s, int cout_pad, int cin_pad, int et) {
  std::vector<uint16_t> dst(tdnn_weight_x3p_elems(cout_pad, cin_pad, s.n_taps), 0);
  for_each_weight(s, [&](int co, int t, int ci, float v) {
    const size_t idx = tdnn_weight_x3p_index(s.n_taps, cin_pad, co, t, ci);
    const HiLo h = split_h16(v, et);
    dst[idx] = h.hi;
    dst[idx + 32] = h.lo;
  });
  return dst;
}

// 8-bit fragments of the f32m form (kernels_tdnn_chainm.hip / kernels_tdnn_x3m.hip, the scaled 8-bit matrix instruction): for the halves
// hi = half(w * scale), lo = w * scale - hi that pack_tdnn_weight_frags splits into, two planes of
// [32-channel output fragment][tap][32-channel input group][lane = (lh, output channel lr)][16]: plane 0 = e4m3(lo 2^6) (|lo| <= 2^-11 |hi|,
// hi < 2^14 under x3_weight_scale), plane 1 = e4m3(hi 2^-6).  Byte q of lane half lh = input channel 32 group + (q < 8 ? 8 lh + q :
// 16 + 8 lh + q - 8) - the channels the lane's two half fragments of the group hold, in their order, so that a kernel may also MAKE plane 1
// from those half fragments in registers (v_cvt_scalef32_pk_fp8_f16: kernels_tdnn_x3m.hip does; the chain kernel kernels_tdnn_chainm.hip
// fetches it - 24 conversions per K step cost its waves more issue time than two more 16-byte loads, profiles/r6s_*).  The kernels' block
// scales undo the 2^6 / 2^-6.
size_t tdnn_weight_mx8_bytes(int cout_pad, int cin_pad, int n_taps) { return 2 * (size_t)(cout_pad / 32) * n_taps * ((cin_pad + 31) / 32) * 1024; }
static size_t tdnn_weight_mx8_index(int n_taps, int cin_pad, int co, int t, int ci) {           // inside a plane
  const int ngroups = (cin_pad + 31) / 32;                    // (a last, partial group is zero-padded: e4m3(0) = 0)
  const int nf = co / 32, lr = co % 32, g = ci / 32, r = ci % 32, kg = r / 16, lh = (r % 16) / 8, q = kg * 8 + r % 8;
  return (((size_t)nf * n_taps + t) * ngroups + g) * 1024 + (size_t)(lh * 32 + lr) * 16 + q;
}
std::vector<uint8_t> pack_tdnn_weight_mx8(const TapWeights &s, int cout_pad, int cin_pad) {
  std::vector<uint8_t> dst(tdnn_weight_mx8_bytes(cout_pad, cin_pad, s.n_taps), 0);
  const size_t plane = dst.size() / 2;
  for_each_weight(s, [&](int co, int t, int ci, float v) {
    const size_t at = tdnn_weight_mx8_index(s.n_taps, cin_pad, co, t, ci);
    const float hi = f16_to_f32_host(f32_to_f16_host(v));
    dst[at] = f32_to_e4m3_host((v - hi) * 64.0f);
    dst[plane + at] = f32_to_e4m3_host(hi * (1.0f / 64.0f));
  });
  return dst;
}

// Pooled-domain layers (1 tap) keep f32 activations; their GEMM runs on the bf16 matrix cores with every operand split into two bf16
// halves, the weight halves in the fragment order kernels_utts.hip walks:
// [32-channel fragment][32-k step][j][lane = (k half lh, channel lr)][8], k = 32 * step + 16 * lh + 8 * j + e
size_t utts_weight_split_elems(int cout_pad, int cin_pad) { return (size_t)(cout_pad / 32) * ((cin_pad + 31) / 32) * 1024; }
static size_t utts_weight_split_index(int cin_pad, int co, int ci) {
  const int ksteps = (cin_pad + 31) / 32, r = ci % 32;
  return (((size_t)(co / 32) * ksteps + ci / 32) * 2 + (r % 16) / 8) * 512 + (size_t)((r / 16) * 32 + co % 32) * 8 + r % 8;
}
void pack_utts_weight_split(const TapWeights &s, int cout_pad, int cin_pad, uint16_t *hi, uint16_t *lo) {
  memset(hi, 0, utts_weight_split_elems(cout_pad, cin_pad) * 2);
  memset(lo, 0, utts_weight_split_elems(cout_pad, cin_pad) * 2);
  for_each_weight(s, [&](int co, int, int ci, float v) {
    const size_t idx = utts_weight_split_index(cin_pad, co, ci);
    const HiLo h = split_h16(v, ET_BF16);
    hi[idx] = h.hi;
    lo[idx] = h.lo;
  });
}

// 3x3 trunk convolutions with 32 / 64 / 128 / 256 channels and the space-to-depth form (4 taps): fragment order of kernels_conv2d.hip,
// [tap][k-group][n-fragment][lane = (k half lh, channel lr)][8], k = kg * 16 + lh * 8 + e
size_t grid_conv_frag_elems(int cin_pad, int cout_pad32, int n_taps) { return (size_t)n_taps * (cin_pad / 16) * (cout_pad32 / 32) * 512; }
static size_t grid_conv_frag_index(int cin_pad, int nfs, int co, int t, int ci) {
  const int kgs = cin_pad / 16, kg = ci / 16, lh = (ci % 16) / 8, e = ci % 8, nf = co / 32, lr = co % 32;
  return ((size_t)(t * kgs + kg) * nfs + nf) * 512 + (size_t)(lh * 32 + lr) * 8 + e;
}
std::vector<uint16_t> pack_grid_conv_frags(const TapWeights &s, int cin_pad, int et) {
  const int nfs = (s.out_ch + 31) / 32;
  std::vector<uint16_t> dst(grid_conv_frag_elems(cin_pad, nfs * 32, s.n_taps), 0);
  for_each_weight(s, [&](int co, int t, int ci, float v) { dst[grid_conv_frag_index(cin_pad, nfs, co, t, ci)] = f32_to_h16_host(v, et); });
  return dst;
}

// f32x grid kernel (kernels_conv2d_x3.hip), chunks of 32 input channels:
// [chunk][tap][k-group][n-fragment][hi | lo][lane = (k half lh, channel lr)][8]: channel nf * 32 + lr, k = chunk * 32 + kg * 16 + lh * 8 + e;
// every weight multiplied by `scale` (a power of two) first; lo = w * scale - hi
size_t grid_conv_x3_frag_elems(int cin_pad, int cout_store, int n_taps) { return (size_t)(cin_pad / 32) * n_taps * 2 * (cout_store / 32) * 2 * 512; }
static size_t grid_conv_x3_frag_index(int n_taps, int cout_store, int co, int t, int ci) {      // of the hi half; the lo half 512 behind it
  const int nft = cout_store / 32, c = ci / 32, kg = (ci % 32) / 16, lh = (ci % 16) / 8, e = ci % 8, nf = co / 32, lr = co % 32;
  return (((((size_t)c * n_taps + t) * 2 + kg) * nft + nf) * 2) * 512 + (size_t)(lh * 32 + lr) * 8 + e;
}
std::vector<uint16_t> pack_grid_conv_x3_frags(const TapWeights &s, int cin_pad, int cout_store, int et) {
  std::vector<uint16_t> dst(grid_conv_x3_frag_elems(cin_pad, cout_store, s.n_taps), 0);
  for_each_weight(s, [&](int co, int t, int ci, float v) {
    const size_t at = grid_conv_x3_frag_index(s.n_taps, cout_store, co, t, ci);
    const HiLo h = split_h16(v, et);
    dst[at] = h.hi;
    dst[at + 512] = h.lo;
  });
  return dst;
}

// Tap-table grid convolution (kernels_conv_taps.hip):
// dense host weight w [out_ch][in_ch][n_taps] -> fragments [chunk][tap][slot pair q][32-channel fragment n][lane = (slot half lh, channel lr)][16 bytes]:
// the 4 f32 / 8 16-bit input channels chunk * (32 | 64) + (2 q + lh) * (4 | 8) + e of output channel n * 32 + lr; zeros beyond the real channels
size_t grid_conv_taps_frag_bytes(int cin_pad, int nf_total, int n_taps, int et) {
  const int chunk_ch = et == ET_F32 ? 32 : 64;
  return (size_t)((cin_pad + chunk_ch - 1) / chunk_ch) * n_taps * 4 * nf_total * 1024;
}
static size_t grid_conv_taps_frag_index(int n_taps, int nf_total, int et, int co, int t, int ci) {
  const int per = et == ET_F32 ? 4 : 8, chunk_ch = per * 8;
  const int c = ci / chunk_ch, slot = (ci % chunk_ch) / per, e = ci % per, q = slot / 2, lh = slot % 2, n = co / 32, lr = co % 32;
  return ((((size_t)(c * n_taps + t) * 4 + q) * nf_total + n) * 64 + (size_t)(lh * 32 + lr)) * per + e;
}
void pack_grid_conv_taps(const float *w, int out_ch, int in_ch, int n_taps, int cin_pad, int nf_total, int et, void *dst) {
  std::vector<int> taps(n_taps);
  for (int t = 0; t < n_taps; ++t) taps[t] = t;                 // every tap of the dense weight, in its order
  memset(dst, 0, grid_conv_taps_frag_bytes(cin_pad, nf_total, n_taps, et));
  for_each_weight(TapWeights{w, out_ch, in_ch, n_taps, 0, taps.data(), n_taps}, [&](int co, int t, int ci, float v) {
    const size_t elem = grid_conv_taps_frag_index(n_taps, nf_total, et, co, t, ci);
    if (et == ET_F32) static_cast<float *>(dst)[elem] = v;
    else static_cast<uint16_t *>(dst)[elem] = f32_to_h16_host(v, et);
  });
}

std::vector<uint16_t> pack_res2_branch_frags(const float *weight, int width, int branches, int dilation, int et) {
  const int W = width, tot = 2 * dilation + 1, taps[3] = {-dilation, 0, dilation};
  const size_t per_branch = tdnn_weight_frag_elems(W, W, 3);
  std::vector<uint16_t> frags(per_branch * branches);
  for (int b = 0; b < branches; ++b)
    pack_tdnn_weight_frags(weight + (size_t)b * W * W * tot, W, W, tot, -dilation, taps, 3, W, W, frags.data() + per_branch * b, nullptr, et);
  return frags;
}

void fold_affine_into(const float *w, const float *bias, const float *s_prev, const float *t_prev, int out_ch, int in_ch, float *w_out, float *bias_out) {
  for (int co = 0; co < out_ch; ++co) {
    double acc = bias[co];
    for (int ci = 0; ci < in_ch; ++ci) {
      const float v = w[(size_t)co * in_ch + ci];
      w_out[(size_t)co * in_ch + ci] = v * s_prev[ci];
      acc += (double)v * (double)t_prev[ci];
    }
    bias_out[co] = (float)acc;
  }
}

}  // namespace asv
