// Stand-alone driver of csrc/weight_pack.cpp for tests/test_weight_pack_host.py (plain C++, no GPU).
// stdin:  int32 header[12] = {layout, out_ch, in_ch, tot_ctx, left_ctx, n_taps, cout_pad, cin_pad, et, scale_mode, aux0, aux1},
//         int32 taps[n_taps], int32 n_floats, float32 data[n_floats]
// stdout: float32 w_scale (scale_mode 1: x3_weight_scale of the data, else 1), then the packed bytes.
// argv[1] (optional): pack that many times and print the seconds of each repeat to stderr (the pack-time measurement).
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <vector>

#include "weight_pack.h"

using namespace asv;

enum { L_PLAIN, L_FRAGS, L_X3P, L_MX8, L_CONV2D, L_UTTS, L_CONV2D_X3, L_CONV_TAPS, L_FOLD, L_RES2 };

static bool read_all(void *dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

int main(int argc, char **argv) {
  int32_t h[12], n_floats = 0;
  if (!read_all(h, sizeof(h)) || h[5] < 0 || h[5] > 64) return 2;
  const int layout = h[0], out_ch = h[1], in_ch = h[2], tot_ctx = h[3], left_ctx = h[4], n_taps = h[5], cout_pad = h[6], cin_pad = h[7], et = h[8], aux0 = h[10], aux1 = h[11];
  std::vector<int32_t> taps(n_taps);
  if (!read_all(taps.data(), n_taps * sizeof(int32_t)) || !read_all(&n_floats, 4) || n_floats < 0) return 2;
  std::vector<float> w(n_floats);
  if (!read_all(w.data(), (size_t)n_floats * 4)) return 2;
  const size_t n_w = layout == L_FOLD ? (size_t)out_ch * in_ch : layout == L_RES2 ? (size_t)aux0 * out_ch * out_ch * (2 * aux1 + 1) : (size_t)out_ch * in_ch * tot_ctx;
  if ((size_t)n_floats < n_w + (layout == L_FOLD ? (size_t)out_ch + 2 * in_ch : 0)) return 2;
  for (int t = 0; t < n_taps; ++t)
    if (taps[t] - left_ctx < 0 || taps[t] - left_ctx >= tot_ctx) return 2;
  const float w_scale = h[9] == 1 ? x3_weight_scale(w.data(), n_w) : 1.0f;
  const TapWeights s{w.data(), out_ch, in_ch, tot_ctx, left_ctx, taps.data(), n_taps, w_scale};

  std::vector<unsigned char> out;
  auto u16 = [&](size_t off) { return reinterpret_cast<uint16_t *>(out.data() + off); };
  auto bytes_of = [&](const auto &v) { out.assign(reinterpret_cast<const unsigned char *>(v.data()), reinterpret_cast<const unsigned char *>(v.data() + v.size())); };
  auto pack = [&]() {
    switch (layout) {
      case L_PLAIN:
        out.assign(tdnn_weight_bytes(cout_pad, cin_pad, n_taps, et), 0xa5);
        pack_tdnn_weight(s.w, out_ch, in_ch, tot_ctx, left_ctx, s.taps, n_taps, cout_pad, cin_pad, et, out.data());
        break;
      case L_FRAGS: {                                       // aux0: also the lo halves, behind the hi halves
        const size_t n = tdnn_weight_frag_elems(cout_pad, cin_pad, n_taps) * 2;
        out.assign(n * (aux0 ? 2 : 1), 0xa5);
        pack_tdnn_weight_frags(s.w, out_ch, in_ch, tot_ctx, left_ctx, s.taps, n_taps, cout_pad, cin_pad, u16(0), aux0 ? u16(n) : nullptr, et, w_scale);
        break;
      }
      case L_X3P: bytes_of(pack_tdnn_weight_x3p(s, cout_pad, cin_pad, et)); break;
      case L_MX8: bytes_of(pack_tdnn_weight_mx8(s, cout_pad, cin_pad)); break;
      case L_CONV2D: bytes_of(pack_grid_conv_frags(s, cin_pad, et)); break;
      case L_UTTS: {                                        // hi halves, then lo halves
        const size_t n = utts_weight_split_elems(cout_pad, cin_pad) * 2;
        out.assign(2 * n, 0xa5);
        pack_utts_weight_split(s, cout_pad, cin_pad, u16(0), u16(n));
        break;
      }
      case L_CONV2D_X3: bytes_of(pack_grid_conv_x3_frags(s, cin_pad, cout_pad, et)); break;      // cout_pad: the layer's cout_store
      case L_CONV_TAPS:                                     // aux0: nf_total; the dense weight is [out][in][n_taps]
        out.assign(grid_conv_taps_frag_bytes(cin_pad, aux0, n_taps, et), 0xa5);
        pack_grid_conv_taps(s.w, out_ch, in_ch, n_taps, cin_pad, aux0, et, out.data());
        break;
      case L_FOLD: {                                        // data = w [out][in] | bias [out] | s [in] | t [in]; out = w_out | bias_out
        const float *bias = s.w + n_w, *sp = bias + out_ch, *tp = sp + in_ch;
        out.assign((n_w + out_ch) * 4, 0xa5);
        fold_affine_into(s.w, bias, sp, tp, out_ch, in_ch, reinterpret_cast<float *>(out.data()), reinterpret_cast<float *>(out.data()) + n_w);
        break;
      }
      case L_RES2: bytes_of(pack_res2_branch_frags(s.w, out_ch, aux0, aux1, et)); break;      // out_ch: width, aux0: branches, aux1: dilation
      default: return false;
    }
    return true;
  };
  const int repeats = argc > 1 ? atoi(argv[1]) : 1;
  for (int r = 0; r < repeats; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!pack()) return 2;
    if (argc > 1) fprintf(stderr, "%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  return fwrite(&w_scale, 4, 1, stdout) == 1 && fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 3;
}
