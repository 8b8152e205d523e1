// Every host-side weight layout of libasv_amd.so: dense checkpoint weights -> the byte orders the kernels read.  Plain C++ with no
// HIP in it (tests/test_weight_pack_host.py compiles it with g++ and pins the bytes of every layout): each layout is an index
// function (co, t, ci) -> element offset plus its size function, next to the comment that states the layout (weight_pack.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "host_convert.h"

namespace asv {

struct TapWeights {            // a dense host weight [out_ch][in_ch][tot_ctx] and the taps taken from it
  const float *w; int out_ch, in_ch, tot_ctx, left_ctx; const int *taps; int n_taps;
  float scale = 1.0f;          // power of two applied to every weight first (f32x half split)
};

// f(co, t, ci, v) for every real (output channel, tap, input channel), v = the weight * s.scale
template <class F>
inline void for_each_weight(const TapWeights &s, F f) {
  for (int co = 0; co < s.out_ch; ++co)
    for (int t = 0; t < s.n_taps; ++t) {
      const float *w = s.w + (size_t)co * s.in_ch * s.tot_ctx + (s.taps[t] - s.left_ctx);
      for (int ci = 0; ci < s.in_ch; ++ci) f(co, t, ci, w[(size_t)ci * s.tot_ctx] * s.scale);
    }
}

inline uint16_t f32_to_h16_host(float f, int et) { return et == ET_F16 ? f32_to_f16_host(f) : f32_to_bf16_host(f); }
inline float h16_to_f32_host(uint16_t h, int et) { return et == ET_F16 ? f16_to_f32_host(h) : bf16_to_f32_host(h); }

struct HiLo { uint16_t hi, lo; };
inline HiLo split_h16(float v, int et) {                  // hi = h16(v), lo = h16(v - back(hi)): v = hi + lo to 16 (bf16) / 22 (half) bits
  const uint16_t hi = f32_to_h16_host(v, et);
  return {hi, f32_to_h16_host(v - h16_to_f32_host(hi, et), et)};
}

float x3_weight_scale(const float *w, size_t n);

// one layer; a destination (or the vector returned) holds the layout's size function worth of elements, zeros where no weight lands
size_t tdnn_weight_bytes(int cout_pad, int cin_pad, int n_taps, int et);
void pack_tdnn_weight(const float *w, int out_ch, int in_ch, int tot_ctx, int left_ctx, const int *taps, int n_taps, int cout_pad, int cin_pad, int et, void *dst);
size_t tdnn_weight_frag_elems(int cout_pad, int cin_pad, int n_taps);
void pack_tdnn_weight_frags(const float *w, int out_ch, int in_ch, int tot_ctx, int left_ctx, const int *taps, int n_taps,
                            int cout_pad, int cin_pad, uint16_t *dst, uint16_t *dst_lo = nullptr, int et = ET_BF16, float scale = 1.0f);
size_t tdnn_weight_x3p_elems(int cout_pad, int cin_pad, int n_taps);
std::vector<uint16_t> pack_tdnn_weight_x3p(const TapWeights &s, int cout_pad, int cin_pad, int et);
size_t tdnn_weight_mx8_bytes(int cout_pad, int cin_pad, int n_taps);
std::vector<uint8_t> pack_tdnn_weight_mx8(const TapWeights &s, int cout_pad, int cin_pad);
size_t utts_weight_split_elems(int cout_pad, int cin_pad);          // of hi and of lo, each
void pack_utts_weight_split(const TapWeights &s, int cout_pad, int cin_pad, uint16_t *hi, uint16_t *lo);
size_t grid_conv_frag_elems(int cin_pad, int cout_pad32, int n_taps = 9);
std::vector<uint16_t> pack_grid_conv_frags(const TapWeights &s, int cin_pad, int et);
size_t grid_conv_x3_frag_elems(int cin_pad, int cout_store, int n_taps);
std::vector<uint16_t> pack_grid_conv_x3_frags(const TapWeights &s, int cin_pad, int cout_store, int et);
size_t grid_conv_taps_frag_bytes(int cin_pad, int nf_total, int n_taps, int et);
void pack_grid_conv_taps(const float *w, int out_ch, int in_ch, int n_taps, int cin_pad, int nf_total, int et, void *dst);

// the fragments of the `branches` 3-tap width -> width convolutions of a Res2 block ([branch][width][width][2 dilation + 1] dense), one after the other
std::vector<uint16_t> pack_res2_branch_frags(const float *weight, int width, int branches, int dilation, int et);

// BatchNorm y = s u + t of the previous layer folded into a 1-tap layer: w_out = w diag(s_prev) (an f32 product each),
// bias_out = bias + w t_prev (a double accumulator, cast to f32 once)
void fold_affine_into(const float *w, const float *bias, const float *s_prev, const float *t_prev, int out_ch, int in_ch, float *w_out, float *bias_out);

}  // namespace asv
