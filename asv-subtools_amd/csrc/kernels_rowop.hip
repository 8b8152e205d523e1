// The row op (asv_rowop_desc_t): the activations the GEMM epilogues do not have, and LayerNorm over the channels, as one
// memory-bound pass over the rows of a frames-, sequence- or utts-domain buffer:
//     z = in[row, 0:C];  z = z * scale0 + shift0;  z = act0(z);  [LayerNorm over the C real channels];  z = act1(z);  z = z * scale1 + shift1
//
// Layout: a row belongs to a GROUP of G = 2^k lanes of one wave (G = 64, the whole wave, from 64 16-byte pieces up; narrower rows
// share a wave, 64 / G rows each), lane l of the group holds the pieces l, l + G, l + 2 G, ... - consecutive lanes load and store
// consecutive 16 bytes - and keeps all its values in registers from the one load to the one store: up to NP pieces per lane, 48 f32
// values at kRowopMaxChannels.  Nothing goes through LDS: the two LayerNorm sums are xor butterflies over the group's lanes.
//
// Arithmetic: the per-channel affines are one fma each; the activations are f32 with the accurate library functions (expf, tanhf,
// erfcf, expm1f - no fast intrinsics), each written in the form that keeps its RELATIVE accuracy in the tails (GELU through
// erfc(-x / sqrt 2) = 1 + erf(x / sqrt 2), which does not cancel for negative x; SELU through expm1; the swishes through
// rowop_x_sigmoid) and stays finite for every finite x.  LayerNorm: mean, then the variance as the mean of (z - mean)^2 - two
// passes over the registers - with the sums, the normalisation and gamma / beta in float64, rounded to f32 once: a result that
// cancels against beta keeps the relative accuracy the 16-bit buffers' last place asks for, which f32 sums cannot give
// (DESIGN.md section 4.5); for the same reason an activation in FRONT of a LayerNorm is evaluated in float64 (rowop_activate64).
// The butterfly adds commute, so every lane of a group holds the same bits; a row's result depends on
// its own values and C alone, never on its neighbours or the batch.
//
// Rows that are not valid and the columns between C and the end of the last piece are written as zeros (eltwise_kernel's rule).
#include "device_utils.h"

namespace asv {
namespace {

template <int N, typename F>
__device__ __forceinline__ void rowop_map(float (&v)[N], F f) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = f(v[i]);
}

// x * sigmoid(t) = x / (1 + e^-t).  Below t = -40 the 1 is far under half a unit in the last place of e^-t, and e^-t overflows
// from t = -88.7 on while x e^t is still a normal number (-88 e^-89 = -2e-37): there the product is formed as (x e^(t/2)) e^(t/2),
// without an intermediate that overflows or goes subnormal before the result does.
__device__ __forceinline__ float rowop_x_sigmoid(float x, float t) {
  if (t < -40.0f) { const float h = expf(0.5f * t); return (x * h) * h; }
  return x / (1.0f + expf(-t));
}

// mish(x) = x tanh(softplus(x)), softplus(x) = x beyond torch's threshold 20 (where tanh is 1 to the last bit).  With e = e^x,
// tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1) = n / (n + 2), n = e (e + 2): the same function from ONE library call and a
// division - about one unit in the last place where expf -> log1pf -> tanhf stack three to four - relative in both tails
// (n / (n + 2) -> e for x << 0), n <= 2.4e17 at the threshold.
__device__ __forceinline__ float rowop_mish(float x) {
  if (x > 20.0f) return x;
  const float e = expf(x), n = e * (e + 2.0f);
  return x * (n / (n + 2.0f));
}

// one activation over the lane's values; the switch is wave-uniform and sits OUTSIDE the unrolled loop
template <int N>
__device__ __forceinline__ void rowop_activate(float (&v)[N], int act, float slope) {
  switch (act) {
    case ASV_ACT_RELU: rowop_map(v, [](float x) { return fmaxf(x, 0.0f); }); break;
    case ASV_ACT_TANH: rowop_map(v, [](float x) { return tanhf(x); }); break;
    case ASV_ACT_SIGMOID: rowop_map(v, [](float x) { return 1.0f / (1.0f + expf(-x)); }); break;
    case ASV_ACT_LEAKY_RELU: rowop_map(v, [slope](float x) { return x > 0.0f ? x : x * slope; }); break;
    case ASV_ACT_SELU:
      rowop_map(v, [](float x) { return 1.0507009873554804934193349852946f * (x > 0.0f ? x : 1.6732632423543772848170429916717f * expm1f(x)); });
      break;
    case ASV_ACT_MISH: rowop_map(v, [](float x) { return rowop_mish(x); }); break;
    case ASV_ACT_SWISH: rowop_map(v, [](float x) { return rowop_x_sigmoid(x, x); }); break;
    case ASV_ACT_GELU: rowop_map(v, [](float x) { return 0.5f * x * erfcf(x * -0.70710678118654752440f); }); break;
    case ASV_ACT_DOUBLE_SWISH: rowop_map(v, [](float x) { return rowop_x_sigmoid(x, x - 1.0f); }); break;
    default: break;
  }
}

// The activation in front of a LayerNorm, in float64, kept as an unevaluated f32 pair hi + lo (48 significant bits): LayerNorm
// subtracts the row mean from it, and where the difference cancels to |y| << |mean| the f32 activation's own error of ~2^-24 |a|
// is many units in the last place of a 16-bit y - one element in a few hundred thousand, measured.  Only this position pays for
// it (the LayerNorm arithmetic behind it is float64 already); leaky_relu / selu / mish / swish / double_swish have the form, relu
// is exact as it is, tanh / sigmoid / gelu keep their f32 value (lo = 0).
__device__ __forceinline__ bool rowop_act_has_f64(int act) {
  return act == ASV_ACT_LEAKY_RELU || act == ASV_ACT_SELU || act == ASV_ACT_MISH || act == ASV_ACT_SWISH || act == ASV_ACT_DOUBLE_SWISH;
}
template <int N, typename F>
__device__ __forceinline__ void rowop_map64(float (&v)[N], float (&lo)[N], F f) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double a = f((double)v[i]);
    v[i] = (float)a;
    lo[i] = (float)(a - (double)v[i]);
  }
}
template <int N>
__device__ __forceinline__ void rowop_activate64(float (&v)[N], float (&lo)[N], int act, float slope) {
  switch (act) {
    case ASV_ACT_LEAKY_RELU: rowop_map64(v, lo, [slope](double x) { return x > 0.0 ? x : x * (double)slope; }); break;
    case ASV_ACT_SELU:
      rowop_map64(v, lo, [](double x) { return 1.0507009873554804934193349852946 * (x > 0.0 ? x : 1.6732632423543772848170429916717 * expm1(x)); });
      break;
    case ASV_ACT_MISH:
      rowop_map64(v, lo, [](double x) { if (x > 20.0) return x; const double e = exp(x), n = e * (e + 2.0); return x * (n / (n + 2.0)); });
      break;
    case ASV_ACT_SWISH: rowop_map64(v, lo, [](double x) { return x / (1.0 + exp(-x)); }); break;
    case ASV_ACT_DOUBLE_SWISH: rowop_map64(v, lo, [](double x) { return x / (1.0 + exp(1.0 - x)); }); break;
    default: break;
  }
}

// sum over the 2^lanes_log2 lanes of a row's group; every lane of the group gets the same bits
__device__ __forceinline__ double rowop_group_sum(double v, int lanes_log2) {
  for (int k = lanes_log2 - 1; k >= 0; --k) v += __shfl_xor(v, 1 << k);
  return v;
}

template <int ET, int NP>
__global__ __launch_bounds__(256) void rowop_kernel(const RowopKernelParams p, int lanes_log2) {
  constexpr int VEC = (ET != ET_F32) ? 8 : 4;
  constexpr int N = NP * VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int group = 1 << lanes_log2, rows_per_wave = 64 >> lanes_log2;
  const int wave_row0 = (blockIdx.x * 4 + wave) * rows_per_wave;
  if (wave_row0 >= p.rows) return;                                  // wave-uniform: the butterflies below need every lane of a live wave
  const int row = wave_row0 + (lane >> lanes_log2), sub = lane & (group - 1);
  const bool row_ok = row < p.rows;
  const bool valid = row_ok && (p.row_valid == nullptr || ((p.row_valid[row >> 5] >> (row & 31)) & 1u));
  const int pieces = (p.channels + VEC - 1) / VEC;
  float v[N];
  auto table = [&](const float *t, int ch, float (&o)[VEC]) {        // [round_up(channels, 16)] floats, zeros behind the channels
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const float4 f = *reinterpret_cast<const float4 *>(t + ch + 4 * q);
      o[4 * q] = f.x; o[4 * q + 1] = f.y; o[4 * q + 2] = f.z; o[4 * q + 3] = f.w;
    }
  };
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int piece = j * group + sub, ch = piece * VEC;
    if (valid && piece < pieces) {
      if constexpr (ET != ET_F32) {
        unpack_h16x8<ET>(*reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.in) + (size_t)row * p.ldi + ch), &v[j * VEC]);
      } else {
        const float4 f = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p.in) + (size_t)row * p.ldi + ch);
        v[j * VEC] = f.x; v[j * VEC + 1] = f.y; v[j * VEC + 2] = f.z; v[j * VEC + 3] = f.w;
      }
      if (p.scale0 != nullptr) {
        float sc[VEC], sh[VEC];
        table(p.scale0, ch, sc); table(p.shift0, ch, sh);
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[j * VEC + i] = fmaf(v[j * VEC + i], sc[i], sh[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[j * VEC + i] = 0.0f;
    }
  }
  float lo[N];
#pragma unroll
  for (int i = 0; i < N; ++i) lo[i] = 0.0f;
  if (p.ln && rowop_act_has_f64(p.act0)) rowop_activate64(v, lo, p.act0, p.slope0);
  else rowop_activate(v, p.act0, p.slope0);
  if (p.ln) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        if ((j * group + sub) * VEC + i < p.channels) s += (double)v[j * VEC + i] + (double)lo[j * VEC + i];
    const double mu = rowop_group_sum(s, lanes_log2) / (double)p.channels;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        if ((j * group + sub) * VEC + i < p.channels) { const double d = ((double)v[j * VEC + i] - mu) + (double)lo[j * VEC + i]; q = fma(d, d, q); }
    const double var = rowop_group_sum(q, lanes_log2) / (double)p.channels;
    const double rstd = 1.0 / sqrt(var + (double)p.eps);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int piece = j * group + sub, ch = piece * VEC;
      float g[VEC], b[VEC];
      if (p.gamma != nullptr && piece < pieces) { table(p.gamma, ch, g); table(p.beta, ch, b); }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        double t = (((double)v[j * VEC + i] - mu) + (double)lo[j * VEC + i]) * rstd;
        if (p.gamma != nullptr && piece < pieces) t = fma(t, (double)g[i], (double)b[i]);
        v[j * VEC + i] = (float)t;
      }
    }
  }
  rowop_activate(v, p.act1, p.slope1);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int piece = j * group + sub, ch = piece * VEC;
    if (!row_ok || piece >= pieces) continue;
    float o[VEC];
    if (valid && p.scale1 != nullptr) {
      float sc[VEC], sh[VEC];
      table(p.scale1, ch, sc); table(p.shift1, ch, sh);
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = fmaf(v[j * VEC + i], sc[i], sh[i]);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = v[j * VEC + i];
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = (valid && ch + i < p.channels) ? o[i] : 0.0f;
    if constexpr (ET != ET_F32) {
      *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(p.out) + (size_t)row * p.ldo + ch) = pack_h16x8<ET>(o);
    } else {
      *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.out) + (size_t)row * p.ldo + ch) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int ET, int NP>
void rowop_launch(const RowopKernelParams &p, int lanes_log2, hipStream_t s) {
  const int rows_per_block = 4 * (64 >> lanes_log2);
  hipLaunchKernelGGL((rowop_kernel<ET, NP>), dim3((unsigned)((p.rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, s, p, lanes_log2);
}

template <int ET>
int rowop_dispatch(const RowopKernelParams &p, hipStream_t s) {
  constexpr int VEC = (ET != ET_F32) ? 8 : 4;
  const int pieces = (p.channels + VEC - 1) / VEC;
  if (pieces <= 64) {
    int k = 0;
    while ((1 << k) < pieces) ++k;
    rowop_launch<ET, 1>(p, k, s);
    return ASV_OK;
  }
  const int np = (pieces + 63) / 64;
  if (np <= 2) rowop_launch<ET, 2>(p, 6, s);
  else if (np <= 3) rowop_launch<ET, 3>(p, 6, s);
  else if (np <= 4) rowop_launch<ET, 4>(p, 6, s);
  else if (np <= 6) rowop_launch<ET, 6>(p, 6, s);
  else if constexpr (ET == ET_F32) {
    if (np <= 8) rowop_launch<ET, 8>(p, 6, s);
    else rowop_launch<ET, 12>(p, 6, s);
  }
  return ASV_OK;
}

}  // namespace

int launch_rowop(const RowopKernelParams &p, int et, hipStream_t s) {
  ASV_REQUIRE(p.channels >= 1 && p.channels <= kRowopMaxChannels, "rowop: %d channels (a row of at most %d lives in one wave's registers)", p.channels, kRowopMaxChannels);
  if (p.rows <= 0) return ASV_OK;
  if (et == ET_BF16) rowop_dispatch<ET_BF16>(p, s);
  else if (et == ET_F16) rowop_dispatch<ET_F16>(p, s);
  else rowop_dispatch<ET_F32>(p, s);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

}  // namespace asv
