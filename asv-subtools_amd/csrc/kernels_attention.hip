// The transformer encoder's own kernels:
//   self_attention_kernel   ragged multi-head self-attention over the rows of a sequence (asv_self_attention_desc_t)
//   posenc_kernel           y = x * scale + pe[row - first row of the segment]           (asv_posenc_desc_t)
//   front_conv_kernel       the first stage of the unpadded stride-2 front: 1 -> C channels, 3 x 3, stride 2, + ReLU, straight
//                           from the feature rows (asv_front_conv_desc_t)
//
// self_attention_kernel<ET, D32>: one workgroup of two waves per (segment, head, tile of 64 query rows); a wave owns 32 query rows.
// Keys and values of the segment stream through LDS in tiles of 64 rows with an online softmax, so any segment length works.
// Every product runs on the matrix cores in the orientation that keeps the QUERY on the lane (cdna_hip_programming.md, "an
// accumulator tile as the next MFMA's operand"):
//   S^T = K Q^T     A = a 32-key block of the K tile (LDS), B = the wave's Q rows (registers, loaded once): the 32 x 32 result has
//                   its query on the lane and its keys in the 16 registers x 2 lane halves, so the softmax statistics of a query
//                   (max, sum, rescale - all f32) are lane-local but for one exchange with lane ^ 32;
//   O^T += V^T P    A = V (16-bit: a transposed LDS image, two 8-byte reads per fragment; f32: the row-major tile, one value),
//                   B = the probabilities as they lie in the registers (16-bit: registers 8s .. 8s + 7 packed pairwise are the
//                   fragment of k-step s, whose k order 16s + 8(j >> 2) + 4h + (j & 3) the V fragment follows; f32: register g
//                   is key (g & 3) + 8 (g >> 2) + 4h of the one-value-per-lane instruction): no lane movement, no LDS round trip,
//                   and the accumulator O^T keeps the query on the lane, so the rescale by exp(m_old - m_new) is lane-local too.
// 16-bit modes: v_mfma_f32_32x32x16_{bf16,f16}; every f32-storage mode (f32, f32x, f32m): the exact v_mfma_f32_32x32x2_f32, as in
// kernels_conv_taps.hip.  Key rows at or behind the segment's end are zeros in the tile and -inf in the scores; they are never
// read from the neighbouring segment.  The workgroup of a segment's last query tile also writes the zeros of the gap rows behind
// the segment (and the one of the first segment those in front of it): the row layout's invariant.
#include "device_utils.h"

namespace asv {
namespace {

__device__ __forceinline__ int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }      // row of register g in a 32 x 32 C/D tile

template <int ET> struct AttnGeo {
  static constexpr bool H16 = ET != ET_F32;
  static constexpr int ES = H16 ? 2 : 4;                   // element size
};

// LDS bytes of one instantiation (test_attention_resources.py reads the same numbers off the compiled kernel)
template <int ET, int D32> struct AttnLds {
  static constexpr int DP = D32 * 32;
  // 16-bit: K [64][DP + 8], V^T [DP][64 + 8]; f32: K [64][DP + 1], V [64][DP + 8]
  static constexpr int K_STRIDE = ET != ET_F32 ? DP + 8 : DP + 1;
  static constexpr int V_STRIDE = ET != ET_F32 ? 64 + 8 : DP + 8;
  static constexpr int K_ELEMS = 64 * K_STRIDE;
  static constexpr int V_ELEMS = ET != ET_F32 ? DP * V_STRIDE : 64 * V_STRIDE;
  static constexpr int K_BYTES = (K_ELEMS * (ET != ET_F32 ? 2 : 4) + 15) / 16 * 16;
  static constexpr int BYTES = K_BYTES + V_ELEMS * (ET != ET_F32 ? 2 : 4);
};

template <int ET, int D32>
__global__ __launch_bounds__(128) void self_attention_kernel(const AttentionKernelParams p) {
  constexpr bool H16 = ET != ET_F32;
  using L = AttnLds<ET, D32>;
  constexpr int DP = L::DP, KS = L::K_STRIDE, VS = L::V_STRIDE;
  constexpr int NQ = H16 ? 2 * D32 : 16 * D32;             // Q fragments of a lane: 16 / 2 head columns per k-step
  __shared__ __attribute__((aligned(16))) unsigned char lds[L::BYTES];

  const int seg = blockIdx.x, tile = blockIdx.y, head = blockIdx.z;
  const int row0 = p.seg_row0[seg], len = p.seg_len[seg];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int dk = p.d_k;
  const size_t hoff = (size_t)head * dk;                   // the head's first column in every view

  // ---- the gap rows around the segment (this head's columns): zeros
  const int last_tile = len > 0 ? (len - 1) >> 6 : 0;
  if (tile == last_tile || (seg == 0 && tile == 0)) {
    const int pieces = dk / 4;                             // 4 elements per store (d_k is a multiple of 16)
    for (int pass = 0; pass < 2; ++pass) {
      int g0, g1;
      if (pass == 0) { if (tile != last_tile) continue; g0 = row0 + len; g1 = seg + 1 < p.segments ? p.seg_row0[seg + 1] : p.rows; }
      else { if (!(seg == 0 && tile == 0)) continue; g0 = 0; g1 = row0; }
      for (int i = tid; i < (g1 - g0) * pieces; i += 128) {
        const size_t at = (size_t)(g0 + i / pieces) * p.ldo + hoff + (size_t)(i % pieces) * 4;
        if constexpr (H16) *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(p.out) + at) = make_uint2(0u, 0u);
        else *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.out) + at) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
  }
  if (tile * 64 >= len) return;                            // (grid.y covers the longest segment of the batch)

  // ---- the wave's queries: lane (r, h) holds its part of row q of Q for every k-step
  const int q = tile * 64 + wave * 32 + r;
  const bool q_ok = q < len;
  uint4 qf16[H16 ? NQ : 1];
  float qf32[H16 ? 1 : NQ];
  if constexpr (H16) {
#pragma unroll
    for (int ks = 0; ks < NQ; ++ks) {
      qf16[ks] = make_uint4(0u, 0u, 0u, 0u);
      if (q_ok && ks * 16 < dk) qf16[ks] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.q) + (size_t)(row0 + q) * p.ldq + hoff + ks * 16 + 8 * h);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < NQ; ++ks) {
      qf32[ks] = 0.0f;
      if (q_ok && ks * 2 < dk) qf32[ks] = reinterpret_cast<const float *>(p.q)[(size_t)(row0 + q) * p.ldq + hoff + ks * 2 + h];
    }
  }

  f32x16_t o[D32];
#pragma unroll
  for (int db = 0; db < D32; ++db)
#pragma unroll
    for (int g = 0; g < 16; ++g) o[db][g] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;                   // running max of the scaled scores; this lane half's part of the sum

  for (int kt0 = 0; kt0 < len; kt0 += 64) {
    __syncthreads();                                       // the previous tile has been read
    // ---- stage K and V rows kt0 .. kt0 + 63: zeros behind the segment's end and behind column d_k
    if constexpr (H16) {
      uint16_t *ks_ = reinterpret_cast<uint16_t *>(lds), *vt = reinterpret_cast<uint16_t *>(lds + L::K_BYTES);
      constexpr int PIECES = DP / 8;
      for (int i = tid; i < 64 * PIECES; i += 128) {
        const int kr = i / PIECES, c = (i % PIECES) * 8;
        uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;
        if (kt0 + kr < len && c < dk) {
          const size_t grow = (size_t)(row0 + kt0 + kr);
          kv = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.k) + grow * p.ldk + hoff + c);
          vv = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.v) + grow * p.ldv + hoff + c);
        }
        *reinterpret_cast<uint4 *>(ks_ + kr * KS + c) = kv;
        const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) vt[(c + e) * VS + kr] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
      }
    } else {
      float *ks_ = reinterpret_cast<float *>(lds), *vs = reinterpret_cast<float *>(lds + L::K_BYTES);
      constexpr int PIECES = DP / 4;
      for (int i = tid; i < 64 * PIECES; i += 128) {
        const int kr = i / PIECES, c = (i % PIECES) * 4;
        float4 kv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vv = kv;
        if (kt0 + kr < len && c < dk) {
          const size_t grow = (size_t)(row0 + kt0 + kr);
          kv = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p.k) + grow * p.ldk + hoff + c);
          vv = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p.v) + grow * p.ldv + hoff + c);
        }
        float *kd = ks_ + kr * KS + c;
        kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
        *reinterpret_cast<float4 *>(vs + kr * VS + c) = vv;
      }
    }
    __syncthreads();

    // ---- S^T = K Q^T for the two 32-key blocks of the tile
    f32x16_t sc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int g = 0; g < 16; ++g) sc[kb][g] = 0.0f;
      if constexpr (H16) {
        const uint16_t *ks_ = reinterpret_cast<const uint16_t *>(lds);
#pragma unroll
        for (int ks = 0; ks < NQ; ++ks) {
          if (ks * 16 >= dk) break;
          const uint4 a = *reinterpret_cast<const uint4 *>(ks_ + (kb * 32 + r) * KS + ks * 16 + 8 * h);
          sc[kb] = mfma16<ET>(a, qf16[ks], sc[kb]);
        }
      } else {
        const float *ks_ = reinterpret_cast<const float *>(lds);
#pragma unroll
        for (int ks = 0; ks < NQ; ++ks) {
          if (ks * 2 >= dk) break;
          sc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ks_[(kb * 32 + r) * KS + ks * 2 + h], qf32[ks], sc[kb], 0, 0, 0);
        }
      }
    }

    // ---- online softmax of this lane's query over the tile's keys (f32)
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const bool k_ok = kt0 + kb * 32 + acc_row(g, h) < len;
        sc[kb][g] = k_ok ? sc[kb][g] * p.scale : -INFINITY;
        tmax = fmaxf(tmax, sc[kb][g]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m_run, tmax);                // finite: key kt0 of the tile is inside the segment
    const float corr = expf(m_run - m_new);                // 0 on the first tile (m_run = -inf)
    float psum = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        sc[kb][g] = expf(sc[kb][g] - m_new);               // exp(-inf) = 0 for the masked keys
        psum += sc[kb][g];
      }
    l_run = l_run * corr + psum;
    m_run = m_new;
#pragma unroll
    for (int db = 0; db < D32; ++db)
#pragma unroll
      for (int g = 0; g < 16; ++g) o[db][g] *= corr;

    // ---- O^T += V^T P
    if constexpr (H16) {
      const uint16_t *vt = reinterpret_cast<const uint16_t *>(lds + L::K_BYTES);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const uint4 b = make_uint4(pack_h16x2<ET>(sc[kb][8 * s], sc[kb][8 * s + 1]), pack_h16x2<ET>(sc[kb][8 * s + 2], sc[kb][8 * s + 3]),
                                     pack_h16x2<ET>(sc[kb][8 * s + 4], sc[kb][8 * s + 5]), pack_h16x2<ET>(sc[kb][8 * s + 6], sc[kb][8 * s + 7]));
#pragma unroll
          for (int db = 0; db < D32; ++db) {
            const uint16_t *vrow = vt + (db * 32 + r) * VS + kb * 32 + 16 * s + 4 * h;
            const uint2 lo = *reinterpret_cast<const uint2 *>(vrow), hi = *reinterpret_cast<const uint2 *>(vrow + 8);
            o[db] = mfma16<ET>(make_uint4(lo.x, lo.y, hi.x, hi.y), b, o[db]);
          }
        }
    } else {
      const float *vs = reinterpret_cast<const float *>(lds + L::K_BYTES);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int g = 0; g < 16; ++g)
#pragma unroll
          for (int db = 0; db < D32; ++db)
            o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vs[(kb * 32 + acc_row(g, h)) * VS + db * 32 + r], sc[kb][g], o[db], 0, 0, 0);
    }
  }

  // ---- out[q][head columns] = O / sum; lane (r, h) holds columns db * 32 + 8 i + 4 h .. + 3 in registers 4 i .. 4 i + 3
  const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
  if (!q_ok) return;
#pragma unroll
  for (int db = 0; db < D32; ++db)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = db * 32 + 8 * i + 4 * h;
      if (d >= dk) continue;
      const size_t at = (size_t)(row0 + q) * p.ldo + hoff + d;
      const float v0 = o[db][4 * i] * inv, v1 = o[db][4 * i + 1] * inv, v2 = o[db][4 * i + 2] * inv, v3 = o[db][4 * i + 3] * inv;
      if constexpr (H16) *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(p.out) + at) = make_uint2(pack_h16x2<ET>(v0, v1), pack_h16x2<ET>(v2, v3));
      else *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.out) + at) = make_float4(v0, v1, v2, v3);
    }
}

template <int ET>
int attention_dispatch(const AttentionKernelParams &p, hipStream_t s) {
  const dim3 grid((unsigned)p.segments, (unsigned)((p.max_len + 63) / 64), (unsigned)p.heads), block(128);
  const int d32 = (p.d_k + 31) / 32;
  if (d32 == 1) hipLaunchKernelGGL((self_attention_kernel<ET, 1>), grid, block, 0, s, p);
  else if (d32 == 2) hipLaunchKernelGGL((self_attention_kernel<ET, 2>), grid, block, 0, s, p);
  else if (d32 == 3) hipLaunchKernelGGL((self_attention_kernel<ET, 3>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((self_attention_kernel<ET, 4>), grid, block, 0, s, p);
  return ASV_OK;
}

// ---- positional encoding: one thread per (row, 16-byte piece)
template <int ET>
__global__ __launch_bounds__(256) void posenc_kernel(const PosencKernelParams p) {
  constexpr int VEC = (ET != ET_F32) ? 8 : 4;
  const int pieces = (p.channels + VEC - 1) / VEC;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)p.rows * pieces) return;
  const int row = (int)(gid / pieces), ch = (int)(gid % pieces) * VEC;
  float v[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) v[i] = 0.0f;
  if ((p.row_valid[row >> 5] >> (row & 31)) & 1u) {
    const int seg = p.row_seg[row];
    const float *pe = p.pe + (size_t)(row - p.seg_row0[seg]) * p.ld_pe + ch;       // [pe_rows][ld_pe], zeros behind the channels
    if constexpr (ET != ET_F32) unpack_h16x8<ET>(*reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(p.in) + (size_t)row * p.ldi + ch), v);
    else { const float4 f = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(p.in) + (size_t)row * p.ldi + ch); v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w; }
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = ch + i < p.channels ? fmaf(v[i], p.scale, pe[i]) : 0.0f;
  }
  if constexpr (ET != ET_F32) *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(p.out) + (size_t)row * p.ldo + ch) = pack_h16x8<ET>(v);
  else *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.out) + (size_t)row * p.ldo + ch) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- first stage of the unpadded stride-2 front: out[(t, f)][c] = relu(b[c] + sum_{i, j < 3} w[c][3 i + j] x[2 t + i][2 f + j]).
// One thread per (grid row, 16-byte piece of channels); the nine features of a position are read by every thread of the row (L1).
// The products are accumulated in f32 in tap order (i outer), each an fma.
template <int ET>
__global__ __launch_bounds__(256) void front_conv_kernel(const FrontConvParams p) {
  constexpr int VEC = (ET != ET_F32) ? 8 : 4;
  const int pieces = p.ldo / VEC;                          // the pad channels of the pitch are written as zeros
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)p.rows * pieces) return;
  const int row = (int)(gid / pieces), ch = (int)(gid % pieces) * VEC;
  float v[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) v[i] = 0.0f;
  if ((p.row_valid[row >> 5] >> (row & 31)) & 1u) {
    const int seg = p.row_seg[row], rel = row - p.g_row0[seg];
    const int t = rel / p.pitch, f = rel % p.pitch;        // a valid row: f < width, so 2 f + 2 < feat_dim, and 2 t + 2 < the segment's frames
    float x[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) x[3 * i + j] = load_elem<ET>(p.x, (size_t)(p.fr_row0[seg] + 2 * t + i) * p.ldx + 2 * f + j);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int c = ch + e;
      if (c >= p.channels) continue;
      float acc = p.bias[c];
#pragma unroll
      for (int k = 0; k < 9; ++k) acc = fmaf(p.w[c * 9 + k], x[k], acc);
      v[e] = fmaxf(acc, 0.0f);
    }
  }
  if constexpr (ET != ET_F32) *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(p.out) + (size_t)row * p.ldo + ch) = pack_h16x8<ET>(v);
  else *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.out) + (size_t)row * p.ldo + ch) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace

int launch_self_attention(const AttentionKernelParams &p, int et, hipStream_t s) {
  ASV_REQUIRE(p.d_k >= 16 && p.d_k <= kAttentionMaxDk && p.d_k % 16 == 0, "self_attention: d_k %d (a multiple of 16 up to %d)", p.d_k, kAttentionMaxDk);
  ASV_REQUIRE(p.heads >= 1 && p.heads <= 65535, "self_attention: %d heads", p.heads);
  if (p.segments <= 0 || p.max_len <= 0) return ASV_OK;
  ASV_REQUIRE((p.max_len + 63) / 64 <= 65535, "self_attention: a segment of %d rows (at most %d)", p.max_len, 65535 * 64);
  if (et == ET_BF16) attention_dispatch<ET_BF16>(p, s);
  else if (et == ET_F16) attention_dispatch<ET_F16>(p, s);
  else attention_dispatch<ET_F32>(p, s);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

int launch_posenc(const PosencKernelParams &p, int et, hipStream_t s) {
  if (p.rows <= 0) return ASV_OK;
  const int vec = et != ET_F32 ? 8 : 4;
  const long long n = (long long)p.rows * ((p.channels + vec - 1) / vec);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (et == ET_BF16) hipLaunchKernelGGL(posenc_kernel<ET_BF16>, grid, block, 0, s, p);
  else if (et == ET_F16) hipLaunchKernelGGL(posenc_kernel<ET_F16>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(posenc_kernel<ET_F32>, grid, block, 0, s, p);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

int launch_front_conv(const FrontConvParams &p, int et, hipStream_t s) {
  if (p.rows <= 0) return ASV_OK;
  const int vec = et != ET_F32 ? 8 : 4;
  const long long n = (long long)p.rows * (p.ldo / vec);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (et == ET_BF16) hipLaunchKernelGGL(front_conv_kernel<ET_BF16>, grid, block, 0, s, p);
  else if (et == ET_F16) hipLaunchKernelGGL(front_conv_kernel<ET_F16>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(front_conv_kernel<ET_F32>, grid, block, 0, s, p);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

}  // namespace asv
