// All-pairs score matrices of the PLDA back-end in float64 on the matrix cores:
//     C[i][j] = sum_k A[i][k] B[j][k] + row[i] + col[j]
// The Kaldi-style LLR (score/pyplda/plda_base.py:109-136) and the two-covariance score (gaussian-plda-scoring.py:23-29) of every
// (enrolment, test) pair both have this shape once everything that depends on one side only has been moved out of the pair loop
// (DESIGN.md section 4.4): the preparation kernels below - one wave per vector - write the operands, the matrix kernel does the rest.
//
// Matrix kernel: v_mfma_f64_16x16x4_f64, one workgroup of 4 waves (2 x 2) per 128 x 128 tile of C, 64 x 64 per wave = 16 accumulators
// of 4 f64.  K runs in chunks of 16 through a double-buffered LDS image (one barrier per chunk; the next chunk's global loads are
// issued before the current chunk's 64 matrix instructions).  The LDS image is K-major with a pitch of 144 f64: the 64 ds_read_b64
// of a fragment (lane -> row lane & 15, k lane >> 4) fall on 32 different 8-byte words modulo 32 per half wave - no bank conflict;
// the rows of a k line are rotated by 4 per k pair (lds_rot) so that the staging stores are conflict-free as well.
// Fragment layout of the f64 instruction: A / B one f64 per lane (row or column lane & 15, k lane >> 4); C / D four f64 per lane
// at column lane & 15, row (lane >> 4) + 4 * reg - NOT the f32 16x16x4 map (row 4 * (lane >> 4) + reg).
#include <hip/hip_runtime.h>

#include "device_utils.h"

namespace asv {
namespace {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;                 // rows and columns of C per workgroup
constexpr int kPitch = kTile + 16;         // f64 per k line of the LDS image (144 = 16 mod 32: the two k lines of a half wave interleave)
constexpr int kKc = kScoreMatrixKChunk;    // 16
static_assert(kKc == 16, "the loaders below move 16 k values of a row as 8 pairs");

// 128 rows x 16 k of a row-major operand [rows][kp]: 8 lanes read the 128 bytes of a row (a pair of f64 each), 32 rows per pass
__device__ __forceinline__ void load_panel(const double *src, int rows, int kp, int row0, int k0, double2 (&regs)[4]) {
  const int t = threadIdx.x, pair = t & 7, r = t >> 3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = row0 + r + 32 * q;
    regs[q] = row < rows ? *reinterpret_cast<const double2 *>(src + (size_t)row * kp + k0 + 2 * pair) : make_double2(0.0, 0.0);
  }
}
// Row r of k line k sits at position (r + lds_rot(k)) mod 128 of the line: without the rotation the 8 lanes that stage the 8 k pairs of
// one row would write words 288 apart = the same bank (8-way); with it the 32 lanes of a half wave (4 rows x 8 pairs) write 32
// different 8-byte words modulo 32.  The two k lines a half wave reads share a rotation, so the fragment reads stay conflict-free.
__device__ __forceinline__ int lds_rot(int k) { return 4 * (k >> 1); }
__device__ __forceinline__ void store_panel(double *lds, const double2 (&regs)[4]) {
  const int t = threadIdx.x, pair = t & 7, r = t >> 3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int pos = (r + 32 * q + 4 * pair) & (kTile - 1);      // rotated by lds_rot(2 pair) = lds_rot(2 pair + 1)
    lds[(2 * pair) * kPitch + pos] = regs[q].x;
    lds[(2 * pair + 1) * kPitch + pos] = regs[q].y;
  }
}

// Two workgroups per CU (2 x 72 KiB of LDS): one's barrier and epilogue hide behind the other's matrix instructions.  Left alone the
// compiler spreads over 198 VGPRs + 128 AGPRs = one workgroup per CU; held to two waves per SIMD it needs 237 registers, no scratch.
template <typename TOut>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void score_matrix_kernel(const double *__restrict__ A, const double *__restrict__ B, const double *__restrict__ row,
                                                           const double *__restrict__ col, TOut *__restrict__ C, int m, int n, int kp) {
  __shared__ double lds_a[2][kKc * kPitch], lds_b[2][kKc * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;     // this wave's 64 x 64 corner inside the tile
  const int fr = lane & 15, fk = lane >> 4;
  f64x4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  double2 ra[4], rb[4];
  load_panel(A, m, kp, i0, 0, ra);
  load_panel(B, n, kp, j0, 0, rb);
  store_panel(lds_a[0], ra);
  store_panel(lds_b[0], rb);
  __syncthreads();
  const int chunks = kp / kKc;
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;
    if (more) {
      load_panel(A, m, kp, i0, (c + 1) * kKc, ra);
      load_panel(B, n, kp, j0, (c + 1) * kKc, rb);
    }
    const double *la = lds_a[c & 1], *lb = lds_b[c & 1];
#pragma unroll
    for (int k4 = 0; k4 < kKc; k4 += 4) {
      double fa[4], fb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) fa[a] = la[(k4 + fk) * kPitch + ((wi + 16 * a + fr + lds_rot(k4 + fk)) & (kTile - 1))];
#pragma unroll
      for (int b = 0; b < 4; ++b) fb[b] = lb[(k4 + fk) * kPitch + ((wj + 16 * b + fr + lds_rot(k4 + fk)) & (kTile - 1))];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    if (more) {
      store_panel(lds_a[(c + 1) & 1], ra);
      store_panel(lds_b[(c + 1) & 1], rb);
    }
    __syncthreads();
  }
  // C / D of the f64 instruction: column lane & 15, row (lane >> 4) + 4 * reg
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int j = j0 + wj + 16 * b + fr;
    if (j >= n) continue;
    const double cj = col ? col[j] : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wi + 16 * a + fk + 4 * r;
        if (i < m) C[(size_t)i * n + j] = (TOut)((acc[a][b][r] + row[i]) + cj);
      }
  }
}


// Enrolment side of the LLR (plda_base.py:116-118, 124, 130): with c = n psi / (n psi + 1), v = 1 + psi / (n psi + 1), mean = c e,
//   A[i] = [ mean / v | 0.5 / (1 + psi) - 0.5 / v | 0 ... ],   row[i] = -0.5 sum (log v + mean^2 / v) + 0.5 sum log(1 + psi).
// The second coefficient is evaluated as -0.5 n psi^2 / ((n psi + 1) (1 + psi) v): the same number without the difference of two
// quotients that both approach 0.5 as psi -> 0.
__global__ __launch_bounds__(256) void plda_llr_enroll_prep_kernel(const float *enroll, int n_enroll, int dim, const float *psi, const int32_t *enroll_n, double *A,
                                                                   int kp, double *row) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n_enroll) return;
  const float *g = enroll + (size_t)i * dim;
  double *a = A + (size_t)i * kp;
  const double n = enroll_n ? (double)enroll_n[i] : 1.0;
  double given = 0.0, without = 0.0;
  for (int d = lane; d < dim; d += 64) {
    const double ps = (double)psi[d];
    const double den = n * ps + 1.0;
    const double mean = n * ps / den * (double)g[d];
    const double var = 1.0 + ps / den;
    const double var0 = ps + 1.0;
    a[d] = mean / var;
    a[dim + d] = -0.5 * (n * ps * ps) / (den * var0 * var);
    given += log(var) + mean * mean / var;
    without += log(var0);
  }
  for (int d = 2 * dim + lane; d < kp; d += 64) a[d] = 0.0;
  given = wave_sum_f64(given);
  without = wave_sum_f64(without);
  if (lane == 0) row[i] = -0.5 * given + 0.5 * without;
}

// Test side of the LLR: B[j] = [ t | t^2 | 0 ... ]
__global__ __launch_bounds__(256) void plda_llr_test_prep_kernel(const float *test, int n_test, int dim, double *B, int kp) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= n_test) return;
  const float *q = test + (size_t)j * dim;
  double *b = B + (size_t)j * kp;
  for (int d = lane; d < dim; d += 64) {
    const double t = (double)q[d];
    b[d] = t;
    b[dim + d] = t * t;
  }
  for (int d = 2 * dim + lane; d < kp; d += 64) b[d] = 0.0;
}

// One side of the two-covariance score (gaussian-plda-scoring.py:23-29): with XL = X Lambda, XG = X Gamma (float64 [n][dim]),
//   enrol (cross_first):  out[i] = [ XL[i] | x_i | 0 ... ]      test:  out[j] = [ x_j | XL[j] | 0 ... ]
//   bias = <XG, x> + <x, c>
__global__ __launch_bounds__(256) void two_cov_prep_kernel(const float *x, int n, int dim, const double *xl, const double *xg, const double *c, int cross_first,
                                                           double *out, int kp, double *bias) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const size_t o = (size_t)i * dim;
  double *dst = out + (size_t)i * kp;
  double s = 0.0, sc = 0.0;
  for (int d = lane; d < dim; d += 64) {
    const double v = (double)x[o + d];
    dst[cross_first ? d : dim + d] = xl[o + d];
    dst[cross_first ? dim + d : d] = v;
    s += xg[o + d] * v;
    sc += v * c[d];
  }
  for (int d = 2 * dim + lane; d < kp; d += 64) dst[d] = 0.0;
  s = wave_sum_f64(s + sc);
  if (lane == 0) bias[i] = s;
}

}  // namespace

template <typename TOut>
int launch_score_matrix(const double *A, int m, const double *B, int n, int kp, const double *row, const double *col, TOut *C, hipStream_t s) {
  ASV_REQUIRE(A && B && row && C && m >= 1 && n >= 1 && kp >= kKc && kp % kKc == 0, "score matrix: bad argument (m %d, n %d, padded K %d)", m, n, kp);
  const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)((m + kTile - 1) / kTile));
  ASV_REQUIRE(grid.y <= 65535u, "score matrix: %d rows are more than one launch covers", m);
  hipLaunchKernelGGL((score_matrix_kernel<TOut>), grid, dim3(256), 0, s, A, B, row, col, C, m, n, kp);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}
template int launch_score_matrix<float>(const double *, int, const double *, int, int, const double *, const double *, float *, hipStream_t);
template int launch_score_matrix<double>(const double *, int, const double *, int, int, const double *, const double *, double *, hipStream_t);

int launch_plda_llr_prep(const float *enroll, int n_enroll, const float *test, int n_test, int dim, const float *psi, const int32_t *enroll_n, double *A, double *B,
                         int kp, double *row, hipStream_t s) {
  hipLaunchKernelGGL(plda_llr_enroll_prep_kernel, dim3((unsigned)((n_enroll + 3) / 4)), dim3(256), 0, s, enroll, n_enroll, dim, psi, enroll_n, A, kp, row);
  hipLaunchKernelGGL(plda_llr_test_prep_kernel, dim3((unsigned)((n_test + 3) / 4)), dim3(256), 0, s, test, n_test, dim, B, kp);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

int launch_two_cov_prep(const float *x, int n, int dim, const double *xl, const double *xg, const double *c, bool enroll_side, double *out, int kp, double *bias,
                        hipStream_t s) {
  hipLaunchKernelGGL(two_cov_prep_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, n, dim, xl, xg, c, enroll_side ? 1 : 0, out, kp, bias);
  ASV_HIP_CHECK(hipGetLastError());
  return ASV_OK;
}

}  // namespace asv
