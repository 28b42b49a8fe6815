// L2-regularised multinomial logistic regression (the linear-probe CLIP baseline, lpclip/linear_probe.py of the reference): one full-batch
// evaluation of
//   F(W, b) = (1/N) sum_i [logsumexp(z_i) - z_i[y_i]] + (l2/2) |W|_F^2,   z_i = W x_i + b,
// and its gradient, and the arg-max prediction.  theta = [W row-major [K, D] | b [K]], grad has the same layout.
//
// Stages of an evaluation (launch_softmax_reg_eval), all on one stream, no floating-point atomics anywhere:
//   sr_gemm<false>  Z = X W^T + b on v_mfma_f32_32x32x2_f32 (the build has no packed fp32 VALU: the matrix pipe is the fast fp32 route).
//                   Block = 4 waves, a 128 x 128 tile, each wave 2 x 2 fragments of 32 x 32; the operands go through LDS in chunks of 16
//                   of the reduction index, stored [k][row] with a pitch of 160 floats, so that the 32 lanes of a half wave read 32
//                   consecutive floats and the two halves (k, k + 1) sit 32 banks apart.  No software pipeline.  Rows, columns and the
//                   reduction are ragged: whatever lies outside is staged as zero and never stored.
//   sr_rows         one wave per row, in DOUBLE from the fp32 logits: max, log-sum-exp, loss, and R = (p - onehot) / N rounded once to
//                   fp32 over Z.  (An fp32 loss resolves 1e-7 of log K; at strong regularisation a line search needs decreases of
//                   1e-11.)  Per-block loss partials in double.
//   sr_gemm<true>   G_W partials = R^T X, the reduction over N split into `slices` row ranges (a function of N, D, K alone), one
//                   [K, D] partial per slice.  The blocks of the first column tile also add up their staged R tile: the column sums of
//                   R are G_b, per slice, in double.
//   sr_finish_a     grad = sum over slices (in slice order, in double) + l2 W, rounded once; per-block partials of max|g|, g.dir, |g|^2
//                   (of the rounded gradient) and |W|^2 in double, by a fixed tree.
//   sr_finish_b     one block adds the partials in a fixed order: stats = {F, max|g|, g.dir, |g|^2}.
// Every sum has an order that depends on (N, D, K) alone, so the bits of every output are a function of the inputs and the shape.
#include <algorithm>

#include "../../include/mvlpt_hip.h"
#include "kernels.h"

namespace mvlpt {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SR_BM = 128, SR_BN = 128, SR_BK = 16;      // block tile and reduction chunk
constexpr int SR_PITCH = 160;                            // LDS floats per k-row: 160 mod 64 = 32
constexpr int SR_FIN = 1024;                             // gradient elements per block of sr_finish_a (4 per thread)
static_assert(SR_BM == SR_TILE && SR_BN == SR_TILE, "kernels.h and softmax_reg.hip disagree");

// TN == false:  Out[m, n] = sum_k A[m, k] B[n, k] + bias[n]       A [M, lda], B [Nn, ldb], the reduction index contiguous (Kr % 4 == 0)
// TN == true:   Out[slice][m, n] = sum_{k in slice} A[k, m] B[k, n]   A [Kr, lda], B [Kr, ldb], k the ROW index; lda, ldb % 4 == 0
//               and colsum[slice][m] = sum_{k in slice} A[k, m] in double (blocks of the first n tile)
template <bool TN>
__global__ __launch_bounds__(256) void sr_gemm(const float* __restrict__ A, const float* __restrict__ B, int M, int Nn, int Kr, int lda,
                                               int ldb, int k_per_slice, const float* __restrict__ bias, float* __restrict__ Out,
                                               int ldo, size_t slice_stride, double* __restrict__ colsum) {
  __shared__ float4 As4[SR_BK * SR_PITCH / 4];
  __shared__ float4 Bs4[SR_BK * SR_PITCH / 4];
  float* As = (float*)As4;
  float* Bs = (float*)Bs4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * SR_BM, n0 = blockIdx.y * SR_BN, slice = blockIdx.z;
  const int kbeg = TN ? slice * k_per_slice : 0;
  const int kend = TN ? min(Kr, kbeg + k_per_slice) : Kr;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int half = lane >> 5, l31 = lane & 31;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  double cs = 0.0;

  for (int k0 = kbeg; k0 < kend; k0 += SR_BK) {
    if (!TN) {
      // a thread owns one row of each tile and 8 consecutive k: two 16-byte loads, eight LDS stores down a column
      const int r = tid & 127, c = (tid >> 7) * 8;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int k = k0 + c + q * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (k < kend) {
          if (m0 + r < M) a = *(const float4*)(A + (size_t)(m0 + r) * lda + k);
          if (n0 + r < Nn) b = *(const float4*)(B + (size_t)(n0 + r) * ldb + k);
        }
        float* ap = As + (c + q * 4) * SR_PITCH + r;
        float* bp = Bs + (c + q * 4) * SR_PITCH + r;
        ap[0] = a.x; ap[SR_PITCH] = a.y; ap[2 * SR_PITCH] = a.z; ap[3 * SR_PITCH] = a.w;
        bp[0] = b.x; bp[SR_PITCH] = b.y; bp[2 * SR_PITCH] = b.z; bp[3 * SR_PITCH] = b.w;
      }
    } else {
      // the tiles are [16 k-rows][128 columns] of row-major arrays: 16-byte pieces straight across
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int f = tid + 256 * q, kk = f >> 5, c4 = (f & 31) * 4;
        const int k = k0 + kk;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (k < kend) {
          const int ca = m0 + c4, cb = n0 + c4;
          if (ca < lda) {      // lda % 4 == 0: the piece lies inside the row; columns >= M (the pad of Z) are dropped below
            a = *(const float4*)(A + (size_t)k * lda + ca);
            if (ca + 0 >= M) a.x = 0.f;
            if (ca + 1 >= M) a.y = 0.f;
            if (ca + 2 >= M) a.z = 0.f;
            if (ca + 3 >= M) a.w = 0.f;
          }
          if (cb < ldb) {
            b = *(const float4*)(B + (size_t)k * ldb + cb);
            if (cb + 0 >= Nn) b.x = 0.f;
            if (cb + 1 >= Nn) b.y = 0.f;
            if (cb + 2 >= Nn) b.z = 0.f;
            if (cb + 3 >= Nn) b.w = 0.f;
          }
        }
        As4[(kk * SR_PITCH + c4) >> 2] = a;
        Bs4[(kk * SR_PITCH + c4) >> 2] = b;
      }
    }
    __syncthreads();

    if (TN && blockIdx.y == 0 && tid < SR_BM) {
#pragma unroll
      for (int kk = 0; kk < SR_BK; ++kk) cs += (double)As[kk * SR_PITCH + tid];
    }
#pragma unroll
    for (int kk = 0; kk < SR_BK; kk += 2) {
      const float* ar = As + (kk + half) * SR_PITCH + wm + l31;
      const float* br = Bs + (kk + half) * SR_PITCH + wn + l31;
      const float a0 = ar[0], a1 = ar[32], b0 = br[0], b1 = br[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  float* out = Out + (TN ? (size_t)slice * slice_stride : (size_t)0);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + j * 32 + l31;
      if (col >= Nn) continue;
      const float bj = (!TN && bias) ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;      // C/D map of the 32x32 MFMA
        if (row < M) out[(size_t)row * ldo + col] = TN ? acc[i][j][r] : acc[i][j][r] + bj;
      }
    }
  if (TN && blockIdx.y == 0 && tid < SR_BM && m0 + tid < M) colsum[(size_t)slice * M + m0 + tid] = cs;
}

__device__ __forceinline__ double sr_wave_sum(double v) {      // the same tree in every lane: all 64 lanes end with the same bits
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256) void sr_rows(float* __restrict__ Z, const int32_t* __restrict__ y, int N, int K, int ldz, double inv_n,
                                               double* __restrict__ lossp) {
  __shared__ double wl[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  double loss = 0.0;
  if (row < (size_t)N) {
    float* z = Z + row * ldz;
    const int yi = y[row];
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    double s = 0.0, zy = 0.0;
    for (int k = lane; k < K; k += 64) {
      const float v = z[k];
      s += exp((double)v - (double)m);
      if (k == yi) zy = (double)v;      // one lane at most; the others add exact zeros
    }
    s = sr_wave_sum(s);
    zy = sr_wave_sum(zy);
    const double lse = (double)m + log(s);
    loss = lse - zy;
    for (int k = lane; k < K; k += 64) {
      const double p = exp((double)z[k] - lse);
      z[k] = (float)((p - (k == yi ? 1.0 : 0.0)) * inv_n);
    }
  }
  if (lane == 0) wl[wave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) lossp[blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

// red[q][256] -> red[q][0], a fixed tree; q < NQ sums, quantity `maxq` (if any) a maximum
template <int NQ>
__device__ __forceinline__ void sr_block_reduce(double (*red)[256], int tid, int maxq) {
  for (int o = 128; o >= 1; o >>= 1) {
    __syncthreads();
    if (tid < o) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) red[q][tid] = q == maxq ? fmax(red[q][tid], red[q][tid + o]) : red[q][tid] + red[q][tid + o];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void sr_finish_a(const float* __restrict__ part, const double* __restrict__ colsum,
                                                   const float* __restrict__ theta, const float* __restrict__ dir, int slices, size_t kd,
                                                   int K, double l2, float* __restrict__ grad, double* __restrict__ bstats) {
  __shared__ double red[4][256];
  const int tid = threadIdx.x;
  const size_t n = kd + K;
  double amax = 0.0, gd = 0.0, gg = 0.0, ww = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t e = (size_t)blockIdx.x * SR_FIN + j * 256 + tid;
    if (e >= n) continue;
    double g = 0.0;
    if (e < kd) {
      for (int s = 0; s < slices; ++s) g += (double)part[(size_t)s * kd + e];
      const double w = (double)theta[e];
      g += l2 * w;
      ww += w * w;
    } else {
      for (int s = 0; s < slices; ++s) g += colsum[(size_t)s * K + (e - kd)];
    }
    const float gf = (float)g;
    grad[e] = gf;
    const double gr = (double)gf;
    amax = fmax(amax, fabs(gr));
    gg += gr * gr;
    if (dir) gd += gr * (double)dir[e];
  }
  red[0][tid] = amax; red[1][tid] = gd; red[2][tid] = gg; red[3][tid] = ww;
  sr_block_reduce<4>(red, tid, 0);
  if (tid < 4) bstats[(size_t)blockIdx.x * 4 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void sr_finish_b(const double* __restrict__ bstats, int fin_blocks, const double* __restrict__ lossp,
                                                   int row_blocks, double inv_n, double l2, double* __restrict__ stats) {
  __shared__ double red[5][256];
  const int tid = threadIdx.x;
  double amax = 0.0, gd = 0.0, gg = 0.0, ww = 0.0, loss = 0.0;
  for (int b = tid; b < fin_blocks; b += 256) {
    amax = fmax(amax, bstats[(size_t)b * 4]);
    gd += bstats[(size_t)b * 4 + 1];
    gg += bstats[(size_t)b * 4 + 2];
    ww += bstats[(size_t)b * 4 + 3];
  }
  for (int b = tid; b < row_blocks; b += 256) loss += lossp[b];
  red[0][tid] = amax; red[1][tid] = gd; red[2][tid] = gg; red[3][tid] = ww; red[4][tid] = loss;
  sr_block_reduce<5>(red, tid, 0);
  if (tid == 0) {
    stats[0] = red[4][0] * inv_n + 0.5 * l2 * red[3][0];
    stats[1] = red[0][0];
    stats[2] = red[1][0];
    stats[3] = red[2][0];
  }
}

// one wave per row: the largest logit (the lowest index among equals, numpy's rule) and the distance to the second largest
__global__ __launch_bounds__(256) void sr_argmax(const float* __restrict__ Z, int N, int K, int ldz, int32_t* __restrict__ pred,
                                                 float* __restrict__ margin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  if (row >= (size_t)N) return;
  const float* z = Z + row * ldz;
  float v1 = -INFINITY, v2 = -INFINITY;
  int i1 = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const float v = z[k];
    if (v > v1 || (v == v1 && i1 == 0x7fffffff)) { v2 = v1; v1 = v; i1 = k; }
    else if (v > v2) v2 = v;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov1 = __shfl_xor(v1, o), ov2 = __shfl_xor(v2, o);
    const int oi1 = __shfl_xor(i1, o);
    const bool other = ov1 > v1 || (ov1 == v1 && oi1 < i1);
    v2 = other ? fmaxf(ov2, v1) : fmaxf(v2, ov1);
    if (other) { v1 = ov1; i1 = oi1; }
  }
  if (lane == 0) {
    pred[row] = i1 < K ? i1 : 0;      // a row of NaNs has no largest logit: class 0
    if (margin) margin[row] = v1 - v2;
  }
}

inline size_t sr_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

SoftmaxRegPlan softmax_reg_plan(int N, int D, int K) {
  SoftmaxRegPlan p;
  p.ldz = (K + 3) & ~3;
  const int tiles = ((K + SR_TILE - 1) / SR_TILE) * ((D + SR_TILE - 1) / SR_TILE);
  const int want = std::max(1, 256 / tiles);                       // about one block per compute unit; never more than 256 slices
  int rows = (int)(((int64_t)N + want - 1) / want);
  rows = std::max(32, (rows + SR_BK - 1) / SR_BK * SR_BK);          // whole reduction chunks, and no slice thinner than 32 rows
  p.rows_per_slice = rows;
  p.slices = (int)(((int64_t)N + rows - 1) / rows);                 // no empty slice
  p.row_blocks = (int)(((int64_t)N + 3) / 4);
  const size_t kd = (size_t)K * D;
  p.fin_blocks = (int)((kd + K + SR_FIN - 1) / SR_FIN);
  p.predict_bytes = sr_align((size_t)N * p.ldz * sizeof(float));
  p.off_part = p.predict_bytes;
  p.off_colsum = p.off_part + sr_align((size_t)p.slices * kd * sizeof(float));
  p.off_lossp = p.off_colsum + sr_align((size_t)p.slices * K * sizeof(double));
  p.off_bstats = p.off_lossp + sr_align((size_t)p.row_blocks * sizeof(double));
  p.ws_bytes = p.off_bstats + sr_align((size_t)p.fin_blocks * 4 * sizeof(double));
  return p;
}

static hipError_t sr_logits(const float* X, const float* theta, int N, int D, int K, float* Z, int ldz, hipStream_t s) {
  const dim3 grid((N + SR_BM - 1) / SR_BM, (K + SR_BN - 1) / SR_BN, 1);
  sr_gemm<false><<<grid, 256, 0, s>>>(X, theta, N, K, D, D, D, 0, theta + (size_t)K * D, Z, ldz, 0, nullptr);
  return hipGetLastError();
}

hipError_t launch_softmax_reg_eval(const float* X, const int32_t* y, const float* theta, const float* dir, int N, int D, int K, double l2,
                                   float* grad, double* stats, void* ws, const SoftmaxRegPlan& p, hipStream_t s) {
  char* base = (char*)ws;
  float* Z = (float*)base;
  float* part = (float*)(base + p.off_part);
  double* colsum = (double*)(base + p.off_colsum);
  double* lossp = (double*)(base + p.off_lossp);
  double* bstats = (double*)(base + p.off_bstats);
  const size_t kd = (size_t)K * D;
  const double inv_n = 1.0 / (double)N;
  hipError_t e = sr_logits(X, theta, N, D, K, Z, p.ldz, s);
  if (e != hipSuccess) return e;
  sr_rows<<<p.row_blocks, 256, 0, s>>>(Z, y, N, K, p.ldz, inv_n, lossp);
  const dim3 grid((K + SR_BM - 1) / SR_BM, (D + SR_BN - 1) / SR_BN, p.slices);
  sr_gemm<true><<<grid, 256, 0, s>>>(Z, X, K, D, N, p.ldz, D, p.rows_per_slice, nullptr, part, D, kd, colsum);
  sr_finish_a<<<p.fin_blocks, 256, 0, s>>>(part, colsum, theta, dir, p.slices, kd, K, l2, grad, bstats);
  sr_finish_b<<<1, 256, 0, s>>>(bstats, p.fin_blocks, lossp, p.row_blocks, inv_n, l2, stats);
  return hipGetLastError();
}

hipError_t launch_softmax_reg_predict(const float* X, const float* theta, int N, int D, int K, int32_t* pred, float* margin, void* ws,
                                      const SoftmaxRegPlan& p, hipStream_t s) {
  float* Z = (float*)ws;
  hipError_t e = sr_logits(X, theta, N, D, K, Z, p.ldz, s);
  if (e != hipSuccess) return e;
  sr_argmax<<<p.row_blocks, 256, 0, s>>>(Z, N, K, p.ldz, pred, margin);
  return hipGetLastError();
}

}  // namespace mvlpt
