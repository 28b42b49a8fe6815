// Tip-Adapter head (Zhang et al., ECCV 2022): zero-shot CLIP plus a key-value cache of few-shot features, all fp32.
//   z[n, c] = s <f_n, w_c> + alpha * sum_{j : cls(j) = c} exp(-beta (1 - <f_n, k_j>)),
// with the keys sorted by class and a CSR table key_ptr [C + 1] (semantics, limits and the order rule: include/mvlpt_hip.h).
// The published code forms exp(...) [N, NK] and multiplies it with a one-hot [NK, C]; here the product with the one-hot matrix is the
// segmented sum it stands for.
//
// Products run on v_mfma_f32_32x32x2_f32 (the build has no packed fp32 VALU: softmax_reg.hip).  tip_product gives a block of 4 waves a
// [128 rows, 64 columns] tile: operands through LDS in chunks of 16 of the reduction index, stored [k][row] as in sr_gemm, each wave
// two 32 x 32 fragments.  Rows, columns and the reduction are ragged: whatever lies outside is staged as zero and never stored.
//
// tip_forward (the one forward kernel; block = 128 rows of F x a run of at most 64 consecutive classes):
//   1. clip tile: z = s * (F W^T), stored from the accumulators.
//   2. for each tile of 64 keys of the block's class run [key_ptr[c0], key_ptr[c1]): t = <f, k> - 1 goes to LDS as T[key][row]; then a
//      thread that owns a ROW walks the tile's keys in ascending order, class by class (the boundaries come from key_ptr, so a wave never
//      diverges): run = run + exp(beta * t_j), from 0 at the class's first key and across tiles.  A class that ends in the tile is
//      finished:  z = z + alpha * run.   Every (row, class) is written by this block alone.
//      LOGITS / TRAIN: one beta; the two halves of the block take the even and the odd classes.  TRAIN also stores A = exp(.) as
//      AT [NK, ldn] (the backward's operand, n contiguous).
//      SEARCH: the halves take alternate groups of TIP_BG betas and every class; the running sums live in the workspace
//      cache [C, nb, R] (R rows of the row chunk, contiguous), clip [C, R].
//   An empty class adds alpha * 0.  A class's keys are added in ascending order whatever the tiles and the grid: the bits of a logit
//   depend on its row, its class's keys and w alone, and are the same in all three modes, so the search counts exactly what tip_logits
//   would give.
// Train: tip_rows (one wave per row, statistics in double from the fp32 logits as sr_rows: loss partial, arg-max with ties to the lowest
//   class, RT [C, ldn] = (softmax - onehot) / N), tip_finish (one block adds the partials in a fixed order);
//   tip_dk: dK = alpha beta (A * r)^T-product with F, the factor A[n, j] r[n, cls(j)] formed while the operand is staged.
// Search: tip_search_rows, thread = row, block.y = beta: the arg-max over c of clip + alpha_a * cache for every alpha in registers (in
//   steps of 8 alphas: 24 for the published 20), then one integer atomic add per wave and grid point.
// Known cost: in LOGITS / TRAIN half of the block idles while the other half walks a class much wider than its neighbours.
// No floating-point atomics anywhere.
#include <algorithm>

#include "../../include/mvlpt_hip.h"
#include "kernels.h"

namespace mvlpt {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TIP_BM = 128, TIP_BN = 64, TIP_BK = 16;      // block tile (rows of F x classes or keys) and reduction chunk
constexpr int TIP_PA = 160, TIP_PB = 96;                   // LDS floats per k-row of the two operands (both = 32 mod 64)
constexpr int TIP_PT = TIP_BM + 1;                         // pitch of T[key][row]: the 32 lanes of a fragment column hit 32 banks
constexpr int TIP_BG = 8;                                  // betas a walking thread carries at once (search)
constexpr int TIP_DT = 128;                                // tip_dk: 128 keys x 128 columns of D
static_assert(TIP_BM == TIP_ROWS, "kernels.h and tip.hip disagree");
static_assert(MVLPT_TIP_MAX_NA == 32, "launch_tip_search dispatches on at most 32 alphas");

enum { TIP_LOGITS = 0, TIP_TRAIN = 1, TIP_SEARCH = 2 };

// A product that feeds a sum stays a ROUNDED product (the library is built with contraction on; see tp_mul in tpt.hip).
__device__ __forceinline__ float tip_mul(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}
// The one place that forms exp(-beta (1 - a)) from t = a - 1, and the one that joins the two terms of a logit.
__device__ __forceinline__ float tip_aff(float beta, float t) { return expf(tip_mul(beta, t)); }
__device__ __forceinline__ float tip_join(float clip, float alpha, float cache) { return __fadd_rn(clip, tip_mul(alpha, cache)); }

// acc[i] (+)= A[m0 .., :] B[n0 .., :]^T over D: rows >= M, rows >= Nn and k >= D are zeros.  D % 4 == 0; all threads call it.
// Fragment map: acc[i][r] is row m0 + wm + 32 i + (r & 3) + 8 (r >> 2) + 4 half, column n0 + wn + l31.
__device__ __forceinline__ void tip_product(const float* __restrict__ A, int M, int m0, const float* __restrict__ B, int Nn, int n0, int D,
                                            float* As, float* Bs, f32x16 (&acc)[2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32, half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  for (int k0 = 0; k0 < D; k0 += TIP_BK) {
    {
      const int r = tid & 127, c = (tid >> 7) * 8;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int k = k0 + c + q * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < D && m0 + r < M) a = *(const float4*)(A + (size_t)(m0 + r) * D + k);
        float* ap = As + (c + q * 4) * TIP_PA + r;
        ap[0] = a.x; ap[TIP_PA] = a.y; ap[2 * TIP_PA] = a.z; ap[3 * TIP_PA] = a.w;
      }
      const int rb = tid & 63, kb = (tid >> 6) * 4, k = k0 + kb;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < D && n0 + rb < Nn) b = *(const float4*)(B + (size_t)(n0 + rb) * D + k);
      float* bp = Bs + kb * TIP_PB + rb;
      bp[0] = b.x; bp[TIP_PB] = b.y; bp[2 * TIP_PB] = b.z; bp[3 * TIP_PB] = b.w;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TIP_BK; kk += 2) {
      const float* ar = As + (kk + half) * TIP_PA + wm + l31;
      const float a0 = ar[0], a1 = ar[32], b0 = Bs[(kk + half) * TIP_PB + wn + l31];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1], 0, 0, 0);
    }
    __syncthreads();
  }
}

struct TipFwdArgs {
  const float *F, *K, *W;
  const int32_t* key_ptr;
  int N, NK, C, D;
  float s, alpha, beta;           // LOGITS / TRAIN
  float* Z; int ldz;              // LOGITS / TRAIN: the logits [N, ldz]
  float* AT; int ldn;             // TRAIN: A^T [NK, ldn]
  const float* betas; int nb;     // SEARCH
  int ct;                         // classes per block, 1 .. TIP_BN: it shapes the grid and no result
  int r0, R;                      // SEARCH: the row chunk [r0, r0 + R) of F; R % TIP_BM == 0
  float *clip, *cache;            // SEARCH: [C, R] and [C, nb, R]
};

template <int MODE>
__global__ __launch_bounds__(256) void tip_forward(const TipFwdArgs a) {
  __shared__ float4 As4[TIP_BK * TIP_PA / 4];
  __shared__ float4 Bs4[TIP_BK * TIP_PB / 4];
  __shared__ float T[TIP_BN * TIP_PT];
  __shared__ int kp[TIP_BN + 1];
  float* As = (float*)As4;
  float* Bs = (float*)Bs4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32, half = lane >> 5, l31 = lane & 31;
  const int mloc = blockIdx.x * TIP_BM;                           // first row of the block inside the chunk (SEARCH) or F
  const int m0 = (MODE == TIP_SEARCH ? a.r0 : 0) + mloc;
  const int c0 = blockIdx.y * a.ct, nc = min(a.ct, a.C - c0);
  if (tid <= nc) kp[tid] = a.key_ptr[c0 + tid];

  f32x16 acc[2];
  tip_product(a.F, a.N, m0, a.W, a.C, c0, a.D, As, Bs, acc);      // its barriers also publish kp
  {
    const int col = wn + l31;
    if (col < nc) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (m0 + rl >= a.N) continue;
          const float v = tip_mul(a.s, acc[i][r]);
          if (MODE == TIP_SEARCH) a.clip[(size_t)(c0 + col) * a.R + mloc + rl] = v;
          else a.Z[(size_t)(m0 + rl) * a.ldz + c0 + col] = v;
        }
    }
  }
  __syncthreads();      // the clip tile is visible to the walking threads of this block

  const int row = tid & 127, side = tid >> 7;
  const bool live = m0 + row < a.N;
  const int jbeg = kp[0], jend = kp[nc];

  // classes without keys: the cache term is alpha * 0
  if (MODE == TIP_SEARCH) {
    for (int lc = 0; lc < nc; ++lc) {
      if (kp[lc + 1] > kp[lc] || !live) continue;
      for (int b = side; b < a.nb; b += 2) a.cache[((size_t)(c0 + lc) * a.nb + b) * a.R + mloc + row] = 0.f;
    }
  } else {
    for (int lc = side; lc < nc; lc += 2) {
      if (kp[lc + 1] > kp[lc] || !live) continue;
      float* z = a.Z + (size_t)(m0 + row) * a.ldz + c0 + lc;
      *z = tip_join(*z, a.alpha, 0.f);
    }
  }

  float run = 0.f;      // LOGITS / TRAIN: the class of this thread that is under way
  for (int ts = jbeg; ts < jend; ts += TIP_BN) {
    const int te = min(ts + TIP_BN, jend);
    tip_product(a.F, a.N, m0, a.K, jend, ts, a.D, As, Bs, acc);
    {
      float* tc = T + (wn + l31) * TIP_PT + wm + 4 * half;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) tc[i * 32 + (r & 3) + 8 * (r >> 2)] = __fsub_rn(acc[i][r], 1.f);
    }
    __syncthreads();

    if (MODE == TIP_SEARCH) {
      for (int b0 = side * TIP_BG; b0 < a.nb; b0 += 2 * TIP_BG) {
        float be[TIP_BG];
#pragma unroll
        for (int q = 0; q < TIP_BG; ++q) be[q] = b0 + q < a.nb ? a.betas[b0 + q] : 0.f;
        for (int lc = 0; lc < nc; ++lc) {
          const int jlo = max(kp[lc], ts), jhi = min(kp[lc + 1], te);
          if (jlo >= jhi) continue;
          if (!live) continue;
          float* dst = a.cache + ((size_t)(c0 + lc) * a.nb + b0) * a.R + mloc + row;
          const bool began_earlier = kp[lc] < ts;
          float sum[TIP_BG];      // the class's running sums: they continue where the previous tile left them
#pragma unroll
          for (int q = 0; q < TIP_BG; ++q) sum[q] = (began_earlier && b0 + q < a.nb) ? dst[(size_t)q * a.R] : 0.f;
          for (int j = jlo; j < jhi; ++j) {
            const float t = T[(j - ts) * TIP_PT + row];
#pragma unroll
            for (int q = 0; q < TIP_BG; ++q) sum[q] = __fadd_rn(sum[q], tip_aff(be[q], t));
          }
#pragma unroll
          for (int q = 0; q < TIP_BG; ++q)
            if (b0 + q < a.nb) dst[(size_t)q * a.R] = sum[q];
        }
      }
    } else {
      for (int lc = side; lc < nc; lc += 2) {
        const int jlo = max(kp[lc], ts), jhi = min(kp[lc + 1], te);
        if (jlo >= jhi) continue;
        if (kp[lc] >= ts) run = 0.f;      // the class begins in this tile
        for (int j = jlo; j < jhi; ++j) {
          const float e = tip_aff(a.beta, T[(j - ts) * TIP_PT + row]);
          run = __fadd_rn(run, e);
          if (MODE == TIP_TRAIN && live) a.AT[(size_t)j * a.ldn + m0 + row] = e;
        }
        if (kp[lc + 1] <= te && live) {
          float* z = a.Z + (size_t)(m0 + row) * a.ldz + c0 + lc;
          *z = tip_join(*z, a.alpha, run);
        }
      }
    }
    __syncthreads();      // T is free for the next tile
  }
}

// cls[j] = the class whose range holds key j: the last c with key_ptr[c] <= j
__global__ __launch_bounds__(256) void tip_key_cls(const int32_t* __restrict__ key_ptr, int C, int NK, int32_t* __restrict__ cls) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= NK) return;
  int lo = 0, hi = C;      // key_ptr[lo] <= j < key_ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (key_ptr[mid] <= j) lo = mid; else hi = mid;
  }
  cls[j] = lo;
}

__device__ __forceinline__ double tip_wave_sum(double v) {      // the same tree in every lane
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One wave per row, as sr_rows: statistics in double from the fp32 logits; RT[c, n] = (p - onehot) / N rounded once.
__global__ __launch_bounds__(256) void tip_rows(const float* __restrict__ Z, const int32_t* __restrict__ y, int N, int C, int ldz, int ldn,
                                                double inv_n, float* __restrict__ RT, double* __restrict__ lossp,
                                                int32_t* __restrict__ corrp) {
  __shared__ double wl[4];
  __shared__ int wc[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * 4 + wave;
  double loss = 0.0;
  int hit = 0;
  if (row < (size_t)N) {
    const float* z = Z + row * ldz;
    const int yi = y[row];
    float m = -INFINITY;
    int im = 0x7fffffff;
    for (int k = lane; k < C; k += 64) {
      const float v = z[k];
      if (v > m || (v == m && im == 0x7fffffff)) { m = v; im = k; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float om = __shfl_xor(m, o);
      const int oi = __shfl_xor(im, o);
      if (om > m || (om == m && oi < im)) { m = om; im = oi; }
    }
    hit = (im < C ? im : 0) == yi ? 1 : 0;      // a row of NaNs has no largest logit: class 0
    double s = 0.0, zy = 0.0;
    for (int k = lane; k < C; k += 64) {
      const float v = z[k];
      s += exp((double)v - (double)m);
      if (k == yi) zy = (double)v;
    }
    s = tip_wave_sum(s);
    zy = tip_wave_sum(zy);
    const double lse = (double)m + log(s);
    loss = lse - zy;
    for (int k = lane; k < C; k += 64) {
      const double p = exp((double)z[k] - lse);
      RT[(size_t)k * ldn + row] = (float)((p - (k == yi ? 1.0 : 0.0)) * inv_n);
    }
  }
  if (lane == 0) { wl[wave] = loss; wc[wave] = hit; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lossp[blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
    corrp[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
  }
}

__global__ __launch_bounds__(256) void tip_finish(const double* __restrict__ lossp, const int32_t* __restrict__ corrp, int row_blocks,
                                                  double inv_n, float* __restrict__ loss, int32_t* __restrict__ correct) {
  __shared__ double red[256];
  __shared__ int redc[256];
  const int tid = threadIdx.x;
  double l = 0.0;
  int c = 0;
  for (int b = tid; b < row_blocks; b += 256) { l += lossp[b]; c += corrp[b]; }
  red[tid] = l; redc[tid] = c;
  for (int o = 128; o >= 1; o >>= 1) {
    __syncthreads();
    if (tid < o) { red[tid] += red[tid + o]; redc[tid] += redc[tid + o]; }
  }
  if (tid == 0) { *loss = (float)(red[0] * inv_n); *correct = redc[0]; }
}

// dK[j, d] = ab * sum_n (AT[j, n] RT[cls(j), n]) F[n, d]: block = 128 keys x 128 columns, the whole reduction over n in order.
__global__ __launch_bounds__(256) void tip_dk(const float* __restrict__ AT, const float* __restrict__ RT, const int32_t* __restrict__ cls,
                                              const float* __restrict__ F, int N, int NK, int D, int ldn, float ab,
                                              float* __restrict__ dK) {
  __shared__ float4 As4[TIP_BK * TIP_PA / 4];
  __shared__ float4 Bs4[TIP_BK * TIP_PA / 4];
  float* As = (float*)As4;
  float* Bs = (float*)Bs4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * TIP_DT, d0 = blockIdx.y * TIP_DT;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, half = lane >> 5, l31 = lane & 31;
  const int rj = tid & 127, ck = (tid >> 7) * 8;
  const bool key_ok = j0 + rj < NK;
  const float* at = AT + (size_t)(key_ok ? j0 + rj : 0) * ldn;
  const float* rt = RT + (size_t)(key_ok ? cls[j0 + rj] : 0) * ldn;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int k0 = 0; k0 < N; k0 += TIP_BK) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = k0 + ck + q * 4;
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      if (key_ok && k < N) {      // ldn % 4 == 0 and k % 4 == 0: the piece lies inside the row; n >= N is dropped
        const float4 x = *(const float4*)(at + k), r = *(const float4*)(rt + k);
        g.x = tip_mul(x.x, r.x);
        if (k + 1 < N) g.y = tip_mul(x.y, r.y);
        if (k + 2 < N) g.z = tip_mul(x.z, r.z);
        if (k + 3 < N) g.w = tip_mul(x.w, r.w);
      }
      float* ap = As + (ck + q * 4) * TIP_PA + rj;
      ap[0] = g.x; ap[TIP_PA] = g.y; ap[2 * TIP_PA] = g.z; ap[3 * TIP_PA] = g.w;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = tid + 256 * q, kk = f >> 5, c4 = (f & 31) * 4;
      const int k = k0 + kk;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < N && d0 + c4 < D) b = *(const float4*)(F + (size_t)k * D + d0 + c4);      // D % 4 == 0
      Bs4[(kk * TIP_PA + c4) >> 2] = b;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TIP_BK; kk += 2) {
      const float* ar = As + (kk + half) * TIP_PA + wm + l31;
      const float* br = Bs + (kk + half) * TIP_PA + wn + l31;
      const float a0 = ar[0], a1 = ar[32], b0 = br[0], b1 = br[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = d0 + wn + j * 32 + l31;
      if (col >= D) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = j0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < NK) dK[(size_t)row * D + col] = tip_mul(ab, acc[i][j][r]);
      }
    }
}

__global__ __launch_bounds__(256) void tip_zero_counts(int32_t* __restrict__ counts, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) counts[i] = 0;
}

// thread = row of the chunk, blockIdx.y = beta: the arg-max over the classes in ascending order (a strict > keeps the lowest index).
// NA: the alphas kept in registers, na rounded up to a multiple of 8 by the launcher.
template <int NA>
__global__ __launch_bounds__(256) void tip_search_rows(const float* __restrict__ clip, const float* __restrict__ cache,
                                                       const int32_t* __restrict__ y, const float* __restrict__ alphas, int N, int C,
                                                       int nb, int na, int r0, int R, int32_t* __restrict__ counts) {
  const int nloc = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const bool live = nloc < R && r0 + nloc < N;
  float al[NA], best[NA];
  int idx[NA];
#pragma unroll
  for (int q = 0; q < NA; ++q) { al[q] = q < na ? alphas[q] : 0.f; best[q] = -INFINITY; idx[q] = 0; }
  if (live) {
    for (int c = 0; c < C; ++c) {
      const float vc = clip[(size_t)c * R + nloc], ch = cache[((size_t)c * nb + b) * R + nloc];
#pragma unroll
      for (int q = 0; q < NA; ++q) {
        const float v = tip_join(vc, al[q], ch);
        if (v > best[q]) { best[q] = v; idx[q] = c; }
      }
    }
  }
  const int yi = live ? y[r0 + nloc] : -1;
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    if (q < na) {      // uniform
      const int hits = __popcll(__ballot(live && idx[q] == yi));
      if ((threadIdx.x & 63) == 0 && hits) atomicAdd(counts + (size_t)b * na + q, hits);
    }
  }
}

inline size_t tip_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

TipPlan tip_plan(int N, int NK, int C, int D, int nb, int na, int mode) {
  (void)D; (void)na;
  TipPlan p;
  p.ldn = (N + 3) & ~3;
  p.row_blocks = (int)(((int64_t)N + 3) / 4);
  if (mode == MVLPT_TIP_TRAIN) {
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += tip_align(bytes); return o; };
    p.off_cls = take((size_t)NK * sizeof(int32_t));
    p.off_at = take((size_t)NK * p.ldn * sizeof(float));
    p.off_rt = take((size_t)C * p.ldn * sizeof(float));
    p.off_z = take((size_t)N * C * sizeof(float));
    p.off_lossp = take((size_t)p.row_blocks * sizeof(double));
    p.off_corrp = take((size_t)p.row_blocks * sizeof(int32_t));
    p.ws_bytes = off;
  } else if (mode == MVLPT_TIP_SEARCH) {
    // a row chunk of R rows keeps clip [C, R] and cache [C, nb, R]: about 512 MiB, never less than one row block
    const size_t per_row = (size_t)C * ((size_t)nb + 1) * sizeof(float);
    const size_t budget = (size_t)512 << 20;
    int64_t R = (int64_t)(budget / per_row) / TIP_ROWS * TIP_ROWS;
    const int64_t all = ((int64_t)N + TIP_ROWS - 1) / TIP_ROWS * TIP_ROWS;
    R = std::min<int64_t>(std::max<int64_t>(R, TIP_ROWS), all);
    p.chunk_rows = (int)R;
    p.off_clip = 0;
    p.off_cache = tip_align((size_t)C * R * sizeof(float));
    p.ws_bytes = p.off_cache + tip_align((size_t)C * nb * R * sizeof(float));
  }
  return p;
}

// Classes per block: TIP_BN, halved down to 8 while the grid has fewer blocks than the device has compute units.  A smaller run costs
// a larger share of zero-shot tile per key tile and changes no bit: every sum runs over a class's keys in ascending order.
static int tip_class_tile(int rows, int C) {
  const long long row_blocks = (rows + TIP_BM - 1) / TIP_BM;
  int ct = TIP_BN;
  while (ct > 8 && row_blocks * ((C + ct - 1) / ct) < 256) ct >>= 1;
  return ct;
}
static dim3 tip_fwd_grid(int rows, int C, int ct) { return dim3((rows + TIP_BM - 1) / TIP_BM, (C + ct - 1) / ct, 1); }

hipError_t launch_tip_logits(const float* F, const float* K, const int32_t* key_ptr, const float* W, float s, float alpha, float beta,
                             int N, int NK, int C, int D, float* logits, hipStream_t st) {
  TipFwdArgs a = {};
  a.F = F; a.K = K; a.W = W; a.key_ptr = key_ptr; a.N = N; a.NK = NK; a.C = C; a.D = D;
  a.s = s; a.alpha = alpha; a.beta = beta; a.Z = logits; a.ldz = C; a.ct = tip_class_tile(N, C);
  tip_forward<TIP_LOGITS><<<tip_fwd_grid(N, C, a.ct), 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_tip_train_fwd(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s,
                                float alpha, float beta, int N, int NK, int C, int D, float* loss, int32_t* correct, float* logits,
                                void* ws, const TipPlan& p, hipStream_t st) {
  char* base = (char*)ws;
  int32_t* cls = (int32_t*)(base + p.off_cls);
  float* Z = logits ? logits : (float*)(base + p.off_z);
  double* lossp = (double*)(base + p.off_lossp);
  int32_t* corrp = (int32_t*)(base + p.off_corrp);
  tip_key_cls<<<(NK + 255) / 256, 256, 0, st>>>(key_ptr, C, NK, cls);
  TipFwdArgs a = {};
  a.F = F; a.K = K; a.W = W; a.key_ptr = key_ptr; a.N = N; a.NK = NK; a.C = C; a.D = D;
  a.s = s; a.alpha = alpha; a.beta = beta; a.Z = Z; a.ldz = C; a.AT = (float*)(base + p.off_at); a.ldn = p.ldn;
  a.ct = tip_class_tile(N, C);
  tip_forward<TIP_TRAIN><<<tip_fwd_grid(N, C, a.ct), 256, 0, st>>>(a);
  const double inv_n = 1.0 / (double)N;
  tip_rows<<<p.row_blocks, 256, 0, st>>>(Z, y, N, C, C, p.ldn, inv_n, (float*)(base + p.off_rt), lossp, corrp);
  tip_finish<<<1, 256, 0, st>>>(lossp, corrp, p.row_blocks, inv_n, loss, correct);
  return hipGetLastError();
}

hipError_t launch_tip_train_bwd(const float* F, float alpha, float beta, int N, int NK, int C, int D, float* dK, void* ws,
                                const TipPlan& p, hipStream_t st) {
  (void)C;
  char* base = (char*)ws;
  const dim3 grid((NK + TIP_DT - 1) / TIP_DT, (D + TIP_DT - 1) / TIP_DT, 1);
  tip_dk<<<grid, 256, 0, st>>>((const float*)(base + p.off_at), (const float*)(base + p.off_rt), (const int32_t*)(base + p.off_cls), F,
                               N, NK, D, p.ldn, alpha * beta, dK);
  return hipGetLastError();
}

hipError_t launch_tip_search(const float* F, const int32_t* y, const float* K, const int32_t* key_ptr, const float* W, float s,
                             const float* betas, const float* alphas, int N, int NK, int C, int D, int nb, int na, int32_t* counts,
                             void* ws, const TipPlan& p, hipStream_t st) {
  char* base = (char*)ws;
  tip_zero_counts<<<(nb * na + 255) / 256, 256, 0, st>>>(counts, nb * na);
  TipFwdArgs a = {};
  a.F = F; a.K = K; a.W = W; a.key_ptr = key_ptr; a.N = N; a.NK = NK; a.C = C; a.D = D;
  a.s = s; a.betas = betas; a.nb = nb; a.R = p.chunk_rows;
  a.clip = (float*)(base + p.off_clip); a.cache = (float*)(base + p.off_cache);
  for (int64_t r0 = 0; r0 < N; r0 += p.chunk_rows) {
    const int rows = (int)std::min<int64_t>(p.chunk_rows, N - r0);
    a.r0 = (int)r0;
    a.ct = tip_class_tile(rows, C);
    tip_forward<TIP_SEARCH><<<tip_fwd_grid(rows, C, a.ct), 256, 0, st>>>(a);
    const dim3 grid((rows + 255) / 256, nb);
    if (na <= 8) tip_search_rows<8><<<grid, 256, 0, st>>>(a.clip, a.cache, y, alphas, N, C, nb, na, (int)r0, p.chunk_rows, counts);
    else if (na <= 16) tip_search_rows<16><<<grid, 256, 0, st>>>(a.clip, a.cache, y, alphas, N, C, nb, na, (int)r0, p.chunk_rows, counts);
    else if (na <= 24) tip_search_rows<24><<<grid, 256, 0, st>>>(a.clip, a.cache, y, alphas, N, C, nb, na, (int)r0, p.chunk_rows, counts);
    else tip_search_rows<32><<<grid, 256, 0, st>>>(a.clip, a.cache, y, alphas, N, C, nb, na, (int)r0, p.chunk_rows, counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

}  // namespace mvlpt
