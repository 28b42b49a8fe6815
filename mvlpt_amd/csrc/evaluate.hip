// Evaluation on the device: the integer counts every figure of MVLPT.test is a function of (trainers/mvlpt.py:1023-1080 and
// trainers/vision_benchmark/datasets/metrics.py:1254-1294 of the reference, which run numpy / sklearn on host copies of the logits).
//
// Kernel 1 (eval_count): streaming class counters, one wave per row.  The wave finds the row's arg-max as numpy does (the lowest index
// among equal maxima, a NaN counts as maximal) over all columns, optionally over the row's own task range [lo_t, hi_t) and optionally
// over the columns a uint8 mask keeps, and lane 0 adds 1 to the caller's int64 counters with ordinary 64-bit vector atomic adds.
// Integer sums: the counters do not depend on the order the rows arrive in, two runs are bit-equal.
//
// Kernel 2 (eval_rank_columns): one workgroup owns one column of scores from start to finish.  Every selected score becomes the item
// (order-preserving 32-bit key of the fp32 score) << 1 | (target is positive), -0.0 folded into +0.0; the items are sorted ascending by a
// bitonic compare-exchange network: columns of at most RK_TILE items (padded to a power of two) in LDS, longer ones tile by tile in LDS
// for the strides below RK_TILE and over a global scratch buffer for the longer strides.  Workgroup barriers are the only
// synchronisation: the scratch of a column is written and read by one workgroup (one compute unit, one L1).  One pass over the sorted
// items then carries three scans (start of the current run of equal keys, positives in the run so far, positives so far) and derives
//   twice_u  = sum over runs [a, b) of (positives in the run) * (a + 1 + b)  -  n_pos * (n_pos + 1)        (int64, exact)
//   interp[i] = max precision tp / cnt over the run starts whose recall tp / n_pos reaches threshold i       (IEEE double divisions)
// which is all _binary_auc and the 11-point walk of metrics.py read from a column.  Run boundaries depend on the keys alone, so the
// place of the positive bit inside a run does not matter.
#include <algorithm>

#include "../../include/mvlpt_hip.h"
#include "kernels.h"

namespace mvlpt {

namespace {

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------ class counters
constexpr int EC_BLOCK = 256;                      // four rows per workgroup
constexpr int EC_NONE = 0x7fffffff;                // "no column seen"

// does candidate (cv, ci) precede (bv, bi) as numpy's arg-max: NaN first, then the larger value, equal ones by the lower index
__device__ __forceinline__ bool ec_beats(float cv, int ci, float bv, int bi) {
  if (ci == EC_NONE) return false;
  if (bi == EC_NONE) return true;
  const bool cn = cv != cv, bn = bv != bv;
  if (cn || bn) return cn && (!bn || ci < bi);
  return cv > bv || (cv == bv && ci < bi);
}

// arg-max of x[c0 .. c1) over the columns `mask` keeps (NULL: all), the same value in every lane; EC_NONE when there is no such column
__device__ __forceinline__ int ec_argmax(const float* x, int c0, int c1, const uint8_t* mask, int lane) {
  float bv = 0.f;
  int bi = EC_NONE;
  for (int c = c0 + lane; c < c1; c += 64) {
    if (mask && !mask[c]) continue;
    const float v = x[c];
    if (ec_beats(v, c, bv, bi)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (ec_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  return bi;
}

__device__ __forceinline__ void ec_add(int64_t* p, size_t i) { atomicAdd((u64*)p + i, 1ull); }

__global__ __launch_bounds__(EC_BLOCK) void eval_count(EvalCountArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (EC_BLOCK / 64) + (threadIdx.x >> 6);
  if (r >= a.n) return;                                                  // whole waves leave: no barrier below
  int row = a.rows ? a.rows[r] : r;
  row = min(max(row, 0), a.B - 1);
  const float* x = a.logits + (size_t)row * a.ld;
  const int pred = ec_argmax(x, 0, a.C, a.col_mask, lane);
  int truth;
  if (a.label_f) {
    const float* y = a.label_f + (size_t)row * a.label_ld;
    truth = ec_argmax(y, 0, a.C, a.col_mask, lane);
    if (a.col_seen)                                                      // every lane stores the same byte: no race to order
      for (int c = lane; c < a.C; c += 64)
        if (y[c] != 0.f) a.col_seen[c] = 1;
  } else {
    const long long l = a.label_i[row];
    truth = l >= 0 && l < a.C ? (int)l : EC_NONE;
  }
  int pred_r = EC_NONE;
  if (a.task) {
    const int t = a.task[row];
    if (t >= 0 && t < a.T) pred_r = ec_argmax(x, max(a.lo[t], 0), min(a.hi[t], a.C), a.col_mask, lane);
  }
  if (lane != 0) return;
  if (pred != EC_NONE) ec_add(a.n_pred, pred);
  if (pred_r != EC_NONE) ec_add(a.n_pred_r, pred_r);
  if (truth == EC_NONE) return;
  if (a.col_seen && a.label_i) a.col_seen[truth] = 1;
  ec_add(a.n_true, truth);
  if (pred == truth) ec_add(a.n_hit, truth);
  if (pred_r == truth) ec_add(a.n_hit_r, truth);
  if (a.cmat && pred != EC_NONE) ec_add(a.cmat, (size_t)truth * a.C + pred);
}

// ------------------------------------------------------------------------------------------------ column rank statistics
constexpr int RK_BLOCK = 1024, RK_WAVES = RK_BLOCK / 64;
constexpr int RK_TILE = MVLPT_EVAL_SORT_TILE;      // items of one LDS tile
constexpr u64 RK_PAD = ~0ull;                      // behind every item (an item has 33 bits)
static_assert((RK_TILE & (RK_TILE - 1)) == 0 && RK_TILE >= 2 * RK_BLOCK, "the tile is a power of two and holds a pair per thread");

struct RankArgs {
  const float* scores; long long ld; int N, C;
  const long long* label; const float* target; long long target_ld;
  const int* rows; int n;                          // n: selected rows (the list's length, or N)
  int P;                                           // n padded to a power of two, >= 2
  double th[MVLPT_EVAL_POINTS];
  long long *n_pos, *n_neg, *twice_u; double* interp; int* flags;
  u64* ws; size_t ws_stride;                       // P items per workgroup (columns longer than the tile)
};

__device__ __forceinline__ void rk_cmpx(u64* p, unsigned i, unsigned j, bool asc) {
  const u64 x = p[i], y = p[j];
  if ((x > y) == asc) { p[i] = y; p[j] = x; }
}

// one (k, j) stage of the network over `len` items at p, whose first item has index `base` of the column; a barrier behind it
__device__ __forceinline__ void rk_stage(u64* p, unsigned len, unsigned base, unsigned k, unsigned j) {
  for (unsigned q = threadIdx.x; q < len / 2; q += RK_BLOCK) {
    const unsigned i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
    rk_cmpx(p, i, i + j, ((base + i) & k) == 0);
  }
  __syncthreads();
}

// the item of selected row e of column col, and its contribution to the positive count and the non-finite flag
__device__ __forceinline__ u64 rk_item(const RankArgs& a, int col, int e, int& n_pos, int& flag) {
  int row = a.rows ? a.rows[e] : e;
  row = min(max(row, 0), a.N - 1);
  unsigned u = __float_as_uint(a.scores[(size_t)row * a.ld + col]);
  if ((u & 0x7f800000u) == 0x7f800000u) flag |= MVLPT_EVAL_FLAG_NONFINITE;
  if ((u << 1) == 0) u = 0;                                              // -0.0 and +0.0 are one run
  const unsigned key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  unsigned pos;
  if (a.label) {
    pos = a.label[row] == col;
  } else {
    const float y = a.target[(size_t)row * a.target_ld + col];
    pos = y == 1.0f;
    if (y != 0.f && !pos) flag |= MVLPT_EVAL_FLAG_SOFT_TARGET;
  }
  n_pos += pos;
  return ((u64)key << 1) | pos;
}

struct RkScan { int start, seg, tot; };            // start of the current run (-1: none yet), positives in it, positives so far
__device__ __forceinline__ RkScan rk_combine(const RkScan& l, const RkScan& r) {
  return RkScan{max(l.start, r.start), r.start >= 0 ? r.seg : l.seg + r.seg, l.tot + r.tot};
}

template <bool RESIDENT>
__global__ __launch_bounds__(RK_BLOCK) void eval_rank_columns(RankArgs a) {
  __shared__ u64 tile[RK_TILE];
  __shared__ RkScan wave_scan[RK_WAVES];
  __shared__ double wave_best[RK_WAVES][MVLPT_EVAL_POINTS];
  __shared__ long long wave_sum[RK_WAVES];
  __shared__ int s_npos, s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n;
  const unsigned P = (unsigned)a.P;
  u64* buf = RESIDENT ? tile : a.ws + (size_t)blockIdx.x * a.ws_stride;

  for (int col = blockIdx.x; col < a.C; col += gridDim.x) {
    if (tid == 0) { s_npos = 0; s_flag = 0; }
    __syncthreads();

    // ---- items, sorted inside every tile (k = 2 .. min(P, RK_TILE))
    int my_pos = 0, my_flag = 0;
    const unsigned T = RESIDENT ? P : (unsigned)RK_TILE;
    for (unsigned base = 0; base < P; base += T) {
      for (unsigned t = tid; t < T; t += RK_BLOCK) tile[t] = (int)(base + t) < n ? rk_item(a, col, base + t, my_pos, my_flag) : RK_PAD;
      __syncthreads();
      for (unsigned k = 2; k <= T; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) rk_stage(tile, T, base, k, j);
      if (!RESIDENT) {
        for (unsigned t = tid; t < T; t += RK_BLOCK) buf[base + t] = tile[t];
        __syncthreads();
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { my_pos += __shfl_xor(my_pos, off); my_flag |= __shfl_xor(my_flag, off); }
    if (lane == 0) { atomicAdd(&s_npos, my_pos); atomicOr(&s_flag, my_flag); }

    // ---- the merges across tiles: long strides over the scratch buffer, the rest tile by tile in LDS
    if (!RESIDENT) {
      for (unsigned k = 2 * T; k <= P; k <<= 1) {
        for (unsigned j = k >> 1; j >= T; j >>= 1) rk_stage(buf, P, 0, k, j);
        for (unsigned base = 0; base < P; base += T) {
          for (unsigned t = tid; t < T; t += RK_BLOCK) tile[t] = buf[base + t];
          __syncthreads();
          for (unsigned j = T >> 1; j > 0; j >>= 1) rk_stage(tile, T, base, k, j);
          for (unsigned t = tid; t < T; t += RK_BLOCK) buf[base + t] = tile[t];
          __syncthreads();
        }
      }
    }
    __syncthreads();
    const int n_pos = s_npos;

    // ---- one pass over the sorted items
    double best[MVLPT_EVAL_POINTS];
#pragma unroll
    for (int t = 0; t < MVLPT_EVAL_POINTS; ++t) best[t] = 0.0;
    long long sum = 0;
    RkScan carry{-1, 0, 0};
    for (int c0 = 0; c0 < n; c0 += RK_BLOCK) {
      const int i = c0 + tid;
      const bool valid = i < n;
      const u64 cur = valid ? buf[i] : 0;
      const int pos = (int)(cur & 1);
      const bool start = valid && (i == 0 || (buf[i - 1] >> 1) != (cur >> 1));
      const bool end = valid && (i == n - 1 || (buf[i + 1] >> 1) != (cur >> 1));
      RkScan s{start ? i : -1, pos, pos};
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        RkScan l{__shfl_up(s.start, off), __shfl_up(s.seg, off), __shfl_up(s.tot, off)};
        if (lane >= off) s = rk_combine(l, s);
      }
      if (lane == 63) wave_scan[wave] = s;
      __syncthreads();
      RkScan before = carry;
      for (int w = 0; w < RK_WAVES; ++w) {
        if (w == wave) s = rk_combine(before, s);
        before = rk_combine(before, wave_scan[w]);
      }
      carry = before;
      if (end) sum += (long long)s.seg * ((long long)s.start + 1 + (i + 1));
      if (start) {
        const int tp = n_pos - (s.tot - pos);
        const double precision = (double)tp / (double)(n - i);
        const double recall = n_pos ? (double)tp / (double)n_pos : 1.0;
#pragma unroll
        for (int t = 0; t < MVLPT_EVAL_POINTS; ++t)
          if (a.th[t] <= recall) best[t] = fmax(best[t], precision);
      }
      __syncthreads();                                                   // wave_scan is rewritten by the next chunk
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off);
#pragma unroll
      for (int t = 0; t < MVLPT_EVAL_POINTS; ++t) best[t] = fmax(best[t], __shfl_xor(best[t], off));
    }
    if (lane == 0) {
      wave_sum[wave] = sum;
#pragma unroll
      for (int t = 0; t < MVLPT_EVAL_POINTS; ++t) wave_best[wave][t] = best[t];
    }
    __syncthreads();
    if (tid < MVLPT_EVAL_POINTS) {
      double b = a.th[tid] <= 0.0 ? 1.0 : 0.0;                           // the closing point (precision 1, recall 0)
      for (int w = 0; w < RK_WAVES; ++w) b = fmax(b, wave_best[w][tid]);
      a.interp[(size_t)col * MVLPT_EVAL_POINTS + tid] = b;
    } else if (tid == 64) {
      long long s = 0;
      for (int w = 0; w < RK_WAVES; ++w) s += wave_sum[w];
      a.n_pos[col] = n_pos;
      a.n_neg[col] = n - n_pos;
      a.twice_u[col] = s - (long long)n_pos * (n_pos + 1);
      a.flags[col] = s_flag;
    }
    __syncthreads();                                                     // the shared words are reset for the next column
  }
}

}  // namespace

hipError_t launch_eval_count(const EvalCountArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int per = EC_BLOCK / 64;
  eval_count<<<(a.n + per - 1) / per, EC_BLOCK, 0, s>>>(a);
  return hipGetLastError();
}

EvalRankPlan eval_rank_plan(int n, int C, int cus) {
  EvalRankPlan p;
  p.P = 2;
  while (p.P < n) p.P <<= 1;
  p.resident = p.P <= RK_TILE;
  p.grid = std::max(1, std::min(C, 2 * cus));                           // workgroups walk the columns; ~100 VGPRs x 1024 threads: one runs per CU
  if (!p.resident) {
    p.grid = std::min<long long>(p.grid, std::max<long long>(1, ((long long)1 << 27) / p.P));      // at most 1 GiB of scratch
    p.ws_bytes = (size_t)p.grid * p.P * sizeof(u64);
  }
  return p;
}

hipError_t launch_eval_rank_columns(const float* scores, long long ld, int N, int C, const long long* label, const float* target,
                                    long long target_ld, const int* rows, int n, const double* thresholds, long long* n_pos,
                                    long long* n_neg, long long* twice_u, double* interp, int* flags, void* ws, const EvalRankPlan& p,
                                    hipStream_t s) {
  RankArgs a;
  a.scores = scores; a.ld = ld; a.N = N; a.C = C;
  a.label = label; a.target = target; a.target_ld = target_ld;
  a.rows = rows; a.n = n; a.P = p.P;
  for (int t = 0; t < MVLPT_EVAL_POINTS; ++t) a.th[t] = thresholds[t];
  a.n_pos = n_pos; a.n_neg = n_neg; a.twice_u = twice_u; a.interp = interp; a.flags = flags;
  a.ws = (u64*)ws; a.ws_stride = (size_t)p.P;
  if (p.resident) eval_rank_columns<true><<<p.grid, RK_BLOCK, 0, s>>>(a);
  else eval_rank_columns<false><<<p.grid, RK_BLOCK, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace mvlpt
