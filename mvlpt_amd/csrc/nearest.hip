// Nearest table rows of a set of query vectors: for every row of q [R, d] the k rows of table [V, d] with the smallest Euclidean
// distance, ascending, without a [R, V] array anywhere (prompt interpretation: the nearest vocabulary tokens of learned context
// vectors, scripts/interpret_prompt.py:49-59 of the reference, which builds the whole cdist matrix and argsorts it).
//
// Arithmetic.  s(row, token) = sum_i (q_i - e_i)^2 in the difference form, fp32: ONE lane owns a (row, token) pair and adds its d terms
// as fmaf(diff, diff, s) for i = 0 .. d-1 in that order, so the bits of s depend on the two vectors alone — not on the token's place
// in the table, the row's place in its tile, the vocabulary slice or the grid.  dist = sqrtf(s) (correctly rounded).
//
// Order.  Every pair gets the 64-bit key (bits of s) << 32 | token: s >= +0 so its bit pattern orders as the number does, a NaN s is
// canonicalised to 0x7fc00000 (behind +inf, as torch.sort places it) and equal s order by token index.  Keys of one row are distinct, so
// "the k smallest keys" is a set that no visiting order can change; the selection is exact.
//
// Kernel 1 (nearest_partial).  Block = 4 waves, NR_ROWS query rows x one vocabulary slice.  The slice goes by in tiles of NR_TOK tokens,
// each lane owning NR_TPL of them, and in chunks of NR_DC columns: the tile's chunk is staged through LDS (global reads in 64-byte
// pieces of a row, prefetched into registers under the previous chunk's arithmetic; a lane then reads ITS tokens' columns as 16-byte
// LDS loads, pitch 20 dwords: 16 lanes on 16 distinct 16-byte slots), the query chunk is read as LDS broadcasts.  Per 16-byte column
// step a wave issues NR_ROWS + NR_TPL LDS loads for 8 * NR_ROWS * NR_TPL VALU instructions (a subtract and an fma per element; the
// library is built without packed fp32).  146 VGPRs and 40.5 KB of LDS: three blocks per compute unit.  Measured (DESIGN.md row i):
// 29 ms for R = 16 000 against the real table, 0.19 ms for R = 16.
// Each WAVE keeps the running best 64 keys of each of its rows sorted across its lanes (lane j = j-th best: 64 = MVLPT_NEAREST_MAX_K
// is the wave width) with the k-th as threshold; a tile's candidates are compared against it with one ballot, and only the rare
// qualifying ones are inserted (a shift across lanes).  No LDS, no atomics, nothing another wave can see.  At the end lanes 0 .. k-1
// store the wave's list: parts = slices * 4 partial lists of k keys per row are the only scratch memory.
// Kernel 2 (nearest_merge).  One wave per row pushes the row's parts * k partial keys through the same insertion and writes idx / dist.
#include <algorithm>

#include "../../include/mvlpt_hip.h"
#include "kernels.h"

namespace mvlpt {

namespace {

constexpr int NR_BLOCK = 256;                      // threads of nearest_partial
constexpr int NR_TPL = 2;                          // tokens per lane
constexpr int NR_TOK = NR_BLOCK * NR_TPL;          // tokens per tile
constexpr int NR_DC = 16;                          // columns per chunk (64 bytes of a table row)
constexpr int NR_PITCH = NR_DC + 4;                // LDS row pitch in dwords: 20 j mod 64 = 4 (5 j mod 16), 16 distinct 16-byte slots
constexpr int NR_LD = NR_TOK * (NR_DC / 4) / NR_BLOCK;   // 16-byte pieces a thread stages per chunk
constexpr unsigned long long NR_NONE = ~0ull;      // "no candidate": behind every key, NaN keys included
static_assert(NR_ROWS == 8 && NR_WAVES * 64 == NR_BLOCK, "kernels.h and nearest.hip disagree");
static_assert(MVLPT_NEAREST_MAX_K == 64, "the running list of a row is one entry per lane of a wave");

__device__ __forceinline__ unsigned long long nr_key(float s, unsigned token) {
  unsigned b = __float_as_uint(s);
  if (s != s) b = 0x7fc00000u;
  return ((unsigned long long)b << 32) | token;
}

// The wave's list `lst` (lane j = j-th smallest key, ascending) takes the wave-uniform key x; the largest entry falls off lane 63.
__device__ __forceinline__ void nr_insert(unsigned long long& lst, unsigned long long x, int lane) {
  const unsigned long long prev = __shfl_up(lst, 1);
  const bool first_behind = lane == 0 || prev < x;
  lst = lst < x ? lst : (first_behind ? x : prev);
}

// Every lane offers one key; those in front of the threshold (the k-th entry of the list) are inserted, lowest lane first.
// Insertion is serial, one shuffle round per qualifying key: rare on a table in no particular order (about k ln(n / k) of a slice's
// n tokens qualify), but a slice whose distances to a row DESCEND with the token index qualifies every token — slower, not wrong.
__device__ __forceinline__ void nr_offer(unsigned long long& lst, unsigned long long& thr, unsigned long long key, int k, int lane) {
  unsigned long long m = __ballot(key < thr);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const unsigned long long x = __shfl(key, src);
    if (x < thr) {             // wave-uniform: the threshold may have moved since the ballot
      nr_insert(lst, x, lane);
      thr = __shfl(lst, k - 1);
    }
  }
}

struct NrStage { float4 e[NR_LD]; float4 q; };

__global__ __launch_bounds__(NR_BLOCK) void nearest_partial(const float* __restrict__ q, const float* __restrict__ table, int R, int V,
                                                            int d, int k, int tiles_per_slice, int parts,
                                                            unsigned long long* __restrict__ part) {
  __shared__ float4 es4[NR_TOK * NR_PITCH / 4];
  __shared__ float4 qs4[NR_ROWS * NR_DC / 4];
  const float* es = (const float*)es4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * NR_ROWS;
  const int n_tiles = (V + NR_TOK - 1) / NR_TOK;
  const int tile_lo = blockIdx.x * tiles_per_slice;
  const int tile_hi = min(n_tiles, tile_lo + tiles_per_slice);
  const int n_chunks = (d + NR_DC - 1) / NR_DC;
  const int n_iter = (tile_hi - tile_lo) * n_chunks;      // >= 1: the host launches no empty slice

  unsigned long long lst[NR_ROWS], thr[NR_ROWS];
  float acc[NR_TPL][NR_ROWS];
#pragma unroll
  for (int r = 0; r < NR_ROWS; ++r) {
    lst[r] = thr[r] = NR_NONE;
#pragma unroll
    for (int j = 0; j < NR_TPL; ++j) acc[j][r] = 0.f;
  }

  // chunk c of tile t -> registers: the thread's NR_LD pieces of the table tile, and (threads 0 .. 31) one piece of the query tile.
  // Columns >= d and tokens >= V are staged as zeros: such a column adds fmaf(0, 0, s) = s, such a token is never offered.
  auto fetch = [&](int it, NrStage& st) {
    const int tile = tile_lo + it / n_chunks, i0 = (it % n_chunks) * NR_DC;
#pragma unroll
    for (int m = 0; m < NR_LD; ++m) {
      const int f = tid + NR_BLOCK * m, tok = tile * NR_TOK + (f >> 2), i = i0 + (f & 3) * 4;
      st.e[m] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (tok < V && i < d) st.e[m] = *(const float4*)(table + (size_t)tok * d + i);
    }
    st.q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < NR_ROWS * NR_DC / 4) {
      const int row = min(row0 + (tid >> 2), R - 1), i = i0 + (tid & 3) * 4;      // rows past R repeat the last one (never stored)
      if (i < d) st.q = *(const float4*)(q + (size_t)row * d + i);
    }
  };

  NrStage st;
  fetch(0, st);
  for (int it = 0; it < n_iter; ++it) {
    __syncthreads();                       // the previous chunk has been read by every wave
#pragma unroll
    for (int m = 0; m < NR_LD; ++m) {
      const int f = tid + NR_BLOCK * m;
      es4[((f >> 2) * NR_PITCH >> 2) + (f & 3)] = st.e[m];
    }
    if (tid < NR_ROWS * NR_DC / 4) qs4[tid] = st.q;
    __syncthreads();
    if (it + 1 < n_iter) fetch(it + 1, st);

#pragma unroll
    for (int i4 = 0; i4 < NR_DC / 4; ++i4) {
      float4 e[NR_TPL];
#pragma unroll
      for (int j = 0; j < NR_TPL; ++j) e[j] = *(const float4*)(es + (tid + NR_BLOCK * j) * NR_PITCH + i4 * 4);
#pragma unroll
      for (int r = 0; r < NR_ROWS; ++r) {
        const float4 qv = qs4[r * (NR_DC / 4) + i4];
#pragma unroll
        for (int j = 0; j < NR_TPL; ++j) {
          float s = acc[j][r], t;
          t = qv.x - e[j].x; s = fmaf(t, t, s);
          t = qv.y - e[j].y; s = fmaf(t, t, s);
          t = qv.z - e[j].z; s = fmaf(t, t, s);
          t = qv.w - e[j].w; s = fmaf(t, t, s);
          acc[j][r] = s;
        }
      }
    }

    if ((it + 1) % n_chunks == 0) {        // the tile is complete: offer its NR_TPL tokens per lane to every row's list
      const int tile = tile_lo + it / n_chunks;
#pragma unroll
      for (int j = 0; j < NR_TPL; ++j) {
        const int tok = tile * NR_TOK + tid + NR_BLOCK * j;
#pragma unroll
        for (int r = 0; r < NR_ROWS; ++r) {
          const unsigned long long key = tok < V ? nr_key(acc[j][r], (unsigned)tok) : NR_NONE;
          nr_offer(lst[r], thr[r], key, k, lane);
          acc[j][r] = 0.f;
        }
      }
    }
  }

  const int p = blockIdx.x * NR_WAVES + wave;
#pragma unroll
  for (int r = 0; r < NR_ROWS; ++r)
    if (row0 + r < R && lane < k) part[((size_t)(row0 + r) * parts + p) * k + lane] = lst[r];
}

__global__ __launch_bounds__(64) void nearest_merge(const unsigned long long* __restrict__ part, int parts, int k,
                                                    int32_t* __restrict__ idx, float* __restrict__ dist) {
  const int lane = threadIdx.x;
  const size_t row = blockIdx.x;
  const unsigned long long* src = part + row * (size_t)parts * k;
  const int n = parts * k;
  unsigned long long lst = NR_NONE, thr = NR_NONE;
  for (int c = 0; c < n; c += 64) {
    const unsigned long long key = c + lane < n ? src[c + lane] : NR_NONE;
    nr_offer(lst, thr, key, k, lane);
  }
  if (lane < k) {
    idx[row * k + lane] = (int32_t)(unsigned)(lst & 0xffffffffull);
    dist[row * k + lane] = sqrtf(__uint_as_float((unsigned)(lst >> 32)));
  }
}

}  // namespace

NearestPlan nearest_plan(int R, int V, int k, int cus) {
  NearestPlan p;
  p.row_tiles = (R + NR_ROWS - 1) / NR_ROWS;
  const int n_tiles = (V + NR_TOK - 1) / NR_TOK;
  // three blocks of 40.5 KB LDS fit a compute unit; slices exist to fill the device when there are few row tiles (R = 16: 2)
  const int want = std::max(1, std::min(n_tiles, (3 * cus + p.row_tiles - 1) / p.row_tiles));
  p.tiles_per_slice = (n_tiles + want - 1) / want;
  p.slices = (n_tiles + p.tiles_per_slice - 1) / p.tiles_per_slice;      // no empty slice
  p.parts = p.slices * NR_WAVES;
  p.ws_bytes = (size_t)R * p.parts * k * sizeof(unsigned long long);
  return p;
}

hipError_t launch_nearest_rows(const float* q, const float* table, int R, int V, int d, int k, int32_t* idx, float* dist, void* ws,
                               const NearestPlan& p, hipStream_t s) {
  unsigned long long* part = (unsigned long long*)ws;
  nearest_partial<<<dim3(p.slices, p.row_tiles), NR_BLOCK, 0, s>>>(q, table, R, V, d, k, p.tiles_per_slice, p.parts, part);
  nearest_merge<<<R, 64, 0, s>>>(part, p.parts, k, idx, dist);
  return hipGetLastError();
}

}  // namespace mvlpt
