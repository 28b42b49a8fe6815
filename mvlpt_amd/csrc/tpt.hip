// Test-time prompt tuning head: V augmented views of every test image g against the image's own C text rows, all fp32.
//   z[g,v,c] = scale <img/|img|, txt/|txt|>,  logp = z - logsumexp_c z,  H[g,v] = -sum_c exp(logp) logp,
//   sel[g] = the k views with the smallest (H, v) (NaN last),  a[g,c] = logsumexp_{v in sel} logp - log k,  loss[g] = -sum_c exp(a) a,
// and the gradient of sum_g w_g loss[g] with respect to the UN-normalised text rows with the selection held constant
// (semantics, limits and the order rule: include/mvlpt_hip.h).  No [G, V, C] array exists unless the caller asks for z.
//
// Arithmetic: the fp32 vector ALU, not the fp32 matrix instruction.  At G V C e = 16 * 64 * 1000 * 512 the product is 1 GFLOP, a
// fraction of a millisecond either way next to a text tower of G * C sequences, and with ONE lane owning a (view, class) pair and
// adding its e terms as fmaf in the order i = 0 .. e-1 the bits of z depend on the two rows alone: not on the view's position, the
// class tile, the group or the grid.  That is what makes two bit-identical views tie exactly.
//
// Forward, six launches on one stream (tpt_normalize once per operand):
//   tpt_normalize   one wave per row of img and of txt: xn = x / |x| and |x| into the workspace.
//   tpt_logits<0>   block = (TP_VT views, group): the C classes go by in tiles of 256 (thread = class) and chunks of TP_DC columns staged
//                   through LDS as in nearest.hip (own row as 16-byte reads at pitch 20 dwords, the views as broadcasts).  Every thread
//                   keeps, per view, the running softmax statistics (m, s, t) = (max, sum exp(z - m), sum exp(z - m)(z - m)) of ITS
//                   classes; they are merged across the wave by shuffles and across the four waves through LDS in a fixed order.
//                   H = log s - t / s has no cancellation (z - m <= 0); m and log s go to the workspace.
//   tpt_select      block = group: rank of a view = number of smaller 64-bit keys (ordered bits of H) << 32 | v.  Keys are distinct, so
//                   the k smallest are a set and an order that no schedule can change.
//   tpt_logits<1>   the same product for the k selected views only, one class tile per block: logp = (z - m) - log s -> workspace.
//   tpt_marginal    block = group: a[c] over the k rows of logp in the order of sel, loss by a fixed-order block sum.
// Backward, two launches; it READS what the forward left in the workspace (normalised rows, |txt|, sel, logp, a) and recomputes
// nothing, so it must follow its forward on the same stream with the same workspace; it may be repeated.
//   tpt_dz          wave = (selected view j, group): d_j = sum_c p u, then dz = (w / k) p (u - d_j).
//   tpt_dtxt        wave = text row: dtn = scale sum_j dz[j] imn[sel_j] (j ascending), dtxt = (dtn - <dtn, tn> tn) / |txt|.
// No atomics anywhere; every sum has one order.
#include <algorithm>

#include "../../include/mvlpt_hip.h"
#include "kernels.h"

namespace mvlpt {

namespace {

constexpr int TP_BLOCK = 256;                      // threads of every kernel here: 4 waves
constexpr int TP_VT = 8;                           // views per block of tpt_logits
constexpr int TP_DC = 16;                          // columns per chunk (64 bytes of a row)
constexpr int TP_PITCH = TP_DC + 4;                // LDS row pitch in dwords: 16 lanes on 16 distinct 16-byte slots
constexpr int TP_LD = TP_BLOCK * (TP_DC / 4) / TP_BLOCK;     // 16-byte pieces of the class tile a thread stages per chunk
static_assert(TP_VT * (TP_DC / 4) <= 64, "one wave stages the views' chunk");

// A product that feeds a sum must stay a ROUNDED product: z - m has to be exactly 0 where m is z, and merge(a, b) has to have the bits
// of merge(b, a).  The library is built with contraction on, under which neither __fmul_rn (a plain operator to the compiler) nor a
// contraction pragma keeps a * b - c from becoming fma(a, b, -c); passing the product through an empty asm does.  Every fused
// multiply-add in this file is an explicit fmaf.
__device__ __forceinline__ float tp_mul(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// Softmax statistics of a set of logits: m = max, s = sum exp(z - m), t = sum exp(z - m) (z - m); the empty set is (-inf, 0, 0).
struct TpStat { float m, s, t; };

// Union of two sets; merge(a, b) and merge(b, a) have the same bits (tp_mul).
__device__ __forceinline__ TpStat tp_merge(const TpStat a, const TpStat b) {
  TpStat r;
  r.m = fmaxf(a.m, b.m);
  const float da = a.s > 0.f ? a.m - r.m : 0.f, db = b.s > 0.f ? b.m - r.m : 0.f;
  const float ea = expf(da), eb = expf(db);
  r.s = __fadd_rn(tp_mul(a.s, ea), tp_mul(b.s, eb));
  r.t = __fadd_rn(tp_mul(ea, __fadd_rn(a.t, tp_mul(da, a.s))), tp_mul(eb, __fadd_rn(b.t, tp_mul(db, b.s))));
  return r;
}

__device__ __forceinline__ float tp_wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = __fadd_rn(x, __shfl_xor(x, o));
  return x;
}

// rows [R, e] -> xn = x / |x| and nrm = |x|; one wave per row, lane l owns the float4s l, l + 64, ...
__global__ __launch_bounds__(TP_BLOCK) void tpt_normalize(const float* __restrict__ x, float* __restrict__ xn, float* __restrict__ nrm,
                                                          long long R, int e) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (TP_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= R) return;
  const int n4 = e >> 2;
  const float4* src = (const float4*)(x + (size_t)row * e);
  float4 v[4];
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = lane + 64 * q;
    v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n4) v[q] = src[i];
    ss = fmaf(v[q].x, v[q].x, ss); ss = fmaf(v[q].y, v[q].y, ss); ss = fmaf(v[q].z, v[q].z, ss); ss = fmaf(v[q].w, v[q].w, ss);
  }
  const float n = sqrtf(tp_wave_sum(ss));
  float4* dst = (float4*)(xn + (size_t)row * e);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = lane + 64 * q;
    if (i < n4) dst[i] = make_float4(v[q].x / n, v[q].y / n, v[q].z / n, v[q].w / n);
  }
  if (nrm && lane == 0) nrm[row] = n;
}

struct TpStage { float4 t[TP_LD]; float4 q; };

// SECOND = 0: all V views, every class tile, statistics -> H, mrow, lsrow (and z when asked for).
// SECOND = 1: the k views of sel, class tile blockIdx.z, logp -> lp [G, k, C].
template <int SECOND>
__global__ __launch_bounds__(TP_BLOCK) void tpt_logits(const float* __restrict__ imn, const float* __restrict__ tn, int V, int C, int e,
                                                       float scale, int k, const int* __restrict__ sel, float* __restrict__ zout,
                                                       float* __restrict__ H, float* __restrict__ mrow, float* __restrict__ lsrow,
                                                       float* __restrict__ lp) {
  __shared__ float4 ts4[TP_BLOCK * TP_PITCH / 4];
  __shared__ float4 qs4[TP_VT * TP_DC / 4];
  __shared__ float red[TP_BLOCK / 64][TP_VT][3];
  const float* ts = (const float*)ts4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.y;
  const int n_views = SECOND ? k : V;
  const int slot0 = blockIdx.x * TP_VT;                         // < n_views: the host launches no empty block
  const int n_tiles = (C + TP_BLOCK - 1) / TP_BLOCK;
  const int tile_lo = SECOND ? (int)blockIdx.z : 0, tile_hi = SECOND ? tile_lo + 1 : n_tiles;
  const int n_chunks = (e + TP_DC - 1) / TP_DC;
  const int n_iter = (tile_hi - tile_lo) * n_chunks;
  const float* tg = tn + (size_t)g * C * e;

  // the view this thread stages (threads 0 .. TP_VT * 4 - 1); slots past the last view repeat it (never stored)
  int my_view = 0;
  if (tid < TP_VT * (TP_DC / 4)) {
    const int s = min(slot0 + (tid >> 2), n_views - 1);
    my_view = SECOND ? sel[(size_t)g * k + s] : s;
    my_view = min(max(my_view, 0), V - 1);
  }
  const float* my_img = imn + ((size_t)g * V + my_view) * e;

  float acc[TP_VT];
  TpStat st[TP_VT];
#pragma unroll
  for (int j = 0; j < TP_VT; ++j) { acc[j] = 0.f; st[j].m = -INFINITY; st[j].s = 0.f; st[j].t = 0.f; }

  // columns >= e and classes >= C are staged as zeros: such a column adds fmaf(0, 0, acc) = acc, such a class is never used
  auto fetch = [&](int it, TpStage& sg) {
    const int tile = tile_lo + it / n_chunks, i0 = (it % n_chunks) * TP_DC;
#pragma unroll
    for (int m = 0; m < TP_LD; ++m) {
      const int f = tid + TP_BLOCK * m, c = tile * TP_BLOCK + (f >> 2), i = i0 + (f & 3) * 4;
      sg.t[m] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C && i < e) sg.t[m] = *(const float4*)(tg + (size_t)c * e + i);
    }
    sg.q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < TP_VT * (TP_DC / 4)) {
      const int i = i0 + (tid & 3) * 4;
      if (i < e) sg.q = *(const float4*)(my_img + i);
    }
  };

  TpStage sg;
  fetch(0, sg);
  for (int it = 0; it < n_iter; ++it) {
    __syncthreads();                       // the previous chunk has been read by every wave
#pragma unroll
    for (int m = 0; m < TP_LD; ++m) {
      const int f = tid + TP_BLOCK * m;
      ts4[((f >> 2) * TP_PITCH >> 2) + (f & 3)] = sg.t[m];
    }
    if (tid < TP_VT * (TP_DC / 4)) qs4[tid] = sg.q;
    __syncthreads();
    if (it + 1 < n_iter) fetch(it + 1, sg);

#pragma unroll
    for (int i4 = 0; i4 < TP_DC / 4; ++i4) {
      const float4 t = *(const float4*)(ts + tid * TP_PITCH + i4 * 4);
#pragma unroll
      for (int j = 0; j < TP_VT; ++j) {
        const float4 q = qs4[j * (TP_DC / 4) + i4];
        float s = acc[j];
        s = fmaf(q.x, t.x, s); s = fmaf(q.y, t.y, s); s = fmaf(q.z, t.z, s); s = fmaf(q.w, t.w, s);
        acc[j] = s;
      }
    }

    if ((it + 1) % n_chunks == 0) {        // the tile is complete
      const int c = (tile_lo + it / n_chunks) * TP_BLOCK + tid;
#pragma unroll
      for (int j = 0; j < TP_VT; ++j) {
        const float z = tp_mul(scale, acc[j]);
        acc[j] = 0.f;
        const int slot = slot0 + j;
        if (c < C && slot < n_views) {
          if (SECOND) {
            const int v = min(max(sel[(size_t)g * k + slot], 0), V - 1);
            const size_t gv = (size_t)g * V + v;
            lp[((size_t)g * k + slot) * C + c] = __fsub_rn(__fsub_rn(z, mrow[gv]), lsrow[gv]);
          } else {
            if (zout) zout[((size_t)g * V + slot) * C + c] = z;
            TpStat one; one.m = z; one.s = 1.f; one.t = 0.f;
            st[j] = tp_merge(st[j], one);
          }
        }
      }
    }
  }

  if (SECOND) return;
#pragma unroll
  for (int j = 0; j < TP_VT; ++j) {
    TpStat a = st[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      TpStat b;
      b.m = __shfl_xor(a.m, o); b.s = __shfl_xor(a.s, o); b.t = __shfl_xor(a.t, o);
      a = tp_merge(a, b);
    }
    if (lane == 0) { red[wave][j][0] = a.m; red[wave][j][1] = a.s; red[wave][j][2] = a.t; }
  }
  __syncthreads();
  if (tid < TP_VT && slot0 + tid < n_views) {
    TpStat a; a.m = red[0][tid][0]; a.s = red[0][tid][1]; a.t = red[0][tid][2];
#pragma unroll
    for (int w = 1; w < TP_BLOCK / 64; ++w) {
      TpStat b; b.m = red[w][tid][0]; b.s = red[w][tid][1]; b.t = red[w][tid][2];
      a = tp_merge(a, b);
    }
    const float ls = logf(a.s);
    const size_t gv = (size_t)g * V + slot0 + tid;
    H[gv] = __fsub_rn(ls, a.t / a.s);
    mrow[gv] = a.m;
    lsrow[gv] = ls;
  }
}

// H [G, V] -> sel [G, k] (and the workspace's own copy): rank by counting over distinct keys.
__global__ __launch_bounds__(128) void tpt_select(const float* __restrict__ H, int V, int k, int* __restrict__ sel, int* __restrict__ sel_ws) {
  __shared__ unsigned long long key[128];
  const int v = threadIdx.x, g = blockIdx.x;
  unsigned long long mine = ~0ull;
  if (v < V) {
    const float h = H[(size_t)g * V + v];
    unsigned b = __float_as_uint(h);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);       // the bit pattern orders as the number does, -0 just in front of +0
    if (h != h) b = 0xffffffffu;                          // NaN behind +inf
    mine = ((unsigned long long)b << 32) | (unsigned)v;
  }
  key[v] = mine;
  __syncthreads();
  if (v >= V) return;
  int rank = 0;
  for (int u = 0; u < V; ++u) rank += key[u] < mine ? 1 : 0;
  if (rank < k) {
    sel[(size_t)g * k + rank] = v;
    sel_ws[(size_t)g * k + rank] = v;
  }
}

// lp [G, k, C] -> a [G, C] and loss [G]
__global__ __launch_bounds__(TP_BLOCK) void tpt_marginal(const float* __restrict__ lp, int C, int k, float* __restrict__ a_ws,
                                                         float* __restrict__ loss) {
  __shared__ float red[TP_BLOCK / 64];
  const int tid = threadIdx.x, g = blockIdx.x;
  const float* l = lp + (size_t)g * k * C;
  const float logk = logf((float)k);
  float part = 0.f;
  for (int c = tid; c < C; c += TP_BLOCK) {
    float mx = l[c];
    for (int j = 1; j < k; ++j) mx = fmaxf(mx, l[(size_t)j * C + c]);
    float s = 0.f;
    for (int j = 0; j < k; ++j) s = __fadd_rn(s, expf(__fsub_rn(l[(size_t)j * C + c], mx)));
    const float a = __fsub_rn(__fadd_rn(mx, logf(s)), logk);
    a_ws[(size_t)g * C + c] = a;
    part = __fadd_rn(part, tp_mul(expf(a), a));
  }
  part = tp_wave_sum(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) {
    float s = red[0];
#pragma unroll
    for (int w = 1; w < TP_BLOCK / 64; ++w) s = __fadd_rn(s, red[w]);
    loss[g] = 0.f - s;
  }
}

// dz [G, k, C] = (w_g / k) p (u - sum_c p u),  p = exp(lp),  u = -(a + 1); wave = (j, g)
__global__ __launch_bounds__(TP_BLOCK) void tpt_dz(const float* __restrict__ lp, const float* __restrict__ a_ws, const float* __restrict__ w,
                                                   int C, int k, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63, g = blockIdx.y;
  const int j = blockIdx.x * (TP_BLOCK / 64) + (threadIdx.x >> 6);
  if (j >= k) return;
  const float* l = lp + ((size_t)g * k + j) * C;
  const float* a = a_ws + (size_t)g * C;
  float d = 0.f;
  for (int c = lane; c < C; c += 64) d = __fadd_rn(d, tp_mul(expf(l[c]), 0.f - __fadd_rn(a[c], 1.f)));
  d = tp_wave_sum(d);
  const float coef = (w ? w[g] : 1.f) / (float)k;
  float* o = dz + ((size_t)g * k + j) * C;
  for (int c = lane; c < C; c += 64)
    o[c] = tp_mul(tp_mul(coef, expf(l[c])), __fsub_rn(0.f - __fadd_rn(a[c], 1.f), d));
}

// dtxt [G*C, e]; wave = text row g*C + c
__global__ __launch_bounds__(TP_BLOCK) void tpt_dtxt(const float* __restrict__ dz, const float* __restrict__ imn, const float* __restrict__ tn,
                                                     const float* __restrict__ nt, const int* __restrict__ sel, int V, int C, int e, int k,
                                                     float scale, long long rows, float* __restrict__ dtxt) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (TP_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int g = (int)(row / C), c = (int)(row - (long long)g * C);
  const int n4 = e >> 2;
  float4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < k; ++j) {
    const float d = dz[((size_t)g * k + j) * C + c];
    const int v = min(max(sel[(size_t)g * k + j], 0), V - 1);
    const float4* im = (const float4*)(imn + ((size_t)g * V + v) * e);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = lane + 64 * q;
      if (i < n4) {
        const float4 x = im[i];
        acc[q].x = fmaf(d, x.x, acc[q].x); acc[q].y = fmaf(d, x.y, acc[q].y);
        acc[q].z = fmaf(d, x.z, acc[q].z); acc[q].w = fmaf(d, x.w, acc[q].w);
      }
    }
  }
  const float4* t4 = (const float4*)(tn + (size_t)row * e);
  float4 t[4];
  float dot = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = lane + 64 * q;
    t[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n4) t[q] = t4[i];
    acc[q].x = tp_mul(scale, acc[q].x); acc[q].y = tp_mul(scale, acc[q].y);
    acc[q].z = tp_mul(scale, acc[q].z); acc[q].w = tp_mul(scale, acc[q].w);
    dot = fmaf(acc[q].x, t[q].x, dot); dot = fmaf(acc[q].y, t[q].y, dot); dot = fmaf(acc[q].z, t[q].z, dot); dot = fmaf(acc[q].w, t[q].w, dot);
  }
  dot = tp_wave_sum(dot);
  const float n = nt[row];
  float4* o = (float4*)(dtxt + (size_t)row * e);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = lane + 64 * q;
    if (i < n4)
      o[i] = make_float4(__fsub_rn(acc[q].x, tp_mul(dot, t[q].x)) / n, __fsub_rn(acc[q].y, tp_mul(dot, t[q].y)) / n,
                         __fsub_rn(acc[q].z, tp_mul(dot, t[q].z)) / n, __fsub_rn(acc[q].w, tp_mul(dot, t[q].w)) / n);
  }
}

size_t tp_round(size_t n) { return (n + 63) & ~(size_t)63; }      // sections start on 256-byte boundaries

}  // namespace

TptPlan tpt_plan(int G, int V, int C, int e, int k) {
  TptPlan p;
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += tp_round(n); return o; };
  p.off_imn = take((size_t)G * V * e);
  p.off_tn = take((size_t)G * C * e);
  p.off_nt = take((size_t)G * C);
  p.off_m = take((size_t)G * V);
  p.off_ls = take((size_t)G * V);
  p.off_sel = take((size_t)G * k);
  p.off_lp = take((size_t)G * k * C);
  p.off_a = take((size_t)G * C);
  p.off_dz = take((size_t)G * k * C);
  p.ws_bytes = off * sizeof(float);
  return p;
}

hipError_t launch_tpt_head_fwd(const float* img, const float* txt, float scale, int G, int V, int C, int e, int k, float* loss, float* H,
                               int32_t* sel, float* z, void* ws, const TptPlan& p, hipStream_t s) {
  float* f = (float*)ws;
  const long long ri = (long long)G * V, rt = (long long)G * C;
  const int wpb = TP_BLOCK / 64;
  tpt_normalize<<<(unsigned)((ri + wpb - 1) / wpb), TP_BLOCK, 0, s>>>(img, f + p.off_imn, nullptr, ri, e);
  tpt_normalize<<<(unsigned)((rt + wpb - 1) / wpb), TP_BLOCK, 0, s>>>(txt, f + p.off_tn, f + p.off_nt, rt, e);
  tpt_logits<0><<<dim3((V + TP_VT - 1) / TP_VT, G), TP_BLOCK, 0, s>>>(f + p.off_imn, f + p.off_tn, V, C, e, scale, k, nullptr, z, H,
                                                                      f + p.off_m, f + p.off_ls, nullptr);
  tpt_select<<<G, 128, 0, s>>>(H, V, k, sel, (int*)(f + p.off_sel));
  tpt_logits<1><<<dim3((k + TP_VT - 1) / TP_VT, G, (C + TP_BLOCK - 1) / TP_BLOCK), TP_BLOCK, 0, s>>>(
      f + p.off_imn, f + p.off_tn, V, C, e, scale, k, (const int*)(f + p.off_sel), nullptr, nullptr, f + p.off_m, f + p.off_ls, f + p.off_lp);
  tpt_marginal<<<G, TP_BLOCK, 0, s>>>(f + p.off_lp, C, k, f + p.off_a, loss);
  return hipGetLastError();
}

hipError_t launch_tpt_head_bwd(const float* w, float scale, int G, int V, int C, int e, int k, float* dtxt, void* ws, const TptPlan& p,
                               hipStream_t s) {
  float* f = (float*)ws;
  const int wpb = TP_BLOCK / 64;
  const long long rt = (long long)G * C;
  tpt_dz<<<dim3((k + wpb - 1) / wpb, G), TP_BLOCK, 0, s>>>(f + p.off_lp, f + p.off_a, w, C, k, f + p.off_dz);
  tpt_dtxt<<<(unsigned)((rt + wpb - 1) / wpb), TP_BLOCK, 0, s>>>(f + p.off_dz, f + p.off_imn, f + p.off_tn, f + p.off_nt,
                                                                 (const int*)(f + p.off_sel), V, C, e, k, scale, rt, dtxt);
  return hipGetLastError();
}

}  // namespace mvlpt
