// Attention forward for heads wider than 64 (ViT-H/14-class image towers: width 1280 = 16 heads of 80): non-causal, single 16-bit
// operands, forward only.  The structure is attn_fwd_stream_kernel's (attention_stream.hip): a workgroup of 4 waves owns 64 queries of
// one (sequence, head), K and V stream in 64-key chunks through a double-buffered LDS ring filled by LDS-DMA, the softmax runs online
// and lane-local on S^T = K Q^T, and the workgroups of one head sit on one XCD.
//   rows      : a row of W 16-bit elements is P = W / 8 pieces of 16 B, stored UNPADDED at a pitch of 2 W bytes (a K or V chunk is
//               P KiB; the ring is 4 P KiB: 40 KiB at W = 80, 64 KiB at W = 128).  K image and V image of a chunk are contiguous, so a
//               chunk is 2 P lane-linear 1 KiB DMA slabs and every wave issues P / 2 of them: the counted vmcnt wait is the same
//               constant in every wave.
//   swizzle   : pitches of 160 and 224 B spread the lane groups of a fragment read over all 64 LDS banks by themselves; 192 and 256 B
//               would put every fourth / every row on the same banks, so for W % 32 == 0 the pieces of row r are rotated by r (piece p
//               sits in slot (p + r) % P; an XOR swizzle needs a power-of-two piece count).
//   K Q^T     : v_mfma_f32_16x16x32 sums 32 along the head dimension and W / 32 is 2.5 or 3.5 for W = 80 / 112.  The last step gives the
//               lanes whose k = 8 * (lane >> 4) + j falls at or beyond W a ZERO fragment on both operands (W = 80: lane >> 4 >= 2 in
//               step 3), nothing is padded in memory or LDS.  (The 16x16x16 instruction would fit 80 = 5 x 16 exactly, at half the
//               rate per instruction: 5 half-rate steps against 3 full-rate ones.)
//   P V       : output columns are W / 16 tiles, no padding.
#include "attn_common.h"

namespace mvlpt {

namespace {

constexpr int WCK = 64;   // keys per streamed chunk

// block -> (sequence*head index, query chunk), all chunks of a head on one XCD (block b runs on XCD b % 8)
__device__ __forceinline__ bool wide_map_block(int nheads, int nchunks, int& nh, int& ch) {
  const int b = blockIdx.x, x = b & 7, r = b >> 3;
  nh = (r / nchunks) * 8 + x;
  ch = r % nchunks;
  return nh < nheads;
}

template <int W> struct WideGeom {
  static constexpr int P = W / 8;              // 16-byte pieces per row
  static constexpr int RB = W * 2;             // row pitch in bytes
  static constexpr int IMG = WCK * RB;         // one 64 x W image = P slabs of 1 KiB
  static constexpr int KS = (W + 31) / 32;     // 32-wide steps of the score product
  static constexpr int DT = W / 16;            // 16-column output tiles
  static constexpr bool ROT = W % 32 == 0;
  // byte offset of piece p of row r (r inside the chunk)
  static __device__ __forceinline__ int at(int r, int p) { return r * RB + (ROT ? (p + r) % P : p) * 16; }
};

// 1 / sqrt(W) in fp32, times log2(e): the scale sits in the exponent's FMA
template <int W> __device__ __forceinline__ constexpr float wide_scale() {
  return (W == 80 ? 0.11180339887498948f : W == 96 ? 0.10206207261596575f : W == 112 ? 0.09449111825230680f : 0.08838834764831845f) *
         1.4426950408889634f;
}

template <typename T, int W>
__global__ __launch_bounds__(256) void attn_fwd_wide_kernel(AttnArgs a, int nqc, int rows) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][K chunk | V chunk]
  using G = WideGeom<W>;
  using v8 = typename Vec<T>::v8;
  using v4 = typename Vec<T>::v4;
  constexpr int P = G::P, KS = G::KS, DT = G::DT;
  const int L = a.L, H = a.H, d = H * W;
  int nh, qc;
  if (!wide_map_block(a.N * H, nqc, nh, qc)) return;
  const int n = nh / H, h = nh % H;
  const size_t ld = (size_t)3 * d;
  const T* base = (const T*)a.qkv + (size_t)n * L * ld + h * W;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int qt = qc * 4 + wave;
  const int qrow = qt * 16 + fr;
  const bool active = qt * 16 < rows;
  const int nch = (L + WCK - 1) / WCK;

  // chunk c -> ring buffer c & 1: slabs wave, wave + 4, ... of the 2 P slabs [K image | V image]; slab t covers the lane-linear pieces
  // 64 t' .. 64 t' + 63 of its image (t' = t or t - P), piece g = row g / P, slot g % P.  Rows >= L re-read row L - 1 (finite; they
  // only ever meet P = 0 / masked scores).
  auto issue = [&](int c) {
    char* buf = smem + (c & 1) * 2 * G::IMG;
#pragma unroll
    for (int i = 0; i < P / 2; ++i) {
      const int t = wave + 4 * i;
      const int v = t >= P ? 1 : 0;
      const int g = (t - v * P) * 64 + lane;
      const int r = g / P, slot = g % P;
      const int p = G::ROT ? (slot + P - r % P) % P : slot;
      int row = c * WCK + r;
      row = row < L ? row : L - 1;
      dma_raw<16>(base + (size_t)row * ld + (size_t)(1 + v) * d + p * 8, buf + t * 1024);
    }
  };
  issue(0);
  const T* qp = base + (size_t)(qrow < L ? qrow : L - 1) * ld + fg * 8;
  v8 q[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (ks * 4 + fg < P) q[ks] = *(const v8*)(qp + ks * 32);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) q[ks][e] = from_f32<T>(0.f);
    }
  }
  // consume the operands here so that the compiler's own vmcnt wait for them sits BEFORE the loop (attn_fwd_stream_kernel)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(q[ks]));

  constexpr float SC = wide_scale<W>();
  float mrun = -INFINITY, sum = 0.f;
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < nch; ++c) {
    if (c > 0) __builtin_amdgcn_s_barrier();                    // every wave is done with the buffer chunk c+1 overwrites
    if (c + 1 < nch) { issue(c + 1); asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P / 2) : "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                               // all pieces of chunk c have landed
    if (!active) continue;
    const char* sK = smem + (c & 1) * 2 * G::IMG;
    const char* sV = sK + G::IMG;
    f32x4 s[4];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int p = ks * 4 + fg;
        v8 kf = *(const v8*)(sK + G::at(u * 16 + fr, p < P ? p : P - 1));
        if ((ks + 1) * 4 > P && p >= P) {
#pragma unroll
          for (int e = 0; e < 8; ++e) kf[e] = from_f32<T>(0.f);
        }
        s[u] = mfma16<T>(kf, q[ks], s[u]);
      }
      if (c * WCK + (u + 1) * 16 > L) {                          // keys >= L: weight exactly 0
#pragma unroll
        for (int r = 0; r < 4; ++r) s[u][r] = c * WCK + u * 16 + fg * 4 + r < L ? s[u][r] : -INFINITY;
      }
      mx = fmaxf(mx, fmaxf(fmaxf(s[u][0], s[u][1]), fmaxf(s[u][2], s[u][3])));
    }
    mx = quad_max(mx) * SC;
    const float mnew = fmaxf(mrun, mx);                         // finite: key c * 64 < L is never masked
    const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
    mrun = mnew;
    sum *= alpha;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) { s[u][r] = __builtin_amdgcn_exp2f(fmaf(s[u][r], SC, -mnew)); sum += s[u][r]; }
    // V^T fragments by hardware transpose (attn_common.h frag_vt, at this kernel's pitch): the lane supplies 4 elements of key
    // kb * 32 + fg * 4 + (fr >> 2) (and of that key + 16), columns dt * 16 + (fr & 3) * 4 ..
    const int koff = fg * 4 + (fr >> 2);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const v8 pf = pack8<T>(s[2 * kb], s[2 * kb + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int piece = dt * 2 + ((fr & 3) >> 1), sub = (fr & 1) * 8;
        const v4 lo = tr_read4<T>(sV + G::at(kb * 32 + koff, piece) + sub);
        const v4 hi = tr_read4<T>(sV + G::at(kb * 32 + 16 + koff, piece) + sub);
        v8 vf;
#pragma unroll
        for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[e + 4] = hi[e]; }
        o[dt] = mfma16<T>(vf, pf, o[dt]);
      }
    }
  }
  if (!active) return;
  sum = quad_sum(sum);
  const float inv = 1.0f / sum;
  if (qrow < rows) {
    T* op = (T*)a.out + ((size_t)n * L + qrow) * d + h * W + fg * 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      v4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = from_f32<T>(o[dt][e] * inv);
      *(v4*)(op + dt * 16) = w;
    }
    if (a.lse && fg == 0) a.lse[((size_t)n * H + h) * L + qrow] = (mrun + log2f(sum)) * 0.6931471805599453f;
  }
}

template <typename T, int W>
hipError_t fwd_wide_t(const AttnArgs& a, hipStream_t s) {
  const int rows = a.q_rows > 0 ? (a.q_rows < a.L ? a.q_rows : a.L) : a.L;
  const int nqc = (rows + WCK - 1) / WCK;
  const long long grid = ((long long)a.N * a.H + 7) / 8 * 8 * nqc;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((attn_fwd_wide_kernel<T, W>), dim3((unsigned)grid), dim3(256), 4 * WideGeom<W>::IMG, s, a, nqc, rows);
  return hipGetLastError();
}
template <typename T>
hipError_t fwd_wide_w(const AttnArgs& a, int w, hipStream_t s) {
  switch (w) {
    case 80: return fwd_wide_t<T, 80>(a, s);
    case 96: return fwd_wide_t<T, 96>(a, s);
    case 112: return fwd_wide_t<T, 112>(a, s);
    case 128: return fwd_wide_t<T, 128>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

bool attn_wide_supported(int head_width) { return head_width == 80 || head_width == 96 || head_width == 112 || head_width == 128; }

hipError_t launch_attn_fwd_wide(int dtype, const AttnArgs& a, int head_width, hipStream_t s) {
  if (!a.qkv || !a.out || a.L <= 0 || a.N <= 0 || a.H <= 0 || a.q_rows < 0 || a.causal) return hipErrorInvalidValue;
  if (dtype == DT_F16) return fwd_wide_w<f16>(a, head_width, s);
  if (dtype == DT_BF16) return fwd_wide_w<bf16>(a, head_width, s);
  return hipErrorInvalidValue;
}

}  // namespace mvlpt
