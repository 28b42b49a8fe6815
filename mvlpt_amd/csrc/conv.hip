// Forward-only convolutional tower kernels (CLIP ModifiedResNet, clip/model.py:10-150) for gfx950.
//
// Activations are NHWC fp16: a [B,H,W,C] map is the [B*H*W, C] matrix an implicit GEMM wants, and the stage-4 output is already
// the [B, HW, E] token matrix of the attention pool.
//   conv2d_kernel        implicit GEMM on v_mfma_f32_16x16x32_f16: M = B*Ho*Wo output pixels, N = Cout, K = k*k*Cin, the weight
//                        pre-packed [Cout, Kp] tap-major (ky, kx, ci) so that every 8-channel run of a tap is one 16-byte load;
//                        epilogue y = acc * scale[c] + shift[c] (+ resid) -> ReLU -> one rounding (BatchNorm in eval mode enters as
//                        the fp32 scale / shift: the fp16 weights are never rescaled, so they are never rounded a second time)
//   avgpool2x2_kernel    AvgPool2d(2): fp32 sum of four, one rounding
//   nchw_to_nhwc8_kernel the image [B,3,R,R] -> [B,R,R,8] fp16, channels 3..7 zero
//   attnpool_tokens_kernel / attnpool_query_kernel: the AttentionPool2d glue around three launch_gemm calls
#include "kernels.h"

namespace mvlpt {
namespace {

constexpr int CV_BM = 64, CV_BN = 64, CV_BK = 32;      // workgroup tile; 4 waves as 2 x 2, 32 pixels x 32 channels each
constexpr int CV_LD = CV_BK + 8;                        // LDS row pitch in halves: 80 bytes (16-byte aligned, rows 20 banks apart)

struct ConvParams {
  const f16* x; const f16* w; const float* scale; const float* shift; const f16* resid; f16* y;
  int B, H, W, Cin, Cout, Ho, Wo, k, stride, pad, Kp, M, relu;
};

// The MFMA runs "transposed": its A operand is the weight tile (rows = output channels), its B operand the pixel tile, so that a
// lane ends up with FOUR CONSECUTIVE CHANNELS of one pixel (D[row = 4*(l>>4) + r][col = l&15], common.h) — one 8-byte NHWC store.
__global__ __launch_bounds__(256) void conv2d_kernel(ConvParams p) {
  __shared__ __attribute__((aligned(16))) f16 As[CV_BM * CV_LD];      // pixels  [m][k]
  __shared__ __attribute__((aligned(16))) f16 Ws[CV_BN * CV_LD];      // weights [n][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;
  // staging role: one 16-byte chunk of A and one of W per thread and K-step
  const int sr = tid >> 2, sc = (tid & 3) * 8;
  const int m = m0 + sr;
  const bool m_ok = m < p.M;
  int ob = 0, oy = 0, ox = 0;
  if (m_ok) { ob = m / (p.Ho * p.Wo); const int rem = m - ob * p.Ho * p.Wo; oy = rem / p.Wo; ox = rem - oy * p.Wo; }
  const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
  const f16* const xb = p.x + (size_t)ob * p.H * p.W * p.Cin;
  const int wn = n0 + sr;
  const bool n_ok = wn < p.Cout;
  const f16* const wrow = p.w + (size_t)(n_ok ? wn : 0) * p.Kp;
  const int K = p.k * p.k * p.Cin;
  // (tap, ci) of this thread's chunk, advanced by CV_BK per step (Cin % 8 == 0: a chunk never straddles two taps)
  int tap = sc / p.Cin, ci = sc - tap * p.Cin;

  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto load_a = [&](int k0) -> f16x8 {
    if (!m_ok || k0 >= K) return zero8;
    const int ky = tap / p.k, kx = tap - ky * p.k;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) return zero8;      // out-of-image tap of THIS pixel
    return *(const f16x8*)(xb + ((size_t)iy * p.W + ix) * p.Cin + ci);
  };
  auto load_w = [&](int k0) -> f16x8 { return n_ok ? *(const f16x8*)(wrow + k0) : zero8; };      // (Kp is zero padded)

  const int wm = (wave & 1) * 32, wnn = (wave >> 1) * 32;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.Kp / CV_BK;
  f16x8 ra = load_a(sc), rw = load_w(sc);
  for (int kt = 0; kt < nk; ++kt) {
    *(f16x8*)(As + sr * CV_LD + sc) = ra;
    *(f16x8*)(Ws + sr * CV_LD + sc) = rw;
    __syncthreads();
    if (kt + 1 < nk) {
      ci += CV_BK;
      while (ci >= p.Cin) { ci -= p.Cin; ++tap; }
      const int k0 = (kt + 1) * CV_BK + sc;
      ra = load_a(k0); rw = load_w(k0);
    }
    const int fo = (lane & 15) * CV_LD + (lane >> 4) * 8;
    f16x8 fw[2], fa[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) fw[j] = *(const f16x8*)(Ws + (wnn + 16 * j) * CV_LD + fo);
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = *(const f16x8*)(As + (wm + 16 * i) * CV_LD + fo);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<f16>(fw[j], fa[i], acc[i][j]);
    __syncthreads();
  }

  // epilogue: lane holds channels n .. n+3 of pixel mm (Cout % 8 == 0: a group of four is inside or outside as a whole)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int mm = m0 + wm + 16 * i + (lane & 15);
    if (mm >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wnn + 16 * j + 4 * (lane >> 4);
      if (n >= p.Cout) continue;
      const f32x4 sc4 = *(const f32x4*)(p.scale + n), sh4 = *(const f32x4*)(p.shift + n);
      const size_t o = (size_t)mm * p.Cout + n;
      f16x4 r4 = {0, 0, 0, 0};
      if (p.resid) r4 = *(const f16x4*)(p.resid + o);
      f16x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = fmaf(acc[i][j][e], sc4[e], sh4[e]);
        if (p.resid) v += (float)r4[e];
        if (p.relu) v = fmaxf(v, 0.f);
        out[e] = (f16)v;
      }
      *(f16x4*)(p.y + o) = out;
    }
  }
}

// w32 [Cout, Cin, k, k] -> out [Cout, Kp]: column (ky*k + kx) * cin_pad + ci, zero for ci >= Cin and behind k*k*cin_pad
__global__ void pack_conv_weight_kernel(const float* w, f16* out, int Cout, int Cin, int k, int cin_pad, int Kp) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)Cout * Kp) return;
  const int co = (int)(i / Kp), col = (int)(i - (size_t)co * Kp);
  float v = 0.f;
  if (col < k * k * cin_pad) {
    const int tap = col / cin_pad, ci = col - tap * cin_pad;
    if (ci < Cin) { const int ky = tap / k, kx = tap - ky * k; v = w[(((size_t)co * Cin + ci) * k + ky) * k + kx]; }
  }
  out[i] = (f16)v;
}

// BatchNorm in eval mode as a per-channel affine map: scale = g / sqrt(var + eps), shift = b - mean * scale
__global__ void bn_affine_kernel(const float* g, const float* b, const float* mean, const float* var, float eps, float* scale,
                                 float* shift, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = g[c] / sqrtf(var[c] + eps);
  scale[c] = s;
  shift[c] = b[c] - mean[c] * s;
}

__global__ void avgpool2x2_kernel(const f16* x, f16* y, int B, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * Ho * Wo * C8) return;
  const int c8 = (int)(i % C8); size_t r = i / C8;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho); const int b = (int)(r / Ho);
  const f16* s = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + c8 * 8;
  const f16x8 a = *(const f16x8*)s, bb = *(const f16x8*)(s + C), c = *(const f16x8*)(s + (size_t)W * C),
              d = *(const f16x8*)(s + (size_t)W * C + C);
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (f16)(((float)a[e] + (float)bb[e] + (float)c[e] + (float)d[e]) * 0.25f);
  *(f16x8*)(y + i * 8) = o;
}

template <typename T>
__global__ void nchw_to_nhwc8_kernel(const T* img, f16* out, int B, int R) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, plane = (size_t)R * R;
  if (i >= (size_t)B * plane) return;
  const size_t b = i / plane, px = i - b * plane;
  const T* s = img + b * 3 * plane + px;
  f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  o[0] = (f16)(float)s[0]; o[1] = (f16)(float)s[plane]; o[2] = (f16)(float)s[2 * plane];
  *(f16x8*)(out + i * 8) = o;
}

// tok [B, 1 + HW, E] = [mean over HW ; pixels] + pos  (clip/model.py AttentionPool2d.forward); one thread per (image, channel)
__global__ void attnpool_tokens_kernel(const f16* x, const float* pos, f16* tok, int B, int HW, int E) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (c >= E) return;
  const f16* xb = x + (size_t)b * HW * E + c;
  f16* tb = tok + (size_t)b * (HW + 1) * E + c;
  float sum = 0.f;
  for (int i = 0; i < HW; ++i) {
    const float v = (float)xb[(size_t)i * E];
    sum += v;
    tb[(size_t)(i + 1) * E] = (f16)(v + pos[(size_t)(i + 1) * E + c]);
  }
  tb[0] = (f16)(sum / (float)HW + pos[c]);
}

// Single-query attention: one wave per (image, head).  q [B, E], kv [B, T, 2E] = [K | V]; out [B, E] = softmax(q.K / 8) V per head.
constexpr int AP_MAX_T = 145;
__global__ __launch_bounds__(64) void attnpool_query_kernel(const f16* q, const f16* kv, f16* out, int T, int E) {
  __shared__ float qs[64];
  __shared__ float ps[AP_MAX_T + 3];
  const int lane = threadIdx.x, h = blockIdx.x, b = blockIdx.y;
  qs[lane] = (float)q[(size_t)b * E + h * 64 + lane];
  __syncthreads();
  const f16* kb = kv + (size_t)b * T * 2 * E + h * 64;
  float mx = -INFINITY;
  for (int t = lane; t < T; t += 64) {
    const f16* kr = kb + (size_t)t * 2 * E;
    float s = 0.f;
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
      const f16x8 k8 = *(const f16x8*)(kr + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(qs[c8 * 8 + e], (float)k8[e], s);
    }
    s *= 0.125f;
    ps[t] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float den = 0.f;
  for (int t = lane; t < T; t += 64) { const float e = __expf(ps[t] - mx); ps[t] = e; den += e; }
  den = wave_sum(den);
  __syncthreads();
  const f16* vb = kb + E + lane;
  float o = 0.f;
  for (int t = 0; t < T; ++t) o = fmaf(ps[t], (float)vb[(size_t)t * 2 * E], o);
  out[(size_t)b * E + h * 64 + lane] = (f16)(o / den);
}

}  // namespace

int conv_kp(int k, int cin_pad) { return (k * k * cin_pad + CV_BK - 1) / CV_BK * CV_BK; }
int attnpool_max_tokens() { return AP_MAX_T; }

const char* conv2d_check(const ConvArgs& a) {
  if (!a.x || !a.w || !a.scale || !a.shift || !a.y) return "null pointer";
  if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.Cin <= 0 || a.Cout <= 0) return "every extent must be positive";
  if (a.k != 1 && a.k != 3) return "kernel size must be 1 or 3";
  if (a.stride != 1 && !(a.stride == 2 && a.k == 3)) return "stride must be 1 (2 only with a 3x3 kernel)";
  if (a.Cin % 8 || a.Cout % 8) return "Cin and Cout must be multiples of 8";
  const long long Ho = (a.H + 2 * (a.k / 2) - a.k) / a.stride + 1, Wo = (a.W + 2 * (a.k / 2) - a.k) / a.stride + 1;
  if ((long long)a.B * Ho * Wo > 0x7fffffffLL - CV_BM) return "too many output pixels";
  return nullptr;
}

hipError_t launch_conv2d(const ConvArgs& a, hipStream_t s) {
  if (conv2d_check(a)) return hipErrorInvalidValue;
  ConvParams p;
  p.x = (const f16*)a.x; p.w = (const f16*)a.w; p.scale = a.scale; p.shift = a.shift; p.resid = (const f16*)a.resid; p.y = (f16*)a.y;
  p.B = a.B; p.H = a.H; p.W = a.W; p.Cin = a.Cin; p.Cout = a.Cout; p.k = a.k; p.stride = a.stride; p.pad = a.k / 2;
  p.Ho = (a.H + 2 * p.pad - a.k) / a.stride + 1; p.Wo = (a.W + 2 * p.pad - a.k) / a.stride + 1;
  p.Kp = conv_kp(a.k, a.Cin); p.M = a.B * p.Ho * p.Wo; p.relu = a.relu;
  dim3 grid((p.M + CV_BM - 1) / CV_BM, (p.Cout + CV_BN - 1) / CV_BN);
  hipLaunchKernelGGL(conv2d_kernel, grid, dim3(256), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_pack_conv_weight(const float* w32, void* out, int Cout, int Cin, int k, int cin_pad, hipStream_t s) {
  const int Kp = conv_kp(k, cin_pad);
  const size_t n = (size_t)Cout * Kp;
  hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w32, (f16*)out, Cout, Cin, k, cin_pad, Kp);
  return hipGetLastError();
}

hipError_t launch_bn_affine(const float* g, const float* b, const float* mean, const float* var, float eps, float* scale, float* shift,
                            int C, hipStream_t s) {
  hipLaunchKernelGGL(bn_affine_kernel, dim3((C + 255) / 256), dim3(256), 0, s, g, b, mean, var, eps, scale, shift, C);
  return hipGetLastError();
}

hipError_t launch_avgpool2x2(const void* x, void* y, int B, int H, int W, int C, hipStream_t s) {
  const size_t n = (size_t)B * (H / 2) * (W / 2) * (C / 8);
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(avgpool2x2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const f16*)x, (f16*)y, B, H, W, C);
  return hipGetLastError();
}

hipError_t launch_nchw_to_nhwc8(const void* image, int image_dtype, void* out, int B, int R, hipStream_t s) {
  const size_t n = (size_t)B * R * R;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (image_dtype == DT_F32) hipLaunchKernelGGL(nchw_to_nhwc8_kernel<float>, grid, block, 0, s, (const float*)image, (f16*)out, B, R);
  else if (image_dtype == DT_F16) hipLaunchKernelGGL(nchw_to_nhwc8_kernel<f16>, grid, block, 0, s, (const f16*)image, (f16*)out, B, R);
  else if (image_dtype == DT_BF16) hipLaunchKernelGGL(nchw_to_nhwc8_kernel<bf16>, grid, block, 0, s, (const bf16*)image, (f16*)out, B, R);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_attnpool_tokens(const void* x, const float* pos, void* tok, int B, int HW, int E, hipStream_t s) {
  hipLaunchKernelGGL(attnpool_tokens_kernel, dim3((E + 255) / 256, B), dim3(256), 0, s, (const f16*)x, pos, (f16*)tok, B, HW, E);
  return hipGetLastError();
}

hipError_t launch_attnpool_query(const void* q, const void* kv, void* out, int B, int T, int E, hipStream_t s) {
  if (T < 1 || T > AP_MAX_T || E % 64 || B > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attnpool_query_kernel, dim3(E / 64, B), dim3(64), 0, s, (const f16*)q, (const f16*)kv, (f16*)out, T, E);
  return hipGetLastError();
}

}  // namespace mvlpt
