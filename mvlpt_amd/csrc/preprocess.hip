// Input pipeline on the device: decoded uint8 HWC images -> the [B,3,R,R] normalised tensor the image tower reads.
// Replaces, bit for bit, what the reference does per image on CPU worker processes with PIL + torchvision
// (Dassl build_transform, configs/trainers/MVLPT/vit_b16.yaml:8-13: random_resized_crop (bicubic) / random_flip /
// normalize; ELEVATER eval: trainers/vision_benchmark/evaluation/feature.py:538-553 Resize(BICUBIC) [+ CenterCrop]):
//   crop box -> Pillow's two-pass antialiased bicubic resample for 8-bit images (22-bit fixed-point coefficients,
//   8-bit intermediate image, horizontal pass first, a pass whose size does not change is skipped) -> optional
//   window of the resized image (CenterCrop) -> optional horizontal flip -> u8/255 -> (x - mean)/std.
// Three kernels per batch, all HBM-bound byte work (no MFMA):
//   pp_coeffs_kernel      per image and pass: tap range + fixed-point weights of every output index, in DOUBLE with
//                         FMA contraction off so that the integers equal the ones Pillow's C code computes
//   pp_horizontal_kernel  one block per (image, source row): u8 x int32 taps -> 8-bit intermediate rows
//   pp_vertical_kernel    one block per (image, output row): taps down the columns (coalesced across x), then
//                         ToTensor / Normalize / flip, written as three coalesced CHW planes (fp32 / f16 / bf16)
// mvlpt_preprocess_aug (augmentations of Dassl's build_transform beyond those three: colorjitter, randomgrayscale, random_crop with
// padding, cutout) runs the same three kernels in their FILL form -- an output index outside the resized image gets an empty tap range,
// which produces 0 (torchvision pad(fill=0) in front of a crop) -- with the vertical pass writing only the flipped 8-bit window, then
//   pp_augment_kernel     one workgroup per image: the colour operations in the drawn order, in place on the 8-bit window
//                         (Pillow's ImageEnhance blends, convert("L"), convert("HSV") and back, restated bit for bit), grayscale,
//                         cutout holes, and the same ToTensor / Normalize.  Contrast needs the mean of L of the image as it
//                         stands at that point of the chain: an integer sum over the workgroup, so any order gives the same bits
#include "kernels.h"

namespace mvlpt {

constexpr int PP_PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ double pp_bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// table layout per (image, pass): int32 bounds[2 * n_out] then int32 kk[ks_max][n_out] (tap-major: coalesced reads)
template <bool FILL>
__global__ __launch_bounds__(256) void pp_coeffs_kernel(const PpDesc* __restrict__ descs, int32_t* __restrict__ tables,
                                                        size_t table_stride, int ks_max, int out_h, int out_w) {
#pragma clang fp contract(off)
  const PpDesc d = descs[blockIdx.x];
  const int pass = blockIdx.y;                                   // 0 horizontal, 1 vertical
  const int in_size = pass == 0 ? d.crop_w : d.crop_h;
  const int rs = pass == 0 ? d.resize_w : d.resize_h;
  const int off = pass == 0 ? d.out_left : d.out_top;
  const int n_out = pass == 0 ? out_w : out_h;
  int32_t* bounds = tables + ((size_t)blockIdx.x * 2 + pass) * table_stride;
  int32_t* kk = bounds + 2 * n_out;
  double scale = (double)in_size / rs, filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 2.0 * filterscale;
  const double ss = 1.0 / filterscale;
  for (int i = threadIdx.x; i < n_out; i += blockDim.x) {
    if (FILL && (off + i < 0 || off + i >= rs)) {                // outside the resized image: no taps, the passes produce 0
      bounds[2 * i] = 0;
      bounds[2 * i + 1] = 0;
      continue;
    }
    if (in_size == rs) {                                         // pass skipped by Pillow: identity tap
      bounds[2 * i] = off + i;
      bounds[2 * i + 1] = -1;
      continue;
    }
    const int xx = off + i;
    const double center = 0.0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += pp_bicubic((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
      double v = pp_bicubic((x + xmin - center + 0.5) * ss);
      if (ww != 0.0) v = v / ww;
      kk[(size_t)x * n_out + i] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << PP_PRECISION_BITS))
                                        : (int32_t)(0.5 + v * (double)(1 << PP_PRECISION_BITS));
    }
    bounds[2 * i] = xmin;
    bounds[2 * i + 1] = xmax;
  }
}

__device__ __forceinline__ uint8_t pp_clip8(int32_t v) {
  v >>= PP_PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// tmp[b][y][i][c] (u8), y over the crop rows the vertical pass reads, i over the output window columns
template <bool FILL>
__global__ __launch_bounds__(256) void pp_horizontal_kernel(const uint8_t* __restrict__ src, const PpDesc* __restrict__ descs,
                                                            const int32_t* __restrict__ tables, size_t table_stride,
                                                            uint8_t* __restrict__ tmp, size_t tmp_stride, int out_h, int out_w) {
  const int b = blockIdx.y, y = blockIdx.x;
  const PpDesc d = descs[b];
  if (y >= d.crop_h) return;
  const int32_t* hb = tables + ((size_t)b * 2 + 0) * table_stride;
  const int32_t* hk = hb + 2 * out_w;
  const int32_t* vb = tables + ((size_t)b * 2 + 1) * table_stride;
  // rows the vertical pass touches: [first tap of the first window row, last tap of the last window row]
  int j0 = 0, j1 = out_h - 1;
  if (FILL) {                                                    // ... of the window rows that lie inside the resized image
    j0 = d.out_top < 0 ? -d.out_top : 0;
    j1 = (int)min((long long)out_h, (long long)d.resize_h - d.out_top) - 1;
    if (j0 > j1) return;
  }
  const int v0 = vb[2 * j0], vl = vb[2 * j1], vn = vb[2 * j1 + 1];
  const int vend = vn < 0 ? vl + 1 : vl + vn;
  if (y < v0 || y >= vend) return;
  const uint8_t* row = src + d.offset + ((size_t)(d.crop_top + y) * d.width + d.crop_left) * 3;
  uint8_t* out = tmp + (size_t)b * tmp_stride + (size_t)y * out_w * 3;
  for (int i = threadIdx.x; i < out_w; i += blockDim.x) {
    const int xmin = hb[2 * i], n = hb[2 * i + 1];
    uint8_t r0, r1, r2;
    if (n < 0) {
      r0 = row[xmin * 3]; r1 = row[xmin * 3 + 1]; r2 = row[xmin * 3 + 2];
    } else {
      int32_t s0 = 1 << (PP_PRECISION_BITS - 1), s1 = s0, s2 = s0;
      const uint8_t* p = row + (size_t)xmin * 3;
      for (int x = 0; x < n; ++x) {
        const int32_t k = hk[(size_t)x * out_w + i];
        s0 += (int32_t)p[3 * x] * k; s1 += (int32_t)p[3 * x + 1] * k; s2 += (int32_t)p[3 * x + 2] * k;
      }
      r0 = pp_clip8(s0); r1 = pp_clip8(s1); r2 = pp_clip8(s2);
    }
    out[3 * i] = r0; out[3 * i + 1] = r1; out[3 * i + 2] = r2;
  }
}

template <typename TO> __device__ __forceinline__ void pp_store(TO* p, float v) { *p = (TO)v; }

template <typename TO>
__global__ __launch_bounds__(256) void pp_vertical_kernel(const PpDesc* __restrict__ descs, const int32_t* __restrict__ tables,
                                                          size_t table_stride, const uint8_t* __restrict__ tmp,
                                                          size_t tmp_stride, TO* __restrict__ out, uint8_t* __restrict__ out_u8,
                                                          int out_h, int out_w, float m0, float m1, float m2, float d0,
                                                          float d1, float d2) {
  const int b = blockIdx.y, j = blockIdx.x;                       // output row j of the window
  const PpDesc d = descs[b];
  const int32_t* vb = tables + ((size_t)b * 2 + 1) * table_stride;
  const int32_t* vk = vb + 2 * out_h;
  const int ymin = vb[2 * j], n = vb[2 * j + 1];
  const uint8_t* t = tmp + (size_t)b * tmp_stride;
  const size_t plane = (size_t)out_h * out_w;
  TO* o = out ? out + (size_t)b * 3 * plane + (size_t)j * out_w : nullptr;
  for (int i = threadIdx.x; i < out_w; i += blockDim.x) {
    uint8_t r0, r1, r2;
    if (n < 0) {
      const uint8_t* p = t + ((size_t)ymin * out_w + i) * 3;
      r0 = p[0]; r1 = p[1]; r2 = p[2];
    } else {
      int32_t s0 = 1 << (PP_PRECISION_BITS - 1), s1 = s0, s2 = s0;
      for (int y = 0; y < n; ++y) {
        const int32_t k = vk[(size_t)y * out_h + j];
        const uint8_t* p = t + ((size_t)(ymin + y) * out_w + i) * 3;
        s0 += (int32_t)p[0] * k; s1 += (int32_t)p[1] * k; s2 += (int32_t)p[2] * k;
      }
      r0 = pp_clip8(s0); r1 = pp_clip8(s1); r2 = pp_clip8(s2);
    }
    const int x = d.flip ? out_w - 1 - i : i;
    if (out_u8) {                                                 // resized 8-bit image (parity tests), HWC
      uint8_t* q = out_u8 + (((size_t)b * out_h + j) * out_w + x) * 3;
      q[0] = r0; q[1] = r1; q[2] = r2;
    }
    if (o) {
      // ToTensor: u8 -> fp32, / 255;  Normalize: (x - mean) / std  — two correctly rounded fp32 divisions, no FMA
      pp_store<TO>(o + x, ((float)r0 / 255.0f - m0) / d0);
      pp_store<TO>(o + plane + x, ((float)r1 / 255.0f - m1) / d1);
      pp_store<TO>(o + 2 * plane + x, ((float)r2 / 255.0f - m2) / d2);
    }
  }
}

hipError_t launch_preprocess(const uint8_t* src, const PpDesc* descs_dev, int B, int max_crop_h, int ks_max, int out_h, int out_w,
                             int32_t* tables, size_t table_stride, uint8_t* tmp, size_t tmp_stride, const float* mean,
                             const float* stdv, void* out, int out_dtype, uint8_t* out_u8, hipStream_t s) {
  hipLaunchKernelGGL(pp_coeffs_kernel<false>, dim3(B, 2), dim3(256), 0, s, descs_dev, tables, table_stride, ks_max, out_h, out_w);
  hipLaunchKernelGGL(pp_horizontal_kernel<false>, dim3(max_crop_h, B), dim3(256), 0, s, src, descs_dev, tables, table_stride, tmp,
                     tmp_stride, out_h, out_w);
#define MVLPT_PP_V(TO) hipLaunchKernelGGL(pp_vertical_kernel<TO>, dim3(out_h, B), dim3(256), 0, s, descs_dev, tables, table_stride, tmp, \
                                          tmp_stride, (TO*)out, out_u8, out_h, out_w, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2])
  if (out_dtype == DT_F32) MVLPT_PP_V(float);
  else if (out_dtype == DT_F16) MVLPT_PP_V(f16);
  else if (out_dtype == DT_BF16) MVLPT_PP_V(bf16);
  else return hipErrorInvalidValue;
#undef MVLPT_PP_V
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ augmentations
// Every function below restates integer / fp32 / double arithmetic of Pillow's C code (Convert.c, Blend.c): contraction off.
__device__ __forceinline__ int pp_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ int pp_clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Image.blend(degenerate d, image x, alpha): clipped only when alpha extrapolates
__device__ __forceinline__ int pp_blend(int d, int x, float alpha) {
#pragma clang fp contract(off)
  const float t = (float)d + alpha * (float)(x - d);
  if (alpha >= 0.0f && alpha <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ void pp_rgb2hsv(int r, int g, int b, int& H, int& S, int& V) {
#pragma clang fp contract(off)
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  V = mx; H = 0; S = 0;
  if (mx == mn) return;
  const float cr = (float)(mx - mn);
  const float s = cr / (float)mx;
  const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
  float h;
  if (r == mx) h = bc - gc;
  else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  double hd = (double)h / 6.0 + 1.0;                              // in [5/6, 11/6]
  hd = hd - floor(hd);                                           // fmod(hd, 1.0): exact for hd >= 0
  h = (float)hd;
  H = pp_clip255((int)((double)h * 255.0));
  S = pp_clip255((int)((double)s * 255.0));
}

__device__ __forceinline__ void pp_hsv2rgb(int H, int S, int V, int& r, int& g, int& b) {
#pragma clang fp contract(off)
  if (S == 0) { r = g = b = V; return; }
  const double hh = (double)(float)H * 6.0 / 255.0;
  const double fi = floor(hh);
  const float f = (float)(hh - fi);
  const float fs = (float)((double)S / 255.0);
  const double v = (double)V;
  const int p = pp_clip255((int)round(v * (1.0 - (double)fs)));
  const int q = pp_clip255((int)round(v * (1.0 - (double)(fs * f))));
  const int t = pp_clip255((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))));
  switch ((int)fi % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// colour operations ops[k0 .. k1) of one image on one pixel; `mean` is the contrast operation's degenerate level
__device__ __forceinline__ void pp_apply_ops(const PpAug& a, int k0, int k1, int mean, int& r, int& g, int& b) {
#pragma unroll
  for (int k = 0; k < PP_AUG_MAX_OPS; ++k) {
    if (k < k0 || k >= k1) continue;
    const int op = a.ops[k];
    if (op == PP_OP_BRIGHTNESS) {
      r = pp_blend(0, r, a.factor[0]); g = pp_blend(0, g, a.factor[0]); b = pp_blend(0, b, a.factor[0]);
    } else if (op == PP_OP_CONTRAST) {
      r = pp_blend(mean, r, a.factor[1]); g = pp_blend(mean, g, a.factor[1]); b = pp_blend(mean, b, a.factor[1]);
    } else if (op == PP_OP_SATURATION) {
      const int l = pp_luma(r, g, b);
      r = pp_blend(l, r, a.factor[2]); g = pp_blend(l, g, a.factor[2]); b = pp_blend(l, b, a.factor[2]);
    } else {                                                     // hue: the round trip runs (and changes pixels) for a shift of 0 too
      int H, S, V;
      pp_rgb2hsv(r, g, b, H, S, V);
      pp_hsv2rgb((H + a.hue_shift) & 255, S, V, r, g, b);
    }
  }
}

constexpr int PP_AUG_THREADS = 1024;

// win[b][y][x][c] (u8): the flipped window the vertical pass wrote; rewritten in place; out: [B,3,out_h,out_w] or null
template <typename TO>
__global__ __launch_bounds__(PP_AUG_THREADS) void pp_augment_kernel(const PpAug* __restrict__ augs, uint8_t* win, TO* __restrict__ out,
                                                                    int out_h, int out_w, float m0, float m1, float m2, float d0,
                                                                    float d1, float d2) {
#pragma clang fp contract(off)
  __shared__ unsigned long long red[PP_AUG_THREADS];
  const PpAug a = augs[blockIdx.x];
  const int n = out_h * out_w;
  uint8_t* w = win + (size_t)blockIdx.x * n * 3;
  int kc = -1;                                                   // position of the contrast operation in the chain
#pragma unroll
  for (int k = 0; k < PP_AUG_MAX_OPS; ++k)
    if (k < a.n_ops && a.ops[k] == PP_OP_CONTRAST) kc = k;
  int mean = 0;
  if (kc >= 0) {                                                 // uniform over the workgroup
    // first part of the chain in place, and the sum of L of what it leaves (integers: the order of the sum does not matter)
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < n; i += PP_AUG_THREADS) {
      uint8_t* p = w + (size_t)i * 3;
      int r = p[0], g = p[1], b = p[2];
      if (kc > 0) {
        pp_apply_ops(a, 0, kc, 0, r, g, b);
        p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
      }
      sum += (unsigned)pp_luma(r, g, b);
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int st = PP_AUG_THREADS / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
      __syncthreads();
    }
    mean = (int)((double)red[0] / (double)n + 0.5);               // int(ImageStat.Stat(L).mean[0] + 0.5)
  }
  // the rest of the chain on the pixels this thread itself left above, grayscale, holes, ToTensor / Normalize
  const size_t plane = (size_t)n;
  TO* o = out ? out + (size_t)blockIdx.x * 3 * plane : nullptr;
  for (int i = threadIdx.x; i < n; i += PP_AUG_THREADS) {
    uint8_t* p = w + (size_t)i * 3;
    int r = p[0], g = p[1], b = p[2];
    pp_apply_ops(a, kc < 0 ? 0 : kc, a.n_ops, mean, r, g, b);
    if (a.grayscale) r = g = b = pp_luma(r, g, b);
    if (a.n_holes > 0) {
      const int y = i / out_w, x = i - y * out_w;
#pragma unroll
      for (int k = 0; k < PP_AUG_MAX_HOLES; ++k)
        if (k < a.n_holes && y >= a.hole[k][0] && y - a.hole[k][0] < a.hole[k][2] && x >= a.hole[k][1] && x - a.hole[k][1] < a.hole[k][3])
          r = g = b = 0;
    }
    p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
    if (o) {
      pp_store<TO>(o + i, ((float)r / 255.0f - m0) / d0);
      pp_store<TO>(o + plane + i, ((float)g / 255.0f - m1) / d1);
      pp_store<TO>(o + 2 * plane + i, ((float)b / 255.0f - m2) / d2);
    }
  }
}

hipError_t launch_preprocess_aug(const uint8_t* src, const PpDesc* descs_dev, const PpAug* augs_dev, int B, int max_crop_h, int ks_max,
                                 int out_h, int out_w, int32_t* tables, size_t table_stride, uint8_t* tmp, size_t tmp_stride, uint8_t* win,
                                 const float* mean, const float* stdv, void* out, int out_dtype, hipStream_t s) {
  if (out && out_dtype != DT_F32 && out_dtype != DT_F16 && out_dtype != DT_BF16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pp_coeffs_kernel<true>, dim3(B, 2), dim3(256), 0, s, descs_dev, tables, table_stride, ks_max, out_h, out_w);
  hipLaunchKernelGGL(pp_horizontal_kernel<true>, dim3(max_crop_h, B), dim3(256), 0, s, src, descs_dev, tables, table_stride, tmp,
                     tmp_stride, out_h, out_w);
  // the vertical pass as it is, asked for its flipped 8-bit window alone (an empty tap range gives 0 there too)
  hipLaunchKernelGGL(pp_vertical_kernel<float>, dim3(out_h, B), dim3(256), 0, s, descs_dev, tables, table_stride, tmp, tmp_stride,
                     (float*)nullptr, win, out_h, out_w, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
#define MVLPT_PP_A(TO) hipLaunchKernelGGL(pp_augment_kernel<TO>, dim3(B), dim3(PP_AUG_THREADS), 0, s, augs_dev, win, (TO*)out, out_h, \
                                          out_w, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2])
  if (!out || out_dtype == DT_F32) MVLPT_PP_A(float);
  else if (out_dtype == DT_F16) MVLPT_PP_A(f16);
  else MVLPT_PP_A(bf16);
#undef MVLPT_PP_A
  return hipGetLastError();
}

}  // namespace mvlpt
