// Fused optimizer step over the flat prompt buffers: ONE launch updates param / state1 / state2 in place with torch.optim's
// single-tensor formulas (SGD with momentum / dampening / nesterov, Adam with L2 decay, AdamW) in fp32.
//
// The flat buffers are the parameter tensors back to back (distributed.FlatParameters / FlatGradients); a segment table says which
// element belongs to which tensor, whether that tensor takes part in this step (`.grad is None` -> untouched, bit for bit) and how
// many steps it has taken (launch - missed).  Pure streaming: every thread owns ONE 16-byte quad of each buffer, so a grid of
// ceil(n / 1024) blocks covers the buffer evenly (554 blocks for UPT-4's 566 400 elements: no tail wave).  The segment table lives in
// LDS (one cooperative load per block, with the per-segment constants: Adam's bias corrections are computed ONCE per segment in
// double, never per element); a thread finds its quad's segment with a binary search over LDS, <= 10 probes, no dependent global
// load.  A quad that lies inside one segment and inside [0, n) moves as dwordx4; a quad that straddles a segment boundary, or the
// last partial one, goes element by element with a search of its own per element.
#include "../../include/mvlpt_hip.h"
#include "kernels.h"

namespace mvlpt {

namespace {

constexpr int OPT_BLOCK = 256;                 // threads per block; 4 elements each
constexpr int OPT_MAX_SEGS = MVLPT_OPTIM_MAX_SEGS;

struct OptimConsts {          // hyper-parameters as the kernel uses them (host: launch_optim_step)
  int kind, nesterov, has_buf;
  float lr, wd, momentum, one_minus_damp;      // SGD
  float beta2, eps, one_minus_beta1, one_minus_beta2, decay_mul;   // Adam / AdamW (decay_mul = 1 - lr * wd)
  double lr_d, beta1_d, beta2_d;                                   // for the per-segment bias corrections
  long long launch;
};

// per-segment constants, by segment kind:  SGD: a = 1 on the segment's first step (buf = d), else 0
//                                          Adam: a = lr / (1 - beta1^t), b = sqrt(1 - beta2^t)
struct SegLds {
  long long begin[OPT_MAX_SEGS];
  long long end[OPT_MAX_SEGS];
  float a[OPT_MAX_SEGS];
  float b[OPT_MAX_SEGS];
  int active[OPT_MAX_SEGS];
};

__device__ __forceinline__ double ipow(double x, long long t) {      // x^t by squaring, t >= 0 (<= 63 multiplications)
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= x;
    x *= x;
    t >>= 1;
  }
  return r;
}

// largest s with begin[s] <= i, or -1 (the table is sorted by begin)
__device__ __forceinline__ int find_seg(const SegLds& T, int n_segs, long long i) {
  int lo = -1, hi = n_segs;      // begin[lo] <= i < begin[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (T.begin[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void sgd_elem(const OptimConsts& c, float first, float& p, float g, float& buf) {
  const float d = c.wd != 0.f ? g + c.wd * p : g;
  float upd = d;
  if (c.has_buf) {
    buf = first != 0.f ? d : c.momentum * buf + c.one_minus_damp * d;
    upd = c.nesterov ? d + c.momentum * buf : buf;
  }
  p -= c.lr * upd;
}

__device__ __forceinline__ void adam_elem(const OptimConsts& c, float step_size, float bc2_sqrt, float& p, float g, float& m, float& v) {
  if (c.kind == 2) p *= c.decay_mul;                       // AdamW: decoupled decay
  else if (c.wd != 0.f) g += c.wd * p;                     // Adam: L2 decay
  m += c.one_minus_beta1 * (g - m);                        // exp_avg.lerp_(grad, 1 - beta1)
  v = c.beta2 * v + c.one_minus_beta2 * (g * g);           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(v) / bc2_sqrt + c.eps;
  p -= step_size * (m / denom);                            // param.addcdiv_(exp_avg, denom, value = -step_size)
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_step_kernel(OptimConsts c, float* __restrict__ param, const float* __restrict__ grad,
                                                               float* __restrict__ s1, float* __restrict__ s2, long long n,
                                                               const MvlptOptimSeg* __restrict__ segs, int n_segs,
                                                               const float* __restrict__ loss, int* __restrict__ skipped) {
  if (loss) {                                              // loss guard: a non-finite loss leaves every buffer as it is
    const float l = *loss;
    if (!(fabsf(l) <= 3.402823466e38f)) {                  // NaN or +-inf
      if (skipped && blockIdx.x == 0 && threadIdx.x == 0) *skipped += 1;      // once per launch
      return;
    }
  }
  __shared__ SegLds T;
  for (int s = threadIdx.x; s < n_segs; s += OPT_BLOCK) {
    const MvlptOptimSeg sg = segs[s];
    const long long t = c.launch - (long long)sg.missed;   // this segment's own step count (1 on its first active step)
    T.begin[s] = sg.begin;
    T.end[s] = sg.end;
    T.active[s] = sg.active && t >= 1;
    if (c.kind == 0) {
      T.a[s] = t <= 1 ? 1.f : 0.f;
      T.b[s] = 0.f;
    } else {
      const long long tt = t >= 1 ? t : 1;
      T.a[s] = (float)(c.lr_d / (1.0 - ipow(c.beta1_d, tt)));
      T.b[s] = (float)sqrt(1.0 - ipow(c.beta2_d, tt));
    }
  }
  __syncthreads();

  const long long i0 = ((long long)blockIdx.x * OPT_BLOCK + threadIdx.x) * 4;
  if (i0 >= n) return;
  const int s0 = find_seg(T, n_segs, i0);
  if (i0 + 4 <= n && s0 >= 0 && i0 + 4 <= T.end[s0]) {     // the whole quad inside one segment: 16-byte loads and stores
    if (!T.active[s0]) return;
    const float a = T.a[s0], b = T.b[s0];
    f32x4 p = *reinterpret_cast<const f32x4*>(param + i0);
    const f32x4 g = *reinterpret_cast<const f32x4*>(grad + i0);
    if (c.kind == 0) {
      f32x4 buf = {0.f, 0.f, 0.f, 0.f};
      if (c.has_buf && a == 0.f) buf = *reinterpret_cast<const f32x4*>(s1 + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { float pe = p[e], be = buf[e]; sgd_elem(c, a, pe, g[e], be); p[e] = pe; buf[e] = be; }
      if (c.has_buf) *reinterpret_cast<f32x4*>(s1 + i0) = buf;
    } else {
      f32x4 m = *reinterpret_cast<const f32x4*>(s1 + i0), v = *reinterpret_cast<const f32x4*>(s2 + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) { float pe = p[e], me = m[e], ve = v[e]; adam_elem(c, a, b, pe, g[e], me, ve); p[e] = pe; m[e] = me; v[e] = ve; }
      *reinterpret_cast<f32x4*>(s1 + i0) = m;
      *reinterpret_cast<f32x4*>(s2 + i0) = v;
    }
    *reinterpret_cast<f32x4*>(param + i0) = p;
    return;
  }
  // a segment boundary (or the end of the buffer) inside the quad: element by element
  for (int e = 0; e < 4; ++e) {
    const long long i = i0 + e;
    if (i >= n) break;
    const int s = find_seg(T, n_segs, i);
    if (s < 0 || i >= T.end[s] || !T.active[s]) continue;
    const float a = T.a[s], b = T.b[s];
    float p = param[i];
    const float g = grad[i];
    if (c.kind == 0) {
      float buf = (c.has_buf && a == 0.f) ? s1[i] : 0.f;
      sgd_elem(c, a, p, g, buf);
      if (c.has_buf) s1[i] = buf;
    } else {
      float m = s1[i], v = s2[i];
      adam_elem(c, a, b, p, g, m, v);
      s1[i] = m;
      s2[i] = v;
    }
    param[i] = p;
  }
}

}  // namespace

hipError_t launch_optim_step(const MvlptOptimHyper& h, float* param, const float* grad, float* state1, float* state2, int64_t n,
                             const MvlptOptimSeg* segs_dev, int n_segs, const float* loss_dev, int32_t* skipped_dev, hipStream_t s) {
  OptimConsts c{};
  c.kind = h.kind;
  c.nesterov = h.nesterov != 0;
  c.has_buf = h.kind == 0 && h.momentum != 0.0;
  // torch.optim holds the hyper-parameters as doubles and hands them, and what it derives from them, to fp32 kernels as scalars:
  // every constant below is formed in double and rounded once
  c.lr = (float)h.lr;
  c.wd = (float)h.weight_decay;
  c.momentum = (float)h.momentum;
  c.one_minus_damp = (float)(1.0 - h.dampening);
  c.beta2 = (float)h.beta2;
  c.eps = (float)h.eps;
  c.one_minus_beta1 = (float)(1.0 - h.beta1);
  c.one_minus_beta2 = (float)(1.0 - h.beta2);
  c.decay_mul = (float)(1.0 - h.lr * h.weight_decay);
  c.lr_d = h.lr;
  c.beta1_d = h.beta1;
  c.beta2_d = h.beta2;
  c.launch = h.launch;
  const int64_t quads = (n + 3) / 4, blocks = (quads + OPT_BLOCK - 1) / OPT_BLOCK;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(optim_step_kernel, dim3((unsigned)blocks), dim3(OPT_BLOCK), 0, s, c, param, grad, state1, state2, (long long)n,
                     segs_dev, n_segs, loss_dev, (int*)skipped_dev);
  return hipGetLastError();
}

}  // namespace mvlpt
