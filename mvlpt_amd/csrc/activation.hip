// Stand-alone MLP activation of the towers whose checkpoint was trained with nn.GELU (Engine::act == ACT_GELU; DESIGN.md "Exact
// GELU"): the MLP-up GEMM stores its pre-activation u = acc + bias with a plain epilogue (EPI_STORE32: fp32, no 16-bit
// rounding in front of the activation), act_fwd_kernel turns it into the A operand of the down-projection, and in the backward act_bwd_kernel multiplies the fp32
// dA of EPI_STORE32 with act'(u).  Element-wise and HBM-bound: eight columns per lane (16-byte loads and stores of the 16-bit planes,
// two 16-byte loads of an fp32 row, 8 bytes of the mixed pair's byte plane), grid-stride over rows x column groups, any row count, no
// atomics, nothing read back.  The three output formats are written with the helpers the GEMM epilogues use (split16 / split_lo8x4,
// four columns at a time as there), so the QuickGELU instantiation, which the engine never takes, reproduces EPI_GELU / EPI_GELU_SPLIT
// bit for bit (tests/test_hip_activation.py).
//
// GELU(u) = u Phi(u) and GELU'(u) = Phi(u) + u phi(u), with Phi(u) = erfc(-u / sqrt 2) / 2: the erfc form.  1 + erf(u / sqrt 2)
// cancels on the negative tail (at u = -6 it keeps no correct bit in fp32), erfc stays accurate to a few ulp of ITSELF down to the
// smallest normal.  phi(u) = exp(-u^2 / 2) / sqrt(2 pi) through the library's expf: one rounding of the argument, as the host
// evaluation the tests' function term is measured on.
#include <algorithm>
#include "kernels.h"

namespace mvlpt {

template <int ACT> __device__ __forceinline__ float act_value(float u);
template <int ACT> __device__ __forceinline__ float act_slope(float u);
template <> __device__ __forceinline__ float act_value<ACT_QUICKGELU>(float u) { return quick_gelu(u); }
template <> __device__ __forceinline__ float act_slope<ACT_QUICKGELU>(float u) { return quick_gelu_grad(u); }
template <> __device__ __forceinline__ float act_value<ACT_GELU>(float u) { return u * (0.5f * erfcf(-u * 0.70710678118654752f)); }
template <> __device__ __forceinline__ float act_slope<ACT_GELU>(float u) {
  return 0.5f * erfcf(-u * 0.70710678118654752f) + u * (0.3989422804014327f * expf(-0.5f * (u * u)));
}

// eight values -> columns c .. c + 7 of output row `row` (pitch ldo 16-bit elements) in format fmt: ACT_FMT_SINGLE [N],
// ACT_FMT_PAIR [hi (N) | lo (N)], ACT_FMT_MIXED [hi (N) | lo8 (N bytes) | unused]
template <typename T>
__device__ __forceinline__ void act_store8(T* row, int fmt, int N, int c, const f32x4& v0, const f32x4& v1) {
  using v4 = typename Vec<T>::v4;
  using v8 = typename Vec<T>::v8;
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  v4 h0, h1;
  if (fmt == ACT_FMT_SINGLE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { h0[e] = from_f32<T>(v0[e]); h1[e] = from_f32<T>(v1[e]); }
  } else if (fmt == ACT_FMT_PAIR) {
    v4 l0, l1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      T h, l;
      split16<T>(v0[e], h, l); h0[e] = h; l0[e] = l;
      split16<T>(v1[e], h, l); h1[e] = h; l1[e] = l;
    }
    __builtin_nontemporal_store(v8{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]}, (v8*)(row + N + c));
  } else {
    u32x2 lo;
    lo[0] = split_lo8x4<T>(v0, h0);
    lo[1] = split_lo8x4<T>(v1, h1);
    __builtin_nontemporal_store(lo, (u32x2*)((char*)row + 2 * (size_t)N + c));
  }
  __builtin_nontemporal_store(v8{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]}, (v8*)(row + c));
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_fwd_kernel(ActArgs a) {
  using v8 = typename Vec<T>::v8;
  const int n8 = a.N >> 3;
  const size_t groups = (size_t)a.M * n8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / n8;
    const int c = (int)(i - m * n8) * 8;
    const float* row = (const float*)a.in + m * (size_t)a.ldi + c;
    const f32x4 u0 = __builtin_nontemporal_load((const f32x4*)row), u1 = __builtin_nontemporal_load((const f32x4*)(row + 4));
    f32x4 r0, r1;
#pragma unroll
    for (int e = 0; e < 4; ++e) { r0[e] = act_value<ACT>(u0[e]); r1[e] = act_value<ACT>(u1[e]); }
    act_store8<T>((T*)a.out + m * (size_t)a.ldo, a.fmt, a.N, c, r0, r1);
    if (a.u16) {      // the saved pre-activation, one 16-bit rounding (as out2 of EPI_GELU)
      v8 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) { w[e] = from_f32<T>(u0[e]); w[4 + e] = from_f32<T>(u1[e]); }
      __builtin_nontemporal_store(w, (v8*)((T*)a.u16 + m * (size_t)a.N + c));
    }
  }
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_bwd_kernel(ActArgs a) {
  using v8 = typename Vec<T>::v8;
  const int n8 = a.N >> 3;
  const size_t groups = (size_t)a.M * n8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / n8;
    const int c = (int)(i - m * n8) * 8;
    const float* row = (const float*)a.in + m * (size_t)a.ldi + c;
    const f32x4 d0 = __builtin_nontemporal_load((const f32x4*)row), d1 = __builtin_nontemporal_load((const f32x4*)(row + 4));
    const size_t um = a.u_rows.row((int)m);      // (ActArgs::u_rows; m < M)
    const v8 u = __builtin_nontemporal_load((const v8*)((const T*)a.u16 + um * (size_t)a.N + c));
    f32x4 r0, r1;
#pragma unroll
    for (int e = 0; e < 4; ++e) { r0[e] = d0[e] * act_slope<ACT>(to_f32<T>(u[e])); r1[e] = d1[e] * act_slope<ACT>(to_f32<T>(u[4 + e])); }
    act_store8<T>((T*)a.out + m * (size_t)a.ldo, a.fmt, a.N, c, r0, r1);
  }
}

// the pitches resolved, or what is wrong with the call (null: legal)
const char* act_check(int dtype, int act, bool bwd, ActArgs& a) {
  if (dtype != DT_F16 && dtype != DT_BF16) return "dtype must be fp16 or bf16";
  if (act != ACT_QUICKGELU && act != ACT_GELU) return "unknown activation";
  if (a.fmt != ACT_FMT_SINGLE && a.fmt != ACT_FMT_PAIR && a.fmt != ACT_FMT_MIXED) return "unknown output format";
  if (!a.in || !a.out || (bwd && !a.u16)) return "null pointer";
  if (a.M <= 0 || a.N <= 0 || (a.N % 8) != 0) return "M, N positive and N a multiple of 8";
  if (!row_map_ok(a.u_rows, a.M) || (a.u_rows.seq && !bwd)) return "u16 row map: backward only, whole sequences";
  const int wi = a.N, wo = a.fmt == ACT_FMT_SINGLE ? a.N : 2 * a.N;
  if (a.ldi == 0) a.ldi = wi;
  if (a.ldo == 0) a.ldo = wo;
  if (a.ldi < wi || (a.ldi % 8) != 0) return "input pitch below the row width or not a multiple of 8";
  if (a.ldo < wo || (a.ldo % 8) != 0) return "output pitch below the row width or not a multiple of 8";
  if ((((uintptr_t)a.in | (uintptr_t)a.out | (uintptr_t)a.u16) & 15) != 0) return "pointers must be 16-byte aligned";
  return nullptr;
}

template <typename T, int ACT>
static hipError_t act_launch_t(bool bwd, const ActArgs& a, hipStream_t s) {
  const size_t groups = (size_t)a.M * (a.N / 8);
  const int grid = (int)std::min<size_t>((groups + 255) / 256, 4096);
  if (bwd) hipLaunchKernelGGL((act_bwd_kernel<T, ACT>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((act_fwd_kernel<T, ACT>), dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}
static hipError_t act_launch(int dtype, int act, bool bwd, ActArgs a, hipStream_t s) {
  if (act_check(dtype, act, bwd, a)) return hipErrorInvalidValue;
  if (dtype == DT_F16) return act == ACT_GELU ? act_launch_t<f16, ACT_GELU>(bwd, a, s) : act_launch_t<f16, ACT_QUICKGELU>(bwd, a, s);
  return act == ACT_GELU ? act_launch_t<bf16, ACT_GELU>(bwd, a, s) : act_launch_t<bf16, ACT_QUICKGELU>(bwd, a, s);
}
hipError_t launch_act_fwd(int dtype, int act, const ActArgs& a, hipStream_t s) { return act_launch(dtype, act, false, a, s); }
hipError_t launch_act_bwd(int dtype, int act, const ActArgs& a, hipStream_t s) { return act_launch(dtype, act, true, a, s); }

}  // namespace mvlpt
