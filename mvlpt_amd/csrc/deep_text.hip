// Deep text prompts (per-layer language contexts): the text-side twins of the image tower's deep-prompt glue (glue.hip
// overwrite_rows_kernel / reduce_prompt_rows_kernel).  The context rows of a text sequence sit where CLASS_TOKEN_POSITION put them,
// so both kernels address them through the ctx_pos table (launch_build_ctx_pos) instead of a fixed row offset.  HBM-bound, coalesced
// along the feature dimension; no scratch, no atomics.  An entry of ctx_pos outside [0, L) is skipped, never dereferenced.
#include "kernels.h"

namespace mvlpt {

// x[c, ctx_pos[c, j], :] = rows[j, :]      (the hidden states are replaced: no positional embedding is added)
__global__ void overwrite_ctx_rows_kernel(const float* __restrict__ rows, const int32_t* __restrict__ ctx_pos, float* __restrict__ x,
                                          int C, int L, int d, int n_ctx) {
  const int d4 = d / 4;
  const size_t total = (size_t)C * n_ctx * d4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % d4), j = (int)((i / d4) % n_ctx);
    const size_t c = i / ((size_t)d4 * n_ctx);
    const int p = ctx_pos[c * n_ctx + j];
    if ((unsigned)p >= (unsigned)L) continue;
    *(f32x4*)(x + (c * L + p) * d + c4 * 4) = *(const f32x4*)(rows + (size_t)j * d + c4 * 4);
  }
}
hipError_t launch_overwrite_ctx_rows(const float* rows, const int32_t* ctx_pos, float* x, int C, int L, int d, int n_ctx, hipStream_t s) {
  if (n_ctx <= 0 || C <= 0) return hipSuccess;
  if (d <= 0 || d % 4) return hipErrorInvalidValue;
  const size_t total = (size_t)C * n_ctx * (d / 4);
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(overwrite_ctx_rows_kernel, dim3(grid), dim3(256), 0, s, rows, ctx_pos, x, C, L, d, n_ctx);
  return hipGetLastError();
}

// out[j, :] = inv_scale * sum_c dx32[c, ctx_pos[c, j], :], then those rows stop carrying a gradient: the overwrite in the forward cut
// the path to the block in front, so they are zeroed in the fp32 stream and in its 16-bit copy (split16 0: [T, d], 1: hi|lo pair
// [T, 2d], 2: mixed pair at the pair's pitch, hi plane + d residual bytes; the unused tail of a mixed row is left alone).
// The reduction is gather_ctx_row's (glue.hip): 16 waves, wave w sums c = w, w + 16, ..., lane = one float4 column, the 16 partials
// added in a fixed order through LDS.  The lane that read a column slice of a row is the one that zeroes it.
template <typename T>
__global__ __launch_bounds__(1024) void gather_zero_ctx_grad_kernel(float* __restrict__ dx32, T* __restrict__ dx16, int split16,
                                                                    const int32_t* __restrict__ ctx_pos, int C, int L, int d, int n_ctx,
                                                                    float* __restrict__ out, const float* scale_dev) {
  __shared__ f32x4 part[16][64];
  const int j = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + lane) * 4;
  const bool ok = c < d;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
#pragma unroll 4
    for (int k = wave; k < C; k += 16) {
      const int p = ctx_pos[(size_t)k * n_ctx + j];
      if ((unsigned)p >= (unsigned)L) continue;
      const size_t row = (size_t)k * L + p;
      float* g = dx32 + row * d + c;
      acc += *(const f32x4*)g;
      *(f32x4*)g = f32x4{0.f, 0.f, 0.f, 0.f};
      if (dx16) {
        typename Vec<T>::v4 z;
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = (T)0.f;
        if (split16 == 2) {                  // [hi (d x 16 bit) | lo8 (d bytes) | unused]: the 4 residual bytes of columns c .. c+3
          T* r16 = dx16 + row * 2 * d;
          *(typename Vec<T>::v4*)(r16 + c) = z;
          *(uint32_t*)((char*)r16 + 2 * (size_t)d + c) = 0u;
        } else if (split16) {
          T* r16 = dx16 + row * 2 * d;
          *(typename Vec<T>::v4*)(r16 + c) = z;
          *(typename Vec<T>::v4*)(r16 + d + c) = z;
        } else {
          *(typename Vec<T>::v4*)(dx16 + row * d + c) = z;
        }
      }
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && ok) {
    f32x4 t = part[0][lane];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += part[w][lane];
    const float inv = scale_dev ? scale_dev[1] : 1.0f;
    *(f32x4*)(out + (size_t)j * d + c) = t * inv;
  }
}
hipError_t launch_gather_zero_ctx_grad(int dtype, float* dx32, void* dx16, int split16, const int32_t* ctx_pos, int C, int L, int d,
                                       int n_ctx, float* out, const float* scale_dev, hipStream_t s) {
  if (n_ctx <= 0) return hipSuccess;
  if (C <= 0 || d <= 0 || d % 4 || split16 < 0 || split16 > 2 || n_ctx > 65535) return hipErrorInvalidValue;
  dim3 grid((d + 255) / 256, n_ctx), block(1024);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gather_zero_ctx_grad_kernel<f16>, grid, block, 0, s, dx32, (f16*)dx16, split16, ctx_pos, C, L, d, n_ctx, out, scale_dev);
  else if (dtype == DT_BF16)
    hipLaunchKernelGGL(gather_zero_ctx_grad_kernel<bf16>, grid, block, 0, s, dx32, (bf16*)dx16, split16, ctx_pos, C, L, d, n_ctx, out, scale_dev);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace mvlpt
