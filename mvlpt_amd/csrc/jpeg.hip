// Baseline JPEG decode on the device: compressed files in device memory -> the packed uint8 HWC RGB buffer that
// mvlpt_preprocess(_aug) reads, bit-identical to Pillow (libjpeg-turbo).  The arithmetic is jpeg_core.h, shared with the CPU build that
// proves its bounds under the sanitizers (tools/jpeg_core_check.cpp); this file is the mapping onto the machine.  Three kernels, no MFMA:
//   jpeg_entropy_kernel   one wave per image; its lanes take the image's restart segments (the whole scan when there is no DRI: one
//                         lane works, the stage is then sequential per image).  The image's four Huffman tables are expanded into
//                         lookahead tables in LDS once; the bit buffer lives in registers; coefficients go de-zigzagged, as int16,
//                         into a workspace the launcher zeroed, so only non-zero ones are written.  Status: OR over the wave, one
//                         ordinary store by lane 0
//   jpeg_idct_kernel      a lane owns a (block, column), then a (block, row); a wave owns 8 blocks, transposed through LDS; a row is
//                         one 8-byte store into the component plane (whole MCUs)
//   jpeg_colour_kernel    fancy chroma upsampling + YCbCr -> RGB, four pixels per lane: three dword stores where the address allows
#include "kernels.h"
#include "jpeg_core.h"

namespace mvlpt {

using namespace jpeg;

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ src, const ImgDesc* __restrict__ descs,
                                                          const Tables* __restrict__ tables, const Seg* __restrict__ segs,
                                                          int16_t* __restrict__ coefs, int32_t* __restrict__ status) {
  __shared__ HuffLut lut;
  const ImgDesc d = descs[blockIdx.x];
  const int lane = threadIdx.x;
  if (lane < 4) build_lut(tables[d.tables], lane, lut);
  __syncthreads();
  const int mcus = d.mcux * d.mcuy;
  int st = 0;
  for (int seg = lane; seg < d.n_segs; seg += 64) {
    const long long first = (long long)seg * d.restart;
    if (first >= mcus) break;
    const int count = mcus - (int)first < d.restart ? mcus - (int)first : d.restart;
    const Seg s = segs[d.seg_first + seg];
    st |= decode_segment(src + d.src_off, s.begin, s.end, d, lut, (int)first, count, coefs);
  }
  for (int off = 32; off > 0; off >>= 1) st |= __shfl_xor(st, off);
  if (lane == 0) status[d.index] = st;
}

constexpr int IDCT_THREADS = 256, IDCT_BLOCKS = IDCT_THREADS / 8;    // 32 coefficient blocks per workgroup

__device__ __forceinline__ void idct_body(const PlaneDesc& p, const int16_t* __restrict__ coefs, const uint8_t* __restrict__ q,
                                          uint8_t* __restrict__ planes, int32_t* ws) {
  const int t = threadIdx.x, slot = t >> 3, i = t & 7;
  const int b = blockIdx.x * IDCT_BLOCKS + slot;
  if (b < p.n_blocks) idct_column(coefs + (p.coef_off + b) * 64, q, i, ws + slot * 64);
  __syncthreads();
  if (b < p.n_blocks) {
    const int by = b / p.blocks_w, bx = b - by * p.blocks_w;
    union { uint8_t px[8]; uint2 v; } o;
    idct_row(ws + slot * 64, i, o.px);
    *(uint2*)(planes + p.plane_off + (int64_t)(by * 8 + i) * p.plane_w + bx * 8) = o.v;
  }
}
__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const PlaneDesc* __restrict__ descs, const Tables* __restrict__ tables,
                                                                 const int16_t* __restrict__ coefs, uint8_t* __restrict__ planes) {
  __shared__ int32_t ws[IDCT_BLOCKS * 64];
  const PlaneDesc p = descs[blockIdx.y];
  idct_body(p, coefs, tables[p.tables].q[p.tq], planes, ws);
}
__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_one_kernel(PlaneDesc p, const uint8_t* __restrict__ q,
                                                                     const int16_t* __restrict__ coefs, uint8_t* __restrict__ planes) {
  __shared__ int32_t ws[IDCT_BLOCKS * 64];
  idct_body(p, coefs, q, planes, ws);
}

__device__ __forceinline__ void colour_body(const ImgDesc& d, const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst) {
  const int gw = (d.width + 3) >> 2;                              // groups of four pixels per row
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)gw * d.height) return;
  const int y = (int)(g / gw), x0 = (int)(g - (long long)y * gw) * 4;
  const int n = d.width - x0 < 4 ? d.width - x0 : 4;
  union { uint8_t b[12]; uint32_t w[3]; } o;
  for (int k = 0; k < 4; ++k)
    if (k < n) pixel_rgb(d, planes, y, x0 + k, o.b + 3 * k);
  uint8_t* out = dst + d.dst_off + ((int64_t)y * d.width + x0) * 3;
  if (n == 4 && ((uintptr_t)out & 3) == 0) {
    uint32_t* w = (uint32_t*)out;
    w[0] = o.w[0]; w[1] = o.w[1]; w[2] = o.w[2];
  } else {
    for (int k = 0; k < 3 * n; ++k) out[k] = o.b[k];
  }
}
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const ImgDesc* __restrict__ descs, const uint8_t* __restrict__ planes,
                                                          uint8_t* __restrict__ dst) {
  const ImgDesc d = descs[blockIdx.y];
  colour_body(d, planes, dst);
}
__global__ __launch_bounds__(256) void jpeg_colour_one_kernel(ImgDesc d, const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst) {
  colour_body(d, planes, dst);
}

hipError_t launch_jpeg_entropy(const uint8_t* src, const ImgDesc* descs_dev, const Tables* tables_dev, const Seg* segs_dev, int n_images,
                               int16_t* coefs, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_images), dim3(64), 0, s, src, descs_dev, tables_dev, segs_dev, coefs, status);
  return hipGetLastError();
}
hipError_t launch_jpeg_idct(const PlaneDesc* planes_dev, int n_planes, int max_blocks, const Tables* tables_dev, const int16_t* coefs,
                            uint8_t* planes, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS, n_planes), dim3(IDCT_THREADS), 0, s, planes_dev,
                     tables_dev, coefs, planes);
  return hipGetLastError();
}
hipError_t launch_jpeg_idct_one(const PlaneDesc& p, const uint8_t* quant_dev, const int16_t* coefs, uint8_t* plane, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_idct_one_kernel, dim3((p.n_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), dim3(IDCT_THREADS), 0, s, p, quant_dev, coefs,
                     plane);
  return hipGetLastError();
}
static unsigned colour_grid(long long groups) { return (unsigned)((groups + 255) / 256); }
hipError_t launch_jpeg_colour(const ImgDesc* descs_dev, int n_images, long long max_groups, const uint8_t* planes, uint8_t* dst,
                              hipStream_t s) {
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(colour_grid(max_groups), n_images), dim3(256), 0, s, descs_dev, planes, dst);
  return hipGetLastError();
}
hipError_t launch_jpeg_colour_one(const ImgDesc& d, const uint8_t* planes, uint8_t* dst, hipStream_t s) {
  const long long groups = (long long)((d.width + 3) >> 2) * d.height;
  hipLaunchKernelGGL(jpeg_colour_one_kernel, dim3(colour_grid(groups)), dim3(256), 0, s, d, planes, dst);
  return hipGetLastError();
}

}  // namespace mvlpt
