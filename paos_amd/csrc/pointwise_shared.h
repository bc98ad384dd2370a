// pointwise_shared.h -- the few definitions of the pointwise kernels (pointwise.h, launched by paos_hip.hip alone) that
// kernels of another unit share with them (wavefront_pass.h): the workgroup size and how a reduction kernel ends, the
// header of a Zernike parameter block, the chunk shape of the Gram sums.
#pragma once
#include <hip/hip_runtime.h>

namespace paos {

constexpr int kPwThreads = 256;

// ---- a sum over the workgroup in a fixed order: shuffle tree per wave, then the waves in order ----
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sh[w];
  return s;  // valid in thread 0
}

// how a reduction kernel ends: this workgroup's sum goes to partial[item][workgroup] (blockIdx.y = item)
__device__ __forceinline__ void store_block_sum(double acc, double* sh, double* partial) {
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ---- Zernike parameter block, per item: [enable, dx, dy, radius, origin_is_y, cos_off, sin_off, inv_wl, then the
// coefficient planes] (pointwise.h, "Zernike phase") ----
enum : int { ZP_ENABLE = 0, ZP_DX, ZP_DY, ZP_RADIUS, ZP_ORIGIN_Y, ZP_COS_OFF, ZP_SIN_OFF, ZP_INV_WL, ZP_HEAD };

// ---- Gram sums (zernike_gram_kernel, wf_gram_kernel): 128-pixel chunks, 256 threads, LDS rows of 129 doubles, at most 64 rows ----
constexpr int kGramMaxK = 64, kGramPix = 128, kGramThreads = 256, kGramRow = kGramPix + 1;

}  // namespace paos
