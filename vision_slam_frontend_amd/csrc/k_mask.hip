// k_mask.hip -- the mask pyramid of cv::ORB::detectAndCompute(image, mask, ...) (include/vsf.h "Detection masks"; restated
// from memory, OpenCV 3.2 orb.cpp): level 0 is the caller's mask, level l >= 1 is
//   resize(level l - 1, size_l, INTER_LINEAR), then threshold(., 254, 0, THRESH_TOZERO)
// of the already thresholded level l - 1, so a pixel of a level >= 1 is 255 exactly where the fixed-point interpolation gives
// 255 and 0 elsewhere.  The taps are vsf_resize.h's (resize_xtap, resize_ytap32, resize_vertical: the statement the image
// pyramid uses level to level), the scales the geometry's (VsfLevel::rscale_x / _y).
//
// What a slot keeps is what k_fast.hip's predicate reads: one byte a pixel, 0xFF where a corner may sit and 0x00 elsewhere,
// every level at its offset and pitch in the layout of one image's pyramid block.  Level 0 is kept as "non-zero" (any
// non-zero value passes KeyPointsFilter::runByPixelsMask), but level 1 is interpolated from the caller's VALUES: the build
// reads them from the caller's mask, and every later level from the kept level below it (0 / 255 there: values and kept
// bytes agree).  Built once per vsf_mask_set: one launch a level, a lane makes four pixels of a row (one dword store).
#include <cstring>

#include "vsf_internal.h"

namespace {

// the kept level 0: non-zero -> 0xFF
__global__ __launch_bounds__(256) void mask_level0_kernel(const uint8_t* __restrict__ src, size_t src_pitch, int w, int h,
                                                          uint8_t* __restrict__ dst, int dst_pitch) {
  const int x4 = 4 * (blockIdx.x * 256 + threadIdx.x), y = blockIdx.y;
  if (x4 >= w || y >= h) return;
  const uint8_t* row = src + (size_t)y * src_pitch;
  uint32_t g = 0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (x4 + j < w && row[x4 + j] != 0) g |= 0xFFu << (8 * j);
  *reinterpret_cast<uint32_t*>(dst + (size_t)y * dst_pitch + x4) = g;  // (x4 + 3 < dst_pitch: a multiple of 64 >= w)
}

// level l from the values of level l - 1
__global__ __launch_bounds__(256) void mask_level_kernel(const uint8_t* __restrict__ src, size_t src_pitch, int sw, int sh,
                                                         uint8_t* __restrict__ dst, int dst_pitch, int dw, int dh, double scale_x,
                                                         double scale_y) {
  const int x4 = 4 * (blockIdx.x * 256 + threadIdx.x), y = blockIdx.y;
  if (x4 >= dw || y >= dh) return;
  const VsfTap32 ty = resize_ytap32(y, scale_y, sh);
  const uint8_t* r0 = src + (size_t)ty.i0 * src_pitch;
  const uint8_t* r1 = src + (size_t)ty.i1 * src_pitch;
  uint32_t g = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (x4 + j >= dw) break;
    const VsfTap t = resize_xtap(x4 + j, scale_x, sw);
    const int h0 = r0[t.i0] * t.c0 + r0[t.i1] * t.c1, h1 = r1[t.i0] * t.c0 + r1[t.i1] * t.c1;
    if (resize_vertical(h0, h1, ty.c0, ty.c1) > 254u) g |= 0xFFu << (8 * j);  // THRESH_TOZERO at 254
  }
  *reinterpret_cast<uint32_t*>(dst + (size_t)y * dst_pitch + x4) = g;
}

double level_scale(const uint32_t bits[2]) {
  double v;
  std::memcpy(&v, bits, 8);
  return v;
}

}  // namespace

void vsf_launch_mask_pyramid(const uint8_t* d_mask, size_t mask_pitch, const VsfLevel* h_levels, int nlevels, uint32_t block_bytes,
                             uint8_t* d_block, hipStream_t s) {
  vsf_note(hipMemsetAsync(d_block, 0, block_bytes, s));  // (the rows' padding and the gaps between levels stay zero)
  const VsfLevel& L0 = h_levels[0];
  hipLaunchKernelGGL(mask_level0_kernel, dim3((L0.w + 1023) / 1024, L0.h), dim3(256), 0, s, d_mask, mask_pitch, L0.w, L0.h,
                     d_block + L0.offset, L0.pitch);
  for (int l = 1; l < nlevels; l++) {
    const VsfLevel& P = h_levels[l - 1];
    const VsfLevel& L = h_levels[l];
    const uint8_t* src = l == 1 ? d_mask : d_block + P.offset;
    const size_t src_pitch = l == 1 ? mask_pitch : (size_t)P.pitch;
    hipLaunchKernelGGL(mask_level_kernel, dim3((L.w + 1023) / 1024, L.h), dim3(256), 0, s, src, src_pitch, P.w, P.h,
                       d_block + L.offset, L.pitch, L.w, L.h, level_scale(L.rscale_x), level_scale(L.rscale_y));
  }
}
