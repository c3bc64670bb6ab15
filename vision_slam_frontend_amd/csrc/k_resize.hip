// k_resize.hip -- cv::resize(src, dst, Size(dw, dh)) of OpenCV 3.2 with its default INTER_LINEAR on CV_8UC1, for a batch of
// images of ANY size, base address and pitch (vsf_resize_gray_batch_dev; the ObserveImage queue's declared input sizes).
//
// The coefficients are vsf_resize.h's (resize_xtap, resize_ytap32: the statement the pyramid kernels use level to level);
// the passes are the integers of imgproc/imgwarp.cpp:
//   HResizeLinear<uchar, int, short, 2048>     H[x] = S[i0] * a0 + S[i1] * a1          (taps clamped, weights kept)
//   VResizeLinear<uchar, int, short, >> 22>    D[x] = (((b0 * (H0[x] >> 4)) >> 16) + ((b1 * (H1[x] >> 4)) >> 16) + 2) >> 2
// cv::resize's one special case, INTER_AREA at an exact 2 x reduction in both axes, is (a + b + c + d + 2) >> 2, which is
// what the integers above give with all four weights 1024 -- no second path.
//
// Memory-shaped: a wave owns 256 output columns (four per lane: one dword store) of kResizeRows output rows.  A lane's four
// x taps are evaluated once and kept.  The wave's columns read ONE contiguous span [i0(first column), i1(last column)] of
// each of an output row's two source rows: its lanes fetch the ALIGNED dwords that hold the span -- consecutive lanes,
// consecutive dwords, whatever the ratio -- into LDS, and every tap is a byte read from there.  A dword is fetched only if
// it holds at least one pixel of the span (an aligned dword never straddles a page: a row may end on the last byte of its
// allocation).  The next output row's dwords are requested before this row's arithmetic.  NLD, the dwords per lane and row,
// is chosen on the host from the ratio (resize_span_dwords): 3 covers ratios up to ~2.9, 10 up to ~9.9; beyond that
// (NLD = 0) every tap fetches the aligned dword that holds its pixel, no LDS.
#include "vsf_internal.h"
#include "vsf_resize.h"

namespace {

struct ResizeArgs {
  const uint8_t* src;
  size_t src_image_stride, src_pitch;
  uint8_t* dst;
  size_t dst_image_stride, dst_pitch;
  int sw, sh, dw, dh;
  double scale_x, scale_y;
};

constexpr int kResizeRows = 8;  // output rows per wave

__device__ __forceinline__ uint32_t vresize(int h0, int h1, int b0, int b1) { return resize_vertical(h0, h1, b0, b1); }

// the pixel at `addr` out of the aligned dword that holds it
__device__ __forceinline__ int pixel_at(uintptr_t addr) {
  const uint32_t d = *reinterpret_cast<const uint32_t*>(addr & ~(uintptr_t)3);
  return (int)((d >> (8u * (uint32_t)(addr & 3u))) & 0xFFu);
}

template <int NLD>
__global__ __launch_bounds__(64) void resize_gray_kernel(ResizeArgs a) {
  constexpr int kLds = NLD > 0 ? 64 * NLD : 1;
  __shared__ uint32_t lds[2][kLds];
  const int lane = threadIdx.x;
  const int xb = blockIdx.x * 256, x4 = xb + 4 * lane;
  const int y0 = blockIdx.y * kResizeRows, y1 = min(y0 + kResizeRows, a.dh);
  const uint8_t* img = a.src + (size_t)blockIdx.z * a.src_image_stride;
  uint8_t* out = a.dst + (size_t)blockIdx.z * a.dst_image_stride;
  // the lane's x taps, once (a lane past the last column repeats it and stores nothing)
  VsfTap t[4];
#pragma unroll
  for (int j = 0; j < 4; j++) t[j] = resize_xtap(min(x4 + j, a.dw - 1), a.scale_x, a.sw);
  // the wave's span of a source row (the taps grow with the column): pixels [s_lo, s_hi]
  const int s_lo = resize_xtap(xb, a.scale_x, a.sw).i0, s_hi = resize_xtap(min(xb + 255, a.dw - 1), a.scale_x, a.sw).i1;

  struct Rows {
    uint32_t d[2][NLD > 0 ? NLD : 1];
    uint32_t skew[2];  // where pixel s_lo lies in the first dword
    int b0, b1;
  };
  auto fetch = [&](int y) -> Rows {
    Rows r;
    const VsfTap32 ty = resize_ytap32(y, a.scale_y, a.sh);
    r.b0 = ty.c0;
    r.b1 = ty.c1;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uintptr_t first = (uintptr_t)img + (size_t)(k ? ty.i1 : ty.i0) * a.src_pitch + (uintptr_t)s_lo;
      const uintptr_t last = first + (uintptr_t)(s_hi - s_lo);  // the span's last pixel
      r.skew[k] = (uint32_t)(first & 3u);
      const uintptr_t base = first - r.skew[k];
#pragma unroll
      for (int m = 0; m < NLD; m++) {
        const uintptr_t p = base + 4u * (uintptr_t)(lane + 64 * m);
        r.d[k][m] = p <= last ? *reinterpret_cast<const uint32_t*>(p) : 0u;
      }
    }
    return r;
  };

  auto emit = [&](int y, uint32_t g) {
    if (x4 >= a.dw) return;
    uint8_t* p = out + (size_t)y * a.dst_pitch + x4;
    if (x4 + 3 < a.dw && ((uintptr_t)p & 3u) == 0) {
      *reinterpret_cast<uint32_t*>(p) = g;
    } else {  // the row's partial last dword, or a row that does not begin on a dword: nothing past column dw - 1 is written
      for (int j = 0; j < 4 && x4 + j < a.dw; j++) p[j] = (uint8_t)(g >> (8 * j));
    }
  };

  if (NLD == 0) {
    for (int y = y0; y < y1; y++) {
      const VsfTap32 ty = resize_ytap32(y, a.scale_y, a.sh);
      const uintptr_t r0 = (uintptr_t)img + (size_t)ty.i0 * a.src_pitch, r1 = (uintptr_t)img + (size_t)ty.i1 * a.src_pitch;
      uint32_t g = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int h0 = pixel_at(r0 + t[j].i0) * t[j].c0 + pixel_at(r0 + t[j].i1) * t[j].c1;
        const int h1 = pixel_at(r1 + t[j].i0) * t[j].c0 + pixel_at(r1 + t[j].i1) * t[j].c1;
        g |= vresize(h0, h1, ty.c0, ty.c1) << (8 * j);
      }
      emit(y, g);
    }
    return;
  }

  Rows cur = fetch(y0);
  for (int y = y0; y < y1; y++) {  // (wave-uniform: every lane of the workgroup meets every barrier)
    Rows nxt = cur;
    if (y + 1 < y1) nxt = fetch(y + 1);
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int m = 0; m < NLD; m++) lds[k][lane + 64 * m] = cur.d[k][m];
    __syncthreads();
    // pixel i of row k: byte i - s_lo + skew[k] of lds[k]  (<= s_hi - s_lo + 3 < 4 * 64 * NLD: resize_span_dwords)
    const uint8_t* l0 = reinterpret_cast<const uint8_t*>(lds[0]) + cur.skew[0];
    const uint8_t* l1 = reinterpret_cast<const uint8_t*>(lds[1]) + cur.skew[1];
    uint32_t g = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i0 = (int)t[j].i0 - s_lo, i1 = (int)t[j].i1 - s_lo;
      const int h0 = l0[i0] * t[j].c0 + l0[i1] * t[j].c1;
      const int h1 = l1[i0] * t[j].c0 + l1[i1] * t[j].c1;
      g |= vresize(h0, h1, cur.b0, cur.b1) << (8 * j);
    }
    emit(y, g);
    __syncthreads();
    cur = nxt;
  }
}

}  // namespace

// (the caller has checked: sizes in 1 .. 32767, pitches >= widths, n >= 1)
void vsf_launch_resize_gray(const uint8_t* d_src, int n, int sw, int sh, size_t src_image_stride, size_t src_pitch, uint8_t* d_dst,
                            int dw, int dh, size_t dst_image_stride, size_t dst_pitch, hipStream_t s) {
  if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return;
  const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
  const int need = resize_span_dwords(sw, dw);
  for (int i0 = 0; i0 < n; i0 += 65535) {  // (the grid's z extent)
    const int ni = n - i0 < 65535 ? n - i0 : 65535;
    const ResizeArgs a{d_src + (size_t)i0 * src_image_stride, src_image_stride, src_pitch, d_dst + (size_t)i0 * dst_image_stride,
                       dst_image_stride, dst_pitch, sw, sh, dw, dh, scale_x, scale_y};
    const dim3 grid((dw + 255) / 256, (dh + kResizeRows - 1) / kResizeRows, ni);
    if (need <= 64 * 3)
      hipLaunchKernelGGL(resize_gray_kernel<3>, grid, dim3(64), 0, s, a);
    else if (need <= 64 * 10)
      hipLaunchKernelGGL(resize_gray_kernel<10>, grid, dim3(64), 0, s, a);
    else
      hipLaunchKernelGGL(resize_gray_kernel<0>, grid, dim3(64), 0, s, a);
  }
}
