// vsf_resize.h -- what the host and the pyramid kernels share of cv::resize (INTER_LINEAR, CV_8UC1): the ONE statement of
// the coefficient formula, and the plan by which a band narrower than a wave has its strips packed into full waves.
// Plain C++ (tests/cpp/test_pyramid_plan.cc compiles it with g++); compile without FMA contraction, as the library is.
#ifndef VSF_RESIZE_H_
#define VSF_RESIZE_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VSF_RESIZE_HD __host__ __device__
#else
#define VSF_RESIZE_HD
#endif

// Resize coefficients of one output column / row (xofs/ialpha resp. yofs/ibeta with the out-of-range taps already
// clamped, weights kept); evaluated in place by k_pyramid.hip, tabulated on the host (vsf_geometry.hip build_taps).
struct VsfTap {
  uint16_t i0, i1;  // source indices of the two taps
  int16_t c0, c1;   // 11-bit fixed-point weights
};

// saturate_cast<short>(f * 2048), f in [0, 1]: round to nearest even, no clamp can trigger
VSF_RESIZE_HD inline int resize_weight(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(f * 2048);
#else
  return (int)nearbyintf(f * 2048);
#endif
}

// imgproc/imgwarp.cpp, cv::resize: fx = (float)((dx + 0.5) * scale_x - 0.5), sx = cvFloor(fx), fx -= sx, then the
// clamps of the linear case and ialpha = saturate_cast<short>(. * INTER_RESIZE_COEF_SCALE).  scale = 1. / ((double)d / s)
VSF_RESIZE_HD inline VsfTap resize_xtap(int dx, double scale_x, int sw) {
  float fx = (float)((dx + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= sx;
  if (sx < 0) fx = 0, sx = 0;
  if (sx >= sw - 1) fx = 0, sx = sw - 1;  // (also the dx >= xmax single-tap case: weight 2048 on S[sx])
  VsfTap t;
  t.i0 = (uint16_t)sx;
  t.i1 = (uint16_t)(sx + 1 < sw - 1 ? sx + 1 : sw - 1);
  t.c0 = (int16_t)resize_weight(1.f - fx);
  t.c1 = (int16_t)resize_weight(fx);
  return t;
}
// ... and yofs / ibeta: the weights are kept, the two rows clamped into the image (VResizeLinear's row pointers).
// In whole registers first: the kernels hand a row's taps across lanes (v_readlane, ds_bpermute) as they come, and
// narrowing them to VsfTap's 16-bit fields on the way would cost a v_and each.
struct VsfTap32 {
  int32_t i0, i1, c0, c1;
};
VSF_RESIZE_HD inline VsfTap32 resize_ytap32(int dy, double scale_y, int sh) {
  float fy = (float)((dy + 0.5) * scale_y - 0.5);
  const int sy = (int)floorf(fy);
  fy -= sy;
  const int lo = sy > 0 ? sy : 0, hi = sy + 1 > 0 ? sy + 1 : 0;
  VsfTap32 t;
  t.i0 = lo < sh - 1 ? lo : sh - 1;
  t.i1 = hi < sh - 1 ? hi : sh - 1;
  t.c0 = resize_weight(1.f - fy);
  t.c1 = resize_weight(fy);
  return t;
}
VSF_RESIZE_HD inline VsfTap resize_ytap(int dy, double scale_y, int sh) {
  const VsfTap32 w = resize_ytap32(dy, scale_y, sh);
  return VsfTap{(uint16_t)w.i0, (uint16_t)w.i1, (int16_t)w.c0, (int16_t)w.c1};
}

// VResizeLinear<uchar, int, short, >> 22> on two HResizeLinear sums (S[i0] * a0 + S[i1] * a1) and the row's weights
VSF_RESIZE_HD inline uint32_t resize_vertical(int h0, int h1, int b0, int b1) {
  return (uint32_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// k_resize.hip (any source size into any destination size): a wave's 256 output columns [256 c, 256 c + 255] read the pixels
// [i0(first), i1(last)] of a source row -- the taps grow with the column -- through the aligned dwords that hold them, and a
// row may begin anywhere in its first dword.  The dwords the widest of a row's waves may need: what the launch sizes its
// per-lane fetch by.
inline int resize_span_dwords(int sw, int dw) {
  const double scale_x = 1. / ((double)dw / sw);
  int need = 0;
  for (int xb = 0; xb < dw; xb += 256) {
    const int xe = xb + 255 < dw - 1 ? xb + 255 : dw - 1;
    const int bytes = (int)resize_xtap(xe, scale_x, sw).i1 - (int)resize_xtap(xb, scale_x, sw).i0 + 1;
    const int dwords = (bytes + 3 + 3) >> 2;  // (+ 3: the first pixel in the last byte of its dword)
    if (dwords > need) need = dwords;
  }
  return need;
}

// Packing plan of a band narrower than a wave.  A strip (R output rows) of such a band is a span of `lanes` lanes, a lane
// being four output columns; the spans of the level's `nstrips` strips lie end to end and wave j takes lanes
// [64 j, 64 j + 64) of that sequence, whatever strips they belong to.  A lane evaluates the y taps of one (strip, row) of
// its wave -- lane e: row e % R of the wave's (e / R)-th strip -- so a wave may touch at most 64 / R strips: the span of a
// very narrow band is padded until that holds.
struct VsfPackPlan {
  int x0;          // the band's first output column
  int lanes;       // lanes per strip (padding included)
  int waves;       // 0: the band is not packed (a wave per strip)
  uint32_t magic;  // floor(2^32 / lanes) + 1: g / lanes == mulhi(g, magic), exact for g < 2^26
};
struct VsfPackedLane {
  int strip, lane;  // lane within the strip's span
};

// The layout alone, whether or not it pays.  dw: the level's width, x0 < dw
VSF_RESIZE_HD inline VsfPackPlan pack_layout(int R, int x0, int dw, int nstrips) {
  VsfPackPlan p;
  p.x0 = x0;
  p.lanes = 64;
  for (int n = (dw - x0 + 3) >> 2; n < 64; n++) {
    const int touched = (64 % n == 0) ? 64 / n : (63 + n - 1) / n + 1;  // strips a wave can reach (waves begin at 64 j)
    if (touched <= 64 / R) {
      p.lanes = n;
      break;
    }
  }
  p.waves = (nstrips * p.lanes + 63) >> 6;
  p.magic = 0xFFFFFFFFu / (uint32_t)p.lanes + 1u;
  return p;
}
// Packed (waves > 0) where the waves it saves outweigh what a packed wave adds (per-lane addresses, tap fetch, operand
// select): VALU instructions per wave of either form, read off the compiled resize_strip_kernel<R> (set-up + R rows;
// pyramid_image_kernel applies the R = 8 pair to its own packed loop).  Where the band is not packed only `waves` says
// so: x0, lanes and magic keep the layout's values and are not to be read.
VSF_RESIZE_HD inline VsfPackPlan pack_plan(int R, int x0, int dw, int nstrips) {
  VsfPackPlan p = pack_layout(R, x0, dw, nstrips);
  const long plain = R == 16 ? 763 : 467, packed = R == 16 ? 847 : 519;
  if (!((long)p.waves * packed < (long)nstrips * plain)) p.waves = 0;
  return p;
}
// g: the lane's place in the level's sequence of spans (wave * 64 + lane of the wave)
VSF_RESIZE_HD inline VsfPackedLane packed_lane(const VsfPackPlan& p, uint32_t g) {
  VsfPackedLane o;
  o.strip = (int)(uint32_t)(((uint64_t)g * p.magic) >> 32);
  o.lane = (int)g - o.strip * p.lanes;
  return o;
}

#endif  // VSF_RESIZE_H_
