// vsf_jpeg_idct_reduced.h -- the arithmetic of libjpeg's reduced-size inverse DCTs (jidctred.c: jpeg_idct_4x4, jpeg_idct_2x2,
// jpeg_idct_1x1), stated ONCE: k_jpeg.hip's kernels and the CPU test program (tests/cpp/test_idct_reduced.cc) both include
// this file, so what the test pins against the system's libjpeg is what the device runs.
//
// These are what cv::imdecode(buf, IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) makes libjpeg run for the luminance component
// (scale_num / scale_denom = 1/2, 1/4, 1/8 -> DCT_scaled_size 4, 2, 1): a block of 64 coefficients gives 4 x 4, 2 x 2 or
// 1 pixel, no resize follows.  CONST_BITS = 13, PASS1_BITS = 2 as in jidctint.c; each form has constants and shifts of its own:
//
//   4 x 4   ignores row 4 and column 4 of the coefficients.   DC << 14; pass 1 DESCALE 12, pass 2 DESCALE 19
//   2 x 2   uses rows and columns 0, 1, 3, 5, 7 only.          DC << 15; pass 1 DESCALE 13, pass 2 DESCALE 20
//   1 x 1   the DC term alone.                                 DESCALE(dequantised DC, 3)
//
// (jidctred.c's shortcuts for all-zero AC terms give the same bits as the general path and are not restated.)
//
// INTEGER WIDTH: libjpeg computes in JLONG -- long, 64 bits on every LP64 build -- and cuts a pass's result to int.  An output
// of one pass is at most 77910 (4 x 4) or 85759 (2 x 2) times the largest |input|, so with every |input| below 2^14 -- any
// block an encoder writes -- 32-bit ring arithmetic gives the same bits; anything larger takes 64 bits, as the 8 x 8 code in
// k_jpeg.hip does.
#ifndef VSF_JPEG_IDCT_REDUCED_H_
#define VSF_JPEG_IDCT_REDUCED_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define VSF_IDCT_FN __host__ __device__ __forceinline__
#else
#define VSF_IDCT_FN inline
#endif

namespace vsf_idct {

constexpr int kRed4Shift1 = 12, kRed4Shift2 = 19;  // CONST_BITS - PASS1_BITS + 1;  CONST_BITS + PASS1_BITS + 3 + 1
constexpr int kRed2Shift1 = 13, kRed2Shift2 = 20;  // CONST_BITS - PASS1_BITS + 2;  CONST_BITS + PASS1_BITS + 3 + 2

VSF_IDCT_FN uint8_t range_limit(int32_t x) {  // sample_range_limit + CENTERJSAMPLE, index x & RANGE_MASK (1023)
  const int t = x & 1023;
  return (uint8_t)(t < 128 ? t + 128 : (t < 512 ? 255 : (t < 896 ? 0 : t - 896)));
}

// jpeg_idct_4x4, one 4-point pass on d[0..7] (d[4] is never read); r[k]: output k before DESCALE
template <class T>
VSF_IDCT_FN void red4_t(const T d[8], T r[4]) {
  const T F0211 = 1730, F0509 = 4176, F0601 = 4926, F0765 = 6270, F0899 = 7373, F1061 = 8697, F1451 = 11893, F1847 = 15137,
          F2172 = 17799, F2562 = 20995;
  const T tmp0e = d[0] * (T)16384;  // << (CONST_BITS + 1)
  const T tmp2e = d[2] * F1847 + d[6] * (-F0765);
  const T tmp10 = tmp0e + tmp2e, tmp12 = tmp0e - tmp2e;
  const T z1 = d[7], z2 = d[5], z3 = d[3], z4 = d[1];
  const T tmp0 = z1 * (-F0211) + z2 * F1451 + z3 * (-F2172) + z4 * F1061;
  const T tmp2 = z1 * (-F0509) + z2 * (-F0601) + z3 * F0899 + z4 * F2562;
  r[0] = tmp10 + tmp2;
  r[3] = tmp10 - tmp2;
  r[1] = tmp12 + tmp0;
  r[2] = tmp12 - tmp0;
}

// jpeg_idct_2x2, one 2-point pass on d[0..7] (only d[0], d[1], d[3], d[5], d[7] are read)
template <class T>
VSF_IDCT_FN void red2_t(const T d[8], T r[2]) {
  const T F0720 = 5906, F0850 = 6967, F1272 = 10426, F3624 = 29692;
  const T tmp10 = d[0] * (T)32768;  // << (CONST_BITS + 2)
  const T tmp0 = d[7] * (-F0720) + d[5] * F0850 + d[3] * (-F1272) + d[1] * F3624;
  r[0] = tmp10 + tmp0;
  r[1] = tmp10 - tmp0;
}

// One pass with its DESCALE(., shift), N = 4 or 2 outputs, as wide as libjpeg's JLONG where that matters (see the head).
template <int N>
VSF_IDCT_FN void red_descaled(const int32_t d[8], int32_t out[N], int shift) {
  static_assert(N == 4 || N == 2, "the 4 x 4 and the 2 x 2 form");
  uint32_t most = 0;
  for (int k = 0; k < 8; k++)
    if (N == 4 ? k != 4 : (k == 0 || (k & 1))) most |= (uint32_t)(d[k] ^ (d[k] >> 31));  // (ones' complement magnitudes)
  if (most < (1u << 14)) {
    uint32_t u[8], r[N];
    for (int k = 0; k < 8; k++) u[k] = (uint32_t)d[k];
    if constexpr (N == 4)
      red4_t<uint32_t>(u, r);
    else
      red2_t<uint32_t>(u, r);
    for (int k = 0; k < N; k++) out[k] = (int32_t)(r[k] + (1u << (shift - 1))) >> shift;
  } else {
    long long w[8], r[N];
    for (int k = 0; k < 8; k++) w[k] = d[k];
    if constexpr (N == 4)
      red4_t<long long>(w, r);
    else
      red2_t<long long>(w, r);
    for (int k = 0; k < N; k++) out[k] = (int32_t)((r[k] + (1ll << (shift - 1))) >> shift);
  }
}

// jpeg_idct_1x1: the dequantised DC term -> the block's one pixel
VSF_IDCT_FN uint8_t red1(int32_t dc) { return range_limit((int32_t)(((long long)dc + 4) >> 3)); }

// DEQUANTIZE as the 8 x 8 path of k_jpeg.hip states it
VSF_IDCT_FN int32_t dequant(int16_t c, uint16_t q) { return (int32_t)c * (int32_t)q; }

// Pass 1 of column `col` (0..7) of a block in natural order -> ws[r * 8 + col], r < 8 / D; columns the form ignores are
// the caller's to skip (used_column).  Pass 2 of workspace row `row` -> 8 / D pixels.
template <int D>
VSF_IDCT_FN bool used_column(int col) {
  return D == 2 ? col != 4 : (D == 4 ? (col == 0 || (col & 1)) : col == 0);
}
template <int D>
VSF_IDCT_FN void pass1_column(const int16_t* coef, const uint16_t* qt, int col, int32_t* ws) {
  static_assert(D == 2 || D == 4, "two passes: the 4 x 4 and the 2 x 2 form");
  int32_t d[8], r[8 / D];
  for (int k = 0; k < 8; k++) d[k] = dequant(coef[8 * k + col], qt[8 * k + col]);
  red_descaled<8 / D>(d, r, D == 2 ? kRed4Shift1 : kRed2Shift1);
  for (int k = 0; k < 8 / D; k++) ws[8 * k + col] = r[k];
}
template <int D>
VSF_IDCT_FN void pass2_row(const int32_t* ws_row, uint8_t* px) {
  static_assert(D == 2 || D == 4, "two passes: the 4 x 4 and the 2 x 2 form");
  int32_t d[8], r[8 / D];
  for (int k = 0; k < 8; k++) d[k] = ws_row[k];
  red_descaled<8 / D>(d, r, D == 2 ? kRed4Shift2 : kRed2Shift2);
  for (int k = 0; k < 8 / D; k++) px[k] = range_limit(r[k]);
}

// A whole block, D = 2, 4 or 8: coef and qt in natural order -> (8 / D) x (8 / D) pixels, row-major.
template <int D>
VSF_IDCT_FN void block_reduced(const int16_t coef[64], const uint16_t qt[64], uint8_t* out) {
  if (D == 8) {
    out[0] = red1(dequant(coef[0], qt[0]));
    return;
  }
  constexpr int DD = D == 8 ? 4 : D;  // (keeps the D = 8 instantiation of the lines below well-formed)
  int32_t ws[64];
  for (int k = 0; k < 64; k++) ws[k] = 0;
  for (int col = 0; col < 8; col++)
    if (used_column<DD>(col)) pass1_column<DD>(coef, qt, col, ws);
  for (int row = 0; row < 8 / DD; row++) pass2_row<DD>(ws + 8 * row, out + (8 / DD) * row);
}

}  // namespace vsf_idct
#endif  // VSF_JPEG_IDCT_REDUCED_H_
