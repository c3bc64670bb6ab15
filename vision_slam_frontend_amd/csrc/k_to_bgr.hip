// k_to_bgr.hip -- the colour image of a raw frame: what src/test/bag_extract.cc:75-88 does between cv::imdecode and cv::imwrite,
//   cv::split(image) -> channel 0;  cv::cvtColor(channel 0, image, COLOR_BayerBG2BGR)
// and what cv_bridge makes of the packed formats for a "bgr8" request.  k_ingest.hip holds the same demosaic fused with BGR2GRAY
// (its header states the arithmetic of imgproc/demosaicing.cpp Bayer2RGB_<uchar>: cross, diag, hor, ver; the one-pixel frame copies
// its inner neighbour, columns first, then rows; a side below 3 gives zeros); here the three sums are stored, blue first.
// 1 byte read + 3 written per pixel.  Reads are the gray kernel's: a lane owns 4 adjacent columns and walks 16 rows with a three-row
// register window of aligned dwords (own + both neighbours).  Stores: the lane's 12 bytes of a row are three aligned dwords (4 pixels x
// 3 bytes begin at a multiple of 12), written by ONE 12-byte store, so a wave's store instruction covers 768 contiguous bytes; only
// the lane that holds the row's end writes dword by dword (bytes behind 3 w - 1 of the last dword are zero, dwords that begin at or
// behind 3 w are not written).
#include "vsf_internal.h"

namespace {

typedef unsigned short v2u __attribute__((ext_vector_type(2)));
typedef uint32_t v3w __attribute__((ext_vector_type(3)));

struct BgrArgs {
  const uint8_t* src;
  size_t src_image_stride;
  int src_pitch;
  uint8_t* dst;
  size_t dst_image_stride;
  int dst_pitch;
  int w, h;
  int swap_rb, flip_rows;  // mosaics: the order as two wave-uniform flags (k_ingest.hip);  packed: swap_rb = the first channel is red
};

__device__ __forceinline__ v2u pick(uint32_t hi, uint32_t lo, uint32_t sel) {
  return __builtin_bit_cast(v2u, __builtin_amdgcn_perm(hi, lo, sel));
}

constexpr int kStripRows = 16;  // output rows per wave

// Four pixels' channels, one dword each (byte j = pixel j), into the lane's 12 bytes B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3.
__device__ __forceinline__ v3w interleave(uint32_t b, uint32_t g, uint32_t r) {
  const uint32_t bg01 = __builtin_amdgcn_perm(g, b, 0x05010400u);  // B0 G0 B1 G1
  const uint32_t bg23 = __builtin_amdgcn_perm(g, b, 0x07030602u);  // B2 G2 B3 G3
  const uint32_t g1r1 = __builtin_amdgcn_perm(r, bg01, 0x0C0C0503u);  // G1 R1 0 0
  v3w d;
  d.x = __builtin_amdgcn_perm(r, bg01, 0x02040100u);
  d.y = __builtin_amdgcn_perm(bg23, g1r1, 0x05040100u);
  d.z = __builtin_amdgcn_perm(r, bg23, 0x07030206u);
  return d;
}

// The lane's 12 bytes of row `row_off` (pixels x4 .. x4 + 3 of a row of w): whole when the row goes on behind them, else the
// dwords that begin before byte 3 w, the last one with zeros behind the row's end.
__device__ __forceinline__ void store_row(v3w d, const __amdgpu_buffer_rsrc_t& rsrc, int x4, int w, uint32_t row_off) {
  const uint32_t off = 3u * (uint32_t)x4, end = 3u * (uint32_t)w;
  if (off + 12u <= end) {
    __builtin_amdgcn_raw_buffer_store_b96(d, rsrc, off, row_off, 0);
    return;
  }
  const uint32_t v[3] = {d.x, d.y, d.z};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t o = off + 4u * k;
    if (o < end) {
      const uint32_t left = end - o;
      const uint32_t keep = left >= 4u ? 0xFFFFFFFFu : (1u << (8u * left)) - 1u;
      __builtin_amdgcn_raw_buffer_store_b32(v[k] & keep, rsrc, o, row_off, 0);
    }
  }
}

// B | G << 8 | R << 16 of interior pixel (x, y) of an RGGB mosaic seen through the two flags (scalar; only for a last column whose
// source column belongs to another wave, i.e. widths of the form 256 k + 1: cf. gray_at in k_ingest.hip)
__device__ __forceinline__ uint32_t bgr_at(const uint8_t* img, int pitch, int x, int y, bool flip_rows) {
  const uint8_t* c = img + (size_t)y * pitch + x;
  const uint8_t* u = c - pitch;
  const uint8_t* d = c + pitch;
  const uint32_t cross = (u[0] + d[0] + c[-1] + c[1] + 2) >> 2, diag = (u[-1] + u[1] + d[-1] + d[1] + 2) >> 2;
  const uint32_t hor = (c[-1] + c[1] + 1) >> 1, ver = (u[0] + d[0] + 1) >> 1, cen = c[0];
  const bool ex = x & 1, ey = (y & 1) != flip_rows;
  const uint32_t G = ex == ey ? cross : cen;
  const uint32_t B = ey ? (ex ? cen : hor) : (ex ? ver : diag);
  const uint32_t R = ey ? (ex ? diag : ver) : (ex ? hor : cen);
  return B | (G << 8) | (R << 16);
}

// cv::cvtColor(COLOR_Bayer??2BGR), dcn = 3.  Stated for RGGB -- red at (even x, even y), blue at (odd, odd) --; the other orders are
//   BGGR: red and blue exchanged;   GBRG: the rows' parity flipped;   GRBG: both
// as in bayer_gray_kernel: both flags are kernel arguments, hence wave-uniform.  flip_rows enters the row parity, swap_rb chooses
// which of the two colour sums is stored first; neither touches the sums.
__global__ __launch_bounds__(256) void bayer_bgr_kernel(BgrArgs a) {
  const bool swap_rb = a.swap_rb != 0, flip_rows = a.flip_rows != 0;
  // wave = 256 columns (4 per lane) x 16 rows, walked top to bottom with a three-row register window (bayer_gray_kernel)
  const int strip = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6)), image = blockIdx.z;
  const int x4 = 4 * (blockIdx.x * 64 + (threadIdx.x & 63));
  const int y0 = strip * kStripRows, y1 = min(y0 + kStripRows, a.h);
  if (x4 >= a.w || y0 >= a.h) return;
  const uint8_t* img = a.src + (size_t)image * a.src_image_stride;
  const uint32_t dst_bytes = (uint32_t)(a.h - 1) * (uint32_t)a.dst_pitch + ((3u * (uint32_t)a.w + 3u) & ~3u);
  const __amdgpu_buffer_rsrc_t dst_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(a.dst + (size_t)image * a.dst_image_stride, 0, dst_bytes, 0x00020000);
  if (a.w < 3 || a.h < 3) {  // OpenCV's loops leave such images zero
    const v3w zero = {0u, 0u, 0u};
    for (int y = y0; y < y1; y++) store_row(zero, dst_rsrc, x4, a.w, (uint32_t)y * (uint32_t)a.dst_pitch);
    return;
  }
  // Frame columns: column 0 copies column 1 and column w - 1 copies column w - 2, fixed up on each channel's packed dword (a byte
  // move inside the lane, or one DPP hop from the left neighbour), so every lane takes the same path.  Columns >= w of the last
  // dword are computed from whatever lies in the row padding and are cut off by store_row.
  const int jr = (a.w - 1) - x4;  // position of the last column inside this lane's dword (0..3 when it is here)
  const bool lone_right = jr == 0 && (threadIdx.x & 63) == 0;  // ... and its source column is in another wave
  const __amdgpu_buffer_rsrc_t src_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(img), 0, a.src_pitch * a.h, 0x00020000);
  struct Row {
    uint32_t p, d, n;
  };
  auto load = [&](int r) -> Row {  // source row r, clamped into the image (the clamped rows feed frame rows only)
    const uint32_t row_off = (uint32_t)min(max(r, 0), a.h - 1) * (uint32_t)a.src_pitch;  // scalar
    return Row{__builtin_amdgcn_raw_buffer_load_b32(src_rsrc, (uint32_t)x4 - 4u, row_off, 0),
               __builtin_amdgcn_raw_buffer_load_b32(src_rsrc, (uint32_t)x4, row_off, 0),
               __builtin_amdgcn_raw_buffer_load_b32(src_rsrc, (uint32_t)min(x4 + 4, a.src_pitch - 4), row_off, 0)};
  };
  // 16-bit pairs (byte k, byte k + 1) of the 12-byte run p d n: on (d, p): bytes 3, 4;  on (n, d): bytes 0..4 of d | n
  const uint32_t s3 = 0x0C040C03u, s4 = 0x0C010C00u, s5 = 0x0C020C01u, s6 = 0x0C030C02u, s7 = 0x0C040C03u;
  const v2u one = {1, 1}, two = {2, 2};
  auto yc_of = [&](int y) -> int { return min(max(y, 1), a.h - 2); };
  // column 0 <- column 1, column w - 1 <- column w - 2 on one channel's dword (byte j = pixel x4 + j); `lone`: that channel of
  // pixel w - 2 when it lives in another wave
  auto frame = [&](uint32_t g, uint32_t lone) -> uint32_t {
    const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)g, 0x138, 0xF, 0xF, false);  // lane - 1's dword
    if (x4 == 0) g = (g & 0xFFFFFF00u) | ((g >> 8) & 0xFFu);
    if (jr == 0) g = (g & 0xFFFFFF00u) | (lone_right ? lone : (left >> 24));
    if (jr >= 1 && jr <= 3) {
      const uint32_t sh = 8u * (uint32_t)jr;
      g = (g & ~(0xFFu << sh)) | (((g >> (sh - 8u)) & 0xFFu) << sh);
    }
    return g;
  };
  // One output row.  A pair of pixels is (even x, odd x) in the (low, high) halves of every packed quantity:
  //   odd row  (ey): even x = green (G cen, B hor, R ver),    odd x = blue site (B cen, G cross, R diag)
  //   even row     : even x = red site (R cen, G cross, B diag), odd x = green (G cen, R hor, B ver)
  // so each channel of the pair is the low half of one quantity and the high half of another, chosen by the row parity (scalar).
  auto emit = [&](int y, const Row& U, const Row& C, const Row& D, bool ey) {
    uint32_t ch[3] = {0u, 0u, 0u};  // B, G, R of RGGB: byte j = pixel j
#pragma unroll
    for (int half = 0; half < 2; half++) {
      v2u ul, uc, ur, cl, cc, cr, dl, dc, dr;
      if (half == 0) {
        ul = pick(U.d, U.p, s3), uc = pick(U.n, U.d, s4), ur = pick(U.n, U.d, s5);
        cl = pick(C.d, C.p, s3), cc = pick(C.n, C.d, s4), cr = pick(C.n, C.d, s5);
        dl = pick(D.d, D.p, s3), dc = pick(D.n, D.d, s4), dr = pick(D.n, D.d, s5);
      } else {
        ul = pick(U.n, U.d, s5), uc = pick(U.n, U.d, s6), ur = pick(U.n, U.d, s7);
        cl = pick(C.n, C.d, s5), cc = pick(C.n, C.d, s6), cr = pick(C.n, C.d, s7);
        dl = pick(D.n, D.d, s5), dc = pick(D.n, D.d, s6), dr = pick(D.n, D.d, s7);
      }
      const v2u ns = uc + dc, we = cl + cr;
      const uint32_t cross = __builtin_bit_cast(uint32_t, (v2u)((ns + we + two) >> two));
      const uint32_t diag = __builtin_bit_cast(uint32_t, (v2u)((ul + ur + dl + dr + two) >> two));
      const uint32_t hor = __builtin_bit_cast(uint32_t, (v2u)((we + one) >> one));
      const uint32_t ver = __builtin_bit_cast(uint32_t, (v2u)((ns + one) >> one));
      const uint32_t cen = __builtin_bit_cast(uint32_t, cc);
      // (low half from the first, high half from the second: every value is below 256, so the pair packs to two bytes)
      const uint32_t bp = ((ey ? hor : diag) & 0xFFFFu) | ((ey ? cen : ver) & 0xFFFF0000u);
      const uint32_t gp = ((ey ? cen : cross) & 0xFFFFu) | ((ey ? cross : cen) & 0xFFFF0000u);
      const uint32_t rp = ((ey ? ver : cen) & 0xFFFFu) | ((ey ? diag : hor) & 0xFFFF0000u);
      const uint32_t sh = 16u * (uint32_t)half;
      ch[0] |= ((bp | (bp >> 8)) & 0xFFFFu) << sh;
      ch[1] |= ((gp | (gp >> 8)) & 0xFFFFu) << sh;
      ch[2] |= ((rp | (rp >> 8)) & 0xFFFFu) << sh;
    }
    uint32_t lone = 0u;
    if (lone_right) lone = bgr_at(img, a.src_pitch, a.w - 2, yc_of(y), flip_rows);
    const uint32_t b = frame(ch[0], lone & 0xFFu), g = frame(ch[1], (lone >> 8) & 0xFFu), r = frame(ch[2], lone >> 16);
    store_row(swap_rb ? interleave(r, g, b) : interleave(b, g, r), dst_rsrc, x4, a.w, (uint32_t)y * (uint32_t)a.dst_pitch);
  };
  // output row y is computed at yc = clamp(y, 1, h - 2) from source rows yc - 1 .. yc + 1 (bayer_gray_kernel's window)
  int yc = min(max(y0, 1), a.h - 2);
  Row U = load(yc - 1), C = load(yc), D = load(yc + 1);
  for (int y = y0; y < y1; y++) {
    const int ycn = min(max(y + 1, 1), a.h - 2);  // next output row's centre row (wave-uniform)
    Row N = D;
    if (ycn != yc) N = load(ycn + 1);  // requested before this row's arithmetic
    emit(y, U, C, D, (yc & 1) != flip_rows);
    if (ycn != yc) {
      U = C;
      C = D;
      D = N;
      yc = ycn;
    }
  }
}

// What cv_bridge's toCvCopy(msg, "bgr8") makes of the packed 8-bit formats: MONO8 -> B = G = R (GRAY2BGR), BGR8 -> a copy, RGB8 -> R
// and B exchanged, BGRA8 / RGBA8 -> alpha dropped (and R, B exchanged for RGBA8).  BPP bytes read + 3 written per pixel, no arithmetic:
// a lane owns 4 adjacent pixels, BPP aligned dwords in, three aligned dwords out (store_row), v_perm_b32 selectors between them.
// A wave owns 256 columns x kStripRows rows and requests kPackedRows rows before the first store (packed_gray_kernel).
// A source dword is read only if it begins before the end of ITS row rounded up to 4 bytes -- inside what packed_gray_kernel may
// read --, anything else counts as zero.
// BPP = 0 is the step in front of the demosaic in vsf_bag_extract_batch, cv::split(image)[0]: three bytes a pixel in, the FIRST of
// them out, one byte a pixel (one aligned dword per lane, zeros behind column w - 1).
constexpr int kPackedRows = 4;  // rows in flight per lane

template <int BPP>
__global__ __launch_bounds__(256) void packed_bgr_kernel(BgrArgs a) {
  constexpr int IN = BPP == 0 ? 3 : BPP;  // source bytes per pixel = source dwords per lane
  const int strip = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6)), image = blockIdx.z;
  const int x4 = 4 * (blockIdx.x * 64 + (threadIdx.x & 63));
  const int y0 = strip * kStripRows, y1 = min(y0 + kStripRows, a.h);
  if (x4 >= a.w || y0 >= a.h) return;
  const uint32_t src_row = ((uint32_t)a.w * IN + 3u) & ~3u;
  const uint32_t dst_row = BPP == 0 ? ((uint32_t)a.w + 3u) & ~3u : (3u * (uint32_t)a.w + 3u) & ~3u;
  const uint32_t src_bytes = (uint32_t)(a.h - 1) * (uint32_t)a.src_pitch + src_row;
  const uint32_t dst_bytes = (uint32_t)(a.h - 1) * (uint32_t)a.dst_pitch + dst_row;
  const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.src) + (size_t)image * a.src_image_stride, 0, src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t dst_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(a.dst + (size_t)image * a.dst_image_stride, 0, dst_bytes, 0x00020000);
  const bool swap = a.swap_rb != 0;  // (wave-uniform: it selects selectors)
  for (int y = y0; y < y1; y += kPackedRows) {
    uint32_t d[kPackedRows][IN];
#pragma unroll
    for (int u = 0; u < kPackedRows; u++)
#pragma unroll
      for (int k = 0; k < IN; k++) {
        const uint32_t o = (uint32_t)x4 * IN + 4u * k;
        d[u][k] = (y + u < y1 && o < src_row)
                      ? __builtin_amdgcn_raw_buffer_load_b32(src_rsrc, o, (uint32_t)(y + u) * (uint32_t)a.src_pitch, 0)
                      : 0u;
      }
#pragma unroll
    for (int u = 0; u < kPackedRows; u++) {
      if (y + u >= y1) break;  // (wave-uniform)
      const uint32_t row_off = (uint32_t)(y + u) * (uint32_t)a.dst_pitch;
      const uint32_t* s = d[u];
      if constexpr (BPP == 0) {  // bytes 0, 3, 6, 9 of the lane's 12
        const uint32_t t = __builtin_amdgcn_perm(s[1], s[0], 0x0C060300u);
        const uint32_t g = __builtin_amdgcn_perm(s[IN - 1], t, 0x05020100u);
        const int left = a.w - x4;
        const uint32_t keep = left >= 4 ? 0xFFFFFFFFu : (1u << (8 * left)) - 1u;
        __builtin_amdgcn_raw_buffer_store_b32(g & keep, dst_rsrc, (uint32_t)x4, row_off, 0);
        continue;
      }
      v3w o;
      if constexpr (BPP == 1) {  // g0 g0 g0 g1 | g1 g1 g2 g2 | g2 g3 g3 g3
        o.x = __builtin_amdgcn_perm(s[0], s[0], 0x01000000u);
        o.y = __builtin_amdgcn_perm(s[0], s[0], 0x02020101u);
        o.z = __builtin_amdgcn_perm(s[0], s[0], 0x03030302u);
      } else if constexpr (BPP == 3 || BPP == 0) {  // a copy, or bytes 2 1 0 5 | 4 3 8 7 | 6 11 10 9 of the lane's 12
        const uint32_t t = __builtin_amdgcn_perm(s[IN - 1], s[0], 0x0C0C0403u);  // byte 3, byte 8
        o.x = swap ? __builtin_amdgcn_perm(s[1], s[0], 0x05000102u) : s[0];
        o.y = swap ? __builtin_amdgcn_perm(t, s[1], 0x03050400u) : s[1];
        o.z = swap ? __builtin_amdgcn_perm(s[IN - 1], s[1], 0x05060702u) : s[IN - 1];
      } else {  // every pixel's dword to B G R 0, then three bytes of each
        const uint32_t sel = swap ? 0x0C000102u : 0x0C020100u;
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; j++) p[j] = __builtin_amdgcn_perm(0u, s[j % IN], sel);
        o.x = __builtin_amdgcn_perm(p[1], p[0], 0x04020100u);
        o.y = __builtin_amdgcn_perm(p[2], p[1], 0x05040201u);
        o.z = __builtin_amdgcn_perm(p[3], p[2], 0x06050402u);
      }
      store_row(o, dst_rsrc, x4, a.w, row_off);
    }
  }
}

}  // namespace

// Any known pixel format -> B G R (an unknown one launches nothing: the callers have refused it).  ONE launch for the batch.
void vsf_launch_to_bgr(int pixfmt, const uint8_t* d_src, int n, int w, int h, size_t src_image_stride, int src_pitch,
                       uint8_t* d_dst, size_t dst_image_stride, int dst_pitch, hipStream_t s) {
  BgrArgs a{d_src, src_image_stride, src_pitch, d_dst, dst_image_stride, dst_pitch, w, h, 0, 0};
  const int nstrips = (h + kStripRows - 1) / kStripRows;
  const dim3 grid((w + 255) / 256, (nstrips + 3) / 4, n), block(256);
  switch (pixfmt) {
    case VSF_PIX_BAYER_RGGB8:
    case VSF_PIX_BAYER_GRBG8:
    case VSF_PIX_BAYER_GBRG8:
    case VSF_PIX_BAYER_BGGR8:
      a.swap_rb = pixfmt == VSF_PIX_BAYER_GRBG8 || pixfmt == VSF_PIX_BAYER_BGGR8;
      a.flip_rows = pixfmt == VSF_PIX_BAYER_GRBG8 || pixfmt == VSF_PIX_BAYER_GBRG8;
      hipLaunchKernelGGL(bayer_bgr_kernel, grid, block, 0, s, a);
      break;
    case VSF_PIX_MONO8:
      hipLaunchKernelGGL(packed_bgr_kernel<1>, grid, block, 0, s, a);
      break;
    case VSF_PIX_BGR8:
    case VSF_PIX_RGB8:
      a.swap_rb = pixfmt == VSF_PIX_RGB8;
      hipLaunchKernelGGL(packed_bgr_kernel<3>, grid, block, 0, s, a);
      break;
    case VSF_PIX_BGRA8:
    case VSF_PIX_RGBA8:
      a.swap_rb = pixfmt == VSF_PIX_RGBA8;
      hipLaunchKernelGGL(packed_bgr_kernel<4>, grid, block, 0, s, a);
      break;
    default:
      break;
  }
}

// cv::split(image)[0] of n B G R images: the first byte of every pixel (bases and pitches multiples of 4, dst_pitch >= (w + 3) & ~3).
void vsf_launch_bgr_channel0(const uint8_t* d_src, int n, int w, int h, size_t src_image_stride, int src_pitch, uint8_t* d_dst,
                             size_t dst_image_stride, int dst_pitch, hipStream_t s) {
  BgrArgs a{d_src, src_image_stride, src_pitch, d_dst, dst_image_stride, dst_pitch, w, h, 0, 0};
  const int nstrips = (h + kStripRows - 1) / kStripRows;
  hipLaunchKernelGGL(packed_bgr_kernel<0>, dim3((w + 255) / 256, (nstrips + 3) / 4, n), dim3(256), 0, s, a);
}
