// k_pyramid.hip -- K1: ORB scale pyramid, level l = resize(level l-1, INTER_LINEAR), CV_8UC1.
//
// Restates cv::resize's 8-bit bilinear path (imgproc/imgwarp.cpp: HResizeLinear<uchar,int,short,2048> +
// VResizeLinear<..., FixedPtCast<int,uchar,22>>) as reached from ORB_Impl::detectAndCompute
// (features2d/orb.cpp), i.e. from slam_frontend.cc:274.  The coefficients (xofs/ialpha, yofs/ibeta) are evaluated IN the
// kernels by the one statement of cv::resize's formula that the host's tables use too (vsf_resize.h: resize_xtap,
// resize_ytap); the host builds its tables only to check, per level, what the kernels rely on (vsf_geometry.hip).
//
// resize_strip_kernel<R> (no LDS, no barriers): a wave owns 256 output columns (lane = 4 adjacent pixels) x a strip of
// R = 8 or 16 output rows.  The lane's four x-taps are loop-invariant: four v_perm_b32 byte selectors and four packed
// weight pairs, evaluated IN the kernel with cv::resize's own double / float steps (no table load ahead of the row
// loads); the y taps are evaluated once per wave (lane r <-> row r, v_readlane -> scalar addresses and weights).  At
// scale 1.04 the R output rows touch at most R + 2 consecutive source rows (checked per level on the host,
// VsfLevel::resize_rows), so every source row goes through the horizontal pass ONCE (one 8-byte load + 4 x (v_perm +
// v_dot2_u32_u16)) and an output row picks its two with a wave-uniform branch; the vertical pass is v_mul_hi_u32_u24 on
// pre-shifted weights.  One launch per level (the level chain is a true dependency), issued as two chains of half
// batches on two streams.  pyramid_image_kernel: when the batch fills the chip, the 26 one-band levels (w <= 256) are
// built by ONE launch, a 1024-thread workgroup per image with the levels ping-ponged through LDS.
// pyramid_slab_kernel: a batch of one to four images (a frame) walks chains of levels per launch, the last level of a
// chain cut into slabs whose workgroups never wait for each other (border rows are computed twice).
// resize_march_kernel is the general fallback for levels that fail the R + 2 check.  A band narrower than a wave has the
// lane spans of its strips packed into full waves (strip_packed).
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "vsf_internal.h"

namespace {


typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(1))) U8B {
  uint32_t lo, hi;
};

struct ResizeArgs {
  const uint8_t* src;
  size_t src_img_stride;
  int src_pitch, sw, sh;
  uint8_t* dst;
  size_t dst_img_stride;
  int dst_pitch, dw, dh;
  double scale_x, scale_y;  // cv::resize: 1. / ((double)dw / sw), 1. / ((double)dh / sh)
  int nstrips;
  // packed last band (resize_strip_kernel; pk.waves == 0: every band is a wave per strip): columns [pk.x0, dw) of all
  // strips laid end to end, pk.lanes lanes per strip, cut into pk.waves waves
  VsfPackPlan pk;
};

// The pieces every form of the computation is put together from.
struct StripX {      // per (level, band, lane): x taps as byte selectors + weight pairs, source window, output column
  uint32_t s0, s1, s2, s3, q0, q1, q2, q3, base;
  int x4;
  bool active;
};
constexpr int kStripXWords = 9;  // s0..s3, q0..q3, base: what a StripX keeps in LDS, [word][lane]
struct H4 {          // horizontal sums of a lane's four pixels on one source row, low 4 bits cleared (VResizeLinear: S >> 4)
  uint32_t a, b, c, d;
};

__device__ __forceinline__ uint32_t pack16(uint32_t lo, uint32_t hi) { return lo | (hi << 16); }  // (lo < 2^16)
__device__ __forceinline__ uint32_t tap_weights(const VsfTap& t) { return pack16((uint16_t)t.c0, (uint16_t)t.c1); }

// The lane's four x taps (loop-invariant), x4: its first output column.  No table load sits in front of the source-row
// loads: a wave's dependency chain is  rows -> arithmetic -> store.
__device__ __forceinline__ StripX strip_setup_at(const ResizeArgs& a, int x4) {
  StripX c;
  c.x4 = x4;
  c.active = x4 < a.dw;
  const VsfTap t0 = resize_xtap(min(x4 + 0, a.dw - 1), a.scale_x, a.sw), t1 = resize_xtap(min(x4 + 1, a.dw - 1), a.scale_x, a.sw),
               t2 = resize_xtap(min(x4 + 2, a.dw - 1), a.scale_x, a.sw), t3 = resize_xtap(min(x4 + 3, a.dw - 1), a.scale_x, a.sw);
  const uint32_t base = (uint32_t)min((int)t0.i0, a.sw - 8);  // 8-byte window [base, base+8) covers all eight taps
  auto selector = [&](const VsfTap& t) -> uint32_t { return (t.i0 - base) | 0x0C000C00u | ((t.i1 - base) << 16); };
  c.base = base;
  c.s0 = selector(t0), c.s1 = selector(t1), c.s2 = selector(t2), c.s3 = selector(t3);
  c.q0 = tap_weights(t0), c.q1 = tap_weights(t1), c.q2 = tap_weights(t2), c.q3 = tap_weights(t3);
  return c;
}
__device__ __forceinline__ StripX strip_setup(const ResizeArgs& a, int band) {
  return strip_setup_at(a, band * 256 + (int)(threadIdx.x & 63) * 4);
}

// A level's x taps pass from the wave that evaluated them to the others through LDS: o[kStripXWords][64]
__device__ __forceinline__ void stripx_store(uint32_t (*o)[64], int lane, const StripX& c) {
  o[0][lane] = c.s0, o[1][lane] = c.s1, o[2][lane] = c.s2, o[3][lane] = c.s3;
  o[4][lane] = c.q0, o[5][lane] = c.q1, o[6][lane] = c.q2, o[7][lane] = c.q3;
  o[8][lane] = c.base;
}
__device__ __forceinline__ StripX stripx_load(const uint32_t (*o)[64], int lane, int x4, int dw) {
  StripX c;
  c.s0 = o[0][lane], c.s1 = o[1][lane], c.s2 = o[2][lane], c.s3 = o[3][lane];
  c.q0 = o[4][lane], c.q1 = o[5][lane], c.q2 = o[6][lane], c.q3 = o[7][lane];
  c.base = o[8][lane];
  c.x4 = x4;
  c.active = x4 < dw;
  return c;
}

// LDS images of a level are reached through LDS-typed pointers where the compiler cannot see that for itself (an
// address computed from a kernel argument): a generic pointer costs a flat instruction per access.
using lds_u8p = __attribute__((address_space(3))) uint8_t*;
using lds_cu8p = const __attribute__((address_space(3))) uint8_t*;
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
__device__ __forceinline__ uint32_t ld32(lds_cu8p p) { return *(const __attribute__((address_space(3))) uint32_t*)p; }
__device__ __forceinline__ void st32(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }
__device__ __forceinline__ void st32(lds_u8p p, uint32_t v) { *(__attribute__((address_space(3))) uint32_t*)p = v; }

// The lane's 8-byte source window of one row: bytes [row + base, row + base + 8) of S (HBM or LDS; `row` is the part
// of the offset that differs per lane, 0 where S already points at the row)
template <bool ALIGNED, class SP>
__device__ __forceinline__ U8B load_window(SP S, uint32_t row, uint32_t base, uint32_t pitch) {
  U8B v;
  if constexpr (ALIGNED) {
    // LDS source: an unaligned 8-byte read is split by the hardware and stalls the LDS queue; three aligned dwords and
    // two v_alignbyte give the same window (levels are padded to their 64-byte pitch, so the third dword exists; it is
    // clamped into the row: when it would start past the pitch none of its bytes is needed)
    const uint32_t b0 = row + (base & ~3u);
    const uint32_t d0 = ld32(S + b0), d1 = ld32(S + (b0 + 4u)), d2 = ld32(S + (row + min((base & ~3u) + 8u, pitch - 4u)));
    v.lo = __builtin_amdgcn_alignbyte(d1, d0, base & 3u);
    v.hi = __builtin_amdgcn_alignbyte(d2, d1, base & 3u);
  } else {
    v = *reinterpret_cast<const U8B*>((const uint8_t*)S + (row + base));
  }
  return v;
}

// HResizeLinear of one window: per pixel one v_perm_b32 (the two taps' bytes) + one v_dot2_u32_u16
__device__ __forceinline__ H4 hpass(const U8B& v, const StripX& c) {
  auto hsum = [&](uint32_t sel, uint32_t q) -> uint32_t {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, __builtin_amdgcn_perm(v.hi, v.lo, sel)),
                                  __builtin_bit_cast(v2u16, q), 0u, false) & 0xFFFFF0u;
  };
  H4 h;
  h.a = hsum(c.s0, c.q0);
  h.b = hsum(c.s1, c.q1);
  h.c = hsum(c.s2, c.q2);
  h.d = hsum(c.s3, c.q3);
  return h;
}

// VResizeLinear of one output dword:  ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2 per pixel, the weights
// pre-shifted (b << 12).  b * (S >> 4) >> 16 is the high word of the 24 x 24-bit product (b << 12) * (S & ~15)
// (b <= 2^11, S <= 255 * 2048 < 2^19): one full-rate v_mul_hi_u32_u24 instead of shift + 32-bit multiply + shift (it
// reads 24 bits: a caller may keep a flag above them).  The four 10-bit sums are shifted as two packed pairs and their
// low bytes gathered with one v_perm
__device__ __forceinline__ uint32_t vblend(const H4& h0, const H4& h1, uint32_t b0, uint32_t b1) {
  auto mulhi24 = [](uint32_t x, uint32_t y) -> uint32_t {
    return (uint32_t)(((uint64_t)(x & 0xFFFFFFu) * (uint64_t)(y & 0xFFFFFFu)) >> 32);
  };
  const uint32_t ta = mulhi24(b0, h0.a) + mulhi24(b1, h1.a) + 2u, tb = mulhi24(b0, h0.b) + mulhi24(b1, h1.b) + 2u;
  const uint32_t tc = mulhi24(b0, h0.c) + mulhi24(b1, h1.c) + 2u, td = mulhi24(b0, h0.d) + mulhi24(b1, h1.d) + 2u;
  const v2u16 lo = __builtin_bit_cast(v2u16, ta | (tb << 16)) >> (v2u16){2, 2};
  const v2u16 hi = __builtin_bit_cast(v2u16, tc | (td << 16)) >> (v2u16){2, 2};
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, hi), __builtin_bit_cast(uint32_t, lo), 0x06040200u);
}

// General form (any scale; the fallback for levels that fail the R + 2 check below): every output row loads its own two
// source rows.
template <int kStripRows>
__global__ __launch_bounds__(256) void resize_march_kernel(ResizeArgs a) {
  const int lane = threadIdx.x & 63;
  const int strip = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), band = blockIdx.z;
  if (strip >= a.nstrips) return;  // wave-uniform
  const StripX c = strip_setup(a, band);
  const uint8_t* S = a.src + (size_t)blockIdx.y * a.src_img_stride;  // wave-uniform; the lane adds `base`
  uint8_t* D = a.dst + (size_t)blockIdx.y * a.dst_img_stride;
  // The y taps are wave-uniform: lane r evaluates output row ys + r once, v_readlane hands the result to the scalar
  // unit, and row addresses / weights live in SGPRs from there on (one tap evaluation per wave instead of one per
  // row, address arithmetic off the vector ALU).
  const int ys = strip * kStripRows;
  const VsfTap32 tyl = resize_ytap32(min(ys + (lane & (kStripRows - 1)), a.dh - 1), a.scale_y, a.sh);
  const uint32_t ty_rows = pack16(tyl.i0, tyl.i1), ty_wts = pack16(tyl.c0, tyl.c1);  // (weights in [0, 2048])
  // Every output row issues its two source-row loads unconditionally (rows shared with the neighbouring output row
  // hit L1): no loop-carried state, so all 2 * kStripRows loads of the strip are in flight together.
  uint32_t wts[kStripRows];
  U8B v0[kStripRows], v1[kStripRows];
#pragma unroll
  for (int r = 0; r < kStripRows; r++) {
    const uint32_t rows = __builtin_amdgcn_readlane(ty_rows, r);
    wts[r] = __builtin_amdgcn_readlane(ty_wts, r);
    v0[r] = load_window<false>(S + (size_t)((rows & 0xFFFFu) * (uint32_t)a.src_pitch), 0u, c.base, 0u);  // scalar rows
    v1[r] = load_window<false>(S + (size_t)((rows >> 16) * (uint32_t)a.src_pitch), 0u, c.base, 0u);
  }
#pragma unroll
  for (int r = 0; r < kStripRows; r++) {
    const uint32_t out = vblend(hpass(v0[r], c), hpass(v1[r], c), (wts[r] & 0xFFFFu) << 12, (wts[r] >> 16) << 12);
    uint8_t* drow = D + (size_t)((uint32_t)min(ys + r, a.dh - 1) * (uint32_t)a.dst_pitch);  // scalar; a row past the
    if (c.active) *reinterpret_cast<uint32_t*>(drow + (uint32_t)c.x4) = out;  // last one rewrites the last row's values
  }
}

// Shared-row variant (levels whose y taps advance by 1 or 2 source rows per output row, VsfLevel::resize_rows): the
// strip's R output rows touch at most R + 2 consecutive source rows, so each source row is loaded and pushed through
// the horizontal pass ONCE (R + 2 row passes instead of 2 R) and an output row picks its two entries with a
// wave-uniform branch.  The kernel is VALU-bound (two pyramid chains overlap), so instruction count is time.
// The strip computation in three steps so that a caller can keep one band's x taps across strips and have the next
// strip's source rows in flight while the current one is computed (pyramid_image_kernel).
template <int R>
struct StripRows {   // per strip: the R + 2 source-row windows and the lane-distributed y taps
  U8B v[R + 2];
  uint32_t ty_i0, ty_wts;
};

// ys: first output row of the strip (any row: the R + 2 window holds for every start, VsfLevel::resize_any8, not only for
// multiples of R)
template <int R, bool ALIGNED = false, class SP = const uint8_t*>
__device__ __forceinline__ void strip_issue_from(const ResizeArgs& a, const StripX& c, SP S, int ys,
                                                 StripRows<R>& o) {  // S = the source level of this image (HBM or LDS)
  const int lane = threadIdx.x & 63;
  // y taps: lane r evaluates output row ys + r (only row index i0 and the two weights are needed)
  const VsfTap32 t = resize_ytap32(min(ys + (lane & (R - 1)), a.dh - 1), a.scale_y, a.sh);
  o.ty_i0 = t.i0;
  o.ty_wts = pack16(t.c0, t.c1);
  const uint32_t first = __builtin_amdgcn_readlane(o.ty_i0, 0);
#pragma unroll
  for (int k = 0; k < R + 2; k++) {
    const SP row = S + (min(first + (uint32_t)k, (uint32_t)(a.sh - 1)) * (uint32_t)a.src_pitch);  // scalar
    o.v[k] = load_window<ALIGNED>(row, 0u, c.base, (uint32_t)a.src_pitch);
  }
}

template <int R>
__device__ __forceinline__ void strip_issue(const ResizeArgs& a, const StripX& c, int image, int strip, StripRows<R>& o) {
  strip_issue_from<R>(a, c, a.src + (size_t)image * a.src_img_stride, strip * R, o);
}

// Output rows [ys, min(ys + R, yend)).  lcopy != nullptr: the rows are also written to an LDS image of the level (same
// pitch as in HBM; lcopy points at where the level's row 0 would be)
template <int R, class LP = uint8_t*>
__device__ __forceinline__ void strip_finish(const ResizeArgs& a, const StripX& c, int image, int ys, int yend,
                                             const StripRows<R>& in, LP lcopy = nullptr, bool to_lds = false) {
  uint8_t* D = a.dst + (size_t)image * a.dst_img_stride;
  const uint32_t first = __builtin_amdgcn_readlane(in.ty_i0, 0);
  H4 H[R + 2];
#pragma unroll
  for (int k = 0; k < R + 2; k++) H[k] = hpass(in.v[k], c);
#pragma unroll
  for (int r = 0; r < R; r++) {
    if (ys + r >= yend) break;  // wave-uniform
    const uint32_t wts = __builtin_amdgcn_readlane(in.ty_wts, r);
    const uint32_t b0 = (wts & 0xFFFFu) << 12, b1 = (wts >> 16) << 12;  // scalar, <= 2^23
    const bool skip = __builtin_amdgcn_readlane(in.ty_i0, r) != first + (uint32_t)r;  // then it is first + r + 1
    uint8_t* drow = D + (size_t)((uint32_t)(ys + r) * (uint32_t)a.dst_pitch);  // scalar
    const LP lrow = lcopy + (uint32_t)(ys + r) * (uint32_t)a.dst_pitch;
    if (skip) {
      const uint32_t out = vblend(H[r + 1], H[r + 2], b0, b1);
      if (c.active) *reinterpret_cast<uint32_t*>(drow + (uint32_t)c.x4) = out;
      if (to_lds && c.active) st32(lrow + (uint32_t)c.x4, out);
      asm volatile("" ::: "memory");  // keeps the two arms distinct (no select of the eight operands)
    } else {
      const uint32_t out = vblend(H[r], H[r + 1], b0, b1);
      if (c.active) *reinterpret_cast<uint32_t*>(drow + (uint32_t)c.x4) = out;
      if (to_lds && c.active) st32(lrow + (uint32_t)c.x4, out);
    }
  }
}

template <int R>
__device__ __forceinline__ void resize_strip_unit(const ResizeArgs& a, int image, int strip, int band) {
  const StripX c = strip_setup(a, band);
  StripRows<R> rows;
  strip_issue<R>(a, c, image, strip, rows);
  strip_finish<R>(a, c, image, strip * R, a.dh, rows);
}

// Packed form of a strip, for a band narrower than a wave (the plan: vsf_resize.h).  The lane spans of neighbouring strips
// of one level of one image share a wave: same x taps per column, same pitch, same source.  Nothing crosses lanes in the
// arithmetic, so a span may begin and end anywhere.  What was wave-uniform becomes per lane: the strip's first source row,
// the row addresses, the y weights and which two of the R + 2 filtered rows an output row blends.  The y taps are still
// evaluated once per (strip, row): lane e takes row e % R of the wave's (e / R)-th strip and a lane fetches its rows'
// taps with ds_bpermute.  The row pick is branch-free: output row r always blends filtered row r + 1 -- as the lower
// tap when cv::resize's yofs has stepped past r, as the upper tap otherwise -- with row r + 2 or row r, so the evaluating
// lane orders the two weights accordingly and flags the step in the sign bit of one of them (above the 24 bits vblend
// reads), and the lane selects ONE operand per pixel.
// strip: the lane's strip (lanes past the last strip repeat it and store nothing), s_lo: lane 0's (wave-uniform)
template <int R, bool ALIGNED = false, class SP = const uint8_t*, class LP = uint8_t*>
__device__ __forceinline__ void strip_packed(const ResizeArgs& a, const StripX& c, int image, int strip, int s_lo, SP S,
                                             LP lcopy = nullptr, bool to_lds = false) {
  const int lane = threadIdx.x & 63;
  const int last = a.nstrips - 1;
  const int sc = min(strip, last);
  const bool live = c.active && strip <= last;
  uint32_t ty_i0, wm, wo;  // of this lane's (strip, row): yofs; weight of filtered row r + 1; of the other row | step flag
  {
    const int r = lane & (R - 1);
    const VsfTap32 t = resize_ytap32(min(min(s_lo + lane / R, last) * R + r, a.dh - 1), a.scale_y, a.sh);
    ty_i0 = t.i0;
    const uint32_t b0 = (uint32_t)t.c0 << 12, b1 = (uint32_t)t.c1 << 12;
    const uint32_t first = (uint32_t)__builtin_amdgcn_ds_bpermute((lane & ~(R - 1)) * 4, (int)ty_i0);
    const bool step = ty_i0 != first + (uint32_t)r;  // then the row's taps are first + r + 1 and first + r + 2
    wm = step ? b0 : b1;
    wo = step ? (b1 | 0x80000000u) : b0;
  }
  const int slot = (sc - s_lo) * (R * 4);  // (byte address of) the lane that evaluated this lane's row 0
  const uint32_t first = (uint32_t)__builtin_amdgcn_ds_bpermute(slot, (int)ty_i0);
  H4 H[R + 2];
  {
    U8B v[R + 2];
#pragma unroll
    for (int k = 0; k < R + 2; k++)
      v[k] = load_window<ALIGNED>(S, min(first + (uint32_t)k, (uint32_t)(a.sh - 1)) * (uint32_t)a.src_pitch, c.base,
                                  (uint32_t)a.src_pitch);
#pragma unroll
    for (int k = 0; k < R + 2; k++) H[k] = hpass(v[k], c);
  }
  uint8_t* D = a.dst + (size_t)image * a.dst_img_stride;
  const int rlast = a.dh - last * R;  // rows of the level's last strip (wave-uniform)
  const uint32_t d0 = (uint32_t)(sc * R) * (uint32_t)a.dst_pitch + (uint32_t)c.x4;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t wmr = (uint32_t)__builtin_amdgcn_ds_bpermute(slot + 4 * r, (int)wm);
    const uint32_t wor = (uint32_t)__builtin_amdgcn_ds_bpermute(slot + 4 * r, (int)wo);
    const bool step = (int)wor < 0;
    const H4 other = {step ? H[r + 2].a : H[r].a, step ? H[r + 2].b : H[r].b, step ? H[r + 2].c : H[r].c,
                      step ? H[r + 2].d : H[r].d};
    const uint32_t out = vblend(H[r + 1], other, wmr, wor);
    const uint32_t doff = d0 + (uint32_t)r * (uint32_t)a.dst_pitch;
    if (live && (r < rlast || strip < last)) {  // (r < rlast is wave-uniform)
      *reinterpret_cast<uint32_t*>(D + doff) = out;
      if (to_lds) st32(lcopy + doff, out);
    }
  }
}

template <int R>
__device__ __forceinline__ void resize_packed_unit(const ResizeArgs& a, int image, int j) {
  const VsfPackedLane at = packed_lane(a.pk, (uint32_t)j * 64u + (threadIdx.x & 63));
  const StripX c = strip_setup_at(a, a.pk.x0 + at.lane * 4);
  strip_packed<R>(a, c, image, at.strip, __builtin_amdgcn_readfirstlane(at.strip), a.src + (size_t)image * a.src_img_stride);
}

// grid: (strips / 4, images, bands); with a packed last band (pk.waves > 0) the last z-slice counts packed waves
// (eight waves per SIMD, as without the packed form: the compiler is held to 64 VGPRs)
template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void resize_strip_kernel(ResizeArgs a) {
  const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (a.pk.waves > 0 && blockIdx.z == gridDim.z - 1) {
    if (unit < a.pk.waves) resize_packed_unit<R>(a, blockIdx.y, unit);
    return;
  }
  if (unit >= a.nstrips) return;  // wave-uniform
  resize_strip_unit<R>(a, blockIdx.y, unit, blockIdx.z);
}

struct PyramidArgs {
  const VsfLevel* levels;
  const uint8_t* img0;
  size_t img0_stride;
  int img0_pitch;
  uint8_t* pyr;
  uint32_t pyr_bytes;
  int l_begin, nlevels;  // pyramid_image_kernel: levels [l_begin, nlevels), l_begin >= 2
};

// A level's ResizeArgs for all images (a launch for a part of the batch moves src and dst on): level l = L from level
// l - 1 = P, level 0 being the caller's images.  8-row strips, nothing packed: a launch with other strips sets both.
// (L, P by reference: pyramid_slab_kernel keeps its chain's entries in LDS -- a scalar load per level and wave from the
// table in HBM sat at the head of every level's dependency chain)
__host__ __device__ __forceinline__ ResizeArgs level_args(const VsfLevel& L, const VsfLevel& P, const PyramidArgs& p, int l) {
  ResizeArgs a;
  if (l >= 2) {
    a.src = p.pyr + P.offset;
    a.src_img_stride = (size_t)p.pyr_bytes;
    a.src_pitch = P.pitch;
  } else {
    a.src = p.img0;
    a.src_img_stride = p.img0_stride;
    a.src_pitch = p.img0_pitch;
  }
  a.sw = P.w;
  a.sh = P.h;
  a.dst = p.pyr + L.offset;
  a.dst_img_stride = (size_t)p.pyr_bytes;
  a.dst_pitch = L.pitch;
  a.dw = L.w;
  a.dh = L.h;
  a.scale_x = __builtin_bit_cast(double, ((unsigned long long)L.rscale_x[1] << 32) | L.rscale_x[0]);
  a.scale_y = __builtin_bit_cast(double, ((unsigned long long)L.rscale_y[1] << 32) | L.rscale_y[0]);
  a.nstrips = (L.h + 7) / 8;
  a.pk = VsfPackPlan{0, 0, 0, 0};
  return a;
}

// Image-major tail of the pyramid for large batches: the levels that are one band wide (w <= 256; 26 of the 49 at
// 640x480) are a chain of ~8 us launch-to-launch latencies when launched one by one.  Here ONE launch walks them: a
// 1024-thread workgroup per image; each level is produced into HBM (for the other stages) AND into one of two LDS
// images, from which the next level is read -- between levels there is one workgroup barrier and no memory round trip.
// 16 waves share a level's strips; the x taps (the same for every wave: one band) are evaluated by wave 0 for the NEXT
// level while the others finish the current one.  (Walking ALL levels this way was no faster than the two chains of
// launches: the large levels are throughput-bound and want the whole chip per level.)  Used when the batch fills the
// CUs (vsf_launch_pyramid); every level of the tail must qualify for the shared-row strips and fit kTailLdsBytes.
constexpr int kTailLdsBytes = 61440;

__global__ __launch_bounds__(1024) void pyramid_image_kernel(PyramidArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t lvl[2][kTailLdsBytes];
  __shared__ uint32_t xs[2][kStripXWords][64];  // StripX of a level, per lane (double buffered)
  const int image = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto level = [&](int l) {
    __builtin_assume(l >= 2);  // (no level of the tail reads the caller's images)
    return level_args(p.levels[l], p.levels[l - 1], p, l);
  };
  auto publish = [&](int l) { stripx_store(xs[l & 1], lane, strip_setup(level(l), 0)); };  // wave 0: the level's x taps
  if (wave == 0) publish(p.l_begin);
  __syncthreads();
  for (int l = p.l_begin; l < p.nlevels; l++) {
    const ResizeArgs a = level(l);
    const StripX c = stripx_load(xs[l & 1], lane, lane * 4, a.dw);
    const bool from_lds = l > p.l_begin;
    uint8_t* lcopy = (l + 1 < p.nlevels) ? lvl[(l - p.l_begin) & 1] : nullptr;
    const uint8_t* lsrc = lvl[(l - p.l_begin + 1) & 1];
    const uint8_t* gsrc = a.src + (size_t)image * a.src_img_stride;
    // narrow levels: the strips' lane spans packed into full waves (strip_packed), where that saves instructions
    const VsfPackPlan pk = pack_plan(8, 0, a.dw, a.nstrips);
    if (pk.waves > 0) {  // (workgroup-uniform)
      for (int j = wave; j < pk.waves; j += 16) {
        // (packed_lane's two lines, written out: through the shared function this kernel compiles to one VALU
        // instruction and two VGPRs more -- v_mul_lo + v_add in place of one v_mad_u64_u32)
        const uint32_t g = (uint32_t)j * 64u + lane;
        VsfPackedLane at;
        at.strip = (int)__umulhi(g, pk.magic);
        at.lane = (int)g - at.strip * pk.lanes;
        const StripX cp = stripx_load(xs[l & 1], at.lane, at.lane * 4, a.dw);
        const int s_lo = __builtin_amdgcn_readfirstlane(at.strip);
        if (from_lds)
          strip_packed<8, true>(a, cp, image, at.strip, s_lo, lsrc, lcopy, lcopy != nullptr);
        else
          strip_packed<8>(a, cp, image, at.strip, s_lo, gsrc, lcopy, lcopy != nullptr);
      }
    } else {
      for (int strip = wave; strip < a.nstrips; strip += 16) {
        StripRows<8> rows;
        if (from_lds)  // (workgroup-uniform; two inlined copies so that the LDS one reads with ds_read_b32)
          strip_issue_from<8, true>(a, c, lsrc, strip * 8, rows);
        else
          strip_issue_from<8>(a, c, gsrc, strip * 8, rows);
        strip_finish<8>(a, c, image, strip * 8, a.dh, rows, lcopy, lcopy != nullptr);
      }
    }
    if (wave == 0 && l + 1 < p.nlevels) publish(l + 1);
    __syncthreads();  // (waits for this wave's LDS writes; the HBM copy is not read in this kernel)
  }
}

// The whole level chain for up to 16 images (vsf_observe_stereo, the host-pointer calls, small batches): there the 48 dependent launches
// are nothing but latency (~6.7 us each against ~1.5 us of work).  A launch of this kernel walks a CHAIN of levels
// [la, lb); the last level's rows are cut into `nslabs` slabs, one 1024-thread workgroup each, and a workgroup computes,
// level by level, exactly the rows its slab of the last level descends from -- a few rows more than its share on the
// earlier levels, which its neighbours compute as well (the same values, written twice) -- so that no workgroup ever
// waits for another.  Levels pass from one to the next through two LDS buffers (and go to HBM for the other stages); the
// chain's first level is read from HBM.  Row ranges follow cv::resize's own yofs; 8-row strips start at any row.
constexpr int kSlabMaxLevels = 32;
constexpr int kSlabBands = 3;                                    // levels up to 768 columns
constexpr size_t kSlabTapBytes = sizeof(uint32_t) * 2 * kSlabBands * kStripXWords * 64;
constexpr size_t kSlabFixedBytes = kSlabTapBytes + 2 * kSlabMaxLevels * sizeof(int) + (kSlabMaxLevels + 1) * sizeof(VsfLevel);

struct SlabArgs {
  PyramidArgs p;    // (l_begin / nlevels unused)
  int la, lb;       // levels [la, lb), la >= 1, lb - la <= kSlabMaxLevels
  int nslabs;
  uint32_t cap;     // bytes of one LDS level buffer
  int32_t* status;  // bit 0 is raised when a slab does not fit `cap` (a host-side sizing error)
};

__global__ __launch_bounds__(1024) void pyramid_slab_kernel(SlabArgs q) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const lds_u8p buf0 = (lds_u8p)smem, buf1 = buf0 + q.cap;
  uint32_t(*xs)[kSlabBands][kStripXWords][64] =
      reinterpret_cast<uint32_t(*)[kSlabBands][kStripXWords][64]>(smem + 2 * (size_t)q.cap);
  int* s_lo = reinterpret_cast<int*>(smem + 2 * (size_t)q.cap + kSlabTapBytes);
  int* s_hi = s_lo + kSlabMaxLevels;
  VsfLevel* s_lev = reinterpret_cast<VsfLevel*>(s_hi + kSlabMaxLevels);  // levels la - 1 .. lb - 1
  const int image = blockIdx.y, slab = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nl = q.lb - q.la;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(q.p.levels + (q.la - 1));
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_lev);
    for (int i = threadIdx.x; i < (nl + 1) * (int)(sizeof(VsfLevel) / 4); i += 1024) dst[i] = src[i];
  }
  __syncthreads();
  auto level = [&](int l) { return level_args(s_lev[l - q.la + 1], s_lev[l - q.la], q.p, l); };
  if (threadIdx.x == 0) {  // the slab's rows [lo, hi) of every level of the chain, from the last level backwards
    const int hz = s_lev[nl].h;
    int lo = (int)((long)hz * slab / q.nslabs), hi = (int)((long)hz * (slab + 1) / q.nslabs);
    bool fits = true;
    s_lo[nl - 1] = lo;
    s_hi[nl - 1] = hi;
    for (int l = q.lb - 1; l > q.la; l--) {
      const ResizeArgs a = level(l);
      if (hi > lo) {
        // cv::resize's yofs of the slab's first and last row: the upper taps' source rows
        const int f = resize_ytap32(min(lo, a.dh - 1), a.scale_y, a.sh).i0, g = resize_ytap32(min(hi - 1, a.dh - 1), a.scale_y, a.sh).i0;
        lo = f;
        hi = min(g + 1, a.sh - 1) + 1;
        fits = fits && (size_t)(hi - lo) * (size_t)a.src_pitch <= (size_t)q.cap;
      }
      s_lo[l - 1 - q.la] = lo;
      s_hi[l - 1 - q.la] = hi;
    }
    if (!fits) {
      atomicOr(q.status, 1);
      s_hi[nl - 1] = s_lo[nl - 1];  // (nothing is computed)
    }
  }
  // the LAST waves evaluate the next level's x taps (one band each, -> xs[l & 1]) while the first ones work on the
  // current level's strips: a level's taps cost about as much as a strip
  auto publish = [&](int l) {
    const ResizeArgs a = level(l);
    const int band = 15 - wave;
    if (band < ((a.dw + 255) >> 8)) stripx_store(xs[l & 1][band], lane, strip_setup(a, band));
  };
  if (wave >= 16 - kSlabBands) publish(q.la);
  __syncthreads();
  if (s_hi[nl - 1] <= s_lo[nl - 1]) return;  // (workgroup-uniform) more slabs than rows, or the sizing error
  for (int l = q.la; l < q.lb; l++) {
    const ResizeArgs a = level(l);
    const int j = l - q.la;
    if (wave >= 16 - kSlabBands && l + 1 < q.lb) publish(l + 1);
    const int ylo = s_lo[j], yhi = s_hi[j];
    const int nb = (a.dw + 255) >> 8;
    const bool from_lds = j > 0;
    // (LDS images are addressed as if they began at the level's row 0)
    const bool to_lds = l + 1 < q.lb;
    const lds_u8p lcopy = ((j & 1) ? buf1 : buf0) - (uint32_t)ylo * (uint32_t)a.dst_pitch;
    const lds_cu8p lsrc = ((j & 1) ? buf0 : buf1) - (uint32_t)(from_lds ? s_lo[j - 1] : 0) * (uint32_t)a.src_pitch;
    const uint8_t* gsrc = a.src + (size_t)image * a.src_img_stride;
    // A strip is one wave's serial instruction stream (~2.5 us for 8 rows): when 8-row strips would leave half the
    // waves idle the level is cut into 4-row strips instead
    auto run = [&](auto rows_tag) {
      constexpr int R = decltype(rows_tag)::value;
      const int nunits = ((yhi - ylo + R - 1) / R) * nb;
      for (int u = wave; u < nunits; u += 16) {
        const int st = u / nb, band = u - st * nb;
        const StripX c = stripx_load(xs[l & 1][band], lane, band * 256 + lane * 4, a.dw);
        const int ys = ylo + st * R;
        StripRows<R> rows;
        if (from_lds)  // (workgroup-uniform; two inlined copies so that the LDS one reads with ds_read_b32)
          strip_issue_from<R, true, lds_cu8p>(a, c, lsrc, ys, rows);
        else
          strip_issue_from<R>(a, c, gsrc, ys, rows);
        strip_finish<R, lds_u8p>(a, c, image, ys, yhi, rows, lcopy, to_lds);
      }
    };
    if (((yhi - ylo + 1) >> 1) * nb <= 16 - kSlabBands)  // (the last waves are busy with the next level's taps)
      run(std::integral_constant<int, 2>{});
    else if (((yhi - ylo + 3) >> 2) * nb <= 16 - kSlabBands)
      run(std::integral_constant<int, 4>{});
    else
      run(std::integral_constant<int, 8>{});
    __syncthreads();  // (waits for this wave's LDS writes; the HBM copy is not read in this kernel)
  }
}

// Sizes a chain [la, lb) for `nslabs` slabs: bytes of the largest LDS level image a workgroup keeps (levels la .. lb - 2),
// from the bound rows(l - 1) <= floor(rows(l) * scale_y) + 4 (two taps per row and the float rounding of yofs).
size_t slab_chain_bytes(const VsfLevel* lv, int la, int lb, int nslabs) {
  long rows = (lv[lb - 1].h + nslabs - 1) / nslabs + 1;
  size_t need = 0;
  for (int l = lb - 1; l > la; l--) {
    const double sy = 1. / ((double)lv[l].h / lv[l - 1].h);
    rows = std::min<long>((long)std::floor((double)rows * sy) + 4, lv[l - 1].h);
    need = std::max(need, (size_t)rows * (size_t)lv[l - 1].pitch);
  }
  return need;
}

PyramidArgs pyramid_args(const VsfDev& d, const VsfGeom& g, const VsfImages& im, int l_begin, int nlevels) {
  PyramidArgs p;
  p.levels = d.levels;
  p.img0 = im.base;
  p.img0_stride = im.image_stride;
  p.img0_pitch = (int)im.row_stride;
  p.pyr = d.pyr;
  p.pyr_bytes = g.pyr_bytes;
  p.l_begin = l_begin;
  p.nlevels = nlevels;
  return p;
}

// A batch of a frame or two (vsf_observe_stereo, the host-pointer calls) is bound by the LATENCY of the level chain, not
// by throughput: it takes pyramid_slab_kernel for every level (VSF_OPT_PYRAMID_CHAIN 0 keeps the launches + tail kernel;
// VSF_OPT_PYRAMID_CHAIN / _ROWS: levels per launch and rows per slab, for experiments).  False: nothing was launched.
// images: 2 -> 105 us (335 as launches), 8 -> 137 (335), 16 -> 212 (348), 32 -> 386 (341)
bool launch_slab_chains(const VsfDev& d, const VsfGeom& g, const VsfLevel* h_levels, const VsfImages& im, hipStream_t s) {
  bool ok = true;
  for (int l = 1; l < g.nlevels; l++) ok = ok && h_levels[l].resize_any8 && h_levels[l].w <= 256 * kSlabBands;
  // (the slab kernel's dynamic LDS exceeds the default limit: vsf_prepare_pyramid_kernels raised it at vsf_create; a
  // device that cannot give a workgroup that much keeps the per-level launches)
  const int chain_env = d.tune ? d.tune->pyramid_chain : 8;
  const int lds_limit = d.tune ? d.tune->lds_limit : 160 * 1024;
  if (!(ok && chain_env > 0 && lds_limit >= 160 * 1024 - 2048)) return false;
  const size_t fixed = kSlabFixedBytes;
  const size_t budget = 144 * 1024;
  for (int la = 1; la < g.nlevels;) {
    int lb = std::min({la + chain_env, la + kSlabMaxLevels, g.nlevels});
    const int rows_env = d.tune ? std::max(1, d.tune->pyramid_rows) : 6;
    int nslabs = std::max(1, std::min(64, h_levels[lb - 1].h / rows_env));
    size_t need = slab_chain_bytes(h_levels, la, lb, nslabs);
    while (2 * need + fixed > budget && (nslabs < 64 || lb > la + 1)) {  // thinner slabs, then a shorter chain
      if (nslabs < 64)
        nslabs = std::min(64, nslabs * 2);
      else
        --lb;
      need = slab_chain_bytes(h_levels, la, lb, nslabs);
    }
    SlabArgs q;
    q.p = pyramid_args(d, g, im, la, lb);
    q.la = la;
    q.lb = lb;
    q.nslabs = nslabs;
    q.cap = (uint32_t)((need + 255) & ~(size_t)255);
    q.status = d.status;
    hipLaunchKernelGGL(pyramid_slab_kernel, dim3(nslabs, im.n), dim3(1024), 2 * (size_t)q.cap + fixed, s, q);
    la = lb;
  }
  return true;
}

// First level of the image-major tail (g.nlevels: none).  A batch that fills the CUs with one workgroup per image (last
// round at least three quarters full) hands its one-band levels to pyramid_image_kernel; `side` doubles as the
// permission (the cross-call prefetch on the aux stream keeps the plain chain).
int choose_l_tail(const VsfDev& d, const VsfGeom& g, const VsfLevel* h_levels, const VsfImages& im, const VsfSideStream* side,
                  bool few) {
  int l_tail = g.nlevels;
  if (side && (im.n >= 64 || few || (d.tune && d.tune->pyramid_tail_min > 0 && im.n >= d.tune->pyramid_tail_min))) {
    static int ncu = 0;
    if (ncu == 0) {
      int dev = 0;
      hipDeviceProp_t prop;
      if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
      if (ncu <= 0) ncu = 256;
    }
    const int rounds = (im.n + ncu - 1) / ncu;
    const int tail_min = d.tune ? d.tune->pyramid_tail_min : 0;
    if (few || 4 * im.n >= 3 * rounds * ncu || (tail_min > 0 && im.n >= tail_min)) {
      while (l_tail > 2 && h_levels[l_tail - 1].w <= 256 && h_levels[l_tail - 1].resize_rows >= 8 &&
             h_levels[l_tail - 1].pitch * h_levels[l_tail - 1].h + 16 <= kTailLdsBytes)
        --l_tail;
      if (g.nlevels - l_tail < 4) l_tail = g.nlevels;  // not worth a launch
    }
  }
  return l_tail;
}

// Levels [1, l_tail), one launch per level.  Level l depends on level l - 1 of the same image only, so the chain of small
// dependent launches is issued once per half of the batch, on two streams, interleaved: the small levels are bound by the
// latency of a launch's dependency chain (~5 us each), not by throughput, and two chains run in the time of one.
// (two chains: with four the host's launch rate, ~4 us per launch, becomes the limit: 0.56 -> 0.94 ms measured)
// `hook` (one chain only): called behind the launch of level hook->level, in front of the first launch for level 0.
void launch_level_chains(const VsfDev& d, const VsfGeom& g, const VsfLevel* h_levels, const VsfImages& im, hipStream_t s,
                         const VsfSideStream* side, int l_tail, const VsfPyramidHook* hook) {
  const PyramidArgs p = pyramid_args(d, g, im, 1, l_tail);
  const int nchains = (side && side->n > 0 && im.n >= 2) ? 2 : 1;
  if (nchains > 1) hook = nullptr;  // (a level is complete on two streams then)
  if (hook && hook->level <= 0) hook->fn(hook->arg, s);
  hipStream_t st[VSF_SIDE_STREAMS + 1] = {s};
  for (int c = 1; c < nchains; c++) st[c] = side->stream[c - 1];
  if (nchains > 1) {
    vsf_note(hipEventRecord(side->fork, s));
    for (int c = 1; c < nchains; c++) vsf_note(hipStreamWaitEvent(st[c], side->fork, 0));
  }
  for (int l = 1; l < l_tail; l++) {
    const VsfLevel& L = h_levels[l];
    for (int c = 0; c < nchains; c++) {  // interleaved issue: the chains advance together
      const int i0 = (int)((long)im.n * c / nchains), n = (int)((long)im.n * (c + 1) / nchains) - i0;
      ResizeArgs a = level_args(L, h_levels[l - 1], p, l);
      a.src += (size_t)i0 * a.src_img_stride;
      a.dst += (size_t)i0 * a.dst_img_stride;
      const int nbands = (L.w + 255) / 256;
      // rows per wave: more bytes in flight per wave on the large levels, more waves on the small ones
      const bool large = (long)L.w * L.h * n >= 4000000;
      if (L.resize_rows >= 8) {
        const int R = (large && L.resize_rows >= 16) ? 16 : 8;
        a.nstrips = (L.h + R - 1) / R;
        // a last band narrower than a wave: its strips packed into full waves, where that saves instructions
        const int x0 = (L.w / 256) * 256;
        if (x0 < L.w) a.pk = pack_plan(R, x0, L.w, a.nstrips);
        const dim3 grid((a.nstrips + 3) / 4, n, nbands);
        if (R == 16)
          hipLaunchKernelGGL(resize_strip_kernel<16>, grid, dim3(256), 0, st[c], a);
        else
          hipLaunchKernelGGL(resize_strip_kernel<8>, grid, dim3(256), 0, st[c], a);
        continue;
      }
      const int rows = large ? 8 : 4;
      a.nstrips = (L.h + rows - 1) / rows;
      const dim3 grid((a.nstrips + 3) / 4, n, nbands);
      if (large)
        hipLaunchKernelGGL(resize_march_kernel<8>, grid, dim3(256), 0, st[c], a);
      else
        hipLaunchKernelGGL(resize_march_kernel<4>, grid, dim3(256), 0, st[c], a);
    }
    if (hook && hook->level == l) hook->fn(hook->arg, s);
  }
  for (int c = 1; c < nchains; c++) {
    vsf_note(hipEventRecord(side->join[c - 1], st[c]));
    vsf_note(hipStreamWaitEvent(s, side->join[c - 1], 0));
  }
}

}  // namespace

hipError_t vsf_prepare_pyramid_kernels(int lds_limit) {
  if (lds_limit < 160 * 1024 - 2048) return hipSuccess;  // (the slab kernel is then never launched)
  return hipFuncSetAttribute(reinterpret_cast<const void*>(pyramid_slab_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             160 * 1024 - 2048);
}

void vsf_launch_pyramid(const VsfDev& d, const VsfGeom& g, const VsfLevel* h_levels, const VsfImages& im,
                        hipStream_t s, const VsfSideStream* side, const VsfPyramidHook* hook) {
  const int few_max = d.tune ? d.tune->pyramid_few : 16;
  const bool few = side && im.n <= few_max;
  if (few && g.nlevels > 1 && launch_slab_chains(d, g, h_levels, im, s)) return;
  // (a hook comes with side == NULL: neither the slab chains above nor the image-major tail below are taken, every level
  // up to the last is a launch of the one chain)
  const int l_tail = choose_l_tail(d, g, h_levels, im, side, few);
  launch_level_chains(d, g, h_levels, im, s, side, l_tail, hook);
  if (l_tail < g.nlevels)
    hipLaunchKernelGGL(pyramid_image_kernel, dim3(im.n), dim3(1024), 0, s, pyramid_args(d, g, im, l_tail, g.nlevels));
}
