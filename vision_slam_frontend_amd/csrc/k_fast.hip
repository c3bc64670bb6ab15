// k_fast.hip -- K2 (+ the border half of K3): FAST-9/16 segment test, cornerScore, 3x3 non-max suppression and
// raster-order compaction, for every level of every image in ONE launch.
//
// Restates cv::FAST_t<16> and cornerScore<16> (features2d/fast.cpp, fast_score.cpp) as called by
// ORB's computeKeyPoints (threshold 20; slam_frontend.cc:274, parameters :205-213) and by
// FastFeatureDetector::detect (threshold 10, slam_frontend.cc:191,271), plus
// KeyPointsFilter::runByImageBorder(31) which is folded into the evaluated rectangle.
//
// Streaming march kernel -- no LDS, no barriers, no divergent corner/score phases:
//  * a wave owns a band of 248 keypoint columns x a strip of 32 rows of one level of one image and walks down the
//    rows; each lane holds 4 adjacent pixels per row (one coalesced 32-bit load) in a 7-row register window (nine
//    rotating register sets incl. two rows of read-ahead, no copies) and gets its neighbours' dwords by DPP wave shifts;
//  * corner test and score are ONE dense computation: with d_k = p_k - v on the 16-pixel circle,
//      A = max over the 16 arcs of min(d over the 9-arc),  B = -min over arcs of max(d over the arc)
//    (computed on the p_k, v subtracted once at the end),
//    the pixel is a FAST-9 corner iff max(A, B) > t and cornerScore is max(A, B) - 1.  Two pixels are processed per
//    VALU lane-op on packed 16-bit halves; circle bytes are pulled out of the window with v_perm_b32.  Arcs 2j and 2j + 1
//    share eight pixels, so max(arc 2j, arc 2j + 1) = min(octet, max(d[2j], d[2j + 9])) (min / max distribute): an octet
//    is two quads, a quad is the minimum of four consecutive circle pixels, and only the four ODD pixel pairs are made
//    on their own: an even quad is min3(pixel, pixel, pair), an odd one min3(pair, pixel, pixel) -> 4 + 8 two-input ops,
//    8 + 8 THREE-input ops and a 4-op reduction = 32 packed ops per polarity (36 with all eight pairs, 59 with prefix /
//    suffix minima of the circle halves, 80 naively).  The three-input ops are gfx950's v_pk_minimum3_f16 /
//    v_pk_maximum3_f16 applied to the pixel values as they sit in the halves: 0..255 are f16 denormals, ordered like the
//    integers and not flushed in the default mode (tools/exp/m3.hip: all 2^24 triples, full issue rate).  The kernels
//    issue 1.22 G wave-instructions per 512-image step (profiles/traffic.json; 1.32 G with 36 ops per polarity), two
//    thirds of them in this network: the vector ALU's issue rate is the floor of a dense score;
//  * the only branch is wave-wide: a row is skipped when v_sad_u8 of every lane's 4 pixels against the rows 3 above
//    and 3 below stays <= t (circle pixels 0 and 8: every 9-arc contains one of them);
//  * scores stay in registers; the strict 8-neighbour NMS is packed too (row-wise 3-maxima shared between the rows
//    above and below), and survivors are appended in raster order with ballot prefix ranks.
// Output per unit: a candidate segment in unit-local raster order + the start offset of every row, which
// vsf_gather.h merges into the level's global raster order.
#include "vsf_gather.h"
#include <algorithm>
#include <cstdlib>

#include "vsf_internal.h"

namespace {

typedef short v2s __attribute__((ext_vector_type(2)));
constexpr int SR = VSF_FAST_STRIP_ROWS;

struct FastArgs {
  const VsfLevel* levels;
  const uint32_t* units;  // full cells, then the packed items
  int nwork_full;
  int nunits;  // cells (strip x band) per image: stride of the row-start tables
  const uint8_t* img0;
  size_t img0_stride;
  int img0_pitch;
  const uint8_t* pyr;
  uint32_t pyr_bytes;
  uint32_t* cand;
  uint32_t cand_entries;
  uint16_t* rowstart;
  int threshold;
  int nms;
  // MASK kernels only (the others never read these): the detection masks of the launch's images, include/vsf.h "Detection masks"
  VsfFastMask mask;
};

__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {  // lane i <- lane i-1
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t wave_shl1(uint32_t v) {  // lane i <- lane i+1
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true);
}

// *p, read by every lane and declared the same in all of them (v_readfirstlane per dword)
template <class T>
__device__ __forceinline__ T uniform_copy(const T* p) {
  static_assert(sizeof(T) % 4 == 0, "dwords");
  T out;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(p);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
  for (size_t i = 0; i < sizeof(T) / 4; i++) dst[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)src[i]);
  return out;
}

// One image row as a lane holds it while the row is inside the 7-row window.  The lane's 4 pixels are bytes 4..7 of the
// 12-byte run {previous lane's dword, own dword, next lane's dword}; b<B> is the pair (byte B, byte B + 2) zero-extended
// into the two 16-bit halves -- the layout the score works on: pixel pairs (x, x + 2) and (x + 1, x + 3), so that the
// second pair's circle pixel at column offset dx IS the first pair's at dx + 1.  Over its seven steps in the window a row
// is asked for exactly the eight pairs b1 .. b8 (as row y +- 3: b3..b6, y +- 2: b2, b3, b6, b7, y +- 1 and y: b1, b2, b7, b8
// and, as the centre row, b4 / b5 themselves), so they are made ONCE when the row enters -- straight from
// the raw dword and its two DPP neighbours: 2 DPP moves, 6 v_perm_b32 and 2 v_and (10 ops; 11 when the even and odd bytes
// were split first and each half shifted across the lanes) -- instead of one v_perm_b32 per use (34 per step in round 3's
// kernel: profiles/r04/).
struct RowP {
  uint32_t d;                            // the raw dword (row pre-check)
  v2s b1, b2, b3, b4, b5, b6, b7, b8;
};

__device__ __forceinline__ v2s as_v2s(uint32_t v) { return __builtin_bit_cast(v2s, v); }
__device__ __forceinline__ uint32_t as_u32(v2s v) { return __builtin_bit_cast(uint32_t, v); }

__device__ __forceinline__ void prep_row(RowP& r) {
  const uint32_t d = r.d, p = wave_shr1(d), n = wave_shl1(d);          // bytes 4..7, 0..3 and 8..11 of the run
  // v_perm_b32: selector bytes 0..3 pick from the second operand, 4..7 from the first, 0x0c gives a zero byte
  r.b1 = as_v2s(__builtin_amdgcn_perm(0u, p, 0x0c030c01u));            // (1, 3)
  r.b2 = as_v2s(__builtin_amdgcn_perm(d, p, 0x0c040c02u));             // (2, 4)
  r.b3 = as_v2s(__builtin_amdgcn_perm(d, p, 0x0c050c03u));             // (3, 5)
  r.b4 = as_v2s(d & 0x00FF00FFu);                                      // (4, 6)
  r.b5 = as_v2s(__builtin_amdgcn_perm(0u, d, 0x0c030c01u));            // (5, 7)
  r.b6 = as_v2s(__builtin_amdgcn_perm(n, d, 0x0c040c02u));             // (6, 8)
  r.b7 = as_v2s(__builtin_amdgcn_perm(n, d, 0x0c050c03u));             // (7, 9)
  r.b8 = as_v2s(n & 0x00FF00FFu);                                      // (8, 10)
}

__device__ __forceinline__ v2s vmin(v2s a, v2s b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ v2s vmax(v2s a, v2s b) { return __builtin_elementwise_max(a, b); }
// Three-input packed minimum / maximum of values 0..255 held in 16-bit halves (see score_from_circle): the nested f16
// minimum / maximum is selected as ONE v_pk_minimum3_f16 / v_pk_maximum3_f16.  Written with the builtins and not as an asm
// statement, so that the compiler knows the instruction: it schedules the ops apart from their consumers and places a wait
// state only where the hardware needs one (behind an asm statement it assumes the worst: 13 s_nop per scoring block of
// this network instead of 4).
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2h as_v2h(v2s v) { return __builtin_bit_cast(v2h, v); }
__device__ __forceinline__ v2s vmin3(v2s a, v2s b, v2s c) {
  return __builtin_bit_cast(v2s, __builtin_elementwise_minimum(__builtin_elementwise_minimum(as_v2h(a), as_v2h(b)), as_v2h(c)));
}
__device__ __forceinline__ v2s vmax3(v2s a, v2s b, v2s c) {
  return __builtin_bit_cast(v2s, __builtin_elementwise_maximum(__builtin_elementwise_maximum(as_v2h(a), as_v2h(b)), as_v2h(c)));
}
// max(a - b, 0) per half (v_pk_sub_u16 with clamp): a, b in 0 .. 255
__device__ __forceinline__ v2s vsubsat(v2s a, v2s b) {
  typedef unsigned short v2us __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(v2s, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2us, a), __builtin_bit_cast(v2us, b)));
}

// Scores of two pixels of the centre row R3 from the 16 circle pixel pairs d[k] and the centre pair v.
// Returns, per 16-bit half, max(cornerScore + 1 - offs, 0) with offs = max(t, 1): zero for a pixel that is no corner (or,
// at t = 0, a corner of score 0, which can never win the strict suppression: cv::FAST_t compares against neighbours >= 0),
// cornerScore - (offs - 1) >= 1 otherwise -- an order-preserving offset, so the suppression compares these values as it
// would the scores and the emitter adds offs - 1 back.  (NMS == false: a marker 1 for every corner, as cv::FAST_t leaves
// the response at 0 then; `toff` = t in that instance.)
template <bool NMS>
__device__ __forceinline__ v2s score_from_circle(const v2s (&d)[16], v2s v, v2s toff) {
  // Arc k = d[k .. k+8] (indices mod 16).  Arcs 2j and 2j+1 share the eight pixels C = d[2j+1 .. 2j+8]:
  //   max(min(d[2j], C), min(C, d[2j+9])) = min(C, max(d[2j], d[2j+9]))                       (distributive lattice)
  // and C is two quads F_j, F_{j+2}, where F_i = min(d[2i+1 .. 2i+4]) is four consecutive pixels:
  //   A = max_j min3(F_j, F_{j+2}, max(d[2j], d[2j+9])),     Bm likewise with min and max exchanged.
  // With the pixel pairs E_i = min(d[2i+1], d[2i+2]) a quad is min(E_i, E_{i+1}); minimum is associative, so one pair of
  // each quad can stay two pixels of a three-input op and only the four ODD pairs are ever made:
  //   i even: F_i = min3(d[2i+1], d[2i+2], E_{i+1}),     i odd: F_i = min3(E_i, d[2i+3], d[2i+4])
  // (the same numbers, whatever the pixels).  4 + 8 two-input ops, 8 + 8 three-input ops and a 4-op reduction = 32 per
  // polarity (36 with all eight pairs and F_i = min(E_i, E_{i+1}); 59 with prefix / suffix minima of the two circle
  // halves).  The three-input ops are gfx950's v_pk_minimum3_f16 / v_pk_maximum3_f16 on the pixel values
  // as they sit in the 16-bit halves: 0..255 are f16 denormals, whose order is the integer order (f16 denormals are
  // never flushed in the default mode; exhaustively checked on MI355X for all 2^24 triples, tools/exp/m3.hip).
  v2s E[8], G[8], F[8], H[8];
#pragma unroll
  for (int j = 1; j < 8; j += 2) {
    E[j] = vmin(d[2 * j + 1], d[(2 * j + 2) & 15]);
    G[j] = vmax(d[2 * j + 1], d[(2 * j + 2) & 15]);
  }
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    F[j] = vmin3(d[2 * j + 1], d[2 * j + 2], E[j + 1]);
    H[j] = vmax3(d[2 * j + 1], d[2 * j + 2], G[j + 1]);
    F[j + 1] = vmin3(E[j + 1], d[(2 * j + 5) & 15], d[(2 * j + 6) & 15]);
    H[j + 1] = vmax3(G[j + 1], d[(2 * j + 5) & 15], d[(2 * j + 6) & 15]);
  }
  v2s ta[8], tb[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    ta[j] = vmin3(F[j], F[(j + 2) & 7], vmax(d[2 * j], d[(2 * j + 9) & 15]));
    tb[j] = vmax3(H[j], H[(j + 2) & 7], vmin(d[2 * j], d[(2 * j + 9) & 15]));
  }
  const v2s A = vmax(vmax3(vmax3(ta[0], ta[1], ta[2]), vmax3(ta[3], ta[4], ta[5]), ta[6]), ta[7]);
  const v2s Bm = vmin(vmin3(vmin3(tb[0], tb[1], tb[2]), vmin3(tb[3], tb[4], tb[5]), tb[6]), tb[7]);
  // cornerScore<16> = max(t, A - v, v - Bm) - 1; a corner iff max(A - v, v - Bm) > t.  Saturating subtractions: 4 ops.
  const v2s sc = vsubsat(vmax(vsubsat(A, v), vsubsat(v, Bm)), toff);
  const v2s one = {1, 1};
  return NMS ? sc : vmin(sc, one);
}

// Pixels 0 and 2 (J0 = 0) or 1 and 3 (J0 = 1) of the lane; R0..R6 are rows y-3 .. y+3.
// Bresenham circle, OpenCV order: (dx,dy) = (0,3)(1,3)(2,2)(3,1)(3,0)(3,-1)(2,-2)(1,-3)(0,-3)(-1,-3)(-2,-2)(-3,-1)
// (-3,0)(-3,1)(-2,2)(-1,3); window row = R[3 + dy]; pair index = 4 + J0 + dx.
template <bool NMS>
__device__ __forceinline__ v2s score_pair0(const RowP& R0, const RowP& R1, const RowP& R2, const RowP& R3, const RowP& R4,
                                           const RowP& R5, const RowP& R6, v2s toff) {
  const v2s d[16] = {R6.b4, R6.b5, R5.b6, R4.b7, R3.b7, R2.b7, R1.b6, R0.b5, R0.b4, R0.b3, R1.b2, R2.b1, R3.b1, R4.b1, R5.b2, R6.b3};
  return score_from_circle<NMS>(d, R3.b4, toff);
}
template <bool NMS>
__device__ __forceinline__ v2s score_pair1(const RowP& R0, const RowP& R1, const RowP& R2, const RowP& R3, const RowP& R4,
                                           const RowP& R5, const RowP& R6, v2s toff) {
  const v2s d[16] = {R6.b5, R6.b6, R5.b7, R4.b8, R3.b8, R2.b8, R1.b7, R0.b6, R0.b5, R0.b4, R1.b3, R2.b2, R3.b2, R4.b2, R5.b3, R6.b4};
  return score_from_circle<NMS>(d, R3.b5, toff);
}

// One score row as the NMS needs it, in the same pair layout: s02 = (s0, s2), s13 = (s1, s3) of the lane's pixels and
// the horizontal maxima of their neighbours.
struct ScoreRow {
  v2s s02, s13;
  v2s h3a, h3b;     // max(s[x-1], s[x], s[x+1]) for pixels (0, 2) and (1, 3)
  v2s h2a, h2b;     // max(s[x-1], s[x+1])
};

__device__ __forceinline__ ScoreRow make_score_row(v2s s02, v2s s13) {
  ScoreRow o;
  o.s02 = s02;
  o.s13 = s13;
  // left / right neighbours of pixels (0, 2) are (prev lane's s3, s1) and (s1, s3); of pixels (1, 3): (s0, s2) and (s2, next s0)
  const v2s x = as_v2s(__builtin_amdgcn_alignbit(as_u32(s13), wave_shr1(as_u32(s13)), 16));
  const v2s y = as_v2s(__builtin_amdgcn_alignbit(wave_shl1(as_u32(s02)), as_u32(s02), 16));
  o.h2a = vmax(x, s13);
  o.h2b = vmax(s02, y);
  o.h3a = vmax3(x, s13, s02);
  o.h3b = vmax3(s02, y, s13);
  return o;
}

// PACK = false: the wave is one unit (cell) of up to 248 keypoint columns x 32 rows of one level.
// PACK = true : the wave is a packed work item (vsf_internal.h): up to VSF_FAST_PACK_SEGS narrow cells of any levels
//               side by side, each on ceil(cols / 4) + 2 consecutive lanes with halo lanes of its own, so that the DPP
//               neighbours of a cell's columns are always the cell's own.  Level, row addresses, row range, masks and
//               the cell's running count are per lane; each cell keeps its own candidate segment and row-start table,
//               so downstream nothing changes.  (The pyramid's 50 levels end in a narrow band almost everywhere:
//               packing them lowers the lanes a 640x480 image keeps busy by 14 %.)
// NMS = false (standalone FAST without suppression only) keeps every corner and a zero response.
// MASK = true: KeyPointsFilter::runByPixelsMask at emission -- a survivor of the suppression is dropped when its own pixel is
//               zero in the mask level of its image (a slot's block: one byte a pixel, 0x00 / 0xFF, in the layout of one image's
//               pyramid block with level 0 at its place).  The row of the cell about to be emitted is requested when its step
//               begins and met where the survivors are known; an image without a mask reads an empty buffer and passes
//               everything.  MASK = false is the kernel without any of it: the launcher takes it whenever no image of the
//               launch has a mask.
// (`work`: index into a.units (PACK = false) or into the packed items -- wave-uniform)
template <bool PACK, bool NMS, bool MASK>
__device__ __forceinline__ void fast_march_body(const FastArgs& a, int work, int image) {
  const int lane = threadIdx.x & 63;
  int level, band, strip, hl, nl, nrows0 = 0;
  bool valid = true, mixed = false, rim = false;
  VsfLevel L;
  if constexpr (PACK) {
    struct Item {
      uint32_t w[VSF_FAST_PACK_WORDS];
    };
    const Item P = uniform_copy(reinterpret_cast<const Item*>(a.units + a.nwork_full) + work);
    uint32_t w0 = P.w[4], w1 = P.w[5];  // the lane's cell: the last one whose first lane is <= lane
#pragma unroll
    for (int k = 1; k < VSF_FAST_PACK_SEGS; k++)
      if (k < (int)P.w[0] && lane >= (int)(P.w[5 + 2 * k] & 0xFFu)) w0 = P.w[4 + 2 * k], w1 = P.w[5 + 2 * k];
    nrows0 = (int)P.w[1];
    mixed = P.w[2] != 0u;
    rim = P.w[3] != 0u;
    level = (int)(w0 >> 24), band = (int)((w0 >> 16) & 0xFF), strip = (int)(w0 & 0x7FFF);
    hl = lane - (int)(w1 & 0xFFu);
    nl = (int)((w1 >> 8) & 0xFFu);
    valid = hl < nl;  // (lanes past the last cell carry nothing)
    L = a.levels[level];
  } else {
    // (explicitly wave-uniform: in the resident kernels' cell loop these loads follow the previous cell's stores, so the
    // compiler will not prove them invariant and use scalar loads; vector loads would make every row address, the buffer
    // descriptor included, a per-lane value)
    const uint32_t ud = uniform_copy(a.units + work);
    level = (int)(ud >> 24), band = (int)((ud >> 16) & 0xFF), strip = (int)(ud & 0x7FFF);
    L = uniform_copy(a.levels + level);
    hl = lane, nl = 64;
  }
  // source rows: level 0 is the input image, levels >= 1 sit in the pyramid block (a packed item never mixes the two)
  const int pitch = level == 0 ? a.img0_pitch : L.pitch, hrow = L.h;
  const uint8_t* src;
  uint32_t src_bytes;
  if constexpr (PACK) {
    const bool lvl0 = __builtin_amdgcn_readfirstlane(level) == 0;
    src = lvl0 ? a.img0 + (size_t)image * a.img0_stride : a.pyr + (size_t)image * a.pyr_bytes;
    src_bytes = lvl0 ? (uint32_t)(a.img0_pitch * __builtin_amdgcn_readfirstlane(hrow)) : a.pyr_bytes;
  } else {
    src = level == 0 ? a.img0 + (size_t)image * a.img0_stride : a.pyr + (size_t)image * a.pyr_bytes + L.offset;
    src_bytes = (uint32_t)(pitch * hrow);
  }
  const int t = a.threshold;
  // score offset (see score_from_circle): the emitter adds offs - 1 back
  const int offs = NMS ? max(t, 1) : t;
  const v2s toff = {(short)offs, (short)offs};
  const int bx0 = L.fast_a0 + VSF_FAST_BAND_COLS * band;
  const int c0 = bx0 - 4 + 4 * hl;  // first column of this lane's 4 pixels (lane 1 of the cell starts the band)
  const bool loadable = valid && c0 >= 0 && c0 + 3 < pitch;
  const int ys = L.y_lo + strip * SR;
  const int nrows = valid ? min(SR, L.y_hi - ys) : 0;  // rows of this lane's cell
  if constexpr (!PACK) nrows0 = nrows;
  // Pixels that may carry a score: FAST's 3-pixel rim and one column beyond the keypoint rectangle (for the NMS).
  const int sx_lo = max(L.x_lo - 1, 3), sx_hi = min(L.x_hi + 1, L.w - 3);
  uint32_t sm02 = 0, sm13 = 0, em02 = 0, em13 = 0;  // per-pixel 16-bit masks in the pair layout: may be scored / emitted
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = c0 + j;
    const uint32_t bit = 0xFFFFu << (16 * (j >> 1));
    // lanes 1 .. nl-2 score and emit; lane 0 scores its last pixel only, lane nl-1 its first (the columns next to the band)
    const bool sc_ok = valid && ((hl >= 1 && hl <= nl - 2) || (hl == 0 && j == 3) || (hl == nl - 1 && j == 0)) &&
                       x >= sx_lo && x < sx_hi;
    const bool em_ok = valid && hl >= 1 && hl <= nl - 2 && x >= L.x_lo && x < L.x_hi && x < bx0 + VSF_FAST_BAND_COLS;
    if (j & 1) {
      if (sc_ok) sm13 |= bit;
      if (em_ok) em13 |= bit;
    } else {
      if (sc_ok) sm02 |= bit;
      if (em_ok) em02 |= bit;
    }
  }
  const int unit_local = strip * L.nbands + band;
  uint16_t* rs = a.rowstart + ((size_t)image * a.nunits + L.unit0 + unit_local) * VSF_FAST_RS_STRIDE;
  const int seg_cap = L.seg_cap;
  // Candidate stores go through a buffer descriptor.  One cell: over the cell's segment, and an entry beyond its capacity
  // is dropped by the range check of the store itself (no compare, no 64-bit address arithmetic per store).  PACK: over
  // the image's candidate buffer, every lane adds its cell's segment offset and checks the capacity itself.
  const __amdgpu_buffer_rsrc_t seg_rsrc =
      PACK ? __builtin_amdgcn_make_buffer_rsrc(a.cand + (size_t)image * a.cand_entries, 0, a.cand_entries * 4, 0x00020000)
           : __builtin_amdgcn_make_buffer_rsrc(a.cand + (size_t)image * a.cand_entries + L.cand_offset +
                                                   (size_t)unit_local * seg_cap,
                                               0, seg_cap * 4, 0x00020000);
  const uint32_t seg_off = PACK ? 4u * (L.cand_offset + (uint32_t)(unit_local * seg_cap)) : 0u;
  // PACK: row starts are stored by the cell's first lane as the rows go (one descriptor over the image's tables)
  const __amdgpu_buffer_rsrc_t rs_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      a.rowstart + (size_t)image * a.nunits * VSF_FAST_RS_STRIDE, 0, a.nunits * VSF_FAST_RS_STRIDE * 2, 0x00020000);
  const uint32_t rs_off = 2u * (uint32_t)((L.unit0 + unit_local) * VSF_FAST_RS_STRIDE);
  const bool rs_lane = PACK && valid && hl == 0;
  // PACK: the lanes of the lane's own cell, and those from its first lane on (64-bit lane masks as two halves)
  const int cfirst = lane - hl, cend = min(cfirst + nl, 64);
  const unsigned long long from_m = ~0ull << cfirst, cell_m = from_m & (cend >= 64 ? ~0ull : (1ull << cend) - 1ull);
  const uint32_t from_lo = (uint32_t)from_m, from_hi = (uint32_t)(from_m >> 32);
  const uint32_t cell_lo = (uint32_t)cell_m, cell_hi = (uint32_t)(cell_m >> 32);
  // MASK: the image's block (wave-uniform), this lane's 4 bytes of cell row 0 in it; reads outside the block return 0
  // (the pair's two pointers are read into values first: a choice between the two FIELDS put them on the stack)
  const uint8_t* mk_block = nullptr;
  if constexpr (MASK) {
    const uint8_t* const mk_even = a.mask.even;
    const uint8_t* const mk_odd = a.mask.odd;
    const uint8_t* const* const mk_table = a.mask.table;
    mk_block = ((image + a.mask.parity) & 1) ? mk_odd : mk_even;
    if (mk_table) mk_block = mk_table[image];
  }
  const bool mk_has = mk_block != nullptr;
  const __amdgpu_buffer_rsrc_t mk_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(mk_block), 0, MASK && mk_has ? a.mask.bytes : 0u, 0x00020000);
  const int mk_pitch = L.pitch;
  // (a lane whose dword is not inside a row of the level gets an offset beyond any block: it emits nothing)
  const uint32_t mk_base = valid && c0 >= 0 && c0 + 3 < mk_pitch ? L.offset + (uint32_t)(c0 + ys * mk_pitch) : 0x40000000u;

  // buffer loads: a lane's column offset sits in a VGPR, the row offset in an SGPR (PACK: both per lane, the row clamp
  // folded into the range of q); reads outside the level return 0
  const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(src), 0, src_bytes, 0x00020000);
  // (a lane outside the row gets an offset beyond the buffer instead of a branch around the load: no divergent control
  // flow, so the row offset stays in an SGPR)
  const uint32_t col_off = loadable ? (uint32_t)c0 : 0xFFFFFFF0u;
  const int qlo = 1 - ys, qhi = hrow - ys;  // 0 <= ys - 1 + q <= hrow - 1
  const uint32_t rbase = loadable ? (level == 0 ? 0u : L.offset) + (uint32_t)(c0 + (ys - 1) * pitch) : 0x40000000u;
  auto load_row = [&](int q) -> uint32_t {  // row ys - 1 + q of this lane's cell
    if (PACK)
      return __builtin_amdgcn_raw_buffer_load_b32(src_rsrc, rbase + (uint32_t)__mul24(min(max(q, qlo), qhi), pitch), 0u,
                                                  0);  // (full-rate multiply)
    const int yc = min(max(ys - 1 + q, 0), hrow - 1);
    return __builtin_amdgcn_raw_buffer_load_b32(src_rsrc, col_off, (uint32_t)(yc * pitch), 0);
  };

  const unsigned long long scorable = __builtin_amdgcn_ballot_w64((sm02 | sm13) != 0u);
  const v2s zero2 = {0, 0};
  ScoreRow S0 = make_score_row(zero2, zero2), S1 = S0, S2 = S0;  // score rows rotate through three sets: q-2, q-1, q
  int count = 0;       // candidates emitted so far by the cell (wave-uniform unless PACK)
  uint32_t my_rs = 0;  // (one cell) lane hl keeps rowstart[hl] of the cell
  // (cell row, first column, score offset) of an emitted candidate: score << 24 | y << 12 | x
  const uint32_t yx0 = ((uint32_t)ys << 12) + (uint32_t)c0 + ((uint32_t)(NMS ? offs - 1 : 0) << 24);
  // rank among the cell's lanes: v_mbcnt counts the set bits below this lane (two instructions per ballot, chained through
  // the accumulator); PACK counts those of the lane's own cell only, and adds the cell's bits to its count
  auto below = [&](unsigned long long b, int acc) -> int {
    if (PACK)
      return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32) & from_hi,
                                            __builtin_amdgcn_mbcnt_lo((uint32_t)b & from_lo, (uint32_t)acc));
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, (uint32_t)acc));
  };
  auto in_cell = [&](unsigned long long b) -> int {
    if (PACK) return __popc((uint32_t)b & cell_lo) + __popc((uint32_t)(b >> 32) & cell_hi);
    return __popcll(b);
  };

  // One step: scores of cell row q - 1 (image row ys - 1 + q) from the window R0..R6 = image rows ys - 4 + q .. ys + 2 + q,
  // then NMS + emission of cell row q - 2.
  auto step = [&](int q, const RowP& R0, const RowP& R1, const RowP& R2, const RowP& R3, const RowP& R4,
                  const RowP& R5, RowP& R6, const ScoreRow& S_up, const ScoreRow& S_mid, ScoreRow& S_dn) {
    prep_row(R6);  // the row that has just entered the window
    uint32_t mk = 0;  // MASK: the mask bytes of this lane's 4 pixels of cell row q - 2
    if constexpr (MASK) {
      if (q >= 2 && q - 2 < nrows0)
        mk = PACK ? __builtin_amdgcn_raw_buffer_load_b32(mk_rsrc, mk_base + (uint32_t)__mul24(q - 2, mk_pitch), 0u, 0)
                  : __builtin_amdgcn_raw_buffer_load_b32(mk_rsrc, mk_base, (uint32_t)((q - 2) * mk_pitch), 0);
    }
    v2s s02 = zero2, s13 = zero2;
    const int sy = ys - 1 + q;
    const bool row_ok = sy >= 3 && sy < hrow - 3;  // (wave-uniform unless PACK; PACK tests it only where a cell needs it)
    // a 9-arc contains circle pixel 0 (row sy+3) or 8 (row sy-3), both in the centre pixel's column
    const uint32_t far = max(__builtin_amdgcn_sad_u8(R0.d, R3.d, 0u), __builtin_amdgcn_sad_u8(R6.d, R3.d, 0u));
    // (one v_cmp; the lanes that may score at all are a ballot taken once, the row test is scalar unless PACK)
    unsigned long long want = __builtin_amdgcn_ballot_w64(far > (uint32_t)t) & scorable;
    if (PACK) {
      if (rim) want &= __builtin_amdgcn_ballot_w64(row_ok);
    } else {
      want &= row_ok ? ~0ull : 0ull;
    }
    if (want != 0ull) {
      s02 = score_pair0<NMS>(R0, R1, R2, R3, R4, R5, R6, toff);  // pixels 0 and 2
      s13 = score_pair1<NMS>(R0, R1, R2, R3, R4, R5, R6, toff);  // pixels 1 and 3
      if (PACK && rim) {
        s02 = as_v2s(as_u32(s02) & (row_ok ? sm02 : 0u));
        s13 = as_v2s(as_u32(s13) & (row_ok ? sm13 : 0u));
      } else {
        s02 = as_v2s(as_u32(s02) & sm02);
        s13 = as_v2s(as_u32(s13) & sm13);
      }
    }
    S_dn = make_score_row(s02, s13);
    const int r = q - 2;  // cell row to emit
    if (r >= 0 && r < nrows0) {
      if (__any((as_u32(S_mid.s02) | as_u32(S_mid.s13)) != 0)) {
        // keep iff score > every 8-neighbour (strict); without NMS every marked corner is kept.  k02 / k13: the score (or
        // marker) of a survivor, 0 elsewhere.
        uint32_t k02, k13;
        if (NMS) {
          const v2s nb02 = vmax3(S_up.h3a, S_dn.h3a, S_mid.h2a), nb13 = vmax3(S_up.h3b, S_dn.h3b, S_mid.h2b);
          k02 = as_u32((nb02 - S_mid.s02) >> 15) & as_u32(S_mid.s02) & em02;  // (all ones where the score exceeds nb)
          k13 = as_u32((nb13 - S_mid.s13) >> 15) & as_u32(S_mid.s13) & em13;
        } else {
          k02 = as_u32(S_mid.s02) & em02;
          k13 = as_u32(S_mid.s13) & em13;
        }
        if (PACK && mixed && r >= nrows) k02 = k13 = 0;  // (a cell of the item may have fewer rows)
        if constexpr (MASK) {  // bytes 0 / 2 and 1 / 3 spread over the halves of the pair layout
          k02 &= mk_has ? __builtin_amdgcn_perm(0u, mk, 0x02020000u) : ~0u;
          k13 &= mk_has ? __builtin_amdgcn_perm(0u, mk, 0x03030101u) : ~0u;
        }
        const uint32_t yx = yx0 + ((uint32_t)r << 12);
        if (NMS) {
          // Strict NMS: two neighbouring pixels cannot both survive, so at most one of pixels 0 / 1 and at most one of
          // pixels 2 / 3 -- slot A (the low halves) and slot B (the high halves), in raster order: two ballots / ranks /
          // stores instead of four.  kk = (score of slot A, score of slot B).
          const uint32_t kk = k02 | k13;
          const bool hasA = (kk & 0xFFFFu) != 0u, hasB = (kk >> 16) != 0u;
          const unsigned long long bA = __ballot(hasA), bB = __ballot(hasB);
          if ((bA | bB) != 0ull) {  // wave-uniform
            const int pos = below(bB, below(bA, count));
            // entry = (score + offs - 1) << 24 | y << 12 | x;  x = c0 + (0 or 1) for slot A, c0 + 2 + (0 or 1) for slot B
            const uint32_t eA = (kk << 24) + yx + ((k13 & 0xFFFFu) != 0u ? 1u : 0u);
            const uint32_t eB = ((kk & 0xFFFF0000u) << 8) + yx + 2u + ((k13 >> 16) != 0u ? 1u : 0u);
            const int posB = pos + (hasA ? 1 : 0);
            if (hasA && (!PACK || pos < seg_cap)) __builtin_amdgcn_raw_buffer_store_b32(eA, seg_rsrc, seg_off + 4u * (uint32_t)pos, 0, 0);
            if (hasB && (!PACK || posB < seg_cap)) __builtin_amdgcn_raw_buffer_store_b32(eB, seg_rsrc, seg_off + 4u * (uint32_t)posB, 0, 0);
            count += in_cell(bA) + in_cell(bB);
          }
        } else {
          const bool k0 = (k02 & 0xFFFFu) != 0, k1 = (k13 & 0xFFFFu) != 0, k2 = (k02 >> 16) != 0, k3 = (k13 >> 16) != 0;
          const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1), b2 = __ballot(k2), b3 = __ballot(k3);
          if ((b0 | b1 | b2 | b3) != 0ull) {  // wave-uniform
            int pos = below(b3, below(b2, below(b1, below(b0, count))));
            // (without NMS cv::FAST_t leaves the response at 0)
            if (k0) {
              if (!PACK || pos < seg_cap) __builtin_amdgcn_raw_buffer_store_b32(yx, seg_rsrc, seg_off + 4u * (uint32_t)pos, 0, 0);
              ++pos;
            }
            if (k1) {
              if (!PACK || pos < seg_cap) __builtin_amdgcn_raw_buffer_store_b32(yx + 1, seg_rsrc, seg_off + 4u * (uint32_t)pos, 0, 0);
              ++pos;
            }
            if (k2) {
              if (!PACK || pos < seg_cap) __builtin_amdgcn_raw_buffer_store_b32(yx + 2, seg_rsrc, seg_off + 4u * (uint32_t)pos, 0, 0);
              ++pos;
            }
            if (k3) {
              if (!PACK || pos < seg_cap) __builtin_amdgcn_raw_buffer_store_b32(yx + 3, seg_rsrc, seg_off + 4u * (uint32_t)pos, 0, 0);
            }
            count += in_cell(b0) + in_cell(b1) + in_cell(b2) + in_cell(b3);
          }
        }
      }
      // rowstart[r + 1] of the cell (rowstart[0] = 0 and rowstart[SR], the cell's total, are written after the march)
      if (r + 1 < SR) {
        if (PACK) {
          if (rs_lane)
            __builtin_amdgcn_raw_buffer_store_b16((unsigned short)min(count, seg_cap), rs_rsrc, rs_off, 2u * (uint32_t)(r + 1), 0);
        } else {
          // the running count goes into lane r + 1 (v_writelane: one instruction; lane select through M0: the value
          // already takes the instruction's one constant-bus slot)
          asm("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0" : "+v"(my_rs) : "s"(min(count, seg_cap)), "s"(r + 1));
        }
      }
    }
  };

  // NINE rotating register sets hold image rows: step q reads rows (ys - 4 + q) .. (ys + 2 + q) from sets q .. q + 6
  // (mod 9), set q + 7 already holds the next row's dword and the row after that is requested into set q + 8 -- the set
  // whose row the previous step used last.  The loop body is nine steps, a multiple of the three score-row sets' period, so
  // neither the image rows nor the score rows are ever copied between registers (a period of seven cost 17 v_mov per step).
  // q runs over 0 .. nrows0 + 1 (score rows ys - 1 .. ys + nrows0).
  RowP A0, A1, A2, A3, A4, A5, A6, A7, A8;
  A0.d = load_row(-3), A1.d = load_row(-2), A2.d = load_row(-1), A3.d = load_row(0), A4.d = load_row(1), A5.d = load_row(2),
  A6.d = load_row(3), A7.d = load_row(4);
  prep_row(A0), prep_row(A1), prep_row(A2), prep_row(A3), prep_row(A4), prep_row(A5);
  const int qe = nrows0 + 1;
#define VSF_FAST_STEP(j, r0, r1, r2, r3, r4, r5, r6, ld, su, sm, sd) \
  if (q + (j) > qe) break;                                             \
  ld.d = load_row(q + (j) + 5);                                        \
  step(q + (j), r0, r1, r2, r3, r4, r5, r6, su, sm, sd);
  for (int q = 0;; q += 9) {
    VSF_FAST_STEP(0, A0, A1, A2, A3, A4, A5, A6, A8, S0, S1, S2)
    VSF_FAST_STEP(1, A1, A2, A3, A4, A5, A6, A7, A0, S1, S2, S0)
    VSF_FAST_STEP(2, A2, A3, A4, A5, A6, A7, A8, A1, S2, S0, S1)
    VSF_FAST_STEP(3, A3, A4, A5, A6, A7, A8, A0, A2, S0, S1, S2)
    VSF_FAST_STEP(4, A4, A5, A6, A7, A8, A0, A1, A3, S1, S2, S0)
    VSF_FAST_STEP(5, A5, A6, A7, A8, A0, A1, A2, A4, S2, S0, S1)
    VSF_FAST_STEP(6, A6, A7, A8, A0, A1, A2, A3, A5, S0, S1, S2)
    VSF_FAST_STEP(7, A7, A8, A0, A1, A2, A3, A4, A6, S1, S2, S0)
    VSF_FAST_STEP(8, A8, A0, A1, A2, A3, A4, A5, A7, S2, S0, S1)
  }
#undef VSF_FAST_STEP
  if (PACK) {
    if (rs_lane) {
      rs[0] = 0;
      rs[SR] = (uint16_t)min(count, seg_cap);
    }
  } else {
    if (hl < SR) rs[hl] = (uint16_t)my_rs;                 // rowstart[0 .. SR-1]
    if (hl == 0) rs[SR] = (uint16_t)min(count, seg_cap);   // rowstart[SR] = cell total
  }
}

// (`first`: the launch walks work items [first, first + nwork) -- the list of full cells may be cut in two,
// vsf_fast_split.h; 0 for the packed items)
template <bool PACK, bool NMS, bool MASK>
__global__ __launch_bounds__(256) void fast_march_kernel(FastArgs a, int first, int nwork) {
  const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (item >= nwork) return;  // wave-uniform
  fast_march_body<PACK, NMS, MASK>(a, first + item, blockIdx.y);
}

// Full cells and the packed items in ONE launch, for batches that leave the chip nearly empty: there a launch lasts as
// long as one cell's march, and two launches in a row last twice that.
template <bool NMS, bool MASK>
__global__ __launch_bounds__(256) void fast_march_both_kernel(FastArgs a, int first, int nfull, int npack) {
  const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (item >= nfull + npack) return;  // wave-uniform
  if (item < nfull)
    fast_march_body<false, NMS, MASK>(a, first + item, blockIdx.y);
  else
    fast_march_body<true, NMS, MASK>(a, item - nfull, blockIdx.y);
}

// The same cells walked by ONE resident workgroup per CU (4 x `waves per SIMD` waves; a second one does not fit beside it, so
// every CU gets its share -- four-wave workgroups were packed five to a CU on some CUs and none on others).  For the batched
// calls that run the blur beside FAST: a grid of one workgroup per four cells occupies every register of the chip for as
// long as cells are left and whatever else is queued waits behind it; a fixed set of resident waves leaves the rest of each
// SIMD's registers to the kernel beside it.  Alone, FAST reaches 93 % of the vector ALU's issue rate with five waves per
// SIMD, the same with four, 92 % of that with three and 76 % with two (occupancy sweep, NOTES.md section 6).
template <bool PACK, bool NMS, bool MASK>
__global__ __launch_bounds__(1024) void fast_march_resident_kernel(FastArgs a, int first, int nwork, int nimages,
                                                                  uint32_t* next_cell) {
  // cells are handed out through a counter (zeroed by the launcher): a wave slowed down by its neighbours takes fewer
  const int total = nwork * nimages;
  while (true) {  // (wave-uniform; the counter passes `total` for every wave)
    // one atomic per wave, issued with the execution mask narrowed to lane 0 inside one asm statement: straight-line code
    // for the compiler (an `if (lane == 0)` in front of a uniform loop exit left it structurising a divergent loop)
    uint32_t r;
    asm volatile(
        "s_mov_b64 s[34:35], exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_add %0, %1, %2, %3 sc0\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_mov_b64 exec, s[34:35]"
        : "=&v"(r)
        : "v"(0u), "v"(1u), "s"(next_cell)
        : "memory", "s34", "s35");
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
    if (u >= (uint32_t)total) break;
    const int image = (int)u / nwork, cell = (int)u - image * nwork;
    fast_march_body<PACK, NMS, MASK>(a, first + cell, image);
  }
}

// Standalone FAST detect: unit segments -> contiguous cv::KeyPoint list in raster order.
__global__ __launch_bounds__(256) void fast_emit_kernel(const VsfLevel* __restrict__ levels,
                                                        const uint32_t* __restrict__ cand, uint32_t cand_entries,
                                                        const uint16_t* __restrict__ rowstart, int nunits,
                                                        int max_keypoints, vsf_keypoint* __restrict__ out,
                                                        int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ int cellpre[2048 + 8];
  __shared__ __attribute__((aligned(4))) uint16_t rs_lds[64 * VSF_FAST_RS_STRIDE];
  __shared__ int lds4[4];
  const int image = blockIdx.x;
  const VsfLevel L = levels[0];
  const uint16_t* rs_img = rowstart + (size_t)image * nunits * VSF_FAST_RS_STRIDE;
  const uint32_t* cand_img = cand + (size_t)image * cand_entries;
  vsf_keypoint* o = out + (size_t)image * max_keypoints;
  const int n = vsf_gather_level<256>(L, cand_img, rs_img, cellpre, 2048, rs_lds, 64, lds4, [](int) {}, [&](int dst, uint32_t cd) {
    if (dst < max_keypoints) {
      vsf_keypoint kp;
      kp.x = (float)VSF_CAND_X(cd);
      kp.y = (float)VSF_CAND_Y(cd);
      kp.size = 7.f;
      kp.angle = -1.f;
      kp.response = (float)VSF_CAND_SCORE(cd);
      kp.octave = 0;
      kp.class_id = -1;
      o[dst] = kp;
    }
  });
  if (threadIdx.x == 0) {
    counts[image] = n;  // true count; the caller clamps to its capacity
    if (n > max_keypoints) atomicOr(status, 1);
  }
}

}  // namespace

namespace {

// The launches of one FAST pass, for kernels with (MASK) or without the mask predicate.
template <bool MASK>
void launch_fast_forms(const FastArgs& a, const VsfDev& d, const VsfImages& im, int nms, hipStream_t s, int resident_waves_per_simd,
                       int n_cus, uint32_t* d_cell_counters, int part, int f0, int nf, int np) {
  if (resident_waves_per_simd > 0 && resident_waves_per_simd <= 4 && nms && d_cell_counters) {
    // (an early part runs on another stream than the late part of the call before it: a counter of its own)
    uint32_t* cnt = part == VSF_FAST_EARLY ? d_cell_counters + 2 : d_cell_counters;
    vsf_note(hipMemsetAsync(cnt, 0, (part == VSF_FAST_EARLY ? 1 : 2) * sizeof(uint32_t), s));
    const dim3 block(256 * resident_waves_per_simd);
    if (nf > 0)
      hipLaunchKernelGGL((fast_march_resident_kernel<false, true, MASK>), dim3(n_cus), block, 0, s, a, f0, nf, im.n, cnt);
    if (np > 0)
      hipLaunchKernelGGL((fast_march_resident_kernel<true, true, MASK>), dim3(n_cus), block, 0, s, a, 0, np, im.n, cnt + 1);
    return;
  }
  const dim3 gf((nf + 3) / 4, im.n), gp((np + 3) / 4, im.n);
  const int both_max = d.tune ? d.tune->fast_both_max : 16;
  if (im.n <= both_max && nf > 0 && np > 0) {
    const dim3 gb((nf + np + 3) / 4, im.n);
    if (nms)
      hipLaunchKernelGGL((fast_march_both_kernel<true, MASK>), gb, dim3(256), 0, s, a, f0, nf, np);
    else
      hipLaunchKernelGGL((fast_march_both_kernel<false, MASK>), gb, dim3(256), 0, s, a, f0, nf, np);
    return;
  }
  if (nms) {
    if (nf > 0) hipLaunchKernelGGL((fast_march_kernel<false, true, MASK>), gf, dim3(256), 0, s, a, f0, nf);
    if (np > 0) hipLaunchKernelGGL((fast_march_kernel<true, true, MASK>), gp, dim3(256), 0, s, a, 0, np);
  } else {
    if (nf > 0) hipLaunchKernelGGL((fast_march_kernel<false, false, MASK>), gf, dim3(256), 0, s, a, f0, nf);
    if (np > 0) hipLaunchKernelGGL((fast_march_kernel<true, false, MASK>), gp, dim3(256), 0, s, a, 0, np);
  }
}

}  // namespace

void vsf_launch_fast(const VsfDev& d, const VsfGeom& g, const VsfImages& im, int threshold, int nms, hipStream_t s,
                     int resident_waves_per_simd, int n_cus, uint32_t* d_cell_counters, int part, int n_early,
                     const VsfFastMask* mask) {
  // the work of this launch: full cells [f0, f0 + nf) and np packed items
  n_early = std::min(std::max(n_early, 0), g.nwork_full);
  const int f0 = part == VSF_FAST_LATE ? n_early : 0;
  const int nf = part == VSF_FAST_EARLY ? n_early : g.nwork_full - f0;
  const int np = part == VSF_FAST_EARLY ? 0 : g.nwork_pack;
  FastArgs a;
  a.levels = d.levels;
  a.units = d.units;
  a.nwork_full = g.nwork_full;
  a.nunits = g.nunits;
  a.img0 = im.base;
  a.img0_stride = im.image_stride;
  a.img0_pitch = (int)im.row_stride;
  a.pyr = d.pyr;
  a.pyr_bytes = g.pyr_bytes;
  a.cand = d.cand;
  a.cand_entries = g.cand_entries;
  a.rowstart = d.rowstart;
  a.threshold = threshold;
  a.nms = nms;
  a.mask = mask ? *mask : VsfFastMask{};
  // the kernels with the predicate only where an image of the launch may have a mask: every other launch is the one it was
  if (a.mask.table || a.mask.even || a.mask.odd)
    launch_fast_forms<true>(a, d, im, nms, s, resident_waves_per_simd, n_cus, d_cell_counters, part, f0, nf, np);
  else
    launch_fast_forms<false>(a, d, im, nms, s, resident_waves_per_simd, n_cus, d_cell_counters, part, f0, nf, np);
}

void vsf_launch_fast_emit(const VsfDev& d, const VsfGeom& g, int n_images, int max_keypoints, vsf_keypoint* d_kp,
                          int32_t* d_counts, hipStream_t s) {
  hipLaunchKernelGGL(fast_emit_kernel, dim3(n_images), dim3(256), 0, s, d.levels, d.cand, g.cand_entries, d.rowstart,
                     g.nunits, max_keypoints, d_kp, d_counts, d.status);
}
