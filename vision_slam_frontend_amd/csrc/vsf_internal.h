// vsf_internal.h -- structures shared by the host side of the C ABI and the gfx950 kernels.
#ifndef VSF_INTERNAL_H_
#define VSF_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vsf.h"
#include "vsf_own.h"     // DevBuf, PinnedBuf, Event, Stream
#include "vsf_fast_split.h"  // which FAST cells are full waves, and where their list is cut by level
#include "vsf_world_points.h"  // the point cloud's arithmetic, shared with the host's AddFeaturePoints
#include "vsf_resize.h"  // VsfTap, the resize coefficient formula, the packing plan

// FAST march kernel: a wave owns a band of 248 keypoint columns (lanes 1..62 x 4 px; lanes 0 and 63 carry the raw halo
// pixels and score the ONE pixel next to the band -- lane 0's last, lane 63's first: their circles reach no further than
// the lane's own dword and its inner neighbour's -- which is all the NMS of the band's edge columns needs) x a strip of 32
// rows.  (Rounds 1-3: 240 columns, lanes 1 and 62 scored four pixels each for the sake of one.)
#define VSF_FAST_BAND_COLS 248
// Cells narrower than a band (a level's last band) share waves: a packed work item is a list of up to VSF_FAST_PACK_SEGS
// segments, each one cell on ceil(cols / 4) + 2 consecutive lanes (its own two halo lanes included).  Item layout
// (VSF_FAST_PACK_WORDS dwords): nseg, rows (the wave's row count: its tallest cell's), mixed (1: a cell has fewer rows),
// rim (1: a cell's score rows reach FAST's 3-pixel rim, so the row test is per lane), then per segment
// level << 24 | band << 16 | strip and first lane | lanes << 8 | rows << 16.
#define VSF_FAST_PACK_SEGS 8
#define VSF_FAST_PACK_WORDS (4 + 2 * VSF_FAST_PACK_SEGS)
#define VSF_FAST_STRIP_ROWS 32
#define VSF_FAST_RS_STRIDE (VSF_FAST_STRIP_ROWS + 2)  // u16 row-start table per unit (SR + 1 used)
static_assert(VSF_FAST_SPLIT_BAND_COLS == VSF_FAST_BAND_COLS && VSF_FAST_SPLIT_STRIP_ROWS == VSF_FAST_STRIP_ROWS,
              "vsf_fast_split.h states the cell size for itself");
#define VSF_BLUR_MMA_ROWS 26     // output rows per step of the matrix-core blur (32 loaded rows - 2 x 3 halo rows)
#define VSF_BLUR_MMA_STEPS 16    // double steps (52 rows) per unit: a workgroup walks this many blocks down its band pair
#define VSF_BLUR_MMA_STEPS_SMALL 2  // ... for batches below 32 images
// The blurred levels are stored in tiles of 4 rows x 32 bytes (= one 128-byte cache line), tiles in row-major order:
// the descriptor kernel gathers 39 x 39 windows from them and a window then touches ~24 lines instead of 39..78,
// while the blur kernel still writes whole 32-byte sectors (8 lanes x 4 bytes).
// Byte offset of pixel (x, y) inside a level of row pitch `pitch` (a multiple of 64; rows padded to a multiple of 8):
#define VSF_BLUR_TILE_OFFSET(pitch, x, y) \
  ((uint32_t)((y) >> 2) * (uint32_t)((pitch) * 4) + ((uint32_t)((x) >> 5) << 7) + ((uint32_t)((y) & 3) << 5) + (uint32_t)((x) & 31))
#define VSF_SORT_LDS_ROWS 4096   // matches of one pair sorted in LDS (8 B each); larger pairs sort in HBM scratch
#define VSF_IC_ITEMS 320         // ICAngles disc items per byte phase: 31 rows x 9 dwords = 279, padded to 5 x 64

// ---- pyramid level descriptor (device-resident table, read through scalar loads) ----
struct VsfLevel {
  int32_t w, h;            // level size (cv::ORB layer size)
  int32_t pitch;           // bytes per row in the pyramid buffers (multiple of 64)
  uint32_t offset;         // byte offset of row 0 inside one image's pyramid block
  float scale;             // layerScale[level]
  int32_t nfeatures;       // per-level budget n_l
  int32_t x_lo, x_hi;      // keypoints may sit at x_lo <= x < x_hi  (runByImageBorder / FAST rim)
  int32_t y_lo, y_hi;
  int32_t fast_a0;         // x_lo rounded down to a multiple of 4: column origin of band 0
  int32_t nbands, nstrips; // FAST units of this level: unit = strip * nbands + band
  int32_t unit0;           // index of this level's first unit (per image)
  uint32_t cand_offset;    // u32 index of this level's first candidate segment (per image)
  int32_t seg_cap;         // capacity of one unit's candidate segment
  int32_t kp_offset;       // index of this level's final-keypoint segment (per image)
  int32_t kp_cap;          // its capacity (vsf_level_kp_cap)
  int32_t blur_vec_end;    // columns [0, blur_vec_end) round half-even (SSE2 path), the rest half-up
  uint32_t xtab, ytab;     // entry offsets of this level's resize tables in the host-side Geometry (level >= 1)
  int32_t resize_rows;     // largest strip height (16, 8, 4) the shared-row resize kernel may use for this level, or 0
  int32_t resize_any8;     // 1: an 8-row strip starting at ANY row stays inside 10 consecutive source rows
  uint32_t rscale_x[2], rscale_y[2];  // bit patterns of cv::resize's double scale_x / scale_y from level - 1 (host-computed)
  uint32_t blur_tcol;      // matrix-core blur: index of this level's first pass-1 operand (4 per 64-column band) in the table
};

// Candidate keypoint, 32 bit: score << 24 | y << 12 | x   (level coordinates, x,y < 4096)
#define VSF_CAND_PACK(x, y, s) (((uint32_t)(s) << 24) | ((uint32_t)(y) << 12) | (uint32_t)(x))
#define VSF_CAND_X(c) ((int)((c)&0xFFFu))
#define VSF_CAND_Y(c) ((int)(((c) >> 12) & 0xFFFu))
#define VSF_CAND_SCORE(c) ((int)((c) >> 24))

// Final per-level keypoint record (level coordinates).
struct VsfLevelKp {
  uint32_t xy;  // y << 12 | x
  float response;
  float angle;     // degrees (k_describe.hip orb_angle_kernel)
  float ca, sb;    // cos / sin of the angle as computeOrbDescriptors takes them
};

// Records one level's segment of VsfDev::lvlkp holds (include/vsf.h, vsf_params::score_type, states the rule).
// HARRIS_SCORE: the first cut's 2 n_l and room for its ties; the second cut's ties sit on a float and are rare.
// FAST_SCORE: the one cut sits on an 8-bit key, so ties are the rule: n_l and the whole headroom the caller bought for the
// image (max_keypoints - nfeatures; max_keypoints <= 0 stands for its default, nfeatures + 256).
inline int vsf_level_kp_cap(int score_type, int n_l, int nfeatures, int max_keypoints) {
  if (score_type != 1) return 2 * n_l + 64;
  const long mk = max_keypoints > 0 ? (long)max_keypoints : (long)nfeatures + 256;
  const long room = mk - nfeatures;
  return n_l + (int)(room > 0 ? room : 0);
}

struct VsfGeom {
  int nlevels;
  int width, height;
  uint32_t pyr_bytes;       // one image's pyramid block
  uint32_t cand_entries;    // one image's candidate buffer (u32 entries)
  int nunits;               // FAST cells (32-row strip x 240-column band) per image
  int nwork_full, nwork_pack;  // FAST work items: waves covering one cell / packed items of narrow cells
  int fast_split_levels;       // levels 0 .. this - 1 have full cells: the most VSF_OPT_FAST_EARLY_LEVELS can mean (vsf_fast_split.h)
  int lvlkp_entries;        // one image's level-keypoint buffer (VsfLevelKp entries)
  int score_type;           // vsf_params::score_type of an ORB geometry (0 HARRIS_SCORE, 1 FAST_SCORE): the selection's form
  uint64_t pyramid_pixels;
};

// Per-context launch choices (vsf_set_option / vsf_get_option; the defaults are what the measurements of NOTES.md
// section 6 settled on).  Nothing in the library reads the environment: a switch is a call on a context.
struct VsfTuning {
  int fast_both_max = 16;  // VSF_OPT_FAST_BOTH_MAX: largest batch (images) whose full and packed FAST work items share one launch
  int select_wide = 1;     // VSF_OPT_SELECT_WIDE: 1 = a frame or two takes the 1024-thread whole-level selection class
  int pipe_priority = 0;     // VSF_OPT_PIPE_PRIORITY: stream priority of the pipelined pyramid chain (0 normal, 1 lowest, -1 highest)
  int pipe_after_fast = 1;   // VSF_OPT_PIPE_AFTER_FAST: the pipelined pyramid of call k + 1 starts behind call k's FAST (1) or at once (0)
  int select_big_class = 1;  // VSF_OPT_SELECT_BIG_CLASS: 1 = the widest levels of a batch take the 9 216-entry class
  int fast_early_levels = 12;  // VSF_OPT_FAST_EARLY_LEVELS: a pipelined call starts FAST on the full cells of this many levels from
                               // inside its pyramid chain, beside the previous call's selection / descriptors (0: one FAST pass;
                               // 12, as a grid: NOTES.md "FAST: the wide levels start beside the previous call")
  int fast_early_form = 0;    // VSF_OPT_FAST_EARLY_FORM: that early launch as a grid (0) or resident with 1..3 waves per SIMD
  int blur_early = 1;         // VSF_OPT_BLUR_EARLY: 1 = a pipelined call's blur follows its pyramid chain on the pipe stream, in front of
                              // its late FAST part, into the other blurred pyramid; 0: forked from the main stream beside FAST
                              // (NOTES.md "Blur: behind the pipelined pyramid chain")
  int jpeg_serial = 0;     // 1: every file through the one-wave-per-image decoder (set when the parallel decoder's LDS is refused)
  int pyramid_few = 16;    // VSF_OPT_PYRAMID_FEW: largest batch (images) that takes the slab kernel for every level
  int pyramid_chain = 8;   // VSF_OPT_PYRAMID_CHAIN: levels per slab launch (0: keep the per-level launches)
  int pyramid_rows = 6;    // VSF_OPT_PYRAMID_ROWS: rows of the chain's last level per slab
  int pyramid_tail_min = 0;  // VSF_OPT_PYRAMID_TAIL_MIN: smallest batch (images) whose one-band levels take the image-major kernel whatever
                             // share of the chip it fills (0: only batches that fill three quarters of a round of workgroups)
  int observe_copy_thread = 1;  // VSF_OPT_OBSERVE_COPY_THREAD: a helper thread takes the right image's staging copy while frames stream in
  int observe_thread = 0;  // VSF_OPT_OBSERVE_THREAD: 1 = an ObserveImage queue of depth >= 4 gets a launcher thread
  int lds_limit = 0;       // largest dynamic LDS a workgroup may ask for on this device (queried at vsf_create)
};

// First HIP error a launcher or a stream-plumbing helper met since the last check (host thread-local: a context is driven
// by one host thread at a time).  Launchers return void; they hand failures to vsf_note() and the entry point that called
// them turns the noted error into VSF_ERR_HIP (VSF_STICKY in vsf_api.hip) -- a failed event wait would otherwise silently
// remove an ordering edge between two kernels.
extern thread_local int vsf_tls_hip_error;
inline void vsf_note(hipError_t e) {
  if (e != hipSuccess && vsf_tls_hip_error == 0) vsf_tls_hip_error = (int)e;
}
// What vsf_comm.hip needs of a context (vsf_ctx is private to vsf_api.hip).
hipStream_t vsf_ctx_stream(const vsf_ctx* ctx);
int vsf_ctx_device(const vsf_ctx* ctx);
void vsf_ctx_set_last_error(vsf_ctx* ctx, int code);  // what vsf_last_hip_error returns
constexpr int VSF_RCCL_ERROR_BASE = 10000;             // vsf_last_hip_error = 10000 + ncclResult_t after a failed RCCL call
// An error a launcher noted belongs to the CONTEXT whose entry point was running.  Every public entry point holds one of
// these: on the way out -- early returns included -- whatever is still noted in the thread's slot moves into the context
// (vsf_ctx::pending_hip) and is returned by that context's next checking call (VSF_STICKY), never by another context that
// happens to be driven from the same host thread.
void vsf_ctx_absorb_noted_error(vsf_ctx* ctx);
// ... and on the way IN every entry point but the ObserveImage queue's own first sends what waits in that queue, so that
// nothing else ever runs beside the queue's launcher thread (vsf_observe.hip).
void vsf_ctx_enter(vsf_ctx* ctx);
struct VsfErrorScope {
  vsf_ctx* ctx;
  explicit VsfErrorScope(vsf_ctx* c, bool enter = true) : ctx(c) {
    if (ctx && enter) vsf_ctx_enter(ctx);
  }
  ~VsfErrorScope() {
    if (ctx && vsf_tls_hip_error != 0) vsf_ctx_absorb_noted_error(ctx);
  }
  VsfErrorScope(const VsfErrorScope&) = delete;
  VsfErrorScope& operator=(const VsfErrorScope&) = delete;
};
// Raises the dynamic-LDS limit of the kernels that need more than the default 64 KB (k_frontend / k_pyramid / k_jpeg);
// called once per context creation, checked.
hipError_t vsf_prepare_sort_kernels(int lds_limit);
hipError_t vsf_prepare_pyramid_kernels(int lds_limit);
hipError_t vsf_prepare_jpeg_kernels(int lds_limit);

// Kernel launchers (implemented in the k_*.hip files). All asynchronous on `s`.
struct VsfDev {
  const VsfLevel* levels;   // [nlevels]
  const uint32_t* units;    // [nwork_full]: level << 24 | band << 16 | strip, then [nwork_pack][VSF_FAST_PACK_WORDS]
  uint8_t* pyr;             // [max_images][pyr_bytes]   unblurred levels 1..L-1 (level 0 is the input)
  uint8_t* blur;            // [max_images][pyr_bytes]   blurred levels 0..L-1
  uint32_t* cand;           // [max_images][cand_entries]  per-unit candidate segments (unit-local raster order)
  uint16_t* rowstart;       // [max_images][nunits][VSF_FAST_RS_STRIDE]  start of each row inside its segment
  uint32_t* scratch;        // [max_images][6 * cand_entries]   selection arrays, rank tables, masks when LDS is too small
  VsfLevelKp* lvlkp;        // [max_images][lvlkp_entries]
  const uint2* ic_table;    // [4][VSF_IC_ITEMS] ICAngles byte weights (k_describe.hip)
  int32_t* lvl_count;       // [max_images][nlevels]
  int32_t* status;          // device status word (bit 0: capacity overflow)
  int status_stride;        // 0: that one word; 1: status[image] (a batch of the ObserveImage queue: one word per image)
  const VsfTuning* tune;    // the context's launch choices (host memory)
};

struct VsfImages {
  const uint8_t* base;      // level-0 images
  size_t image_stride;
  size_t row_stride;
  int n;
};

// Optional extra streams a launcher may fork independent kernel chains onto (joined back before it returns).
#define VSF_SIDE_STREAMS 1
struct VsfSideStream {
  hipStream_t stream[VSF_SIDE_STREAMS];
  hipEvent_t fork, join[VSF_SIDE_STREAMS];
  int n;
};
void vsf_launch_bayer_bg_gray(const uint8_t* d_src, int n, int w, int h, size_t src_image_stride, int src_pitch,
                              uint8_t* d_dst, size_t dst_image_stride, int dst_pitch, hipStream_t s);
// ... and for every VSF_PIX_* format (RGGB: the launch above; MONO8: a copy); src_pitch >= w * bytes per pixel
void vsf_launch_to_gray(int pixfmt, const uint8_t* d_src, int n, int w, int h, size_t src_image_stride, int src_pitch,
                        uint8_t* d_dst, size_t dst_image_stride, int dst_pitch, hipStream_t s);
// `hook` (single chain only, side == NULL): called once, right behind the launch that produces level hook->level (0: before
// the first launch) -- the caller records an event there and starts work on the levels that exist by then.
struct VsfPyramidHook {
  int level;
  void (*fn)(void* arg, hipStream_t s);
  void* arg;
};
void vsf_launch_pyramid(const VsfDev& d, const VsfGeom& g, const VsfLevel* h_levels, const VsfImages& im,
                        hipStream_t s, const VsfSideStream* side, const VsfPyramidHook* hook = nullptr);
// threshold: FAST threshold; nms == 0 keeps every corner (standalone FAST only).
// d_cell_counters: [3] for the resident forms: full cells, packed items, full cells of an early part.
// part / n_early: VSF_FAST_ALL = every work item; VSF_FAST_EARLY = full cells [0, n_early) only; VSF_FAST_LATE = the full cells
// from n_early on and every packed item (the two parts together are the whole list: vsf_fast_split.h).
enum { VSF_FAST_ALL = 0, VSF_FAST_EARLY = 1, VSF_FAST_LATE = 2 };
// Detection masks of a launch's images (include/vsf.h "Detection masks"; k_mask.hip builds a slot's block: one byte a pixel,
// 0x00 / 0xFF, every level at its VsfLevel::offset and pitch of the ORB geometry -- level 0 included, which the stand-alone
// detector's one-level geometry shares).  Image i of the launch reads table[i] when there is a table (device-visible memory),
// else `odd` when parity + i is odd and `even` otherwise; a null block is no mask.  All null: the launch takes the kernels
// without the predicate.
struct VsfFastMask {
  const uint8_t* even = nullptr;
  const uint8_t* odd = nullptr;
  const uint8_t* const* table = nullptr;
  int parity = 0;
  uint32_t bytes = 0;  // of one block
};
void vsf_launch_fast(const VsfDev& d, const VsfGeom& g, const VsfImages& im, int threshold, int nms, hipStream_t s,
                     int resident_waves_per_simd = 0, int n_cus = 0, uint32_t* d_cell_counters = nullptr,
                     int part = VSF_FAST_ALL, int n_early = 0, const VsfFastMask* mask = nullptr);
// k_mask.hip: a slot's block from the caller's mask (w x h at any base address and pitch, device memory), level by level on `s`
// (h_levels: the ORB geometry's; d_block: pyr_bytes bytes).
void vsf_launch_mask_pyramid(const uint8_t* d_mask, size_t mask_pitch, const VsfLevel* h_levels, int nlevels, uint32_t block_bytes,
                             uint8_t* d_block, hipStream_t s);
void vsf_launch_select(const VsfDev& d, const VsfGeom& g, const VsfLevel* h_levels, const VsfImages& im,
                       hipStream_t s);
void vsf_launch_retain_best_test(uint2* d_data, uint32_t* d_tables, int n, int n_points, int use_lds, int mode,
                                 int* d_out_n, hipStream_t s);
// d_scratch: [6][cand_entries] words, as one image's share of VsfDev::scratch; false: no such form
bool vsf_launch_select_form_test(int form, uint32_t* d_scratch, uint32_t cand_entries, uint32_t cand_offset, int level_cap,
                                 int stage, int n, int n_points, int* d_out_n, hipStream_t s);
// Matrix-core blur (k_blur.hip, round 3): units = level << 24 | band pair << 16 | first double step << 8 | double steps.
void vsf_launch_blur_mma(const VsfDev& d, const VsfGeom& g, const VsfImages& im, const uint32_t* d_units, int nunits,
                         const uint4* d_tcol, const uint4* d_tv, int bias, hipStream_t s);
void vsf_launch_describe(const VsfDev& d, const VsfGeom& g, const VsfImages& im, int max_keypoints,
                         vsf_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts, hipStream_t s);
// Consecutive output keypoints per wave of one describe launch over n_images images (k_describe.hip has the measurements):
// eight needs a launch that still fills the chip with waves -- 512 images x 10 000 keypoints; 64-192 images of 8 000
// (1920x1080) run 1-2 % faster with four.  The one statement of the choice: the launcher and vsf_debug_describe_form read it.
inline int vsf_describe_kp_per_wave(int max_keypoints, int n_images) {
  return (max_keypoints >= 4096 && (long)n_images * max_keypoints >= 3000000L) ? 8 : 4;
}
void vsf_launch_fast_emit(const VsfDev& d, const VsfGeom& g, int n_images, int max_keypoints, vsf_keypoint* d_kp,
                          int32_t* d_counts, hipStream_t s);
void vsf_launch_knn2(const uint8_t* d_desc, const int32_t* d_counts, size_t set_stride, const int32_t* d_q_set,
                     const int32_t* d_t_set, int n_pairs, int max_rows, int32_t* d_idx2, int32_t* d_dist2,
                     hipStream_t s, int rows_hint = 0);  // rows_hint: expected rows per set (0: unknown), speed only
void vsf_launch_ratio_compact(const int32_t* d_counts, const int32_t* d_q_set, const int32_t* d_t_set, int n_pairs,
                              int max_rows, const int32_t* d_idx2, const int32_t* d_dist2, uint32_t ratio_num,
                              uint32_t ratio_shift, vsf_dmatch* d_matches, int32_t* d_nmatches, int32_t* d_status,
                              hipStream_t s);

// k_frontend.hip.  The fundamental matrix: h_F (host, 9 floats) travels by value in the kernel
// arguments; with h_F == NULL the kernel reads d_F (device-visible memory: vsf_observe's pinned per-call parameters).
struct VsfF9 {
  float v[9];
};
void vsf_launch_stereo_filter(const vsf_keypoint* d_kp, const uint8_t* d_desc, const vsf_dmatch* d_matches,
                              const int32_t* d_nmatches, int n_frames, int max_rows, const float* d_F, const float* h_F,
                              int order, const float* d_thr_override, float thr_in, float* d_residual, float* d_mean, float* d_thr,
                              vsf_keypoint* d_kp_out, uint8_t* d_desc_out, int32_t* d_counts_out, hipStream_t s);
void vsf_launch_stereo_residuals(const vsf_keypoint* d_kp, const vsf_dmatch* d_matches, const int32_t* d_nmatches,
                                 int n_frames, int max_rows, const float* d_F, const float* h_F, int order, float* d_residual,
                                 float* d_mean, hipStream_t s);
void vsf_launch_stereo_filter_only(const vsf_keypoint* d_kp, const uint8_t* d_desc, const vsf_dmatch* d_matches,
                                   const int32_t* d_nmatches, int n_frames, int max_rows, const float* d_residual,
                                   const float* d_thr, vsf_keypoint* d_kp_out, uint8_t* d_desc_out,
                                   int32_t* d_counts_out, hipStream_t s, const int32_t* d_out_sets = nullptr,
                                   int32_t* d_set_counts = nullptr);
// RemoveAmbigStereo of one frame in one launch (residuals, ordered mean, threshold hand-over through *d_thr_state, filter);
// false: the frame's capacity does not fit the kernel's LDS and nothing was launched.
bool vsf_launch_stereo_one_frame(const vsf_keypoint* d_kp, const uint8_t* d_desc, const vsf_dmatch* d_matches,
                                 const int32_t* d_nmatches, int max_rows, const float* h_F, int order, float* d_mean,
                                 float* d_thr, float* d_thr_state, vsf_keypoint* d_kp_out, uint8_t* d_desc_out,
                                 int32_t* d_counts_out, const int32_t* d_out_sets, int32_t* d_set_counts, hipStream_t s);
// k_points.hip (SURVEY 8(f) row f2 + the compact gather payload)
void vsf_launch_stereo_thresholds(const float* d_means, int n, float* d_state, float* d_thr, hipStream_t s);
void vsf_launch_fill_stereo_sets(int32_t* d_sets, int n_frames, hipStream_t s);  // [0..n): 2f + 1, [n..2n): 2f
void vsf_launch_vision_features(const vsf_keypoint* d_kp, const int32_t* d_counts, const uint64_t* d_pairs,
                                const int32_t* d_npairs, int n_frames, int max_rows, const vsf_calibration& c,
                                vsf_vision_feature* d_out, int32_t* d_nfeatures, int32_t* d_npoints, hipStream_t s);
void vsf_launch_pack_outputs(const vsf_vision_feature* d_features, const int32_t* d_nfeatures, int n_frames,
                             const uint64_t* d_pairs, const int32_t* d_npairs, int n_pairs, int max_rows,
                             uint8_t* d_payload, uint32_t cap_bytes, uint32_t* d_offsets, int32_t* d_status,
                             hipStream_t s);
void vsf_launch_sort_trim(const vsf_dmatch* d_matches, const int32_t* d_nmatches, int n_pairs, int max_rows,
                          float best_percent, const float* d_best_percent_of, void* d_scratch, uint64_t* d_pairs,
                          int32_t* d_npairs, hipStream_t s, bool force_serial = false, int lds_limit = 160 * 1024);
// The ObserveImage queue's output kernel (k_frontend.hip): one compact result per frame of a batch, written into pinned
// host memory.
#define VSF_OBSERVE_MAX_PAIRS 64
struct VsfObserveFrame {  // per frame of a batch; pinned host memory the kernels read directly
  int32_t left_set;  // descriptor set that holds the filtered left frame
  int32_t n_past;    // kept frames it is matched against (temporal factors)
  int32_t tp0;       // index of its first temporal pair in the batch's pair list (its right -> left pair is pair f)
  int32_t out_slot;  // result slot: out + out_slot * out_stride
};
// ... and its parameters where a batch holds frames of several streams (vsf_observe_set_streams), pinned as well
struct VsfObserveParam {
  int32_t stream;       // whose threshold state and window the frame belongs to
  int32_t calib;        // index into the batch's table of distinct calibrations
  float best_percent;   // of its temporal pairs (the pair list carries it per pair)
  int32_t prev, tail;   // the threshold chain inside the batch (vsf_observe_plan.h)
};
void vsf_launch_stereo_residuals_table(const vsf_keypoint* d_kp, const vsf_dmatch* d_matches, const int32_t* d_nmatches,
                                       int n_frames, int max_rows, const VsfObserveParam* d_par, const vsf_calibration* d_calibs,
                                       int order, float* d_residual, float* d_mean, hipStream_t s);
void vsf_launch_stereo_thresholds_streams(const float* d_means, int n, const VsfObserveParam* d_par, float* d_state,
                                          float* d_thr, hipStream_t s);
void vsf_launch_vision_features_table(const vsf_keypoint* d_kp, const int32_t* d_counts, const uint64_t* d_pairs,
                                      const int32_t* d_npairs, int n_frames, int max_rows, const VsfObserveParam* d_par,
                                      const vsf_calibration* d_calibs, vsf_vision_feature* d_out, int32_t* d_nfeatures,
                                      int32_t* d_npoints, hipStream_t s);
// The RViz point cloud (k_cloud.hip; arithmetic: vsf_world_points.h): per frame the features that pass AddFeaturePoints'
// predicate, in feature order, as M_f * point3d in three doubles.  The stand-alone call carries up to VSF_WORLD_CHUNK
// transforms in the kernel arguments (frames [f0, f0 + n_frames), frame f to slot f); the queue's batch reads them from its
// pinned block and writes frame f's points and count into slot frames[f].out_slot of pinned rings.
#define VSF_WORLD_CHUNK 64
struct VsfWorldTransforms {
  vsfwp::Affine m[VSF_WORLD_CHUNK];
};
void vsf_launch_world_points(const vsf_vision_feature* d_features, const int32_t* d_nfeatures, int f0, int n_frames, int max_rows,
                             const VsfWorldTransforms& tf, double* d_points, int32_t* d_npoints, hipStream_t s);
void vsf_launch_world_points_table(const vsf_vision_feature* d_features, const int32_t* d_nfeatures, int n_frames, int max_rows,
                                   const vsfwp::Affine* tf, const VsfObserveFrame* frames, double* points, int32_t* npoints,
                                   hipStream_t s);
struct VsfObserveArgs {
  int n_frames, max_rows;
  const int32_t* counts_raw;          // [2n] keypoints of the left / right images
  const int32_t* nmatches;            // [n] raw stereo matches
  const int32_t* counts_f;            // [2n] features of the filtered left / right frames
  const int32_t* npoints;             // [n] triangulated points
  const float* means;                 // [n]
  const float* thr;                   // [n] thresholds applied
  const vsf_vision_feature* features; // [n][max_rows]
  const vsf_keypoint* kp_f;           // [2n][max_rows] filtered keypoints (left, right per frame)
  const uint8_t* desc_sets;           // descriptor sets [..][max_rows][32]
  const uint64_t* pairs;              // [pairs][max_rows][2]
  const int32_t* npairs;              // [pairs]
  int32_t* status;                    // [2n] a status word per image of the batch: read into the header and cleared
  const VsfObserveFrame* frames;      // [n]
  uint8_t* out;                       // pinned host memory (device-visible)
  size_t out_stride;
  uint32_t out_cap;
};
void vsf_launch_observe_pack(const VsfObserveArgs& a, int max_pairs_per_frame, hipStream_t s);
// The queue's debug images (k_draw.hip, vsf_observe_set_debug_images): per frame of a batch, the operations of
// CreateStereoDebugImage / CreateMatchDebugImage (slam_frontend.cc:74-115) built from the filtered keypoints and the sorted
// pairs, drawn into device canvases [n][stereo 2w x h x 3 | match w x h x 3]; then the newest frame's keypoints are kept for
// the next batch and the colour cursor advances.  Header words 14 / 15 of each result: images present (bit 0 stereo, bit 1
// match), colours used.
// With a generator per stream (vsf_observe_set_debug_seeds: `rand_state` set) a kernel of its own runs first -- one wave per
// stream present in the batch draws the colours of that stream's frames, in their order, from the stream's state in device
// memory --, the stereo lines take them from `stream_colours`, and everything that crosses frames exists per stream: a frame's
// newest kept frame is `params[f].prev` or prev_kp[its stream], and every stream present leaves its last frame there.
struct VsfObserveDebugArgs {
  int n_frames, max_rows, width, height;
  const uint8_t* images;          // the batch's uploaded images: frame f left at 2f * image_stride, right one stride on
  size_t image_stride, image_pitch;
  const vsf_keypoint* kp_f;       // [2n][max_rows] filtered keypoints (left, right)
  const int32_t* counts_f;        // [2n]
  const uint64_t* pairs;          // [pairs][max_rows][2]
  const int32_t* npairs;
  const VsfObserveFrame* frames;  // [n]
  vsf_keypoint* prev_kp;          // [streams][max_rows] each stream's newest kept frame of earlier batches
  int32_t* prev_n;                // [streams]
  const uint32_t* colours;        // pinned ring of packed b | g << 8 | r << 16, drawn from rand() by the host
  int64_t colour_ring;
  int64_t* colour_cursor;         // colours used by every frame launched before this batch
  vsf_draw_op* ops;               // [n][5 max_rows]
  void* canvases;                 // [2n] canvas table (k_draw.hip)
  uint8_t* canvas;                // [n][canvas_stride]
  size_t canvas_stride;
  uint64_t* winners;              // [n][3 w h], zero between batches
  uint8_t* out;                   // result ring: header words 14 / 15
  size_t out_stride;
  const VsfObserveParam* params;  // [n] with a generator per stream (stream, prev, tail); nullptr: ONE stream, frame f - 1
  uint32_t* rand_state;           // [streams] vsfrand::State (vsf_glibc_random.h), carried from batch to batch; nullptr: `colours`
  uint32_t* stream_colours;       // [n][max_rows] packed colours the colour kernel writes and the operations read
};
void vsf_launch_observe_debug(const VsfObserveDebugArgs& a, hipStream_t s);

// k_jpeg.hip (cv::imdecode(IMREAD_GRAYSCALE) for baseline JPEG)
#ifdef __cplusplus
#include <vector>
struct VsfJpegPlan {  // layout of one upload: [image descriptors | decode order | table sets | progressive scans | their
                      // Huffman tables | entropy-coded segments]
  size_t off_images = 0, off_index = 0, off_tables = 0, off_scans = 0, off_prog_huff = 0, off_stream = 0, total = 0;
  std::vector<uint8_t> head;                // everything in front of the segments
  std::vector<size_t> scan_begin;           // per file: where its entropy-coded segment starts
  std::vector<uint32_t> stream_off, stream_len;
  int n_par = 0;             // files without restart intervals: they take the self-synchronising parallel decode
  int n_prog = 0;            // progressive files: scan after scan into the coefficient buffer, one wave per file
  int n_prog_huff = 0;       // ... and the Huffman tables of their scans (expanded on the device)
  int max_luma_blocks = 0;   // luminance blocks of the (padded) image, largest over the batch
  int max_slots = 1;         // Huffman tables one file's scan uses, largest over the batch
  int reduce = 1;            // the files are decoded at 1 / reduce (1, 2, 4, 8): IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8
  bool colour = false;       // the files are read as IMREAD_COLOR (vsf_imdecode_bgr_batch): chroma is kept, see k_jpeg.hip
  size_t off_qt_chroma = 0;  // ... [n][2][64] quantisation tables of components 1 and 2 (in front of the segments)
  size_t max_plane = 0;      // ... bytes of the largest block-padded luminance plane of the batch
};
// width x height: the OUTPUT size; a file of W x H is taken when ceil(W / reduce) == width and ceil(H / reduce) == height.
vsf_status vsf_jpeg_plan(const uint8_t* const* jpeg, const size_t* nbytes, int n, int width, int height, bool force_serial,
                         VsfJpegPlan* plan, int reduce = 1, bool colour = false);
// libjpeg's colour-space decision for three components (jdapimin.c): VSF_OK = YCbCr, VSF_ERR_UNSUPPORTED = it reads RGB.
vsf_status vsf_jpeg_colourspace(bool saw_jfif, bool saw_adobe, int adobe_transform, const int cid[3]);
void vsf_jpeg_fill(const VsfJpegPlan& plan, const uint8_t* const* jpeg, int n, uint8_t* dst);
#endif
// k_png.hip / vsf_png_host.cc (row f4: cv::imdecode(IMREAD_GRAYSCALE) for grayscale PNG)
#ifdef __cplusplus
struct VsfPngPlan {  // layout of one upload: [image descriptors | ends of the IDAT payloads | palette / gamma tables | zlib streams]
  size_t off_images = 0, off_pieces = 0, off_tables = 0, off_stream = 0, total = 0;
  std::vector<uint8_t> head;
  std::vector<uint32_t> piece_first, piece_off, piece_len;  // per file: its IDAT payloads (offset in the file, length)
  std::vector<uint32_t> stream_off, stream_len;
  size_t filtered_stride = 0;  // device scratch per image: the inflated scanlines
  bool any_rgb = false;        // a file of colour type 2 or 6 among them (a kernel of its own)
  bool any_general = false;    // a palette file or an interlaced gray one among them (another)
  bool bgr = false;            // the files are read as IMREAD_COLOR: three bytes a pixel, blue first (vsf_imdecode_bgr_batch)
};
vsf_status vsf_png_plan(const uint8_t* const* png, const size_t* nbytes, int n, int width, int height, VsfPngPlan* plan,
                        bool bgr = false);
void vsf_png_fill(const VsfPngPlan& plan, const uint8_t* const* png, int n, uint8_t* dst);
#endif
// ---- one decode path for compressed payloads (the C ABI's decoders and the ObserveImage queue) ----
// What the decode kernels of ONE stream need beside the upload.  Grown by decode_runs (vsf_ingest.hip), never shrunk; the
// capacities are bytes.
struct VsfDecodeScratch {
  vsfi::DevBuf<uint8_t> clean;        // JPEG, parallel decode: the de-stuffed streams and their segment-major copies
  vsfi::DevBuf<int16_t> coef;         // JPEG: luminance coefficients, then the expanded Huffman tables of progressive scans
  vsfi::DevBuf<int32_t> flags;        // JPEG: per progressive file "damaged: decode again scan after scan"
  vsfi::DevBuf<uint8_t> filtered;     // PNG: the inflated scanlines
  vsfi::DevBuf<int32_t> file_status;  // PNG: per file, what its inflate made of the stream
  vsfi::DevBuf<uint8_t> planes;       // JPEG, colour read: per file the luminance and the two chroma planes in front of the finishing kernel
  size_t clean_cap = 0, coef_cap = 0, flags_cap = 0, filtered_cap = 0, file_status_cap = 0, planes_cap = 0;
  size_t bytes() const { return clean_cap + coef_cap + flags_cap + filtered_cap + file_status_cap + planes_cap; }
};
struct VsfDecodeNeed {  // bytes of each; the needs of several runs on one stream combine by maximum
  size_t clean = 0, coef = 0, flags = 0, filtered = 0, file_status = 0, planes = 0;
};
// Pinned staging + its device copy for ONE upload.  `uploaded` (optional): recorded behind the upload, and waited for before
// the host writes the pair again -- an owner that knows the pair to be free by other means leaves it null.
struct VsfStaging {
  vsfi::PinnedBuf<uint8_t> h;
  vsfi::DevBuf<uint8_t> d;
  size_t cap = 0;
  vsfi::Event uploaded;
};
// Each launcher owns everything derived from its plan: offsets into the upload, strides and positions inside the scratch,
// which kernels a run takes.  `n` files of width x height land at d_dst + i * dst_image_stride.
// status_stride: 0 = every file reports into *d_status; 1 = file i into d_status[i] (the ObserveImage queue).
// prog_serial: progressive files scan after scan in one wave (otherwise the pipelined form up to its file limit).
VsfDecodeNeed vsf_jpeg_scratch_need(const VsfJpegPlan& plan);
VsfDecodeNeed vsf_png_scratch_need(const VsfPngPlan& plan, int n);
void vsf_launch_jpeg_decode(const uint8_t* d_blob, const VsfJpegPlan& plan, int n, int width, int height,
                            const VsfDecodeScratch& scratch, uint8_t* d_dst, size_t dst_image_stride, int dst_pitch,
                            int32_t* d_status, int status_stride, bool prog_serial, hipStream_t s);
void vsf_launch_png_decode(const uint8_t* d_blob, const VsfPngPlan& plan, int n, int width, int height,
                           const VsfDecodeScratch& scratch, uint8_t* d_dst, size_t dst_image_stride, int dst_pitch,
                           int32_t* d_status, int status_stride, hipStream_t s);

// vsf_ingest_host.cc (plain C++, no HIP call): what a list of files is, and the host half of decoding it.
enum { VSF_FILE_NONE = 0, VSF_FILE_JPEG = 1, VSF_FILE_PNG = 2 };  // (ObserveFrame::kind: 0 is the raw frame there)
enum { VSF_OUT_GRAY = 0, VSF_OUT_BGR = 1 };  // what a decode writes: cv::IMREAD_GRAYSCALE's byte or cv::IMREAD_COLOR's three
int vsf_file_kind(const uint8_t* file, size_t nbytes);  // by the first bytes, as cv::imdecode's findDecoder tells them apart
int vsf_run_end(const uint8_t* kinds, int n, int i0);   // one past the last file of the run of one kind that starts at i0
int vsf_jpeg_frame_components(const uint8_t* file, size_t nbytes);  // Nf of the first SOF0 / SOF1 / SOF2 segment; 0: none found
// The denominators a decode takes, stated ONCE: 1 (full size) and cv::IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8.
inline bool vsf_reduce_ok(int reduce) { return reduce == 1 || reduce == 2 || reduce == 4 || reduce == 8; }
// what cv::resize on the device takes on either side (vsf_resize_gray_batch_dev): VsfTap's 16-bit fields hold the taps
inline bool vsf_resize_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 32767 && h <= 32767; }
struct VsfDecodeRun {  // files [i0, i0 + n) of one format; its upload starts `off` bytes (a multiple of 256) into the blob
  int i0 = 0, n = 0, kind = VSF_FILE_NONE;
  size_t off = 0;
  VsfJpegPlan jp;  // (the one of `kind`)
  VsfPngPlan pp;
};
struct VsfDecodeRuns {
  std::vector<VsfDecodeRun> runs;  // in file order; files of kind VSF_FILE_NONE belong to none
  size_t total = 0;                // bytes of the ONE upload
};
// reduces (optional; null: 1 everywhere): file i decodes at 1 / reduces[i] into width x height -- a run also ends where the
// denominator changes, so one upload carries files of several.  reduces[i] > 1 (2, 4, 8) with a PNG file is
// VSF_ERR_UNSUPPORTED (cv::imdecode decodes a PNG at full size and calls cv::resize, which is not built here); a value
// outside {1, 2, 4, 8} VSF_ERR_INVALID_ARG.
// out_format = VSF_OUT_BGR (cv::IMREAD_COLOR): the files are planned for three bytes a pixel at full size (JPEG files keep
// their chroma: vsf_jpeg_plan's `colour`); a denominator above 1 is VSF_ERR_UNSUPPORTED in that format.
vsf_status vsf_plan_runs(const uint8_t* const* files, const size_t* nbytes, const uint8_t* kinds, int n, int width, int height,
                         bool force_serial, VsfDecodeRuns* out, const uint8_t* reduces = nullptr, int out_format = VSF_OUT_GRAY);
void vsf_fill_runs(const VsfDecodeRuns& plan, const uint8_t* const* files, uint8_t* dst);
// ---- one encode path for JPEG / PNG files (the C ABI's encoders and the ObserveImage queue's debug files) ----
// cv::imencode(".jpg", img, {IMWRITE_JPEG_QUALITY, quality}) / cv::imencode(".png", img) of n equally sized images: image i
// at d_src + i * src_image_stride, its file at d_out + i * out_stride and the file's size in d_out_bytes[i].
struct VsfEncodeJob {
  int kind = VSF_FILE_NONE;  // VSF_FILE_JPEG / VSF_FILE_PNG
  int n = 0, width = 0, height = 0, channels = 0;
  size_t src_image_stride = 0, src_row_stride = 0;
  int quality = 0;     // JPEG: 1 .. 100; PNG: ignored
  size_t out_stride = 0;
  size_t out_cap = 0;  // bytes a file may take of its slot (0: all out_stride of them)
  size_t cap() const { return out_cap == 0 || out_cap > out_stride ? out_stride : out_cap; }
};
// What each format brings (k_jpeg_enc.hip, k_png_enc.hip): the launches its launcher issues -- stated beside that launcher --,
// the scratch a job needs (16- / 64-byte aligned; it reads the SAME layout and the same cap() as the launcher, so a buffer
// sized for a job holds that job) and the launcher itself, asynchronous on `s`.
int vsf_jpeg_enc_launches();
size_t vsf_jpeg_enc_scratch_need(const VsfEncodeJob& job);
void vsf_jpeg_enc_launch(const VsfEncodeJob& job, const uint8_t* d_src, void* d_scratch, uint8_t* d_out, int32_t* d_out_bytes,
                         int32_t* d_status, hipStream_t s);
int vsf_png_enc_launches();
size_t vsf_png_enc_scratch_need(const VsfEncodeJob& job);
void vsf_png_enc_launch(const VsfEncodeJob& job, const uint8_t* d_src, void* d_scratch, uint8_t* d_out, int32_t* d_out_bytes,
                        int32_t* d_status, hipStream_t s);
inline size_t vsf_encode_capacity(int kind, int w, int h, int ch) {
  return kind == VSF_FILE_PNG ? vsf_png_encode_capacity(w, h, ch) : vsf_jpeg_encode_capacity(w, h, ch);
}
inline int vsf_encode_launches(int kind) { return kind == VSF_FILE_PNG ? vsf_png_enc_launches() : vsf_jpeg_enc_launches(); }
inline size_t vsf_encode_scratch_need(const VsfEncodeJob& j) { return j.kind == VSF_FILE_PNG ? vsf_png_enc_scratch_need(j) : vsf_jpeg_enc_scratch_need(j); }
inline void vsf_launch_encode(const VsfEncodeJob& j, const uint8_t* d_src, void* d_scratch, uint8_t* d_out, int32_t* d_out_bytes,
                              int32_t* d_status, hipStream_t s) {
  (j.kind == VSF_FILE_PNG ? vsf_png_enc_launch : vsf_jpeg_enc_launch)(j, d_src, d_scratch, d_out, d_out_bytes, d_status, s);
}
// What the encode calls of ONE context need: both encoders launch only on the context's stream, one call after the other, so
// they share one scratch and one staging buffer.  A call that needs more takes a new allocation without waiting (grow_scratch
// retires the outgrown buffer, which an encode already queued may still be using, until the next vsf_sync).  Bytes; never shrunk.
struct VsfEncodeScratch {
  vsfi::DevBuf<uint8_t> scratch;  // *_encode_batch_dev: the encoder's work buffers (a quarter of headroom when it grows)
  vsfi::DevBuf<uint8_t> staging;  // the host-pointer calls: images | files | byte counts on the device (grown to the need)
  size_t scratch_cap = 0, staging_cap = 0;
};
// The queue's debug files (k_frontend.hip): file i (d_bytes[i] bytes at d_files + i * file_stride; nothing when negative) goes to
// h_ring + ((slot0 + i) % depth) * slot_stride + file_off and its size to the i32 at that slot + 4 * which.  16 bytes per lane.
// A frame whose result header (results + frames[i].out_slot * result_stride, word 14) lacks bit `which` has no such image: size 0.
void vsf_launch_files_home(const uint8_t* d_files, size_t file_stride, const int32_t* d_bytes, int n, uint8_t* h_ring,
                           size_t slot_stride, size_t file_off, int which, int slot0, int depth, const VsfObserveFrame* frames,
                           const uint8_t* results, size_t result_stride, hipStream_t s);
// The queue's ingest finish (k_ingest.hip): every image of [0, n) whose status word carries bit 1 (its decoder refused the
// data) becomes all zero, `rows` rows of `pitch` bytes.
void vsf_launch_ingest_finish(uint8_t* d_img, size_t image_stride, int pitch, int rows, const int32_t* d_status, int n,
                              hipStream_t s);
// vsf_observe_submit_dev (k_ingest.hip): ONE launch copies a call's 2 n device-resident images -- any base address, any
// pitch >= w -- into the slots (slot0 + f) % depth, f = 0 .. n - 1, of the queue's device ring (left, right per slot;
// image_stride bytes each, rows at dst_pitch, a multiple of 16 >= (w + 15) & ~15 with h * dst_pitch <= image_stride).
// Where an image comes from: up to VSF_INGEST_INLINE images ride in the kernel arguments (`inl`, by image); a longer call
// names `table`, device-visible pinned memory indexed by 2 * slot + side, which must stay as it is until the kernel has run.
struct VsfIngestSrc {
  const uint8_t* src;
  size_t pitch;
};
#define VSF_INGEST_INLINE 8
void vsf_launch_ingest_ring(uint8_t* d_ring, size_t image_stride, int dst_pitch, int w, int h, int slot0, int depth, int n_frames,
                            const VsfIngestSrc* inl, const VsfIngestSrc* table, hipStream_t s);

// k_to_bgr.hip (bag_extract.cc:75-88): n raw images of any VSF_PIX_* format -> B G R, three bytes a pixel, ONE launch; bases and
// pitches are multiples of 4, src_pitch >= w * bpp, dst_pitch >= (3 w + 3) & ~3 (the callers have checked).  An unknown format
// launches nothing.  And cv::split(image)[0]: the first byte of every B G R pixel, one byte a pixel (dst_pitch >= (w + 3) & ~3).
void vsf_launch_to_bgr(int pixfmt, const uint8_t* d_src, int n, int w, int h, size_t src_image_stride, int src_pitch, uint8_t* d_dst,
                       size_t dst_image_stride, int dst_pitch, hipStream_t s);
void vsf_launch_bgr_channel0(const uint8_t* d_src, int n, int w, int h, size_t src_image_stride, int src_pitch, uint8_t* d_dst,
                             size_t dst_image_stride, int dst_pitch, hipStream_t s);
// vsf_bag_extract_batch: the images between its stages (the mosaics | the demosaiced B G R | the colour reads), what goes home (files
// | byte counts) and the pinned buffer it goes through, on the context's stream.  Grown as the decoders' scratch is (a quarter of headroom, no wait; never shrunk).
struct VsfBagScratch {
  vsfi::DevBuf<uint8_t> images, files;
  vsfi::PinnedBuf<uint8_t> home;  // the files of one call packed one behind the other, on their way to the caller's slots
  size_t images_cap = 0, files_cap = 0, home_cap = 0;
};

// k_resize.hip: cv::resize (INTER_LINEAR, CV_8UC1) of n images of sw x sh into dw x dh, any base address and pitch on either
// side; ONE launch (per 65535 images).  The caller has checked the sizes (1 .. 32767) and the pitches (>= the widths).
void vsf_launch_resize_gray(const uint8_t* d_src, int n, int sw, int sh, size_t src_image_stride, size_t src_pitch, uint8_t* d_dst,
                            int dw, int dh, size_t dst_image_stride, size_t dst_pitch, hipStream_t s);

#endif  // VSF_INTERNAL_H_
