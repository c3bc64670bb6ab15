/*
 * vsf.h -- C ABI of the MI355X (gfx950) stereo feature frontend.
 *
 * This is the drop-in seam for the two private methods of slam::Frontend that call into OpenCV in
 * the reference (ut-amrl/vision_slam_frontend):
 *
 *   Frontend::ExtractFeatures  src/slam_frontend.cc:266-280  -> cv::Feature2D::detectAndCompute (ORB,
 *                              parameters :205-213) or FastFeatureDetector::detect (:271, built :191)
 *   Frontend::GetMatches       src/slam_frontend.cc:521-538  -> cv::BFMatcher(NORM_HAMMING)::knnMatch(k=2)
 *                              (:525, matcher built :247) + the ratio test (:529-536)
 *
 * Plain pointers and sizes only; every function returns a vsf_status (never aborts, never throws;
 * the reference's glog CHECK / cv::Exception / exit(1) paths become status codes).  A context owns one
 * GPU's device memory and stream and is used by one host thread at a time.  Host-pointer entry points
 * are synchronous; *_dev entry points take device pointers, are asynchronous on the context's stream (none of them waits
 * for the GPU: the one measuring call, vsf_tune_fast_resident, is explicit and says so) and are what the batched /
 * multi-GPU path uses.  A HIP failure inside an asynchronous call (a launch, an event record or wait) is returned by that
 * call as VSF_ERR_HIP -- or, if it could only be noticed later, by the next call on the context that checks (every
 * entry point that launches, and vsf_sync).
 *
 * Output record layouts are the reference's: vsf_keypoint == cv::KeyPoint (28 B), vsf_dmatch ==
 * cv::DMatch (16 B), descriptors are row-major N x 32 uint8 (cv::Mat CV_8U, 256 bit).
 */
#ifndef VSF_H_
#define VSF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSF_VERSION 2 /* 2: round 6 -- the ObserveImage queue; five options of retired kernel variants removed */
#define VSF_DESC_BYTES 32
#define VSF_MAX_LEVELS 64

typedef enum {
  VSF_OK = 0,
  VSF_ERR_INVALID_ARG = 1, /* null pointer, bad size, image geometry != context geometry */
  VSF_ERR_CAPACITY = 2,    /* an output or an internal segment overflowed; results are truncated */
  VSF_ERR_HIP = 3,         /* a HIP runtime call failed (vsf_last_hip_error gives the code) */
  VSF_ERR_UNSUPPORTED = 4, /* parameter combination outside the north-star path (e.g. WTA_K != 2) */
  VSF_ERR_NO_DEVICE = 5    /* no usable gfx950 device */
} vsf_status;

/* cv::KeyPoint */
typedef struct {
  float x, y;      /* pt, level-0 pixel coordinates */
  float size;      /* 31 * scale_l (ORB) / 7 (FAST) */
  float angle;     /* degrees, [0,360) (ORB) / -1 (FAST) */
  float response;  /* Harris response (ORB, HARRIS_SCORE) / FAST score (ORB with FAST_SCORE; FAST) */
  int32_t octave;  /* pyramid level */
  int32_t class_id;/* -1 */
} vsf_keypoint;

/* cv::DMatch */
typedef struct {
  int32_t queryIdx, trainIdx, imgIdx; /* imgIdx is always 0 */
  float distance;                     /* (float) Hamming distance */
} vsf_dmatch;

/* vsf_params::score_type, numbered as cv::ORB's enum */
#define VSF_SCORE_HARRIS 0
#define VSF_SCORE_FAST 1

typedef struct {
  /* --- cv::ORB::create arguments (reference literals slam_frontend.cc:205-213) --- */
  int32_t nfeatures;      /* 10000 in the reference; BASELINE configs use 2000 / 8000 */
  /* 1.04f.  Any value > 1 whose pyramid the resize kernels can build: for every level l >= 1, with cv::resize's own
   * INTER_LINEAR taps from level l - 1, the taps of each group of four adjacent output pixels must lie inside one
   * 8-byte window of the source row (ratios w(l-1) / w(l) up to about 2: 640 -> 320 fits, 333 -> 166 = 2.006 does not,
   * 2.5 never does), and level l - 1 must be at least 8 pixels wide.  vsf_create returns VSF_ERR_INVALID_ARG otherwise;
   * nothing is computed approximately.  Above 1 + 1/7 no level shares source rows between output rows any more: the
   * frame-latency chain and the image-major tail are not taken, every level is one launch of the general resize kernel. */
  float scale_factor;
  int32_t nlevels;        /* 50 (<= VSF_MAX_LEVELS) */
  /* 31.  Any value >= 22: keypoints sit at edge_threshold <= x < w - edge_threshold, edge_threshold <= y < h - edge_threshold
   * of their level (runByImageBorder).  22 is the reach of what is read around a keypoint (the rotated pattern, 19, on a
   * level blurred over 3 more pixels; the IC-angle disc reaches 15, Harris 4): the borders of a level are not
   * materialised, so vsf_create returns VSF_ERR_UNSUPPORTED below it.  A level no larger than 2 * edge_threshold in either
   * direction has no keypoints, as in the reference.  A border of at least half the image leaves every level empty: such a
   * context is created all the same, and every call on it returns VSF_OK with zero counts and writes no keypoint or
   * descriptor.  (tests/test_gpu_edge_threshold.py) */
  int32_t edge_threshold;
  int32_t first_level;    /* 0 (only value supported) */
  int32_t wta_k;          /* 2 (only value supported) */
  /* 0 = cv::ORB::HARRIS_SCORE (the reference's, the default); 1 = cv::ORB::FAST_SCORE; anything else VSF_ERR_UNSUPPORTED.
   * FAST_SCORE (OpenCV 3.2 computeKeyPoints): per level FAST + runByImageBorder, then ONE retainBest(n_l) on the FAST
   * score -- no HarrisResponses, no second cut -- and everything behind it (ICAngles, GaussianBlur, the descriptors) as in
   * HARRIS mode; vsf_keypoint::response is the FAST score.  The cut sits on an 8-bit key and retainBest keeps, beyond
   * its n_l, every candidate whose score is not below that of element n_l - 1 as std::nth_element left it (one of the
   * best n_l, not always the lowest of them): a level keeps between n_l and n_l + every candidate that shares the cut's
   * score, and an image can hold MORE than nfeatures keypoints (640x480, nfeatures 2000: 2039 on a natural-looking
   * scene, 2388 on a checkerboard of period 8, where counting every tie would give 2057 and 2698).
   * Room, the one rule: an image holds max_keypoints keypoints and, in FAST_SCORE mode, a level holds
   * n_l + max(max_keypoints - nfeatures, 0) of them -- the headroom the caller buys with max_keypoints (256 by default) is
   * available to every level.  A level or an image that needs more is VSF_ERR_CAPACITY, as in HARRIS mode (results
   * truncated per level / per image, counts as documented at vsf_extract; in the ObserveImage queue on that frame's
   * ticket alone), never a silent cut.  In HARRIS mode a level holds 2 n_l + 64 whatever max_keypoints is: unchanged.
   * vsf_debug_level_room states both for a parameter set without a device.  (tests/test_gpu_score_type.py) */
  int32_t score_type;
  int32_t patch_size;     /* 31 (only value supported) */
  int32_t fast_threshold; /* 20 */
  /* 1: GaussianBlur column pass rounds like OpenCV's SSE2 SymmColumnVec_32s8u (half-even) on columns
   * [0, w - w%4) and like the scalar tail (half-up) beyond; 0: half-up everywhere (non-SSE2 build). */
  int32_t blur_sse2;
  /* --- cv::FastFeatureDetector::create(10, true) (slam_frontend.cc:191), FREAK branch only --- */
  int32_t fast_detector_threshold; /* 10 */
  int32_t fast_detector_nms;       /* 1 */
  /* --- matcher: ratio test  dist1 < nn_match_ratio * dist2  with nn_match_ratio a double holding 0.6f
   * (slam_frontend.cc:523,533,555)  ==  dist1 * 2^ratio_shift < ratio_num * dist2  exactly --- */
  uint32_t ratio_num;   /* 5033165  (0.6f == 10066330 / 2^24, kept in lowest terms) */
  uint32_t ratio_shift; /* 23 */
  /* --- geometry and capacities (fixed per context) --- */
  int32_t width, height;   /* image size in pixels */
  int32_t max_images;      /* images per batch (2 per stereo frame) */
  int32_t max_keypoints;   /* per-image capacity of keypoint/descriptor outputs; 0 = nfeatures + 256 */
  /* --- RemoveAmbigStereo (slam_frontend.cc:381-383): order in which the three-term dot products of
   * left_ph.transpose() * F * right_ph are summed.  0 (default): a0*b0 + (a1*b1 + a2*b2), what Eigen 3.3's unrolled
   * reduction of a fixed-size-3 lazy product does; 1: (a0*b0 + a1*b1) + a2*b2. --- */
  int32_t residual_order;
} vsf_params;

typedef struct vsf_ctx vsf_ctx;

/* Fills *p with the reference literals for the given image size and batch capacity. */
vsf_status vsf_params_default(vsf_params* p, int width, int height, int max_images);
/* ratio as the reference stores it: a float widened to double. Sets ratio_num / ratio_shift (lowest terms: ratio_num odd
 * or ratio_shift 0).  VSF_ERR_INVALID_ARG, with *p left unchanged, for a float that is not finite, not inside (0, 256),
 * or needs more than 31 fractional bits (ratio_shift <= 31): 0.001f == 8 589 935 / 2^33 is refused, 2^-31 is the
 * smallest power of two accepted. */
vsf_status vsf_params_set_ratio(vsf_params* p, float nn_match_ratio);

vsf_status vsf_create(const vsf_params* p, int device, vsf_ctx** out);
void vsf_destroy(vsf_ctx* ctx);
const char* vsf_status_string(vsf_status s);
/* The hipError_t of the context's last VSF_ERR_HIP -- or 10000 + the ncclResult_t when it was an RCCL call that failed
 * (vsf_comm_create, vsf_allgather_dev, vsf_gather_payload_dev).  An error belongs to the context whose call met it: one
 * noted inside an asynchronous call is returned by that call or by the same context's next call that checks, never by
 * another context driven from the same host thread. */
int vsf_last_hip_error(const vsf_ctx* ctx);
vsf_status vsf_get_params(const vsf_ctx* ctx, vsf_params* out);
/* Use an existing hipStream_t (e.g. the caller's framework stream) instead of the context's own. NULL restores it.  The
 * handle must be a live stream of the context's device (the HIP runtime does not validate stream handles). */
vsf_status vsf_set_stream(vsf_ctx* ctx, void* hip_stream);
/* Batched entry points split a batch in `lanes` halves (1 or 2, default 1) that run concurrently: one on the context's
 * stream, one on an internal stream forked from / joined back into it with events, so the caller still sees ONE
 * stream-ordered operation.  Frames are independent (slam_frontend.cc:411-416), results do not depend on it. */
vsf_status vsf_set_lanes(vsf_ctx* ctx, int lanes);
/* Cross-call pipelining for streams of batches (off by default).  With it on, the caller promises that the input
 * images of every *_batch_dev call are COMPLETE in device memory when the call is made (not merely ordered before it
 * on the stream); images produced by this library's own vsf_bayer_bg_to_gray_batch_dev on the same context are the
 * exception -- the pipelined pyramid waits for that conversion by itself.  The scale pyramid of a call -- which depends on nothing else -- is then built on internal streams
 * into the second of two pyramid buffers while the previous call's later stages are still running; all other stages
 * and all outputs stay ordered on the context's stream as before. */
vsf_status vsf_set_pipeline(vsf_ctx* ctx, int on);
/* Input readiness as an explicit event, for ANY producer (a decoder on another context or stream, the caller's own
 * kernel, a copy engine; slam_frontend_main.cc:98-132 is where frames arrive): hip_event is a hipEvent_t the caller
 * recorded behind the last operation that writes the images of the NEXT vsf_extract_batch_dev / vsf_stereo_batch_dev
 * call.  That call -- including its pipelined pyramid, which is otherwise not ordered after anything (vsf_set_pipeline)
 * -- waits for the event ON THE GPU; the host never does.  With it the promise of vsf_set_pipeline relaxes to "complete
 * when the event fires".  One-shot: the vsf_extract_batch_dev / vsf_stereo_batch_dev call that follows consumes it -- a call
 * refused with VSF_ERR_INVALID_ARG launches nothing and forgets it too (hand it over again with the corrected call) (the wait captures the event's state at that
 * moment, so the caller may record the same event again afterwards); NULL withdraws it.  The way back is ordinary
 * stream order: whatever the caller records on the context's stream after the call fires once the call has read its
 * inputs. */
vsf_status vsf_set_input_event(vsf_ctx* ctx, void* hip_event);
/* Batched entry points (>= 32 images per call) run the Gaussian blur of a call -- matrix cores and memory -- on an
 * internal stream forked behind the pyramid and joined in front of the descriptors, i.e. beside FAST and the keypoint
 * selection, which live on the vector ALU and on latency (default: on; the caller still sees ONE stream-ordered
 * operation, results do not depend on it).  With it on, the per-stage timer of the blur (vsf_profile_read) is the wall
 * span of a kernel that shares the chip, not its own duration.  0 puts the blur back in line. */
vsf_status vsf_set_blur_overlap(vsf_ctx* ctx, int on);
/* With the blur beside it, FAST can run as one RESIDENT workgroup per CU (`waves` = 2..4 waves per SIMD, fed with cells
 * through a counter) instead of a grid that fills every register of the chip for as long as cells are left, so that the
 * blur's workgroups find room beside it.  -1 (default): the form vsf_tune_fast_resident measured for this batch size, the
 * grid form for a size it has not measured; 0: always the grid form; 2..4: always resident.  Speed only: results do not
 * depend on it. */
vsf_status vsf_set_fast_resident(vsf_ctx* ctx, int waves);
/* What a batched call of the last tuned size does now: *waves = 0 (grid form) or 2..4 (resident, waves per SIMD). */
vsf_status vsf_get_fast_resident(const vsf_ctx* ctx, int* waves);
/* BLOCKING (the one *_dev-shaped call that is): runs vsf_extract_batch_dev on the given images 1 + 2 * samples times
 * (samples >= 1, 3 is a good value) -- one warm-up, then the grid form and the resident form of FAST alternately, each run
 * timed by itself between two events and waited for -- and keeps the form with the smaller MEDIAN for batches of n_images
 * images (vsf_set_fast_resident(ctx, -1) semantics).  *ms_grid / *ms_resident receive the two medians, so that the ranks of
 * a multi-GPU job can agree on one form (all-reduce the pair, then vsf_set_fast_resident with the common winner).  Batches
 * the blur does not run beside (fewer than 32 images, vsf_set_blur_overlap(ctx, 0), two lanes) are left on the grid form
 * and report 0 / 0.  No other entry point measures anything or waits for the GPU behind the caller's back. */
vsf_status vsf_tune_fast_resident(vsf_ctx* ctx, const uint8_t* d_imgs, int n_images, size_t image_stride,
                                  size_t row_stride, vsf_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts,
                                  int samples, float* ms_grid, float* ms_resident);
/* Launch choices of a context (speed / A-B measurements only: results never depend on them).  Nothing in the library
 * reads the environment.  vsf_set_option waits for the context's stream first. */
typedef enum {
  VSF_OPT_FAST_BOTH_MAX = 0, /* 16: largest batch (images) whose full and half-wave FAST cells share one launch */
  VSF_OPT_SELECT_WIDE = 1,   /* 1: a frame or two takes the 1024-thread whole-level selection class; 0: never */
  VSF_OPT_PYRAMID_FEW = 2,   /* 16: largest batch (images) whose pyramid is built by the slab kernel */
  VSF_OPT_PYRAMID_CHAIN = 3, /* 8: levels per slab launch; 0: per-level launches even for a frame or two */
  VSF_OPT_PYRAMID_ROWS = 4,  /* 6: rows of a chain's last level per slab */
  VSF_OPT_SELECT_BIG_CLASS = 5, /* 1: a batch's widest levels keep their candidate array in LDS (9 216 entries, tables in HBM) */
  VSF_OPT_PIPE_AFTER_FAST = 6, /* 1: the pipelined pyramid of a call waits for the previous call's FAST kernel; 0: it starts as soon
                                * as its inputs are ready (a step whose FAST shares the chip with a decoder) */
  VSF_OPT_PIPE_PRIORITY = 7,   /* stream priority of the pipelined pyramid chain: 0 normal, 1 lowest, -1 highest; set it before
                                * vsf_set_pipeline(ctx, 1) */
  VSF_OPT_OBSERVE_THREAD = 8,  /* 1: an ObserveImage queue of depth >= 4 gets a launcher thread -- the caller stages frames, the
                                * thread sends the batches (a host whose launches, 0.1-0.3 ms per batch, are what bounds the
                                * caller); 0 (default): the caller launches too.  Read when the queue is built */
  VSF_OPT_PYRAMID_TAIL_MIN = 9, /* smallest batch (images) whose one-band pyramid levels are one launch (a workgroup per image)
                                 * even when that fills less than three quarters of the chip; 0: never */
  VSF_OPT_OBSERVE_COPY_THREAD = 10, /* 1 (default): while frames stream into an ObserveImage queue of depth >= 4 a second host thread
                                     * takes the right image's staging copy; 0: the caller copies both.  Read when the queue is built */
  VSF_OPT_FAST_EARLY_LEVELS = 11, /* pipelined calls (vsf_set_pipeline): n > 0 = FAST on the full-width cells of pyramid levels
                                   * 0 .. n - 1 is a launch of its own that starts from inside the call's pyramid chain, as soon as
                                   * level n - 1 exists, beside the previous call's selection and descriptors; the rest of FAST
                                   * follows the pyramid as before.  0: one FAST pass; default 12.  Clamped to the levels that have such a
                                   * cell; read by every call, so it may change between two calls */
  VSF_OPT_FAST_EARLY_FORM = 12,   /* that early launch as a grid of one workgroup per four cells (0) or as one resident
                                   * workgroup per CU with 1 .. 3 waves per SIMD; default 0 */
  VSF_OPT_BLUR_EARLY = 13,        /* pipelined calls of 32 images or more: 1 (default) = the call's blur is queued behind its
                                   * pyramid chain on that chain's stream, into the other of two blurred pyramids: it starts
                                   * beside the end of the PREVIOUS call's matcher, before the call's own stream has reached its
                                   * FAST; 0: forked from the call's own stream, beside its FAST.  Read by every call, so it
                                   * may change between two calls */
  VSF_OPT_COUNT = 14
} vsf_option;
vsf_status vsf_set_option(vsf_ctx* ctx, int option, int value);
vsf_status vsf_get_option(const vsf_ctx* ctx, int option, int* value);
/* Waits for the stream and returns VSF_ERR_CAPACITY if any kernel since the last sync overflowed. */
vsf_status vsf_sync(vsf_ctx* ctx);
/* BLOCKING set-up call: sizes the scratch the batched *_dev calls keep inside the context (2-NN tables, residuals, the
 * temporal pairs' matches and sort keys, Calculate3DPoints' pair lists, the pack offsets) for batches of up to n_frames
 * stereo frames and n_pairs (past, current) pairs.  vsf_create reserves for max_images / 2 frames and as many pairs; a
 * context that serves larger batches than its own max_images suggests (the tail context of the multi-GPU composition:
 * max_images = 2, B frames, B x window pairs) calls this once.  A *_dev call beyond the reservation still works and
 * still does not wait for the GPU: it takes a new allocation (the host time of a hipMalloc) and the outgrown buffer,
 * which kernels already queued may be using, is released by the next vsf_sync / vsf_reserve / vsf_destroy. */
vsf_status vsf_reserve(vsf_ctx* ctx, int n_frames, int n_pairs);

/* Pyramid geometry the context derived (cv::ORB layer sizes / scales / per-level feature budgets). */
vsf_status vsf_level_info(const vsf_ctx* ctx, int level, int* w, int* h, float* scale, int* nfeatures);

/* ---------------- multi-GPU exchange (BASELINE configs[3]; SURVEY.md 8(b): "vsf_gather_* for multi-GPU") ----------------
 * One process (or thread) per GPU, one context and one communicator each.  What has to cross GPUs is what the reference's
 * algorithm forces: the per-frame mean residuals (the static threshold of RemoveAmbigStereo crosses frames,
 * slam_frontend.cc:353, 392-394), every rank's last frames for the temporal GetFeatureMatches (cc:424-434) and the packed
 * VisionFeature / FeatureMatch payloads one process assembles into the SLAMProblem (cc:498-503; caller
 * slam_frontend_main.cc:251, 132).  RCCL is loaded at run time by the first of these calls (VSF_ERR_UNSUPPORTED if there is
 * none); both transfers are asynchronous, ordered on the context's stream like any *_dev call. */
#define VSF_COMM_ID_BYTES 128
typedef struct vsf_comm vsf_comm;
/* ncclGetUniqueId: called by ONE rank; the caller carries the 128 bytes to the other ranks (shared memory between the
 * threads of a process, a file, MPI, the launcher's own process group ...). */
vsf_status vsf_comm_unique_id(uint8_t* id);
/* ncclCommInitRank on the context's device: collective over the `world` ranks that hold the same id. */
vsf_status vsf_comm_create(vsf_ctx* ctx, const uint8_t* id, int rank, int world, vsf_comm** out);
void vsf_comm_destroy(vsf_comm* comm);
vsf_status vsf_comm_info(const vsf_comm* comm, int* rank, int* world, int* rccl_version);
/* d_recv[r * bytes_per_rank ...] = rank r's d_send[0 .. bytes_per_rank) on every rank (ncclAllGather of bytes). */
vsf_status vsf_allgather_dev(vsf_ctx* ctx, vsf_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);
/* Every rank sends `bytes` bytes of d_send to `root`; on the root rank r's bytes land at d_recv + r * recv_stride (d_recv is
 * ignored elsewhere).  One group of point-to-point transfers: over xGMI each peer -> root copy rides its own link.  `bytes`
 * is the same on all ranks (the payload sizes are exchanged first: vsf_pack_outputs_dev writes them into the header). */
vsf_status vsf_gather_payload_dev(vsf_ctx* ctx, vsf_comm* comm, const uint8_t* d_send, size_t bytes, uint8_t* d_recv,
                                  size_t recv_stride, int root);

/* ---------------- host-pointer, synchronous: one call == one reference call ---------------- */

/* detectAndCompute(image, noArray(), kps, desc)  (slam_frontend.cc:274-277).  kp_out/desc_out hold `cap`
 * records; *n_out = number of keypoints found (<= cap written). */
vsf_status vsf_extract(vsf_ctx* ctx, const uint8_t* img, int w, int h, size_t stride, vsf_keypoint* kp_out,
                       uint8_t* desc_out, int cap, int* n_out);
/* The two detectAndCompute calls of one stereo frame (slam_frontend.cc:411-412) as ONE batch of two images: one
 * upload, one set of launches, one download.  Same results as two vsf_extract calls; needs max_images >= 2. */
vsf_status vsf_extract_pair(vsf_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int w, int h, size_t stride,
                            vsf_keypoint* kp0, uint8_t* desc0, int* n0, vsf_keypoint* kp1, uint8_t* desc1, int* n1,
                            int cap);
/* fast_feature_detector_->detect(image, kps)  (slam_frontend.cc:271): FAST-9/16 + NMS on the full-resolution
 * image, raster order.  threshold < 0 uses params.fast_detector_threshold. */
vsf_status vsf_fast_detect(vsf_ctx* ctx, const uint8_t* img, int w, int h, size_t stride, int threshold, int nms,
                           vsf_keypoint* kp_out, int cap, int* n_out);
/* matcher_->knnMatch(q, t, matches, 2)  (slam_frontend.cc:525): idx2/dist2 are nq x 2, ordered by
 * (distance, train index); absent neighbours are idx -1 / dist INT32_MAX. */
vsf_status vsf_knn2_hamming(vsf_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx2,
                            int32_t* dist2);
/* Frontend::GetMatches(query, train, nn_match_ratio)  (slam_frontend.cc:521-538): matches in ascending
 * queryIdx.  nt < 2 yields no matches (the reference reads out of bounds there). */
vsf_status vsf_get_matches(vsf_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, vsf_dmatch* out,
                           int cap, int* n_out);

/* GetMatches of n_sets query sets against ONE train set -- the temporal loop of slam_frontend.cc:424-434, every past
 * frame against the new one -- in one upload / launch / download.  q[s] points at nq[s] rows; the matches of set s
 * are written at out + s * cap_per_set, their number to n_out[s].  Same results as n_sets vsf_get_matches calls. */
vsf_status vsf_get_matches_multi(vsf_ctx* ctx, const uint8_t* const* q, const int* nq, int n_sets, const uint8_t* t,
                                 int nt, vsf_dmatch* out, int cap_per_set, int* n_out);

/* ---------------- device-pointer, asynchronous, batched ---------------- */

/* detectAndCompute on n_images images resident in HBM.  d_imgs: image i starts at d_imgs + i*image_stride,
 * rows `row_stride` bytes apart (both multiples of 16, base 16-byte aligned).  Outputs: d_kp
 * [n_images][max_keypoints], d_desc [n_images][max_keypoints][32], d_counts [n_images]. */
vsf_status vsf_extract_batch_dev(vsf_ctx* ctx, const uint8_t* d_imgs, int n_images, size_t image_stride,
                                 size_t row_stride, vsf_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts);
/* knnMatch(k=2) + ratio test for n_pairs (query set, train set) pairs.  Set s of a descriptor array starts
 * at base + s*set_stride bytes and holds d_n*[s] rows.  pair p matches query set q_set[p] against train set
 * t_set[p] (device int32 arrays; both NULL means q_set[p] = 2p, t_set[p] = 2p+1: left vs right of stereo frame p).
 * Outputs per pair: d_idx2/d_dist2 [n_pairs][max_keypoints][2] (may be NULL), d_matches
 * [n_pairs][max_keypoints], d_nmatches [n_pairs]. */
vsf_status vsf_match_batch_dev(vsf_ctx* ctx, const uint8_t* d_desc, const int32_t* d_counts, size_t set_stride,
                               const int32_t* d_q_set, const int32_t* d_t_set, int n_pairs, int32_t* d_idx2,
                               int32_t* d_dist2, vsf_dmatch* d_matches, int32_t* d_nmatches);
/* The benchmarked hot path for a batch of stereo frames: extract(left) + extract(right) + GetMatches(left,
 * right) (slam_frontend.cc:411-416).  d_imgs is [n_frames][2][h][w]-like with the strides above (image
 * index 2f = left, 2f+1 = right). */
vsf_status vsf_stereo_batch_dev(vsf_ctx* ctx, const uint8_t* d_imgs, int n_frames, size_t image_stride,
                                size_t row_stride, vsf_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts,
                                vsf_dmatch* d_matches, int32_t* d_nmatches);

/* ---------------- Detection masks: detectAndCompute's second argument (slam_frontend.cc:274-277) ----------------
 * The reference passes cv::noArray() there; a rig with its hood, the other eye's housing, a rectification wedge or a time
 * stamp in view passes a mask instead.  The rule below is RESTATED FROM MEMORY (OpenCV 3.2 orb.cpp / keypoint.cpp), not read
 * from the sources:
 *   - detectAndCompute builds a mask pyramid beside the image pyramid: level 0 is the caller's mask unchanged; level l >= 1 is
 *     resize(level l - 1, size_l, INTER_LINEAR) followed by threshold(., 254, 0, THRESH_TOZERO), taken from the already
 *     thresholded level l - 1.  A pixel of a level >= 1 is therefore 255 or 0, and 255 only where the fixed-point
 *     interpolation gives exactly 255; a masked region erodes from level to level.
 *   - computeKeyPoints, per level: FAST, then KeyPointsFilter::runByPixelsMask drops a corner whose own pixel
 *     mask_l[(int)(y + 0.5f)][(int)(x + 0.5f)] is 0, then runByImageBorder, retainBest(2 n_l), HarrisResponses,
 *     retainBest(n_l) (FAST_SCORE: the one cut), angles, blur, descriptors as without a mask.  The filter runs BEFORE both
 *     cuts: a slot a masked corner frees goes to the next-best corner of that level.  Level 0 passes any non-zero value,
 *     levels >= 1 only 255-derived pixels (a mask of 254 everywhere leaves level-0 keypoints only).
 *   - FastFeatureDetector::detect(image, kps, mask) (vsf_fast_detect) is the level-0 rule alone.
 * A mask is context state, set once per rig and kept in a slot: vsf_mask_set builds the slot's pyramid on the device (one byte
 * a pixel and level: vsf_mask_slot_bytes), and FAST applies the predicate where it emits its candidates -- no launch is added
 * and, with no mask in a launch, the kernels are the ones without the predicate.  Every capacity rule stays: a mask only
 * removes candidates.  With no mask set every output of every call is what it was.
 * Ordering: vsf_mask_set, vsf_mask_set_dev and vsf_mask_clear FLUSH INSIDE -- they send every frame that waits in the
 * ObserveImage queue, wait for every stream of the context, change the slot, and (set) return when the slot's pyramid is built:
 * every frame submitted before the call is extracted with the slot as it was, every frame and call after it sees the new
 * state.  They are calls for when the rig changes, not per frame. */
#define VSF_MAX_MASKS 64 /* 32 streams x 2 eyes */
/* mask: w x h bytes (the context's size), rows `stride` >= w bytes apart, any base address; host memory, resp. device memory
 * that stays valid until the call returns.  VSF_ERR_INVALID_ARG (slot unchanged): a null pointer, another size, stride < w,
 * slot outside [0, VSF_MAX_MASKS). */
vsf_status vsf_mask_set(vsf_ctx* ctx, int slot, const uint8_t* mask, int w, int h, size_t stride);
vsf_status vsf_mask_set_dev(vsf_ctx* ctx, int slot, const uint8_t* d_mask, int w, int h, size_t stride);
/* The slot holds no mask again (its memory is kept for the next set): images that name it are extracted without a mask. */
vsf_status vsf_mask_clear(vsf_ctx* ctx, int slot);
/* *is_set: 1 while the slot holds a mask. */
vsf_status vsf_mask_is_set(const vsf_ctx* ctx, int slot, int* is_set);
/* Bytes of device memory a set slot holds: one image's pyramid block, level 0 included. */
vsf_status vsf_mask_slot_bytes(const vsf_ctx* ctx, size_t* bytes);
/* Which slot the images of vsf_extract, vsf_extract_pair, vsf_extract_batch_dev, vsf_stereo_batch_dev, vsf_observe_stereo*
 * and vsf_fast_detect take: image i of a call `even_slot` when i is even (the left eye), `odd_slot` when i is odd; -1: no
 * mask.  Default (-1, -1).  A slot that holds no mask when the call is made is no mask.  Not for the ObserveImage queue's
 * submits: vsf_observe_set_stream_masks. */
vsf_status vsf_set_image_masks(vsf_ctx* ctx, int even_slot, int odd_slot);
vsf_status vsf_get_image_masks(const vsf_ctx* ctx, int* even_slot, int* odd_slot);
/* The queue's frames of `stream` (every submit form: raw, pix, compressed, reduced, device frames) take left_slot for the left
 * image and right_slot for the right one; -1: no mask; default (-1, -1), kept until set again.  A frame takes what its stream
 * names when it is SUBMITTED (as it takes the stream's pose), and the mask applies to the frame as the context extracts it:
 * after decode, gray conversion and the resize of a declared input size -- a mask is at the context's size.  Frames of several
 * streams with different slots, and frames without, share batches. */
vsf_status vsf_observe_set_stream_masks(vsf_ctx* ctx, int stream, int left_slot, int right_slot);
/* Test hook: level `level` of the slot's pyramid as 0 / non-zero bytes, level_w x level_h (vsf_level_info) at `ostride`. */
vsf_status vsf_debug_mask_level(vsf_ctx* ctx, int slot, int level, uint8_t* out, size_t ostride);

/* ---------------- the reference's own steps between matcher and outputs, on the device ---------------- */

/* Frontend::RemoveAmbigStereo (slam_frontend.cc:353-398) for n_frames stereo frames in time order, applied to the
 * outputs of vsf_stereo_batch_dev (same layouts: image 2f = left, 2f+1 = right of frame f).  F: the fundamental
 * matrix, 9 floats row major (HOST pointer).  thr_in: the threshold in force before frame 0 (the reference's static
 * starts at 10000, cc:353).  d_thr_override: NULL, or a DEVICE array of n_frames thresholds applied as they are
 * (multi-GPU: every rank derives them from all ranks' means, vision_slam_frontend_amd/distributed.py).
 * Outputs (device): d_means [n_frames]: mean residual over ALL matches of the frame, summed in match order (NaN for
 * a frame without matches: 0/0 as in the reference, whose static is then NaN for exactly the next frame -- that frame
 * keeps nothing -- and finite again afterwards; reproduced); d_thr
 * [n_frames + 1]: threshold applied to each frame and the one in force after the batch (written without override);
 * d_kp_out / d_desc_out / d_counts_out: both frames rebuilt from the surviving pairs in match order (row i of the
 * left frame matches row i of the right frame, cc:396-397), layouts as the inputs. */
vsf_status vsf_remove_ambig_stereo_batch_dev(vsf_ctx* ctx, const vsf_keypoint* d_kp, const uint8_t* d_desc,
                                             const vsf_dmatch* d_matches, const int32_t* d_nmatches, int n_frames,
                                             const float* F, float thr_in, const float* d_thr_override,
                                             float* d_means, float* d_thr, vsf_keypoint* d_kp_out,
                                             uint8_t* d_desc_out, int32_t* d_counts_out);
/* Frontend::GetFeatureMatches (slam_frontend.cc:282-309) for n_pairs (past set, current set) pairs: GetMatches, then
 * std::sort by DMatch::operator< (distance only; the permutation is libstdc++'s), then the cut to
 * int(size * best_percent).  Set addressing as vsf_match_batch_dev.  d_pairs: [n_pairs][max_keypoints][2] uint64
 * (FeatureMatch::feature_idx_initial = index in the past set, feature_idx_current = index in the current set),
 * d_npairs [n_pairs].  Needs max_keypoints < 65536. */
vsf_status vsf_feature_matches_batch_dev(vsf_ctx* ctx, const uint8_t* d_desc, const int32_t* d_counts,
                                         size_t set_stride, const int32_t* d_q_set, const int32_t* d_t_set,
                                         int n_pairs, float best_percent, uint64_t* d_pairs, int32_t* d_npairs);

/* The three steps of vsf_remove_ambig_stereo_batch_dev as separate calls, for the multi-GPU path: a rank computes the
 * residuals and per-frame means of ITS frames, all ranks exchange the means (one float per frame), every rank derives
 * the thresholds of the whole time-ordered step and filters its own frames (slam_frontend.cc:353, 392-394).
 * vsf_stereo_residuals_batch_dev keeps the residuals inside the context for the vsf_stereo_filter_batch_dev that follows. */
vsf_status vsf_stereo_residuals_batch_dev(vsf_ctx* ctx, const vsf_keypoint* d_kp, const vsf_dmatch* d_matches,
                                          const int32_t* d_nmatches, int n_frames, const float* F, float* d_means);
/* d_means [n]: the means of n consecutive frames in time order (all ranks' frames of one step).  d_thr_state: ONE device
 * float, the threshold in force before frame 0 (initialise it to 10000, cc:353); it is advanced to the value in force
 * after frame n - 1.  d_thr [n]: thr[0] = state, thr[k] = means[k - 1] + 2. */
vsf_status vsf_stereo_thresholds_dev(vsf_ctx* ctx, const float* d_means, int n, float* d_thr_state, float* d_thr);
vsf_status vsf_stereo_filter_batch_dev(vsf_ctx* ctx, const vsf_keypoint* d_kp, const uint8_t* d_desc,
                                       const vsf_dmatch* d_matches, const int32_t* d_nmatches, int n_frames,
                                       const float* d_thr, vsf_keypoint* d_kp_out, uint8_t* d_desc_out,
                                       int32_t* d_counts_out);

/* ---------------- VisionFeature on the device ---------------- */

/* Stereo calibration as Frontend uses it (FrontendConfig, slam_frontend.cc:565-644); all row-major floats. */
typedef struct {
  float projection_left[12];   /* config_.projection_left  = K_left  * [I | 0]   (cc:595-600, 619-622) */
  float projection_right[12];  /* config_.projection_right = K_right * A_right   (cc:602-611) */
  float camera_matrix_left[9]; /* config_.camera_matrix_left (cc:575-578) */
  float distortion_left[5];    /* k1 k2 p1 p2 k3 (cc:623-628) */
  float fundamental[9];        /* config_.fundamental (cc:635-644) */
  /* Rows of the DLT system cv::triangulatePoints solves per point: 6 = OpenCV <= 3.4.1 incl. the pinned 3.2.0
   * (x*P2-P0, y*P2-P1, x*P1-y*P0 per view), 4 = OpenCV >= 3.4.2 (third row dropped).  0 means 6. */
  int32_t triangulate_rows;
} vsf_calibration;

/* slam_types::VisionFeature (slam_types.h:60-75 / VisionFeature.msg) as a 28-byte record: uint64 feature_idx (two
 * words, little endian), Vector2f pixel, Vector3f point3d. */
typedef struct {
  uint32_t feature_idx_lo, feature_idx_hi;
  float pixel[2];
  float point3d[3];
} vsf_vision_feature;
/* slam_types::FeatureMatch (slam_types.h:77-89 / FeatureMatch.msg). */
typedef struct {
  uint64_t feature_idx_initial, feature_idx_current;
} vsf_feature_match;

/* The tail of Frontend::ObserveImage (slam_frontend.cc:437-443) for n_frames frames whose left / right frames were
 * rebuilt by RemoveAmbigStereo (layouts of vsf_remove_ambig_stereo_batch_dev's outputs: set 2f = left, 2f + 1 = right):
 * Calculate3DPoints (GetFeatureMatches(right, left) with best_percent 1, cv::triangulatePoints in sorted-match order,
 * (x,y,z)/w), VisionFeature(i, keypoint i, points[i]) -- a zero point where the reference's points[i] does not exist
 * (its quirk Q5) -- and UndistortFeaturePoints (cv::undistortPoints with P = K_left).
 * d_features [n_frames][max_keypoints], d_nfeatures [n_frames]; d_npoints [n_frames] (may be NULL): triangulated points
 * per frame.  Floating point: agrees with OpenCV to rounding (1e-5 relative), not bit for bit. */
vsf_status vsf_vision_features_batch_dev(vsf_ctx* ctx, const vsf_calibration* calib, const vsf_keypoint* d_kp,
                                         const uint8_t* d_desc, const int32_t* d_counts, int n_frames,
                                         vsf_vision_feature* d_features, int32_t* d_nfeatures, int32_t* d_npoints);

/* ---------------- The RViz point cloud of the reference's driver (slam_frontend_main.cc:155-173, 194-225) ----------------
 * slam_types::RobotPose as the driver's PublishVisualization reads it from a SLAMNode: Translation3f(loc) * Quaternionf. */
typedef struct {
  float loc[3];
  float quat_xyzw[4];
} vsf_pose;
/* AddFeaturePoints for n_frames frames whose vsf_vision_feature records are in device memory (the layouts of
 * vsf_vision_features_batch_dev's d_features / d_nfeatures).  Frame f keeps, IN FEATURE ORDER, every feature whose point3d
 * has three finite coordinates, (double)z > 0.1, (double)norm > 0.5 and (double)norm < 20.0 -- norm the float sqrtf of the
 * float sum of squares, as Vector3f::norm() -- and writes M_f * point3d widened to double, three consecutive doubles per point
 * (the body of a geometry_msgs/Point[]): d_points [n_frames][max_keypoints][3], d_npoints [n_frames].  M_f =
 * (Translation(poses[f].loc) * poses[f].quat) * cam_to_robot, evaluated in float; `poses` (n_frames of them) and cam_to_robot
 * (3 x 4 row-major: config.left_cam_to_robot) are HOST memory, read before the call returns.  Nothing is written behind
 * d_npoints[f] points of a frame.  The zero points of quirk Q5 have norm 0 and fall out by the predicate.  Rounding and
 * summation order: vision_slam_frontend_amd/csrc/vsf_world_points.h, which the host mirror's AddFeaturePoints includes as well
 * -- the two agree bit for bit.  Deterministic (no atomics); asynchronous on the context's stream like every *_dev call. */
vsf_status vsf_world_points_batch_dev(vsf_ctx* ctx, const vsf_vision_feature* d_features, const int32_t* d_nfeatures,
                                      int n_frames, const vsf_pose* poses, const float cam_to_robot[12], double* d_points,
                                      int32_t* d_npoints);

/* The same for ONE frame whose records are in HOST memory, synchronous (upload, the kernel, download): what the host
 * Frontend's per-call mode runs once per node.  points_out holds `cap` points of three doubles; *n_out = points kept
 * (VSF_ERR_CAPACITY and nothing copied if that is more than cap; n_features above max_keypoints likewise). */
vsf_status vsf_world_points(vsf_ctx* ctx, const vsf_vision_feature* features, int n_features, const vsf_pose* pose,
                            const float cam_to_robot[12], double* points_out, int cap, int* n_out);

/* Compact output payload of a batch (what a rank sends to rank 0): counts first, then records sized by the counts.
 *   u32 magic 'VSF1', n_frames, n_pairs, total_bytes | u32 nfeatures[n_frames] | u32 npairs[n_pairs] |
 *   vsf_vision_feature x sum(nfeatures), frame after frame | vsf_feature_match x sum(npairs), pair after pair
 * d_pairs / d_npairs: outputs of vsf_feature_matches_batch_dev ([n_pairs][max_keypoints][2] uint64); n_pairs may be 0.
 * Needs payload_cap >= vsf_packed_outputs_capacity(ctx, n_frames, n_pairs) to be safe for any counts. */
size_t vsf_packed_outputs_capacity(const vsf_ctx* ctx, int n_frames, int n_pairs);
vsf_status vsf_pack_outputs_dev(vsf_ctx* ctx, const vsf_vision_feature* d_features, const int32_t* d_nfeatures,
                                int n_frames, const uint64_t* d_pairs, const int32_t* d_npairs, int n_pairs,
                                uint8_t* d_payload, size_t payload_cap);

/* ---------------- Frontend::ObserveImage (slam_frontend.cc:400-472) as a queue of stereo frames ---------------- */

/* Everything ObserveImage computes between OdomCheck and the node / factor bookkeeping, for stereo frames given as host
 * images: upload (pinned staging), ExtractFeatures x 2 (cc:411-412), GetMatches (cc:414), RemoveAmbigStereo (cc:417, the
 * threshold lives in the context like the reference's file-static), GetFeatureMatches against the <= frame_life frames kept
 * from earlier calls (cc:424-434; their filtered descriptors stay resident in HBM), Calculate3DPoints (cc:437),
 * VisionFeature assembly + UndistortFeaturePoints (cc:438-443), one compact result per frame.  Every frame joins the window
 * and the oldest leaves once frame_life are kept (cc:467-470).
 *
 * vsf_observe_submit copies the two images into pinned staging and returns a ticket; vsf_observe_collect waits for that
 * frame and hands over its result; vsf_observe_stereo is submit + collect.  Frontend::ObserveImage returns what OdomCheck
 * decided (cc:404-409), so nothing in the reference's control flow needs a frame's result before the next frame arrives: a
 * caller may keep up to `depth` frames submitted and not collected.  Frames that wait are COALESCED: they leave for the GPU
 * as one batched extraction + one batched tail (the threshold chain and the temporal window run through the batch in frame
 * order) -- a frame's chain of ~25 launch-bound kernels costs the same whether it carries one frame or thirty.  A batch
 * leaves: when the GPU is idle and no frame has arrived for 100 us (a lone frame whose caller collects it leaves at once: the
 * synchronous call is a batch of one); when `min_batch` frames wait and fewer than `in_flight` batches are on the GPU; when
 * a full batch (max_images / 2 frames, at most `depth`) waits; or when a waiting frame is collected.  While the GPU is busy
 * or frames keep arriving, frames accumulate: the batch size follows the caller's rate.  Results are those of one frame at
 * a time, bit for bit, whatever the batches were (tests/test_gpu_observe.py).  A queue of depth >= 4 owns a host thread that
 * takes half of a streaming frame's staging copy (VSF_OPT_OBSERVE_COPY_THREAD; host memory only) and, on request, a launcher
 * thread (VSF_OPT_OBSERVE_THREAD: the caller then only stages and collects; every other entry point of the context first
 * sends what waits in the queue, so nothing ever runs beside it).
 * Tickets are collected in the order they were issued; a submit beyond `depth` uncollected frames returns
 * VSF_ERR_INVALID_ARG.  Consecutive frames with different calibrations or best_percent never share a batch; frame_life
 * changes only while the queue is empty (the window starts over).  These calls feed stream 0 of the queue's streams
 * (vsf_observe_set_streams, below): with the default of one stream that is the whole queue.
 *
 * Result (little endian, *out_bytes bytes, at most vsf_observe_capacity()):
 *   u32 magic 'VSFO', n_pairs, nfeat, total_bytes, n_left, n_right (raw keypoints), n_stereo_matches, n_points,
 *   f32 mean residual, threshold applied, threshold in force afterwards, u32 result overflow, u32 extraction overflow
 *   (either makes the collect return VSF_ERR_CAPACITY -- for THIS frame only), u32 decoder status (word 13; compressed
 *   frames: bit 0 the LEFT, bit 1 the RIGHT file was refused on the device -- the collect returns VSF_ERR_INVALID_ARG for
 *   THIS frame only; always 0 for raw frames), 2 x u32 reserved (the debug images' words)                   (64 bytes)
 *   u32 npairs[n_pairs], padded to a multiple of 4 words
 *   vsf_vision_feature x nfeat
 *   vsf_feature_match x npairs[p], p = 0 .. n_pairs-1: the temporal factors, oldest kept frame first (the order of
 *     frame_list_), and LAST the right->left matches of Calculate3DPoints in sorted order (n_pairs = kept frames + 1)
 *   vsf_keypoint x nfeat, then 32-byte descriptors x nfeat: the left frame as RemoveAmbigStereo rebuilt it (cc:396)
 * vsf_observe_reset forgets the window and puts the threshold back to 10000 (cc:353). */
size_t vsf_observe_capacity(const vsf_ctx* ctx, int frame_life);
/* depth: frames that may be submitted and not collected (0: max_images / 2; up to 1024 -- the staging and result rings are
 * pinned host memory, depth x (2 images + vsf_observe_capacity)); a batch holds min(depth, max_images / 2) frames at most.
 * min_batch (0 = a whole batch when depth >= two batches, else half the depth): while the GPU is busy, fewer waiting frames than this do not leave -- an idle GPU takes
 * whatever waits, a collect sends everything -- because a batch costs the host ~45 launches whatever it carries.  in_flight (0 = 2, at most 3): batches on the GPU at a time.  Call it before the first submit or while
 * the queue is empty; changing depth rebuilds the queue (window and threshold start over). */
vsf_status vsf_observe_configure(vsf_ctx* ctx, int depth, int min_batch, int in_flight);
vsf_status vsf_observe_stereo(vsf_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride,
                              const vsf_calibration* calib, float best_percent, int frame_life, uint8_t* out,
                              size_t cap, size_t* out_bytes);
vsf_status vsf_observe_submit(vsf_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride,
                              const vsf_calibration* calib, float best_percent, int frame_life, int64_t* ticket);
vsf_status vsf_observe_collect(vsf_ctx* ctx, int64_t ticket, uint8_t* out, size_t cap, size_t* out_bytes);
/* The same without the copy: *out points at the result inside the context's pinned result ring; it stays valid until `depth`
 * further frames have been submitted (the first word, the magic, reads 0 there). */
vsf_status vsf_observe_collect_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** out, size_t* out_bytes);
/* The same frames as sensor_msgs::CompressedImage payloads (the reference's caller, slam_frontend_main.cc:98-133: cv::imdecode
 * IMREAD_GRAYSCALE, then for bayer_rggb8 topics COLOR_BayerBG2BGR + COLOR_BGR2GRAY): baseline / progressive JPEG or PNG of the
 * context's size, left and right told apart by their first bytes, each whatever it is.  The submit does the decoders' host
 * half for the two files (every marker, table and chunk length checked: what vsf_imdecode_gray_batch refuses is refused here
 * with the same status) and copies them into a pinned ring of depth x 2 slots of `cap` bytes (vsf_observe_set_compressed_cap;
 * a larger file: VSF_ERR_CAPACITY).  A refused submit issues no ticket and leaves the queue as it was.  When the batch
 * leaves, its files go up in ONE copy command, are decoded on the queue's copy stream (beside the previous batch's
 * extraction and tail) into the batch's image buffer, demosaiced there when `bayer` is set, and the batched extraction and
 * tail run as for raw frames: results equal those of vsf_observe_submit on the decoded images, byte for byte.  A batch may
 * mix formats and raw frames; frames with different `bayer` never share one.
 * DEFINED DEVIATION -- a file the DEVICE refuses (PNG data libpng answers with png_error, a JPEG stream that broke off at a
 * missing restart marker; what sets bit 1 of vsf_sync's status after the batched decoders): a frame is never taken out of
 * the queue once it has a ticket, so that image is replaced by an ALL-ZERO image before extraction (no corners: a node
 * without features; the threshold chain takes the NaN of a frame without stereo matches, as the reference's does), result
 * header word 13 says which file it was and THAT ticket's collect returns VSF_ERR_INVALID_ARG; every other frame is what it
 * would be had the refused image been submitted raw as zeros.  (The reference hands ObserveImage whatever cv::imdecode
 * returned: an empty Mat.)  No call of the queue waits for the GPU that does not wait for raw frames. */
vsf_status vsf_observe_submit_compressed(vsf_ctx* ctx, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                         size_t right_bytes, int bayer, const vsf_calibration* calib, float best_percent,
                                         int frame_life, int64_t* ticket);
vsf_status vsf_observe_stereo_compressed(vsf_ctx* ctx, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                         size_t right_bytes, int bayer, const vsf_calibration* calib, float best_percent,
                                         int frame_life, uint8_t* out, size_t cap, size_t* out_bytes);
/* Bytes a compressed file may have (0: vsf_observe_default_compressed_cap of the context's size).  Before the first
 * compressed submit or while the queue is empty; the ring (vsf_observe_compressed_ring_bytes(depth, cap) of pinned memory)
 * is built by the next compressed submit. */
vsf_status vsf_observe_set_compressed_cap(vsf_ctx* ctx, size_t cap_per_image);
/* The default of that cap: width x height + 64 KB (a lossless file of a noisy image is a little larger than the image; a
 * camera's JPEG is a tenth of it).  0 for a size below 1 x 1.  No context, no device. */
size_t vsf_observe_default_compressed_cap(int width, int height);
/* The size a JPEG / PNG file's header states (PNG: IHDR; JPEG: the first SOF0 / SOF1 / SOF2): what sizes a context for a
 * stream of such files.  Nothing else of the file is checked.  VSF_ERR_UNSUPPORTED for another format.  No context. */
vsf_status vsf_compressed_image_size(const uint8_t* file, size_t nbytes, int* width, int* height);
/* Does not wait and sends nothing: *ready = 1 when the frame's result is there (its collect will not wait), 0 while it still
 * waits in staging or is on the GPU.  What a caller that books results as they come asks before each collect. */
vsf_status vsf_observe_poll(vsf_ctx* ctx, int64_t ticket, int* ready);
vsf_status vsf_observe_reset(vsf_ctx* ctx);
/* STREAMS: several independent sequences of frames -- several cameras or robots on one GPU, several bags replayed at once --
 * through ONE context and ONE queue.  Every stream has its own RemoveAmbigStereo threshold (10000 at first), its own temporal
 * window of frame_life kept frames and its own calibration and best_percent; frames of different streams wait in the same
 * queue and leave for the GPU in the same batch, so n cameras that have four frames waiting each fill a batch of 4 n instead
 * of paying n batches' ~45 launches.  Each stream's results are, byte for byte, those of a context of its own fed that
 * stream's frames alone (tests/test_gpu_observe_streams.py).
 *   n_streams: 1 .. VSF_OBSERVE_MAX_STREAMS, 1 by default.  Before the first submit or while the queue is empty, like
 * vsf_observe_configure; another value rebuilds the queue (every window and threshold starts over).
 *   What one more stream costs in HBM: its ring of filtered descriptor sets and their counts,
 *       (frame_life + bmax) x (32 x max_keypoints + 4) + 4 bytes,   bmax = min(depth, max_images / 2) frames per batch
 * (2.4 MB at 2000 keypoints, frame_life 5, 32 frames per batch) -- against the ~25 MB per frame of extraction buffers and the
 * tail's scratch that a context of its own would own again.  The pinned staging and result rings are the queue's: `depth`
 * counts the uncollected frames of all streams together.
 *   Tickets are global and are collected in the order they were issued, whatever the streams.  frame_life is one value per
 * context.  The cut rule is per stream: a frame whose calibration or best_percent differs from the waiting frame of ITS OWN
 * stream in front of it starts a new batch; frames of different streams may differ in both and share one.  Frames with
 * different `bayer` never share a batch.
 *   A stream outside [0, n_streams): VSF_ERR_INVALID_ARG, no ticket, the queue as it was.
 *   Debug images of several streams need vsf_observe_set_debug_seeds, which gives every stream rand()'s colour sequence of
 * its own.  Without that call vsf_observe_set_debug_images / _jpeg / _png with more than one stream return
 * VSF_ERR_UNSUPPORTED, and so does vsf_observe_set_streams(> 1) while debug images are on: the stereo lines' colours would
 * come from ONE sequence, the process's rand(), whatever stream a frame belongs to. */
#define VSF_OBSERVE_MAX_STREAMS 64
vsf_status vsf_observe_set_streams(vsf_ctx* ctx, int n_streams);
vsf_status vsf_observe_submit_stream(vsf_ctx* ctx, int stream, const uint8_t* left, const uint8_t* right, int w, int h,
                                     size_t stride, const vsf_calibration* calib, float best_percent, int frame_life,
                                     int64_t* ticket);
vsf_status vsf_observe_submit_compressed_stream(vsf_ctx* ctx, int stream, const uint8_t* left, size_t left_bytes,
                                                const uint8_t* right, size_t right_bytes, int bayer,
                                                const vsf_calibration* calib, float best_percent, int frame_life,
                                                int64_t* ticket);
/* The same frames read as cv::imdecode(msg.data, IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) reads them (reduce = 2, 4, 8; reduce = 1
 * is vsf_observe_submit_compressed_stream with bayer = 0): JPEG files of up to `reduce` times the context's size a side, decoded
 * inside the batch by libjpeg's reduced inverse DCTs (vsf_imdecode_reduced_gray_batch) straight to the context's size.  Every
 * rule of vsf_observe_submit_compressed_stream holds, with the size rule applied per file: a file of W x H is taken when
 * ceil(W / reduce) x ceil(H / reduce) (vsf_reduced_size) is the context's size -- VSF_ERR_INVALID_ARG otherwise, and for a
 * reduce outside {1, 2, 4, 8}; a PNG file with reduce > 1 is VSF_ERR_UNSUPPORTED (cv::imdecode would decode it whole and call
 * cv::resize: that is a declared input size, vsf_observe_set_input_size, not this call).  A file the host refuses issues no ticket and leaves the queue as it was; a file the
 * device refuses fails its own ticket through status word 13, as for full-size files.  The byte cap
 * (vsf_observe_set_compressed_cap) applies to the file as it is: files of a larger camera usually need a larger cap than the
 * default of the context's size.
 *   There is no `bayer` argument: a mosaic cannot be reduced in the DCT domain (the reduced image of a mosaic is not the
 * mosaic of the reduced image); bayer_rggb8 topics stay at full size through the calls above.
 *   THE CALIBRATION IS THE CALLER'S, FOR THE REDUCED IMAGE.  The library scales nothing: K, the distortion terms and the
 * fundamental matrix handed in must describe the ceil(W / reduce) x ceil(H / reduce) image the extraction sees.
 *   BATCHING: frames of different `reduce` -- and full-size compressed frames and raw frames -- SHARE a batch and its one
 * upload; inside the upload a decode run ends where the format or the denominator changes.  Results do not depend on it: each
 * frame's result is, byte for byte, that of vsf_observe_submit on the images the library decodes.
 *   vsf_observe_stats value [23] counts the frames launched with reduce > 1. */
vsf_status vsf_observe_submit_compressed_reduced(vsf_ctx* ctx, int stream, const uint8_t* left, size_t left_bytes,
                                                 const uint8_t* right, size_t right_bytes, int reduce,
                                                 const vsf_calibration* calib, float best_percent, int frame_life,
                                                 int64_t* ticket);
/* submit (stream 0) + collect of one such frame, as vsf_observe_stereo_compressed is for full-size files. */
vsf_status vsf_observe_stereo_compressed_reduced(vsf_ctx* ctx, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                                 size_t right_bytes, int reduce, const vsf_calibration* calib,
                                                 float best_percent, int frame_life, uint8_t* out, size_t cap,
                                                 size_t* out_bytes);
/* Forgets ONE stream's window and puts its threshold back to 10000: its next frame is the first frame of a fresh context.
 * Legal while no frame of that stream is submitted and not collected (else VSF_ERR_INVALID_ARG); the other streams, frames
 * in flight included, are untouched.  vsf_observe_reset stays "all streams" (and drops what waits). */
vsf_status vsf_observe_reset_stream(vsf_ctx* ctx, int stream);
/* A DECLARED INPUT SIZE per stream: the frames of `stream` arrive at width x height -- any size in 1 .. 32767 a side, larger or
 * smaller than the context's, each axis by its own ratio -- and the queue brings them to the context's size with
 * cv::resize(img, Size(ctx width, ctx height)) (INTER_LINEAR, vsf_resize_gray_batch_dev's kernel) on its copy stream, where
 * decode and demosaic already run beside the previous batch's extraction.  From there on such a frame is a frame like any
 * other: each result is, byte for byte, that of vsf_observe_submit on the resized images.  (0, 0): the context's size again.
 *   Legal while no frame of that stream is submitted and not collected (else VSF_ERR_INVALID_ARG, the rule of
 * vsf_observe_reset_stream); VSF_ERR_INVALID_ARG too for a stream outside [0, n_streams) or a side outside 1 .. 32767.  The
 * size is kept across vsf_observe_reset and vsf_observe_reset_stream and dropped when vsf_observe_set_streams changes the
 * number of streams.  A stream that was never told a size behaves exactly as without this call: same bytes, same launches.
 *   What each submit takes on such a stream:
 *     vsf_observe_submit_stream (vsf_observe_submit / vsf_observe_stereo for stream 0): w, h must be the declared size.
 *     vsf_observe_submit_dev: the images have the declared size, at any base address and pitch >= its width.
 *     vsf_observe_submit_compressed_stream: the FILE's own size must be the declared size; it is decoded whole (`bayer`:
 *       demosaiced at that size), then resized -- cv::resize(DecodeImage(msg)).  For a PNG topic that is what
 *       cv::imdecode(IMREAD_REDUCED_GRAYSCALE_N) does: declare the file's W x H on a context of (W / N) x (H / N), floor
 *       division.  The byte cap stays sized by the context: raise it with vsf_observe_set_compressed_cap.
 *     vsf_observe_submit_compressed_reduced: VSF_ERR_INVALID_ARG for reduce > 1 -- a reduced JPEG decode combined with a
 *       declared size is not built.
 *   A frame of another size than its stream's declared one is VSF_ERR_INVALID_ARG: no ticket, nothing booked or launched, the
 * queue as it was.  A Bayer frame wider than 16384 is VSF_ERR_UNSUPPORTED (the demosaic's limit).
 *   BATCHING: frames of streams with different declared sizes, and of streams with none, SHARE a batch; a batch issues one
 * resize launch per run of consecutive frames of one size.  Results do not depend on it.
 *   THE CALIBRATION IS THE CALLER'S, FOR THE RESIZED IMAGE: the library scales nothing.  Debug images are drawn from the
 * resized images.
 *   WHAT IT COSTS, built by the first frame that needs it and sized by the LARGEST declared size: an image's place is its
 * height x (width rounded up to 64) bytes rounded up to 256, a slot two of them.  Raw host frames wait in a pinned ring of
 * `depth` slots (629 MB at depth 256 and 1280 x 960 -- choose the depth accordingly) and are uploaded into one of four
 * device buffers of bmax slots, which compressed frames are decoded into as well; device frames wait in a device ring of
 * `depth` slots and are resized out of it without a copy.  Declaring a LARGER size later makes the next submit send what
 * waits, wait for the device and rebuild these buffers.
 *   vsf_observe_stats values [26] frames resized, [27] kernel launches and copy commands this path issued, [28] bytes of
 * every buffer it owns -- all 0 for a queue that never saw a declared size -- and [29] batches whose frames came in at more
 * than one size. */
vsf_status vsf_observe_set_input_size(vsf_ctx* ctx, int stream, int width, int height);
/* Frames that ALREADY LIVE IN DEVICE MEMORY -- a tensor of the caller's framework, the output of vsf_imdecode_gray_batch /
 * vsf_bayer_bg_to_gray_batch_dev on the caller's own stream, a camera SDK's or video decoder's buffer, the caller's own
 * preprocessing kernel -- enter the queue without crossing to the host: what vsf_set_input_event is to the batched calls.
 *   frames[0 .. n) are n CONSECUTIVE frames of queue stream `stream`, oldest first; tickets[i] is frame i's (consecutive).
 * Each image is width x height bytes (the context's size) at ANY base address and ANY pitch >= width; left and right are
 * independent of each other.  pixfmt: VSF_PIX_MONO8, or VSF_PIX_BAYER_RGGB8 -- mosaics that go through
 * COLOR_BayerBG2BGR + COLOR_BGR2GRAY on the device, as the compressed frames' `bayer` does (frames with different `bayer`
 * never share a batch).
 *   ORDERING: the call is stream-ordered on `producer_stream` (a hipStream_t; NULL = the default stream), like
 * hipMemcpyAsync.  The images may still be being produced by work queued earlier on that stream, and they may be
 * overwritten by work queued on that stream after the call returns.  The call never waits for the GPU.
 *   What it does: ONE kernel launch on the producer's stream copies the 2 n images into the frames' slots of a device ring
 * (vsf_observe_device_ring_bytes(depth) bytes of HBM, built by the first such call) and an event recorded behind it is
 * what the batch's copy stream waits for; when the batch leaves, its device frames go from the ring into the batch's image
 * buffer in one copy command per contiguous run of them (two where the run wraps the ring), beside the raw frames' upload
 * and the decoders' output.  The kernel reads only aligned 4-byte words that hold at least one pixel of the image: a row
 * may end on the last byte of its allocation.  Everything behind that -- cut rules, tickets, collect / poll / view,
 * reset / reset_stream, debug images and their files -- is as for raw frames, and so are the results, byte for byte.
 *   THE CALLER'S PROMISE, as with vsf_set_stream: the pointers are device memory of the context's device and
 * producer_stream is a stream of that device that is not being captured into a graph.  Neither is checked.
 *   A refused call issues no ticket, books nothing and launches nothing.  VSF_ERR_INVALID_ARG: a null pointer (ctx, frames,
 * an image, calib, tickets), n < 1, n larger than the free slots (depth - frames submitted and not collected), a pitch
 * smaller than the width, a stream outside [0, n_streams), an unknown pixfmt -- and whatever vsf_observe_submit refuses
 * (triangulate_rows, another frame_life while frames wait, a queue whose launch failed; VSF_ERR_UNSUPPORTED for
 * max_keypoints >= 65536). */
typedef struct {
  const void* left;
  const void* right;
  size_t left_pitch, right_pitch;
} vsf_dev_frame;
/* PIXEL FORMATS of raw frames.  The codes 2 .. 15 are unknown and STAY unknown for good (every call that takes a pixfmt
 * answers them, negatives and codes above 22 with VSF_ERR_INVALID_ARG): new formats start at 16.
 *   MONO8: the bytes are the gray image.
 *   BAYER_*8, one byte per pixel: COLOR_Bayer*2BGR + COLOR_BGR2GRAY (slam_frontend_main.cc:101-106) -- imgproc's
 * Bayer2RGB_<uchar>, bilinear, the one-pixel frame copied from its inner neighbour (columns first, then rows), then
 * RGB2Gray<uchar>.  The order is named as sensor_msgs names it, by the first two pixels of the first two rows, i.e. by
 * where RED sits:  RGGB (even x, even y),  GRBG (odd x, even y),  GBRG (even x, odd y),  BGGR (odd x, odd y).  An image
 * with a side below 3 comes out all zero (OpenCV's loops leave it so); a mosaic is at most 16384 wide.
 *   BGR8 / RGB8 (3 bytes per pixel), BGRA8 / RGBA8 (4): RGB2Gray<uchar> on the channels in the order the name gives,
 * gray = (1868 B + 9617 G + 4899 R + 8192) >> 14; alpha is ignored.
 *   16-bit, YUV and planar formats are not taken: the reference states no rule for them. */
enum {
  VSF_PIX_MONO8 = 0,
  VSF_PIX_BAYER_RGGB8 = 1,
  VSF_PIX_BAYER_GRBG8 = 16,
  VSF_PIX_BAYER_GBRG8 = 17,
  VSF_PIX_BAYER_BGGR8 = 18,
  VSF_PIX_BGR8 = 19,
  VSF_PIX_RGB8 = 20,
  VSF_PIX_BGRA8 = 21,
  VSF_PIX_RGBA8 = 22
};
/* Bytes per pixel of a format: 1, 3 or 4; 0 for an unknown code.  No context, no device. */
int vsf_pixfmt_bytes_per_pixel(int pixfmt);
/* The format of a sensor_msgs/Image encoding: "mono8", "bayer_rggb8", "bayer_grbg8", "bayer_gbrg8", "bayer_bggr8", "bgr8",
 * "rgb8", "bgra8", "rgba8".  Anything else is VSF_ERR_UNSUPPORTED (a null pointer VSF_ERR_INVALID_ARG), *pixfmt untouched.
 * No context, no device. */
vsf_status vsf_pixfmt_from_encoding(const char* ros_encoding, int* pixfmt);
/* (vsf_observe_submit_dev takes EVERY format above.  An image is width x height pixels of vsf_pixfmt_bytes_per_pixel bytes:
 * a pitch must be >= width x that, and the launch's rule about what it reads holds for rows of that many bytes.  Mosaics of
 * the four orders wait in the device ring as MONO8 does; packed colour waits in a device ring of big slots -- the ring
 * vsf_observe_set_input_size builds, sized by BYTES per row -- and becomes gray inside the batch.) */
vsf_status vsf_observe_submit_dev(vsf_ctx* ctx, int stream, const vsf_dev_frame* frames, int n, int pixfmt,
                                  void* producer_stream, const vsf_calibration* calib, float best_percent, int frame_life,
                                  int64_t* tickets);
/* RAW HOST FRAMES OF ANY PIXEL FORMAT: sensor_msgs/Image as the driver publishes it (vsf_pixfmt_from_encoding maps its
 * `encoding`).  left / right: width x height pixels, rows stride_bytes apart, stride_bytes >= width x bytes per pixel;
 * width x height is the stream's declared size (vsf_observe_set_input_size) or the context's.
 *   VSF_PIX_MONO8: this IS vsf_observe_submit_stream, byte for byte and launch for launch.
 *   Mosaics are staged and uploaded as gray frames are -- the batch's one copy -- into the buffer compressed mosaics are
 * decoded into, and ONE launch on the copy stream (where decode, demosaic and resize run) makes the batch's gray images.
 *   Packed colour waits in the pinned ring of big slots that a declared input size builds, sized by bytes per row (3 - 4 x
 * the pinned memory and 3 - 4 x the bytes of the upload, which is what bounds this path); the first frame that needs more
 * room than the slots have does what declaring a larger size does: what waits is sent, the device is waited for, the
 * buffers are rebuilt.  One launch converts a run of such frames straight into the batch's images.
 *   With a declared input size the order is cv::resize(to_gray(frame)): gray at the arriving size, then the resize.
 *   BATCHES: a batch holds frames of ONE pixel format -- the rule `bayer` follows: a frame of another format sends what
 * waits first.  Results do not depend on how frames were batched, and they are those of vsf_observe_submit_stream fed the
 * gray images, byte for byte.
 *   A refused call issues no ticket (*ticket = -1), books nothing and launches nothing.  VSF_ERR_INVALID_ARG: an unknown
 * pixfmt (2 .. 15, negative, above 22), stride_bytes < width x bytes per pixel, another size than the stream's, and
 * whatever vsf_observe_submit_stream refuses.  VSF_ERR_UNSUPPORTED: a mosaic wider than 16384, a colour image of 2^31
 * bytes or more.
 *   vsf_observe_stats [30] frames that came in one of the formats 16 .. 22 or as a raw host mosaic, [31] launches and copy
 * commands issued for them (a batch's conversion, the uploads out of the big slots), [32] bytes of every buffer such a frame
 * made the queue build or enlarge (the mosaics' buffer and the big slots: shared with the compressed and resize paths and
 * counted in [13] / [28] too) -- all 0 for a queue that never saw such a frame. */
vsf_status vsf_observe_submit_stream_pix(vsf_ctx* ctx, int stream, const uint8_t* left, const uint8_t* right, int width,
                                         int height, size_t stride_bytes, int pixfmt, const vsf_calibration* calib,
                                         float best_percent, int frame_life, int64_t* ticket);
/* The Bayer order of a stream's COMPRESSED mosaics: what vsf_observe_submit_compressed(_stream) decodes with bayer != 0 is
 * demosaiced in this order (one of the four VSF_PIX_BAYER_* codes; anything else is VSF_ERR_INVALID_ARG).  A stream never
 * told is RGGB, so the existing calls and their `bayer` argument mean what they meant.  Legal when
 * vsf_observe_reset_stream is (no frame of the stream submitted and not collected, else VSF_ERR_INVALID_ARG); kept across
 * resets, dropped when vsf_observe_set_streams changes the count. */
vsf_status vsf_observe_set_bayer_order(vsf_ctx* ctx, int stream, int pixfmt);
/* HBM the device ring takes in a queue of `depth` frames (0: the depth vsf_observe_configure set, or its default):
 * depth x 2 images at the staging pitch (width rounded up to 64) -- 157 MB at depth 256 and 640 x 480.  0 for a depth outside
 * [0, 1024].  No device work. */
size_t vsf_observe_device_ring_bytes(const vsf_ctx* ctx, int depth);
/* What the queue did since it was built: out[0..n) of { frames launched, batches, largest batch, batches of one frame that
 * ran on one stream, launches forced by a collect or a change of parameters, launches that had to wait for a batch slot,
 * depth, frames per batch at most, then the host's nanoseconds inside staging copies, batch launches, waits for results,
 * compressed frames launched, copy commands + kernel launches the compressed path issued, bytes of every buffer the
 * compressed path owns (file ring, blobs, decoder scratch, mosaics) -- the last three are 0 for a queue that has only seen
 * raw frames; [14] launches of the compressed debug images; [15] streams (vsf_observe_set_streams), [16] batches that
 * carried frames of more than one stream; [17] device frames launched (vsf_observe_submit_dev), [18] kernel launches and
 * copy commands the device path issued (a submit's one launch, a batch's copies out of the ring, its demosaic where no
 * compressed frame brings one), [19] bytes of the device ring -- the last three are 0 for a queue that has seen no device
 * frame; [20] .. [22] the point cloud's (vsf_observe_set_world_points); [23] frames launched at a reduced size
 * (vsf_observe_submit_compressed_reduced with reduce > 1); [24], [25] the colour generators' (vsf_observe_set_debug_seeds);
 * [26] .. [29] vsf_observe_set_input_size's; [30] .. [32] the pixel formats' (vsf_observe_submit_stream_pix) }. */
vsf_status vsf_observe_stats(const vsf_ctx* ctx, int64_t* out, int n);
/* The queue's debug images (the Frontend's, slam_frontend.cc:74-115, 167-171, 458-466).  With the switch on, every batch's
 * tail also builds each frame's drawing operations on the device from the filtered keypoints and sorted pairs it holds,
 * draws the stereo image (2w x h) and the match image (w x h) -- GRAY2BGR, 3 bytes per pixel, as vsf_draw_canvases draws --
 * and copies them into a pinned debug ring beside the result ring.  The stereo lines' colours are
 * cv::Scalar(rand() % 255, rand() % 255, rand() % 255) from the process's rand(), drawn ahead at submit (GCC's right-to-left
 * argument order: the first call is channel 2) and taken in frame and match order, so the colours are the reference's
 * sequence while rand() itself may run ahead of it.  Result header word 14 then says which images the frame has (bit 0
 * stereo: not without a right -> left match, cc:131-133; bit 1 match: not without a kept frame), word 15 how many colours
 * it took.  Off (the default): results, launches and their cost are exactly those without the switch.  It changes only
 * before the queue's first frame (or after vsf_observe_reset); the queue is then rebuilt with the threshold carried over. */
vsf_status vsf_observe_set_debug_images(vsf_ctx* ctx, int on);
/* A colour generator per stream, on the device: stream s takes the colours that srand(seeds[s]) followed by rand(), rand(),
 * ... gives in glibc (csrc/vsf_glibc_random.h states the generator once, for the device and the host) -- in the reference's
 * order, three calls per stereo pair, the first being channel 2, a frame taking clamp(pairs, 0, max_keypoints) of them.
 * Seed 1 is a fresh process; seed 0 is 1, as in glibc.  The states live in device memory (31 words and a position per
 * stream), seeded when the queue is built, by vsf_observe_reset, and by vsf_observe_reset_stream for that stream alone; in
 * every batch's tail one more kernel -- one wave per stream present -- draws the colours of that stream's frames in
 * submission order, carrying on where the stream's previous frame ended.  The process's rand() is never called, there is no
 * pinned colour ring and the submitting thread draws nothing.  The match image's previous frame is kept per stream as well.
 *   With seeds installed the three debug switches are accepted for any number of streams, and each stream's images, files
 * and header words 14 / 15 are those of a one-stream context of its own after srand(seeds[s])
 * (tests/test_gpu_observe_stream_debug.py).  One stream with a seed is legal: the old switch's bytes after srand(seed).
 *   The order of use is: streams, seeds, switch.  n must be the number of streams; (NULL, 0) goes back to the process's
 * rand().  Legal only while debug images are off and before the queue's first frame or after vsf_observe_reset; and with
 * seeds installed vsf_observe_set_streams with another count is refused: VSF_ERR_INVALID_ARG each, the queue as it was.
 *   Never called: statuses, bytes, launches and the use of rand() are exactly what they were.  vsf_observe_stats values
 * [24] frames whose colours came from a stream's generator, [25] launches of the colour kernel: 0 without seeds. */
vsf_status vsf_observe_set_debug_seeds(vsf_ctx* ctx, const uint32_t* seeds, int n);
/* A collected frame's debug images inside the pinned debug ring (NULL where the frame has none); valid under the rule of
 * vsf_observe_collect_view (until `depth` further frames have been submitted). */
vsf_status vsf_observe_debug_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** stereo, const uint8_t** match);
/* The debug images as JPEG FILES (an addition the reference does not have; its publish loop would put them into
 * sensor_msgs/CompressedImage): quality 1 .. 100 switches it on, 0 (the default) off.  Needs vsf_observe_set_debug_images on and
 * follows its rules (only before the queue's first frame or after vsf_observe_reset).  With it on each batch's tail encodes the
 * canvases it has just drawn as vsf_jpeg_encode_batch_dev does -- the files are what cv::imencode(".jpg") writes for the raw
 * canvases -- and only the files go home, into a pinned ring of depth slots of vsf_jpeg_encode_capacity(2w, h, 3) +
 * vsf_jpeg_encode_capacity(w, h, 3) bytes; the raw canvases stay on the device and vsf_observe_debug_view returns
 * VSF_ERR_INVALID_ARG.  Results (header words 14 / 15 included) are those of vsf_observe_set_debug_images alone.  Off: launches,
 * results and cost are exactly those without the call (vsf_observe_stats value 14 counts what the path launched). */
vsf_status vsf_observe_set_debug_jpeg(vsf_ctx* ctx, int quality);
/* A collected frame's two files inside that ring (NULL / 0 where the frame has no such image); lifetime as
 * vsf_observe_debug_view.  VSF_ERR_CAPACITY if a file did not fit its slot (the bound of vsf_jpeg_encode_capacity rules it out). */
vsf_status vsf_observe_debug_jpeg_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** stereo, size_t* stereo_bytes,
                                       const uint8_t** match, size_t* match_bytes);
/* The debug images as PNG FILES, lossless: on != 0 switches it on.  The rules of vsf_observe_set_debug_jpeg word for word (needs
 * vsf_observe_set_debug_images; only before the queue's first frame or after vsf_observe_reset): each batch's tail encodes the
 * canvases it has just drawn as vsf_png_encode_batch_dev does -- the files are what cv::imencode(".png") writes for the raw
 * canvases, so every byte of a canvas survives -- and only the files go home, into a pinned ring of depth slots of
 * vsf_png_encode_capacity(2w, h, 3) + vsf_png_encode_capacity(w, h, 3) bytes; the raw canvases stay on the device and
 * vsf_observe_debug_view returns VSF_ERR_INVALID_ARG.  Mutually exclusive with the JPEG form: whichever is asked for second
 * returns VSF_ERR_INVALID_ARG.  Results (header words 14 / 15 included) are those of vsf_observe_set_debug_images alone.  Off:
 * launches, results and cost are exactly those without the call (vsf_observe_stats value 14 counts what either path launched). */
vsf_status vsf_observe_set_debug_png(vsf_ctx* ctx, int on);
/* A collected frame's two PNG files inside that ring (NULL / 0 where the frame has no such image); lifetime as
 * vsf_observe_debug_view.  VSF_ERR_CAPACITY if a file did not fit its slot (the bound of vsf_png_encode_capacity rules it out). */
vsf_status vsf_observe_debug_png_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** stereo, size_t* stereo_bytes,
                                      const uint8_t** match, size_t* match_bytes);

/* The queue's point cloud: with the switch on, every batch's tail also runs vsf_world_points_batch_dev's kernel over the
 * VisionFeature records it has just made -- ONE more launch per batch, which writes each frame's points and their count
 * straight into the frame's slot of a pinned ring of points (depth x max_keypoints x 24 bytes, built only when the switch is
 * on; like the result ring it is written by the kernel itself, so no copy command and no host wait are added).  A node's pose
 * never changes once it is booked, so what the caller keeps is append-only: the concatenation of the collected frames' views.
 *   cam_to_robot: 3 x 4 row-major, config.left_cam_to_robot; read when `on` is not 0 (it may be NULL otherwise).
 *   Callable before the queue's first frame or after vsf_observe_reset, like vsf_observe_set_debug_images (the queue is then
 * rebuilt with the thresholds carried over); VSF_ERR_INVALID_ARG once the queue has issued a ticket.  The same switch with the
 * same matrix again changes nothing and is always accepted.
 *   Off (the default): results, launches, copies and their cost are exactly those without the call.  On or off, the result
 * record of vsf_observe_collect and vsf_observe_capacity are byte for byte the same.
 *   vsf_observe_stats values [20] frames whose points were launched, [21] kernel launches + copy commands of this path (one
 * per batch), [22] bytes of the ring of points and its counts: all 0 while the switch is off. */
vsf_status vsf_observe_set_world_points(vsf_ctx* ctx, int on, const float* cam_to_robot);
/* The pose the frames submitted AFTERWARDS on queue stream `stream` carry -- what Frontend::ObserveOdometry is to
 * ObserveImage.  Sticky; identity (loc 0, quaternion 0 0 0 1) at first; captured by each of the five submit calls when it is
 * made, so it may change between any two frames.  vsf_observe_reset_stream puts that stream's pose back to identity,
 * vsf_observe_reset every stream's.  Host bookkeeping only: it never waits, sends nothing, and is legal at any time, also with
 * the switch off (the pose is then never read).  loc: 3 floats, quat_xyzw: 4 floats. */
vsf_status vsf_observe_set_pose(vsf_ctx* ctx, int stream, const float* loc, const float* quat_xyzw);
/* A stream's own left_cam_to_robot (3 x 4 row-major) in place of vsf_observe_set_world_points' -- two cameras on one robot
 * never share one; m == NULL: the context's again.  Host bookkeeping like vsf_observe_set_pose: legal at any time, sticky,
 * captured by each submit, read only with the point cloud on.  Extrinsics belong to the camera, not to the sequence: kept
 * across vsf_observe_reset and vsf_observe_reset_stream, dropped when vsf_observe_set_streams changes the number of streams.
 * A stream outside [0, n_streams): VSF_ERR_INVALID_ARG. */
vsf_status vsf_observe_set_stream_cam_to_robot(vsf_ctx* ctx, int stream, const float* m);
/* A collected frame's points inside the pinned ring: *xyz points at *n points of three doubles (NULL where n is 0); lifetime
 * and ticket rules of vsf_observe_debug_view (collected, and fewer than `depth` frames submitted since).
 * VSF_ERR_INVALID_ARG with the switch off. */
vsf_status vsf_observe_world_points_view(vsf_ctx* ctx, int64_t ticket, const double** xyz, int32_t* n);

/* ---------------- Host checks of the compressed path (no context, no device) ----------------
 * What vsf_observe_submit_compressed computes and checks on the host, callable on their own so that tests without a GPU --
 * the sanitizer build among them -- reach it.  Not needed by a caller of the queue. */
/* Bytes of one file's slot in the pinned ring: the cap rounded up to 64; 0 for a cap of 0 or above 1 GB. */
size_t vsf_observe_compressed_slot_bytes(size_t cap_per_image);
/* Bytes of the ring: depth x 2 slots; 0 for a depth outside 1..1024 or a cap without a slot. */
size_t vsf_observe_compressed_ring_bytes(int depth, size_t cap_per_image);
/* What a submit does with ONE payload before anything is booked: *kind = 1 (JPEG) / 2 (PNG) and VSF_OK, or
 * VSF_ERR_UNSUPPORTED (neither format), VSF_ERR_CAPACITY (larger than cap_per_image; before it is parsed), or the
 * refusal of that decoder's host half.  force_serial: the context's one-wave-JPEG switch (vsf_debug_jpeg_serial), which
 * changes the plan that is laid out, never what is refused. */
vsf_status vsf_observe_probe_compressed(const uint8_t* file, size_t nbytes, int width, int height, size_t cap_per_image,
                                        int force_serial, int* kind);
/* The same for vsf_observe_submit_compressed_reduced: width x height is the context's size, the file must reduce to it
 * (VSF_ERR_INVALID_ARG otherwise, and for a reduce outside {1, 2, 4, 8}); a PNG file with reduce > 1 is VSF_ERR_UNSUPPORTED.
 * The cap applies to the file as it is. */
vsf_status vsf_observe_probe_compressed_reduced(const uint8_t* file, size_t nbytes, int reduce, int width, int height,
                                                size_t cap_per_image, int force_serial, int* kind);

/* ---------------- Debug images: cv::circle / cv::line onto GRAY2BGR canvases (slam_frontend.cc:74-115) ----------------
 * Each canvas is GRAY2BGR of one grey image, or of two side by side (cv::hconcat), 3 bytes per pixel, with its slice of the
 * operation list drawn in list order as OpenCV 3.2's drawing.cpp does at thickness 1 / LINE_8 / shift 0: a circle is the
 * integer midpoint Circle() and writes only the pixels inside the canvas; a line is LineIterator (8-connected, left to
 * right) after clipLine.  Later operations overwrite earlier ones.  Coordinates are integers (cvRound is the caller's:
 * round half to even); |coordinate| must stay below 2^29, and a radius above 65535 draws nothing. */
enum { VSF_DRAW_CIRCLE = 0, VSF_DRAW_LINE = 1 };
typedef struct {
  int32_t kind;    /* VSF_DRAW_CIRCLE: centre (x0, y0), radius x1 (0 .. 65535); VSF_DRAW_LINE: (x0, y0)-(x1, y1) */
  int32_t x0, y0, x1, y1;
  uint8_t bgr[4];  /* the colour's bytes in canvas order (cv::Scalar channels 0, 1, 2); bgr[3] is ignored */
} vsf_draw_op;     /* 24 bytes */
typedef struct {
  const uint8_t* src0;    /* grey source */
  const uint8_t* src1;    /* NULL, or a second grey source of the same size drawn to the right of src0 */
  int32_t width, height;  /* of one source: the canvas is (src1 ? 2 : 1) * width x height */
  int64_t src_pitch;      /* bytes between rows of either source */
  uint8_t* out;           /* the canvas, 3 bytes per pixel */
  int64_t out_pitch;
  int32_t op_begin, op_count;  /* its operations: ops[op_begin, op_begin + op_count) */
} vsf_draw_canvas;
/* n canvases in one batch on the context's stream (does not wait).  `canvases` is host memory; its src0 / src1 / out and
 * d_ops (n_ops operations) are device pointers. */
vsf_status vsf_draw_canvases_dev(vsf_ctx* ctx, const vsf_draw_canvas* canvases, int n, const vsf_draw_op* d_ops, int n_ops);
/* The same with every pointer in host memory (sources, canvases, operations): uploads, draws, copies the canvases back and
 * waits.  What the host Frontend calls. */
vsf_status vsf_draw_canvases(vsf_ctx* ctx, const vsf_draw_canvas* canvases, int n, const vsf_draw_op* ops, int n_ops);

/* SURVEY section 8(f) row f4, the decode itself: DecodeImage's cv::imdecode(msg.data, cv::IMREAD_GRAYSCALE)
 * (slam_frontend_main.cc:99-100) for n JPEG files in HOST memory (the CompressedImage payloads), all of width x height:
 * ITU-T T.81 Huffman decoding + libjpeg's ISLOW inverse DCT of the luminance component, which is what OpenCV's reader
 * computes for a gray read (JCS_GRAYSCALE; chroma is parsed and dropped).  Baseline files (SOF0 / SOF1: what a camera
 * driver writes; also when their components come in several scans) and progressive files (SOF2; any scan script that
 * brings every luminance coefficient to full precision), gray and YCbCr with sampling factors up to 4, restart intervals,
 * custom tables.  Arithmetic-coded, 12-bit and lossless files and progressive files whose scans stop short of full
 * precision (libjpeg shows an approximation of those) return VSF_ERR_UNSUPPORTED, files of another size or with malformed headers
 * VSF_ERR_INVALID_ARG (nothing is launched then).
 * Sampling factors: every component's horizontal and vertical factor may be 1 .. 4, the chroma components' need not be equal,
 * and a one-component file has one block per MCU whatever its factors say (T.81 A.2.2).  As libjpeg does, an interleaved scan
 * -- the one scan of a baseline file, or any scan of several components in a multi-scan or progressive file -- may hold at
 * most 10 blocks per MCU (D_MAX_BLOCKS_IN_MCU): more is VSF_ERR_INVALID_ARG, as libjpeg refuses such a file.  A file whose
 * scans never interleave its components may carry up to 4 x 4 luminance blocks per MCU.  One deviation from libjpeg: the
 * luminance component must carry the largest horizontal AND vertical factor of the frame; a file in which a chroma component
 * is sampled more finely (Y 1 x 1 beside Cb 2 x 2, Y 2 x 1 beside Cb 1 x 2), whose luminance libjpeg would upsample, is
 * VSF_ERR_UNSUPPORTED -- refused, never decoded differently.  Accepted files are bit for bit libjpeg's at every layout
 * (tests/test_gpu_jpeg_sampling.py).
 * The images land at d_dst + i * dst_image_stride (DEVICE memory, rows dst_row_stride apart; base and strides multiples
 * of 4) -- the input of vsf_bayer_bg_to_gray_batch_dev or of the extraction.  The files are copied before the call
 * returns; the decode is asynchronous on the context's stream (one wave per image: run it on a context / stream of its
 * own beside other work).  A call whose files do not fit the context's pinned staging and device copies (the first
 * call, or a larger batch than any before) allocates anew without waiting for the GPU; what it outgrew is released by the
 * next vsf_sync.  A stream that breaks off inside its entropy-coded data decodes as libjpeg does (zero bits) and
 * makes the next vsf_sync return VSF_ERR_INVALID_ARG.  PNG files take vsf_png_decode_gray_batch. */
vsf_status vsf_jpeg_decode_gray_batch(vsf_ctx* ctx, const uint8_t* const* jpeg, const size_t* nbytes, int n_images,
                                      int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                      size_t dst_row_stride);

/* The same for n PNG files (the other format a CompressedImage carries: image_transport's lossless setting): chunk walk and
 * CRC checks on the host (a damaged critical chunk fails the call, as it fails png_read_*; a damaged ancillary chunk is
 * skipped), RFC 1951 inflate and the PNG row filters on the device.  Every colour type, interlaced (Adam7) or not: colour type 0 at 1, 2,
 * 4, 8 and 16 bits and colour type 4 at 8 and 16 bits -- 16-bit samples keep their high byte, alpha is dropped, 1 / 2 / 4-bit
 * samples are replicated to 8 bits (grfmt_png.cpp's libpng settings for IMREAD_GRAYSCALE) --, colour types 2 and 6 at 8 and 16
 * bits and palettes of 1 to 8 bits as libpng's rgb_to_gray(1, 0.299, 0.587) makes them (the truncated / rounded integer sum,
 * or, with a gAMA outside 0.95 .. 1.05 or an sRGB chunk, the sum of the linearised samples through libpng's two tables).
 * VSF_ERR_UNSUPPORTED, never a guess: beside colour samples iCCP, more than one gAMA / sRGB, one out of range, cHRM
 * other than sRGB's primaries next to a gamma chunk, 16-bit samples with a gamma that matters.  Files of another size or with malformed
 * chunks VSF_ERR_INVALID_ARG (nothing is launched then); compressed data that breaks (what libpng answers with png_error)
 * makes the next vsf_sync return VSF_ERR_INVALID_ARG -- that includes what zlib still reads behind the image's last byte in the
 * call that delivers libpng's last row (the rest of the <= 8192-byte piece of one IDAT chunk it was fed: end-of-block code,
 * further block headers, the Adler-32) and what cv::imdecode's png_read_end makes of the rest: it drains the stream with no
 * row to fill, where zlib's errors and data behind the image are warnings, but IDAT data that runs out before the stream has
 * ended is png_error("Not enough image data") -- a file cut inside its last bytes is refused although every pixel was there.
 * Held against the real libpng driven as grfmt_png.cpp drives it (tests/png_ref.py).  Arguments and the asynchronous contract
 * as for the JPEG call. */
vsf_status vsf_png_decode_gray_batch(vsf_ctx* ctx, const uint8_t* const* png, const size_t* nbytes, int n_images,
                                     int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                     size_t dst_row_stride);

/* cv::imdecode(msg.data, cv::IMREAD_GRAYSCALE) as DecodeImage calls it (slam_frontend_main.cc:99-100), whatever the payloads
 * are: every file is told by its first bytes (JPEG: FF D8 FF, PNG: its 8-byte signature) and runs of one format go to
 * vsf_jpeg_decode_gray_batch / vsf_png_decode_gray_batch, whose rules apply; image i lands at d_dst + i * dst_image_stride.
 * A file of neither format returns VSF_ERR_UNSUPPORTED (imdecode's other decoders are not built); nothing decoded so far is
 * undone when a later run is refused. */
vsf_status vsf_imdecode_gray_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images,
                                   int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                   size_t dst_row_stride);

/* cv::imdecode(data, cv::IMREAD_COLOR) of OpenCV 3.2 -- the other way the reference reads a CompressedImage (bag_extract.cc:73)
 * -- for n JPEG / PNG files in HOST memory: the contract of vsf_imdecode_gray_batch (format told by the first bytes, runs of
 * one format, one upload per run, asynchronous on the context's stream, data errors at the next vsf_sync, nothing decoded so far
 * is undone when a later run is refused), three bytes a pixel.
 * Destination: DEVICE memory, image i at d_dst + i * dst_image_stride; a row is 3 * width bytes, blue, green, red per pixel --
 * the layout vsf_jpeg_encode_batch_dev(channels = 3), vsf_png_encode_batch_dev and vsf_to_gray_batch_dev(VSF_PIX_BGR8) read.  d_dst,
 * dst_image_stride and dst_row_stride are multiples of 4, dst_row_stride >= (3 * width + 3) & ~3 and dst_image_stride >=
 * height * dst_row_stride, else VSF_ERR_INVALID_ARG.  Exactly the 3 * width bytes of each of the height rows are written: not
 * the rest of a row's last dword, no padding, no row below.
 * JPEG (vsf_jpeg_decode_bgr_batch): what grfmt_jpeg.cpp makes libjpeg do -- out_color_space = JCS_RGB, three output components,
 * the library's defaults otherwise (fancy upsampling, hence no merged upsampling), red and blue swapped afterwards.  Every
 * component takes the ISLOW inverse DCT at full size into a plane of its own; one kernel then upsamples the chroma planes as
 * libjpeg-turbo's jdsample.c does for the component's ratio (1 x 1 as it is; 2 x 1 and 2 x 2 by the triangle filters when the
 * component's row has more than two samples, by replication otherwise; 1 x 2 by its two-row filter; any other integral ratio by
 * replication; the rows next to the first and last row of the component are those rows again), applies jdcolor.c's 16-bit
 * fixed-point YCbCr -> RGB with range limiting and stores B, G, R.  A one-component file gives B = G = R = Y, in every process
 * the gray call reads.  Bit for bit the library's bytes (tests/jpeg_ref_bgr.py).
 * A three-component file is decoded when libjpeg reads it as YCbCr (jdapimin.c: a JFIF marker; else the Adobe marker's transform
 * flag; else the component ids), in every process the gray call reads: one interleaved scan (SOF0 / SOF1, with or without
 * restart intervals), several sequential scans, progressive (SOF2; every coefficient of EVERY component must reach full
 * precision).  VSF_ERR_UNSUPPORTED, never a guess: a file libjpeg reads as RGB (Adobe transform 0; ids 'R' 'G' 'B' without a
 * JFIF marker), four components, a luminance component below the frame's largest factors, and what the gray call answers so
 * (arithmetic-coded, 12-bit, lossless, progressive scans that stop short of full precision).  VSF_ERR_INVALID_ARG: a layout libjpeg refuses for a colour
 * read although it takes it for a gray one -- a chroma factor that does not divide the luminance's (JERR_FRACT_SAMPLE_NOTIMPL) --
 * and what the gray call answers so (more than 10 blocks in an interleaved MCU, another size, malformed headers).
 * PNG (vsf_png_decode_bgr_batch): grfmt_png.cpp's settings for an 8-bit three-channel destination -- strip_16, strip_alpha (a
 * palette's tRNS included), palette_to_rgb, expand_gray_1_2_4_to_8, set_bgr for files with the colour bit and gray_to_rgb for
 * the others.  Inflate, row filters, Adam7 and every refusal of the chunks and of the stream are those of
 * vsf_png_decode_gray_batch; no gamma transform is asked of libpng on this path, so gAMA / sRGB / iCCP / cHRM change nothing and
 * the files the gray call refuses for them are read.  Bit for bit libpng's bytes (tests/png_ref_bgr.py).
 * No reduced sizes, no resize, no CMYK. */
vsf_status vsf_imdecode_bgr_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images, int width,
                                  int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride);
vsf_status vsf_jpeg_decode_bgr_batch(vsf_ctx* ctx, const uint8_t* const* jpeg, const size_t* nbytes, int n_images, int width,
                                     int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride);
vsf_status vsf_png_decode_bgr_batch(vsf_ctx* ctx, const uint8_t* const* png, const size_t* nbytes, int n_images, int width,
                                    int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride);

/* The siblings of that flag: cv::imdecode(data, cv::IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) for reduce = 2, 4, 8.  For a JPEG
 * file OpenCV sets libjpeg's scale_num / scale_denom = 1 / reduce, and libjpeg decodes with its reduced inverse DCTs
 * (jidctred.c: 4 x 4, 2 x 2 or 1 x 1 pixels per block of coefficients) -- no resize runs -- to
 *     ceil(W / reduce) x ceil(H / reduce)   pixels (vsf_reduced_size).
 * `width` and `height` are that OUTPUT size: a file of W x H is accepted when it reduces to exactly width x height, so files
 * that differ below the denominator (127 x 95 and 128 x 96 at reduce 2) share a call; any other size is VSF_ERR_INVALID_ARG
 * for that file (nothing is launched).  Entropy decoding, restart handling and every refusal are those of
 * vsf_jpeg_decode_gray_batch; only the inverse DCT and what it stores differ.  Bit for bit what the library gives
 * (tests/jpeg_ref_reduced.py).  reduce = 1 IS vsf_imdecode_gray_batch; a reduce other than 1, 2, 4, 8 returns
 * VSF_ERR_INVALID_ARG and launches nothing (libjpeg's other N / 8 scales are not what imdecode asks for).
 * A PNG file with reduce > 1 returns VSF_ERR_UNSUPPORTED: cv::imdecode decodes a PNG at full size and then calls cv::resize,
 * which is another call: vsf_png_decode_gray_batch, then vsf_resize_gray_batch_dev to (W / reduce) x (H / reduce), floor
 * division.  Destination and asynchronous contract as for vsf_jpeg_decode_gray_batch. */
vsf_status vsf_imdecode_reduced_gray_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images,
                                           int reduce, int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                           size_t dst_row_stride);
/* The size an image of w x h has after IMREAD_REDUCED_GRAYSCALE_<reduce>: *rw = ceil(w / reduce), *rh = ceil(h / reduce)
 * (libjpeg's jpeg_calc_output_dimensions); reduce in {1, 2, 4, 8}, w, h >= 1, else VSF_ERR_INVALID_ARG and 0 x 0.  With
 * vsf_compressed_image_size -- which keeps reporting the FILE's own size -- it sizes a context for a stream of reduced
 * files.  No context, no device. */
vsf_status vsf_reduced_size(int w, int h, int reduce, int* rw, int* rh);

/* SURVEY section 8(f) row f4, the part behind cv::imdecode: DecodeImage's cvtColor(COLOR_BayerBG2BGR) +
 * cvtColor(COLOR_BGR2GRAY) (slam_frontend_main.cc:101-106) for n 8-bit mosaics of width x height resident in HBM, in
 * one pass.  d_src / d_dst: image i at base + i * image_stride, rows row_stride bytes apart; bases and strides multiples
 * of 4, dst_row_stride >= (width + 3) & ~3 (the padding bytes of a destination row up to that width are overwritten).
 * The result is the input of vsf_extract_batch_dev / vsf_stereo_batch_dev (whose own alignment rules apply).
 * Asynchronous on the context's stream. */
vsf_status vsf_bayer_bg_to_gray_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height,
                                          size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst,
                                          size_t dst_image_stride, size_t dst_row_stride);
/* The same for every pixel format (VSF_PIX_*, defined above vsf_observe_submit_dev): n raw images of width x height pixels
 * resident in HBM -> their gray images, in ONE launch on the context's stream.  VSF_PIX_BAYER_RGGB8 is
 * vsf_bayer_bg_to_gray_batch_dev, launch for launch; VSF_PIX_MONO8 is a copy.
 *   STRIDES: image i at base + i * image_stride, rows row_stride bytes apart; both bases and all four strides are multiples
 * of 4.  A source row is width x vsf_pixfmt_bytes_per_pixel(pixfmt) bytes: src_row_stride >= that;
 * dst_row_stride >= (width + 3) & ~3; image_stride >= row_stride x height on either side.  width <= 16384 (the demosaic's
 * limit, kept for every format), height and n_images <= 65535, src_row_stride x height < 2^31.
 *   READS: mosaics as vsf_bayer_bg_to_gray_batch_dev reads them (whole dwords of a row, its padding included, inside the
 * image's row_stride x height bytes; padding never reaches a pixel of the result).  Packed colour and MONO8: only aligned
 * dwords that begin before the end of the image's last row, rounded up to 4 bytes.
 *   WRITES: bytes [0, (width + 3) & ~3) of each of the height destination rows and nothing else.  The up to 3 bytes behind
 * column width - 1 are zero for packed colour and MONO8 and unspecified for mosaics.
 *   COST: one pass, bpp bytes read and 1 written per pixel; no scratch memory.
 *   VSF_ERR_INVALID_ARG: a null pointer, an unknown pixfmt, a size or stride outside these rules; nothing is launched then. */
vsf_status vsf_to_gray_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int pixfmt,
                                 size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst, size_t dst_image_stride,
                                 size_t dst_row_stride);
/* The same HOST TO HOST (upload, the one launch, download; synchronous): n raw images in host memory -> n gray images of
 * width x height bytes in host memory.  ANY addresses and strides with src_row_stride >= width x bytes per pixel and
 * dst_row_stride >= width (with more than one image: image strides that hold an image); exactly width bytes of each
 * destination row are written.  width <= 16384, height <= 32767.  What slam::Frontend's per-call mode converts with. */
vsf_status vsf_to_gray(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int pixfmt, size_t src_image_stride,
                       size_t src_row_stride, uint8_t* dst, size_t dst_image_stride, size_t dst_row_stride);

/* The COLOUR image of a raw frame: the link between cv::imdecode(data, 1) and cv::imwrite in src/test/bag_extract.cc:75-88,
 *     if format contains "bayer_rggb8":  cv::split(image) -> channel 0;  cv::cvtColor(channel 0, image, cv::COLOR_BayerBG2BGR)
 * for n raw images of width x height pixels resident in HBM -> their B G R images, in ONE launch on the context's stream
 * (k_to_bgr.hip).  The sibling of vsf_to_gray_batch_dev: vsf_to_gray_batch_dev(vsf_to_bgr_batch_dev(x), VSF_PIX_BGR8) is
 * vsf_to_gray_batch_dev(x), byte for byte, for every format.
 *   FORMATS: the four VSF_PIX_BAYER_* orders are cv::cvtColor(COLOR_Bayer??2BGR) of OpenCV 3.2 (demosaicing.cpp Bayer2RGB_<uchar>,
 * three destination channels): bilinear inside, the one-pixel frame copies its inner neighbour (columns first, then rows), an image
 * narrower or lower than 3 pixels is all zero.  VSF_PIX_BAYER_RGGB8 is the reference's COLOR_BayerBG2BGR.  The packed formats
 * are what cv_bridge makes of them for a "bgr8" request: VSF_PIX_MONO8 B = G = R; VSF_PIX_BGR8 a copy; VSF_PIX_RGB8 red and blue
 * exchanged; VSF_PIX_BGRA8 / VSF_PIX_RGBA8 alpha dropped.
 *   SOURCE: the rules of vsf_to_gray_batch_dev -- image i at base + i * image_stride, rows row_stride bytes apart, base and both
 * strides multiples of 4, src_row_stride >= width x vsf_pixfmt_bytes_per_pixel(pixfmt), src_image_stride >= src_row_stride x
 * height, src_row_stride x height < 2^31.  READS: mosaics as vsf_bayer_bg_to_gray_batch_dev reads them (whole dwords of a row, its
 * padding included, inside the image's row_stride x height bytes; padding never reaches a pixel of the result).  Packed colour and
 * MONO8: only aligned dwords that begin before the end of their own row rounded up to 4 bytes.
 *   DESTINATION: the layout of vsf_imdecode_bgr_batch, which the BGR encoders and vsf_to_gray_batch_dev(VSF_PIX_BGR8) read: a row is
 * 3 * width bytes, blue, green, red per pixel; d_dst, dst_image_stride and dst_row_stride are multiples of 4, dst_row_stride >=
 * (3 * width + 3) & ~3, dst_image_stride >= dst_row_stride x height, dst_row_stride x height < 2^31.
 *   WRITES: bytes [0, (3 * width + 3) & ~3) of each of the height destination rows and nothing else.  The up to 3 bytes behind
 * byte 3 * width - 1 are zero.
 *   LIMITS: width <= 16384 (the demosaic's limit, kept for every format), height and n_images <= 65535.
 *   COST: one pass, bpp bytes read and 3 written per pixel; no scratch memory.
 *   VSF_ERR_INVALID_ARG: a null pointer, an unknown pixfmt, a size or stride outside these rules; nothing is launched then. */
vsf_status vsf_to_bgr_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int pixfmt,
                                size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst, size_t dst_image_stride,
                                size_t dst_row_stride);
/* The same HOST TO HOST (upload, the one launch, download; synchronous): ANY addresses and strides with src_row_stride >= width x
 * bytes per pixel and dst_row_stride >= 3 * width (with more than one image: image strides that hold an image); exactly
 * 3 * width bytes of each destination row are written.  width <= 16384, height <= 32767. */
vsf_status vsf_to_bgr(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int pixfmt, size_t src_image_stride,
                      size_t src_row_stride, uint8_t* dst, size_t dst_image_stride, size_t dst_row_stride);

/* src/test/bag_extract.cc:73-90 as ONE call, for n JPEG / PNG payloads of width x height pixels in HOST memory -> n JPEG files
 * in HOST memory; synchronous:
 *     image = cv::imdecode(data, 1)                                   (:73)   vsf_imdecode_bgr_batch
 *     if format contains "bayer_rggb8":                               (:75)   bayer_pixfmt != 0
 *         cv::split(image) -> channel 0                               (:77-78)
 *         cv::cvtColor(channel 0, image, cv::COLOR_BayerBG2BGR)       (:82)   vsf_to_bgr_batch_dev
 *     cv::imwrite("....jpg", image)                                   (:88)   vsf_jpeg_encode_batch_dev, channels 3
 * The result is what those three calls give by hand; nothing goes home between the stages, and the images between them live in
 * scratch the context owns (grown like the decoders' scratch, never shrunk).
 *   bayer_pixfmt: 0 -- the topic is no mosaic: colour read, colour encode; one of the four VSF_PIX_BAYER_* codes -- colour read,
 * channel 0, demosaic in that order, colour encode (VSF_PIX_BAYER_RGGB8 is the reference's own case; width <= 16384 then); any
 * other code is VSF_ERR_INVALID_ARG.
 *   The mosaic is channel 0 of the COLOUR read, always: Y for a one-component JPEG and the gray of a gray PNG (B = G = R there),
 * the BLUE channel of a three-component file -- never the gray read of it.  Decided per file from its frame header: a
 * one-component JPEG is decoded by the gray decoders straight into its mosaic (the same bytes, the same refusals); every other
 * file takes the colour decode and one more kernel keeps the first byte of each pixel.
 *   quality: as in vsf_jpeg_encode (1 .. 100; 0 = 95, which is what cv::imwrite uses).
 *   File i is written at out + i * out_stride and its size to out_bytes[i].  A file that does not fit out_stride gives
 * out_bytes[i] = -1 and VSF_ERR_CAPACITY, the other files are delivered (vsf_jpeg_encode_capacity(width, height, 3) always fits).
 * On any other status than VSF_OK / VSF_ERR_CAPACITY every out_bytes[i] is -1: no partial delivery.  The statuses are the
 * decoders': VSF_ERR_UNSUPPORTED / VSF_ERR_INVALID_ARG as vsf_imdecode_bgr_batch gives them (a file of another size among them:
 * VSF_ERR_INVALID_ARG, nothing launched; a stream that breaks off inside its data: VSF_ERR_INVALID_ARG). */
vsf_status vsf_bag_extract_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images, int width,
                                 int height, int bayer_pixfmt, int quality, uint8_t* out, size_t out_stride, int32_t* out_bytes);

/* cv::resize(src, dst, Size(dst_width, dst_height)) of OpenCV 3.2 with its default interpolation (INTER_LINEAR) on CV_8UC1,
 * for n images resident in HBM, device to device, in ONE launch (k_resize.hip).  Independent of the context's own image
 * size.  Bit for bit cv::resize's integers: the coefficients of csrc/vsf_resize.h (the pyramid's), HResizeLinear's and
 * VResizeLinear's fixed-point passes; cv::resize's switch to INTER_AREA at an exact 2 x reduction in both axes is
 * (a + b + c + d + 2) >> 2, which those integers give as well.
 *   Any ratio per axis, independently: reduction, enlargement, or 1 (a copy).  Both sizes lie in 1 .. 32767 a side.  Image i
 * at base + i * image_stride, rows row_stride bytes apart: ANY source base address, ANY pitch >= the width on either side
 * (no alignment rule).  Bytes of a destination row beyond dst_width are not written.  A destination row that begins on a
 * 4-byte boundary is written in dwords; one that does not (an odd pitch, or an odd base) is written byte by byte, four stores
 * per lane where there was one: correct, and slower in stores -- give rows a pitch and base that are multiples of 4 where the
 * rate matters (the queue's own destination is).  The source is read only in aligned
 * 4-byte words that hold at least one pixel of the image: a row may end on the last byte of its allocation.
 *   VSF_ERR_INVALID_ARG: a null pointer, n_images < 1, a size outside 1 .. 32767, a pitch below its width, with more than one
 * image an image stride below (height - 1) * pitch + width; nothing is launched then.  Asynchronous on the context's stream like every *_dev call.
 * Not built: other interpolations, colour or 16-bit images. */
vsf_status vsf_resize_gray_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int src_width, int src_height,
                                     size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst, int dst_width,
                                     int dst_height, size_t dst_image_stride, size_t dst_row_stride);

/* The same for host pointers, synchronous: the images go up, are resized by the same kernel and come back (what a caller
 * without a queue -- slam::Frontend's per-call mode with FrontendConfig::resize_width_ -- uses).  Same sizes, strides and
 * refusals; the image strides are not looked at for n_images == 1. */
vsf_status vsf_resize_gray(vsf_ctx* ctx, const uint8_t* src, int n_images, int src_width, int src_height, size_t src_image_stride,
                           size_t src_row_stride, uint8_t* dst, int dst_width, int dst_height, size_t dst_image_stride,
                           size_t dst_row_stride);

/* The way OUT of the device for pixels: cv::imencode(".jpg", img, {IMWRITE_JPEG_QUALITY, quality}) as OpenCV 3.2 drives libjpeg
 * (the reference's own instance: src/test/bag_extract.cc:90) for n equally sized images resident in HBM -- baseline, the
 * standard tables of jpeg_set_quality(quality, TRUE), ISLOW forward DCT, the standard Huffman tables, no restart interval, a
 * JFIF 1.01 APP0.  channels 1: one component.  channels 3: B G R in, YCbCr with 2x2 chroma subsampling out.  The FILES equal
 * libjpeg's byte for byte.  Any width / height in 1 .. 65535 whatever the context's geometry; an image whose worst-case file
 * (vsf_jpeg_encode_capacity) exceeds 2^31 - 1 bytes returns VSF_ERR_UNSUPPORTED.  quality 1 .. 100, 0 = 95.
 * Image i is read at d_src + i * src_image_stride, rows src_row_stride >= width * channels bytes apart (no alignment rule;
 * bytes between rows are never read into a file); its file is written at d_out + i * out_stride and its size to d_out_bytes[i]
 * (DEVICE memory).  A file that does not fit out_stride sets d_out_bytes[i] = -1 and makes the next vsf_sync return
 * VSF_ERR_CAPACITY; nothing is written outside a slot, and out_stride >= vsf_jpeg_encode_capacity() never overflows.
 * Asynchronous on the context's stream; scratch grows without waiting for the GPU, as for the decoders. */
size_t vsf_jpeg_encode_capacity(int width, int height, int channels); /* no context; worst case incl. stuffing; 0: bad arguments */
vsf_status vsf_jpeg_encode_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int channels,
                                     size_t src_image_stride, size_t src_row_stride, int quality, uint8_t* d_out,
                                     size_t out_stride, int32_t* d_out_bytes);
/* The same with HOST pointers, synchronous.  out_bytes[i] = -1 and VSF_ERR_CAPACITY when file i does not fit out_stride (the
 * other files are delivered). */
vsf_status vsf_jpeg_encode(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int channels,
                           size_t src_image_stride, size_t src_row_stride, int quality, uint8_t* out, size_t out_stride,
                           int32_t* out_bytes);

/* The lossless way out: cv::imencode(".png", img) without parameters as OpenCV 3.2 drives libpng 1.6 and zlib 1.2.11 (filter Sub,
 * compression level 1, strategy Z_RLE, png_set_bgr) for n equally sized images resident in HBM -- 8 bits, no interlace, IDAT
 * chunks of 8192 bytes.  channels 1: gray, colour type 0.  channels 3: B G R in memory, colour type 2 (R G B) in the file.  The
 * FILES equal libpng's byte for byte, the window bits of small images and the filter type 0 of images one pixel wide included.
 * Any width / height in 1 .. 65535 whatever the context's geometry; an image whose worst-case file (vsf_png_encode_capacity)
 * exceeds 2^31 - 1 bytes returns VSF_ERR_UNSUPPORTED.
 * Image i is read at d_src + i * src_image_stride, rows src_row_stride >= width * channels bytes apart (no alignment rule;
 * bytes between rows are never read); its file is written at d_out + i * out_stride and its size to d_out_bytes[i] (DEVICE
 * memory).  A file that does not fit out_stride sets d_out_bytes[i] = -1 and makes the next vsf_sync return VSF_ERR_CAPACITY;
 * nothing is written outside a slot, and out_stride >= vsf_png_encode_capacity() never overflows.
 * Asynchronous on the context's stream; scratch grows without waiting for the GPU, as for the decoders. */
size_t vsf_png_encode_capacity(int width, int height, int channels); /* no context; every block stored + chunk framing; 0: bad arguments */
vsf_status vsf_png_encode_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int channels,
                                    size_t src_image_stride, size_t src_row_stride, uint8_t* d_out, size_t out_stride,
                                    int32_t* d_out_bytes);
/* The same with HOST pointers, synchronous.  out_bytes[i] = -1 and VSF_ERR_CAPACITY when file i does not fit out_stride (the
 * other files are delivered). */
vsf_status vsf_png_encode(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int channels,
                          size_t src_image_stride, size_t src_row_stride, uint8_t* out, size_t out_stride, int32_t* out_bytes);

/* ---------------- introspection for kernel-level parity tests and the roofline model ---------------- */

/* The PNG encoder's host half alone: the signature and the IHDR chunk (33 bytes), then the two header bytes of the zlib stream
 * (which follow the first IDAT's length and type in a file) -- 35 bytes.  *n_bytes is set even when cap is short
 * (VSF_ERR_CAPACITY).  No context, no device. */
vsf_status vsf_debug_png_encode_header(int width, int height, int channels, uint8_t* out, size_t cap, size_t* n_bytes);
/* The whole PNG encoder on the CPU, serially, from the same per-block code the kernels run: what tests without a GPU compare with
 * the real library.  VSF_ERR_CAPACITY when the file does not fit cap.  No context, no device. */
vsf_status vsf_debug_png_encode_cpu(const uint8_t* src, int width, int height, int channels, size_t src_row_stride, uint8_t* out,
                                    size_t cap, size_t* n_bytes);

/* The encoder's host half alone: every byte from SOI to the end of the SOS header (<= 640).  *n_bytes is set even when cap is
 * short (VSF_ERR_CAPACITY).  No context, no device. */
vsf_status vsf_debug_jpeg_encode_header(int width, int height, int channels, int quality, uint8_t* out, size_t cap,
                                        size_t* n_bytes);

/* Test hook for the error plumbing: the next entry point that launches returns VSF_ERR_HIP (vsf_last_hip_error == code),
 * as if one of its event records / waits had failed; the call after that works again. */
vsf_status vsf_debug_inject_hip_error(vsf_ctx* ctx, int code);
/* Copies level `level` of image `image` from the last extract to host (blurred: 0 = FAST/Harris/angle input,
 * 1 = descriptor input).  out has `ostride` bytes per row. */
vsf_status vsf_debug_level_image(vsf_ctx* ctx, int image, int level, int blurred, uint8_t* out, size_t ostride);
/* FAST+NMS candidates of (image, level) in raster order after the border filter (x, y, score) -> kp_out
 * with size 7, angle -1, response = score.  */
vsf_status vsf_debug_fast_candidates(vsf_ctx* ctx, int image, int level, vsf_keypoint* kp_out, int cap,
                                     int* n_out);
/* Host only, no device needed: the FAST work items vsf_create (orb != 0) or vsf_fast_detect (orb == 0, nms) would build for
 * *p.  words[0 .. *n_words) receives the full-cell words (level << 24 | band << 16 | strip; *n_full of them), then the
 * packed items of VSF_FAST_PACK_WORDS words each (layout in csrc/vsf_internal.h).  levels_out (10 ints per level, up to
 * level_cap levels): w, h, x_lo, x_hi, y_lo, y_hi, fast_a0, nbands, nstrips, unit0.  VSF_ERR_CAPACITY if cap is short. */
vsf_status vsf_debug_fast_work(const vsf_params* p, int orb, int nms, uint32_t* words, int cap, int* n_words, int* n_full,
                               int32_t* levels_out, int level_cap);
/* Final per-level keypoints in level coordinates, with angle: after both retainBest cuts in HARRIS_SCORE mode; in
 * FAST_SCORE mode after its one cut (response = the FAST score) -- there the list "after the first cut" and the final
 * list are the same list. */
vsf_status vsf_debug_level_keypoints(vsf_ctx* ctx, int image, int level, vsf_keypoint* kp_out, int cap,
                                     int* n_out);
/* Host only, no device needed: the keypoint room vsf_create would give *p (vsf_params::score_type states the rule).
 * room[l], l < min(nlevels, cap): records level l's segment holds; nfeat[l] (may be NULL): its budget n_l;
 * *records_per_image: their sum, one image's share of the level-keypoint buffer (20 bytes a record).
 * VSF_ERR_UNSUPPORTED for a score_type vsf_create refuses, VSF_ERR_INVALID_ARG for a geometry it refuses. */
vsf_status vsf_debug_level_room(const vsf_params* p, int32_t* room, int32_t* nfeat, int cap, int64_t* records_per_image);
/* Which form of the describe kernel ONE launch over n_images images takes in this context: 4 or 8 consecutive output
 * keypoints per wave (a batched call is one launch with one lane, one launch per half with two: vsf_set_lanes).  The
 * launcher's own choice, read back; VSF_ERR_INVALID_ARG (1) for a null context or n_images < 1.  n_images may exceed
 * max_images: a small context with the same max_keypoints answers for a large one.  Host only, nothing is launched. */
int vsf_debug_describe_form(const vsf_ctx* ctx, int n_images);
/* Test hook of the order-exact selection (cv::KeyPointsFilter::retainBest as left by libstdc++'s nth_element +
 * partition): applies retainBest(n_points) on the GPU to n (key, id) pairs given as two host arrays, in place.
 * mode 0: keys are float bit patterns compared as floats; mode 1: only the top byte of the key is compared
 * (packed FAST candidates).  use_lds: run on an LDS copy when n <= 4096.  *n_out = surviving count. */
vsf_status vsf_debug_retain_best(vsf_ctx* ctx, uint32_t* key_bits, uint32_t* ids, int n, int n_points, int use_lds,
                                 int mode, int* n_out);
/* The same, in the forms production runs: one stage of the selection kernel on chosen keys, with the template arguments,
 * memory plan (LDS arrays, HBM scratch blocks, mask carve-out, table placement, the stage-1 LDS hand-over), element types,
 * comparators and residency rule of the production kernel.  form 0..3: the wide (1024 threads, 12288 entries), common
 * (256, 3072), 9216-entry (256, 16-bit tables in HBM) and tiny (64, 1536) instances.  stage 1: 32-bit candidates
 * (key_bits[i] in 0..255 is the score byte, ids[i] < 2^24), in LDS when n <= entries; stage 2: (float bits, id) pairs, in
 * LDS when n <= 512.  level_cap >= n, >= 1: the capacity of the level's slice of each scratch block, as a level's segment
 * capacity is in production.  key_bits and ids hold level_cap entries each: the first n are the array, the rest lie behind
 * it in the slice and come back as the device left them.  *n_out = surviving count. */
vsf_status vsf_debug_retain_best_form(vsf_ctx* ctx, int form, int stage, uint32_t* key_bits, uint32_t* ids, int n,
                                      int n_points, int level_cap, int* n_out);
/* Test hook of the order-exact sort of Frontend::GetFeatureMatches (slam_frontend.cc:289-291): n_lists lists of n host
 * matches each (list i at matches + i * n; the context's max_keypoints bounds n) go through the device's std::sort
 * restatement + the cut to int(n * best_percent); pairs_out[i * n * 2 ...] receives (queryIdx, trainIdx) of the survivors
 * in sorted order and counts_out[i] their number.  serial != 0 forces the one-lane kernel. */
vsf_status vsf_debug_sort_trim(vsf_ctx* ctx, const vsf_dmatch* matches, int n_lists, int n, float best_percent,
                               int serial, uint64_t* pairs_out, int32_t* counts_out);

/* Test hook of the JPEG ingest: on != 0 sends every file through the one-wave-per-image decoder (which otherwise takes the
 * files with restart intervals and, a second time, damaged progressive files), so that the parallel forms can be held
 * against it file by file.  Waits for the context's stream. */
vsf_status vsf_debug_jpeg_serial(vsf_ctx* ctx, int on);

/* Per-stage device timing (hipEvents recorded on the context's stream around every stage of the batched entry
 * points).  vsf_profile_read synchronises the stream, adds the elapsed milliseconds and launch counts of every
 * stage executed since the last reset into ms_total[] / launches[] (VSF_STAGE_COUNT entries each). */
#define VSF_STAGE_COUNT 8
enum { VSF_STAGE_PYRAMID = 0, VSF_STAGE_FAST, VSF_STAGE_SELECT, VSF_STAGE_BLUR, VSF_STAGE_DESCRIBE, VSF_STAGE_KNN2,
       VSF_STAGE_RATIO, VSF_STAGE_TAIL /* residuals, thresholds, filter, sort + trim, 3-D points, pack */ };
vsf_status vsf_profile_enable(vsf_ctx* ctx, int on);
vsf_status vsf_profile_read(vsf_ctx* ctx, double* ms_total, int64_t* launches, int reset);
const char* vsf_stage_name(int stage);

/* Algorithmic HBM bytes of one extract of one image: SURVEY.md section 8(d) B_img for this geometry. */
uint64_t vsf_algorithmic_bytes_per_image(const vsf_ctx* ctx);
/* Total pyramid pixels P = sum_l w_l*h_l. */
uint64_t vsf_pyramid_pixels(const vsf_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* VSF_H_ */
