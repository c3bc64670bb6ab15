// vsf_ctx.h -- the context behind the C ABI (include/vsf.h) and the helpers its entry points share.  Private to the
// library: vsf_geometry.hip builds the per-size tables, vsf_api.hip owns creation / options / scratch and the two
// composed stages (extract_on, match_on), vsf_batch.hip the batched *_dev entry points, vsf_observe.hip the ObserveImage
// queue, vsf_host.hip the host-pointer calls, vsf_ingest.hip the decoders' entry points, vsf_debug.hip the test hooks.
#ifndef VSF_CTX_H_
#define VSF_CTX_H_

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "vsf_extract_plan.h"
#include "vsf_internal.h"
#include "vsf_observe_plan.h"
#include "vsf_observe_queue.h"

namespace vsfi {

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

struct Geometry {
  VsfGeom g{};
  std::vector<VsfLevel> levels;
  std::vector<uint32_t> units;
  std::vector<VsfTap> xt, yt;
  // matrix-core blur (k_blur.hip blur_mma_kernel): work units and constant MFMA operands
  std::vector<uint32_t> blur_mma_units, blur_mma_units_small;  // long strips (batches) / short strips (a frame or two)
  std::vector<uint4> blur_tcol, blur_tv;
  int blur_bias = 0;
};

struct DevSet {  // device copies of one Geometry + its work buffers: the owners, and the view `d` alloc_devset fills from them
  VsfDev d{};
  vsfi::DevBuf<VsfLevel> levels;
  vsfi::DevBuf<uint32_t> units;
  vsfi::DevBuf<uint32_t> blur_mma_units;
  vsfi::DevBuf<uint32_t> blur_mma_units_small;
  vsfi::DevBuf<uint4> blur_tcol;
  vsfi::DevBuf<uint4> blur_tv;
  vsfi::DevBuf<uint2> ic_table;
  vsfi::DevBuf<uint8_t> pyr, blur;
  vsfi::DevBuf<uint32_t> scratch, cand;
  vsfi::DevBuf<VsfLevelKp> lvlkp;
  vsfi::DevBuf<int32_t> lvl_count;
  vsfi::DevBuf<uint16_t> rowstart;
  bool ready = false;
};

// vsf_geometry.hip
bool build_geometry(const vsf_params& p, bool orb, bool nms, Geometry* out);
void gaussian_taps(int k[4]);
std::vector<uint2> build_ic_table();
std::vector<int> orb_umax(int patch_size);

}  // namespace vsfi

struct vsf_ctx {
  vsf_params p{};
  int device = 0;
  int n_cus = 256;
  // Ownership: every stream the context creates is declared here, BEFORE the events recorded on it and the buffers
  // its queued work touches -- members die in reverse order, so a stream outlives them.  `stream` is a view: own_stream or the
  // caller's (vsf_set_stream).
  vsfi::Stream own_stream;
  hipStream_t stream = nullptr;
  // Second lane of the batched entry points: half of a batch runs on `stream`, the other half on `aux_stream`
  // (frames are independent), so latency-bound stages of one half overlap VALU-bound stages of the other.
  vsfi::Stream aux_stream;
  vsfi::Event ev_fork, ev_join;
  // the blur (matrix cores + memory) beside FAST (vector ALU) in batched calls: its own stream, forked after the pyramid
  vsfi::Stream blur_stream;
  vsfi::Event ev_blur_fork, ev_blur_done;
  struct SideOwner {  // what the view `side` points at; stream[0] stays empty: side.stream[0] is aux_stream
    vsfi::Stream stream[VSF_SIDE_STREAMS];
    vsfi::Event fork, join[VSF_SIDE_STREAMS];
  } side_own;
  VsfSideStream side{};  // aux_stream, for the pyramid's second launch chain
  // Cross-call pipelining (vsf_set_pipeline): the pyramid of call k + 1 is built on side streams, into the other of
  // two pyramid buffers, while call k's later stages still run.
  bool pipeline = false;
  vsfi::Stream pipe_stream;  // the pipelined chain's own stream when VSF_OPT_PIPE_PRIORITY asks for a priority
  int pipe_stream_priority = 0;
  vsfi::Event ev_pyr_done, ev_pyr_free[2], ev_fast_done;
  // ... and FAST on the full cells of its first levels (VSF_OPT_FAST_EARLY_LEVELS) starts from inside that chain, on
  // blur_stream: it writes the candidate buffers while call k's selection still reads its own, so a call with an early
  // part takes the other of two pairs (dorb.d.cand / .rowstart point at the pair the LAST call used -- what every other path
  // and the debug hooks use).  ev_cand_free[i]: behind the pipelined selection that last read pair i.
  vsfi::Event ev_cand_free[2], ev_early_go, ev_early_done;
  // ... and its blur (VSF_OPT_BLUR_EARLY) follows that chain on the same stream, not ordered behind call k's descriptors: it
  // writes the other of two blurred pyramids (dorb.blur / blur_alt) while call k's descriptors may still read theirs.
  // ev_blur_free[i]: behind the descriptors that last read buffer i, the only reader.  last_blur: the buffer the last call's
  // blur wrote, for the debug hooks.
  vsfi::Event ev_blur_free[2];
  // Which buffer of each pair a call takes, which of these events it waits for and records, and which have been recorded:
  // the books of vsf_extract_plan.h, which states the whole schedule (extract_on issues it).
  VsfExtractState extract_state;
  const uint8_t* last_blur = nullptr;
  // A producer the library owns (the Bayer ingest) records this on the context's stream; a pipelined pyramid, which is
  // NOT ordered after that stream's earlier work, waits for it.
  vsfi::Event ev_ingest_done;
  bool ingest_done_valid = false;
  // ... and ANY other producer hands over an event of its own (vsf_set_input_event): the next batched call -- its
  // pipelined pyramid included -- waits for it; one-shot.
  hipEvent_t input_event = nullptr;  // (the caller's: a view)
  const uint8_t* last_pyr = nullptr;
  int lanes = 1;  // 1 = everything on `stream` (default), 2 = two concurrent half batches (vsf_set_lanes)
  int blur_overlap = 1;  // the blur on blur_stream beside FAST / selection (vsf_set_blur_overlap)
  int fast_resident = -1;  // vsf_set_fast_resident
  int fast_force = -1;     // vsf_tune_fast_resident only: the form of the run it is timing
  VsfTuning tuning;        // vsf_set_option
  int last_hip = 0;
  int pending_hip = 0;  // an error noted during one of THIS context's calls that returned before checking (VsfErrorScope)
  // The ObserveImage queue (vsf_observe.hip): frames wait in pinned staging and leave for the GPU in batches.
  static constexpr int kObserveBatchSlots = 4;
  struct ObserveBatchMeta;  // pinned, device-visible: read by the kernels over PCIe (no copy command)
  struct ObserveBatch {     // what one batch's extraction writes and its tail reads
    vsfi::DevBuf<uint8_t> d_img;        // [2 bmax] images at the staging pitch
    vsfi::DevBuf<vsf_keypoint> kp_raw;  // [2 bmax][K]
    vsfi::DevBuf<uint8_t> desc_raw;     // [2 bmax][K][32]
    vsfi::DevBuf<int32_t> counts_raw;   // [2 bmax]
    vsfi::DevBuf<vsf_dmatch> matches;   // [bmax][K] raw stereo matches
    vsfi::DevBuf<int32_t> nmatches;     // [bmax]
    vsfi::DevBuf<int32_t> status;       // [2 bmax] a status word per image
    vsfi::PinnedBuf<ObserveBatchMeta> h_meta;
    // compressed frames: the batch's ONE upload (every run's headers / tables / entropy-coded or IDAT bytes); free once the
    // slot's previous batch has left the GPU (ev_done)
    VsfStaging blob;
    // frames of a declared input size (vsf_observe_set_input_size): [bmax] big slots -- the raw host frames' upload and the
    // compressed frames' decoded images, at the index the frame has in the batch -- and the upload of THEIR files (a staging
    // pair of its own, with its event: a batch that holds compressed frames of several sizes decodes them size by size)
    vsfi::DevBuf<uint8_t> d_in;
    VsfStaging blob_in;
    vsfi::Event ev_uploaded, ev_extracted, ev_done;
    bool used = false;               // ev_done has been recorded at least once
    hipStream_t done_stream = nullptr;  // the stream its tail ran on (a view)
  };
  struct ObserveFrame {  // per frame slot (ticket % depth), host side
    vsf_calibration calib;
    float best_percent = 0.f;
    int batch = -1;  // batch slot it was launched in, -1 while it waits
    uint8_t kind[2] = {0, 0};    // left / right: 0 a raw image in h_img, VSF_FILE_JPEG / VSF_FILE_PNG: a file in h_cmp,
                                 // kObserveKindDevice (both): the images are in the slot of the device ring d_ring
    uint32_t nbytes[2] = {0, 0};  // ... and the files' sizes
    int pixfmt = 0;              // VSF_PIX_*: what the (decoded) images are -- not MONO8: they become gray inside the batch
    bool pix_new = false;        // vsf_observe_stats [30]: it came in a format or through a call the queue did not have before
    int in_w = 0, in_h = 0;      // the size it was handed in at (vsf_observe_set_input_size), 0 x 0: the context's
    uint8_t reduce = 1;          // compressed frames: both files decode at 1 / reduce (vsf_observe_submit_compressed_reduced)
    int dev_event = -1;          // device frames: the slot whose event in dev_ev follows the copy into the ring ...
    hipStream_t dev_stream = nullptr;  // ... and the producer's stream it was recorded on (a view)
    int stream = 0;              // vsf_observe_submit_stream: whose sequence it belongs to
    int64_t k = 0;               // frames of its stream in front of it (since the queue was built or the stream reset)
    vsf_pose pose{};             // vsf_observe_set_pose: what its stream's pose was when it was submitted (read with `cloud`)
    int mask_slot[2] = {-1, -1};  // vsf_observe_set_stream_masks: its stream's left / right slot when it was submitted
    float cam_to_robot[12] = {0};  // ... and its stream's left_cam_to_robot (vsf_observe_set_stream_cam_to_robot, or the context's)
  };
  struct ObserveStream {  // host side of one sequence of frames (vsf_observe_set_streams)
    int64_t frames = 0;        // submitted since the queue was built or the stream was reset: the next frame's k
    int64_t last_ticket = -1;  // its newest frame (the cut rule compares a frame with the one of ITS stream in front of it)
    int uncollected = 0;       // submitted and not collected (vsf_observe_reset_stream wants 0)
  };
  struct DebugForm {  // how the queue's debug images leave: raw canvases, or files of ONE kind
    int kind = VSF_FILE_NONE;  // VSF_FILE_JPEG / VSF_FILE_PNG
    int quality = 0;           // JPEG: 1 .. 100; PNG: 1
    bool operator==(const DebugForm& o) const { return kind == o.kind && quality == o.quality; }
  };
  struct Observe {
    // (`o = Observe()` releases everything a queue owns)
    vsfi::Stream copy_stream, tail_stream;  // before everything their work touches
    // vsf_observe_queue.h: the tickets, the lock, who launches and when (there while `ready`); a host thread that takes half
    // of a frame's staging copy while frames stream in.  (free_observe stops their threads before the buffers below go.)
    std::unique_ptr<vsfi::ObserveQueue> queue;
    std::unique_ptr<vsfi::ObserveCopyHelper> copy_helper;
    bool ready = false;
    int frame_life = 0;
    bool debug = false;  // built with ob_debug: the batches' tails draw the debug images
    // vsf_observe_set_world_points: built with ob_cloud -- the batches' tails run k_cloud.hip's kernel, which writes each frame's
    // points and their count into the frame's slot of these pinned rings (nothing of this exists with the switch off)
    bool cloud = false;
    float cam_to_robot[12] = {0};
    vsfi::PinnedBuf<double> h_wp;     // pinned [depth][K][3]
    vsfi::PinnedBuf<int32_t> h_wp_n;  // pinned [depth]
    // debug images: device canvases [bmax][dbg_stride], winners [bmax][3 w h], operations [bmax][5 K], canvas table [2 bmax],
    // the newest kept frame's keypoints, {colour cursor (i64), its count}; pinned: the debug ring [depth][dbg_stride] and the
    // colour ring [col_ring] (colours drawn: col_generated, taken by collected frames: col_retired)
    vsfi::DevBuf<uint8_t> dbg_canvas;
    vsfi::DevBuf<uint64_t> dbg_win;
    vsfi::DevBuf<vsf_draw_op> dbg_ops;
    vsfi::DevBuf<void> dbg_table;
    vsfi::DevBuf<vsf_keypoint> dbg_prev_kp;  // [n_streams][K]
    vsfi::DevBuf<int64_t> dbg_ints;          // {colour cursor}, then i32 [n_streams]: the kept frames' counts
    // vsf_observe_set_debug_seeds: built with ob_seeded -- each stream's generator (vsf_glibc_random.h) in device memory, the
    // colours a batch's frames took from them; the pinned colour ring h_col does not exist then and rand() is never called
    bool seeded = false;
    std::vector<uint32_t> seeds;               // [n_streams] what the states were seeded with
    vsfi::DevBuf<uint32_t> dbg_rand;           // [n_streams] vsfrand::State
    vsfi::DevBuf<uint32_t> dbg_stream_colours; // [bmax][K]
    size_t dbg_stride = 0;
    vsfi::PinnedBuf<uint8_t> h_dbg;
    vsfi::PinnedBuf<uint32_t> h_col;
    int64_t col_ring = 0, col_generated = 0, col_retired = 0;
    // vsf_observe_set_debug_jpeg / _png: the canvases stay on the device; each batch's tail encodes them (k_jpeg_enc.hip /
    // k_png_enc.hip) into device slots and a kernel carries the FILES into the pinned ring h_ring [depth][slot].  A slot: i32 stereo
    // bytes, i32 match bytes, then (16-byte aligned) the stereo file at off[0] and the match file at off[1], each with room for
    // cap[] = vsf_encode_capacity() bytes.  h_dbg does not exist then.
    struct DebugFiles {
      DebugForm form;                // what the queue was built with (kind 0: raw canvases, nothing below exists)
      size_t off[2] = {0, 0}, cap[2] = {0, 0}, slot = 0;
      vsfi::DevBuf<uint8_t> d_slots;    // [bmax][slot]
      vsfi::DevBuf<int32_t> d_bytes;    // [2][bmax] the files' sizes: stereo, match; [1] the encoder's status word
      vsfi::DevBuf<uint8_t> d_scratch;  // the encoder's scratch for bmax canvases of either size
      vsfi::PinnedBuf<uint8_t> h_ring;
    } files;
    int depth = 0;      // frames that may be submitted and not collected
    int bmax = 0;       // frames per batch at most
    int n_streams = 1;  // vsf_observe_set_streams
    int ring = 0;       // descriptor sets [s ring, (s + 1) ring): the kept left frames of stream s (its frame k in set
                        // s ring + k % ring); [n_streams ring, n_streams ring + bmax): the right frames of the batch in the tail
    int max_pairs = 0;  // bmax * (frame_life + 1)
    vsfi::DevBuf<uint8_t> sets;        // [n_streams ring + bmax][K][32]
    vsfi::DevBuf<int32_t> set_counts;  // [n_streams ring + bmax]
    // the tail's scratch exists once: tails run one after the other (they carry the threshold and the window)
    vsfi::DevBuf<float> residual;      // [bmax][K]
    vsfi::DevBuf<float> floats;        // means [bmax] | thr [bmax + 1] | thr_state [n_streams]
    vsfi::DevBuf<vsf_keypoint> kpf;    // [2 bmax][K]
    vsfi::DevBuf<int32_t> ints;        // counts_f [2 bmax] | nfeat [bmax] | npoints [bmax]
    vsfi::DevBuf<int32_t> ex_idx2, ex_dist2;  // [bmax][K][2] the extraction side's matcher scratch
    vsfi::DevBuf<int32_t> t_idx2, t_dist2;    // [max_pairs][K][2] the tail's
    vsfi::DevBuf<vsf_dmatch> t_matches;                  // [max_pairs][K]
    vsfi::DevBuf<int32_t> t_nmatches;
    vsfi::DevBuf<void> t_sortkeys;
    vsfi::DevBuf<uint64_t> pairs;      // [max_pairs][K][2]
    vsfi::DevBuf<int32_t> npairs;
    vsfi::DevBuf<vsf_vision_feature> features;  // [bmax][K]
    vsfi::PinnedBuf<uint8_t> h_img;       // pinned [depth][2] images at the staging pitch
    vsfi::PinnedBuf<uint8_t> h_out;       // pinned [depth][out_stride], written by observe_pack_kernel
    // vsf_observe_submit_compressed; nothing of this exists before the first compressed frame.  The files wait in a pinned
    // ring of their own; a batch's decode runs on the copy stream (one batch after the other: ONE set of decoder scratch)
    vsfi::PinnedBuf<uint8_t> h_cmp;       // pinned [depth][2][cmp_slot] the files as submitted
    size_t cmp_cap = 0, cmp_slot = 0;  // bytes a file may have / bytes of its slot (vsf_observe_compressed_slot_bytes)
    vsfi::DevBuf<uint8_t> d_bayer;     // [2 bmax] images at the staging pitch: the decoded mosaics of a Bayer batch
    VsfDecodeScratch ing_scratch;   // the decoders' scratch on the copy stream
    // vsf_observe_submit_dev; nothing of this exists before the first device frame.  The frames wait in a DEVICE ring in the
    // staging ring's layout; the submit's one launch on the producer's stream fills their slots and records the event of the
    // call's last slot behind it; the batch's copy stream waits for that event and moves the slots into the batch's images.
    vsfi::DevBuf<uint8_t> d_ring;            // [depth][2] images at the staging pitch
    vsfi::PinnedBuf<VsfIngestSrc> h_dev_src;  // pinned [depth][2]: where a long call's images are (read by its launch)
    std::vector<vsfi::Event> dev_ev;         // [depth]
    // vsf_observe_set_input_size; nothing of this exists before the first frame of a declared size.  Rings of big slots
    // (vsf_observe_plan.h: 2 * in_half bytes, an image every in_half) beside the rings above: pinned for raw host frames, in
    // HBM for device frames; the mosaics of a Bayer batch's resized frames, [bmax] big slots.
    size_t in_half = 0;                       // what the buffers that exist were built for
    vsfi::PinnedBuf<uint8_t> h_in;            // pinned [depth] big slots
    vsfi::DevBuf<uint8_t> d_in_ring;          // [depth] big slots
    vsfi::DevBuf<uint8_t> d_bayer_in;         // [bmax] big slots
    // launch_batch's: what every frame of the batch is and the commands of its ingest (vsf_observe_plan.h; kept from batch to
    // batch, as `plan` is: no allocation per batch); ingest()'s: the batch's files, their sizes, kinds and denominators per decode
    vsfi::ObserveIngestPlan ingest;
    std::vector<const uint8_t*> dec_files;
    std::vector<size_t> dec_sizes;
    std::vector<uint8_t> dec_kinds, dec_reduces;
    bool pix_seen = false;                   // a frame with pix_new has been submitted (vsf_observe_stats [30] .. [32])
    int64_t stat_dev_commands = 0;           // the caller's share of vsf_observe_stats value 18 (the submits' launches)
    size_t out_cap = 0, out_stride = 0;
    ObserveBatch batch[kObserveBatchSlots];
    std::vector<ObserveFrame> frames;  // [depth]
    std::vector<ObserveStream> streams;  // [n_streams]
    std::vector<vsfi::ObservePlanIn> plan_in;  // launch_batch's: the batch as vsf_observe_plan.h takes it ...
    vsfi::ObservePlan plan;                    // ... and plans it (kept from batch to batch: no allocation per batch)
    int last_batch = -1;       // slot of the batch launched last
    int64_t stat_copy_ns = 0, stat_wait_ns = 0;  // the caller's time in staging copies and waits (vsf_observe_stats)
  } ob;
  // vsf_observe_configure (before the queue is built by the first submit; 0 = defaults)
  int ob_depth = 0, ob_min_batch = 0, ob_in_flight = 2;
  int ob_streams = 1;  // vsf_observe_set_streams
  bool ob_debug = false;  // vsf_observe_set_debug_images: the queue draws the debug images
  bool ob_cloud = false;   // vsf_observe_set_world_points: the queue makes the point cloud ...
  float ob_cam_to_robot[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // ... with this left_cam_to_robot (3 x 4 row-major)
  vsf_pose ob_pose[VSF_OBSERVE_MAX_STREAMS];  // vsf_observe_set_pose: each stream's sticky pose (identity: vsf_create)
  // vsf_observe_set_debug_seeds: every stream draws its stereo lines' colours from a generator of its own (srand(seed), rand(), ...)
  bool ob_seeded = false;
  uint32_t ob_seeds[VSF_OBSERVE_MAX_STREAMS] = {0};
  // vsf_observe_set_stream_cam_to_robot: a stream's own left_cam_to_robot in place of ob_cam_to_robot
  bool ob_stream_c2r_set[VSF_OBSERVE_MAX_STREAMS] = {false};
  float ob_stream_c2r[VSF_OBSERVE_MAX_STREAMS][12] = {{0}};
  // vsf_observe_set_input_size: the size a stream's frames arrive at (0 x 0: the context's), brought to the context's by
  // k_resize.hip inside the batch.  Kept across resets, dropped when vsf_observe_set_streams changes the count.
  int ob_in_w[VSF_OBSERVE_MAX_STREAMS] = {0}, ob_in_h[VSF_OBSERVE_MAX_STREAMS] = {0};
  // vsf_observe_set_bayer_order: the order of a stream's compressed mosaics (`bayer` != 0); RGGB until told otherwise.  Kept
  // and dropped as the declared sizes are.
  int ob_bayer_order[VSF_OBSERVE_MAX_STREAMS] = {0};  // (0: never told)
  DebugForm ob_debug_form;  // vsf_observe_set_debug_jpeg / _png: ... and hands them out as files (in force while ob_debug is)
  size_t ob_cmp_cap = 0;  // vsf_observe_set_compressed_cap: bytes per compressed file (0: the default for the image size)
  // ---- buffers: every stream above, the queue's two included, outlives them ----
  // Detection masks (vsf_mask.hip, include/vsf.h "Detection masks"): a slot's block is built once, by vsf_mask_set, and read by
  // FAST's predicate (VsfFastMask); a slot that is not set is no mask.  mask_even / mask_odd: vsf_set_image_masks.
  struct MaskSlot {
    vsfi::DevBuf<uint8_t> block;  // [orb.g.pyr_bytes], kept across vsf_mask_clear
    bool set = false;
  };
  MaskSlot masks[VSF_MAX_MASKS];
  int mask_even = -1, mask_odd = -1;
  struct StreamMasks {  // vsf_observe_set_stream_masks: what the queue's frames of a stream take (kept like the poses)
    int left = -1, right = -1;
  } ob_masks[VSF_OBSERVE_MAX_STREAMS];
  // a vsf_observe_stereo* call is submitting its frame, which takes mask_even / mask_odd (set and cleared by stereo_call's scope
  // around the submit; a context is driven by one host thread at a time, vsf_internal.h, and the launcher thread never reads it:
  // the frame's slots are captured on the caller's thread when it is booked)
  bool ob_sync_call = false;
  vsfi::DevBuf<uint8_t> pyr_alt;  // the other pyramid buffer of cross-call pipelining
  vsfi::DevBuf<uint8_t> blur_alt;  // ... and the other blurred pyramid (buffer 1 of vsf_extract_plan.h; buffer 0 is dorb.blur)
  vsfi::DevBuf<uint32_t> cand_alt;      // ... and the other pair of FAST's candidate segments and row-start tables
  vsfi::DevBuf<uint16_t> rowstart_alt;  //     (pair 0 is dorb.cand / dorb.rowstart)
  vsfi::Geometry orb, fast;
  vsfi::DevSet dorb, dfast;
  // Status words (bit 0: capacity overflow, bit 1: a JPEG stream broke off): word 0 belongs to the context's own stream
  // (batched and host-pointer calls, vsf_sync), words 1..6 to the frames that may be in flight (vsf_observe_submit) --
  // a frame's kernels run on its slot's stream beside another frame's, so each frame sets, copies and clears its own word.
  vsfi::DevBuf<int32_t> d_status;     // [1 + VSF_OBSERVE_MAX_SLOTS]
  vsfi::DevBuf<uint32_t> fast_cells;  // [3] cell counters of the resident FAST kernels (k_fast.hip): full, packed, early part
  struct FastTune {  // resident FAST or one workgroup per four cells: what vsf_tune_fast_resident measured, per batch size
    int n = 0, choice = -1;
    vsfi::Event ev[2];
  } fast_tune;
  vsfi::PinnedBuf<int32_t> h_status;  // pinned
  // staging for the host-pointer entry points
  vsfi::DevBuf<uint8_t> st_img;
  size_t st_img_pitch = 0, st_img_stride = 0;
  vsfi::DevBuf<vsf_keypoint> st_kp;
  vsfi::DevBuf<uint8_t> st_desc;
  vsfi::DevBuf<int32_t> st_counts;
  // matcher work buffers
  vsfi::DevBuf<int32_t> m_idx2;
  vsfi::DevBuf<int32_t> m_dist2;
  int m_pairs = 0, m_rows = 0;
  // f1 work buffers: residuals [frames][rows], F (9 floats), matches / counts / sort keys of the temporal pairs
  vsfi::DevBuf<float> f_residual;
  int f_frames = 0;
  vsfi::DevBuf<vsf_dmatch> t_matches;
  vsfi::DevBuf<int32_t> t_nmatches;
  vsfi::DevBuf<void> t_sortkeys;
  int t_pairs = 0;
  // f2 work buffers: right->left pairs of every frame, their set indices, the pack kernel's offsets
  vsfi::DevBuf<uint64_t> v_pairs;
  vsfi::DevBuf<int32_t> v_npairs;
  vsfi::DevBuf<int32_t> v_sets;   // [2][v_frames]: q_set = 2f + 1, t_set = 2f
  int v_frames = 0;
  vsfi::DevBuf<uint32_t> pk_offsets;
  int pk_entries = 0;
  // Scratch a *_dev call has outgrown.  Such a call takes a NEW allocation (hipMalloc does not wait for the GPU) and
  // parks the old one here, because hipFree would wait for the whole device behind the caller's back; released by
  // vsf_sync / vsf_reserve / vsf_destroy, when every stream of the context is known to be idle.
  std::vector<vsfi::DevBuf<void>> retired;
  std::vector<vsfi::PinnedBuf<void>> retired_host;  // ... and pinned host buffers (the ingest's staging)
  // vsf_draw_canvases(_dev) (k_draw.hip): per-pixel winners (all zero between calls: the resolve clears what it read),
  // the canvas table (device, and its host image until the upload has left: dr_uploaded), the host call's staging
  vsfi::DevBuf<uint64_t> dr_win;
  size_t dr_win_cap = 0;
  vsfi::DevBuf<void> dr_canv;
  int dr_canv_cap = 0;
  std::vector<uint8_t> dr_canv_host;
  vsfi::Event dr_uploaded;
  vsfi::DevBuf<uint8_t> dr_buf;
  size_t dr_buf_cap = 0;
  // vsf_jpeg_decode_gray_batch / vsf_png_decode_gray_batch: two staging pairs, used alternately (the host fills one while the
  // previous call's upload / decode still use the other; `uploaded`: the last upload out of the pair has finished), and the
  // decoders' scratch on the context's stream
  VsfStaging ingest_stage[2];
  int ingest_flip = 0;
  VsfDecodeScratch ingest_scratch;
  VsfEncodeScratch encode;  // vsf_jpeg_encode* / vsf_png_encode*
  VsfBagScratch bag;        // vsf_bag_extract_batch
  vsfi::DevBuf<uint8_t> mh_desc;  // host-API descriptor staging: 2 sets
  vsfi::DevBuf<int32_t> mh_counts;
  vsfi::DevBuf<vsf_dmatch> mh_matches;
  vsfi::DevBuf<int32_t> mh_nmatches;
  int mh_rows = 0;
  // vsf_get_matches_multi staging: sets x rows descriptors, per-set counts / set indices / matches
  vsfi::DevBuf<uint8_t> mm_desc;
  vsfi::DevBuf<int32_t> mm_counts;  // [sets + 1] counts, then [sets] q_set, [sets] t_set
  vsfi::DevBuf<vsf_dmatch> mm_matches;
  vsfi::DevBuf<int32_t> mm_nmatches;
  int mm_sets = 0, mm_rows = 0;
  vsfi::DevBuf<uint8_t> wp_buf;  // vsf_world_points (host pointers): one frame's records | its points | {nfeatures, npoints}
  VsfImages last_images{};
  bool last_valid = false;
  bool fast_nms = true;  // NMS mode the standalone-FAST geometry was built for
  // per-stage hipEvent profiling
  bool prof_on = false;
  std::vector<vsfi::Event> ev_pool;  // pairs
  std::vector<int> ev_stage;        // stage of pair i
  std::vector<int> ev_launches;
  size_t ev_used = 0;               // pairs in flight
  double prof_ms[VSF_STAGE_COUNT] = {0};
  int64_t prof_launches[VSF_STAGE_COUNT] = {0};
};

#define VSF_HIP(call)                     \
  do {                                    \
    hipError_t e_ = (call);               \
    if (e_ != hipSuccess) {               \
      ctx->last_hip = (int)e_;            \
      return VSF_ERR_HIP;                 \
    }                                     \
  } while (0)
// End of an entry point that launched: a failed launch (hipGetLastError) or anything a launcher / stream helper noted
// (vsf_note: event records and waits, memsets) becomes this call's VSF_ERR_HIP.
#define VSF_STICKY()                                               \
  do {                                                             \
    hipError_t e_ = hipGetLastError();                             \
    if (e_ == hipSuccess) e_ = (hipError_t)vsf_tls_hip_error;      \
    if (e_ == hipSuccess) e_ = (hipError_t)ctx->pending_hip;       \
    vsf_tls_hip_error = 0;                                         \
    ctx->pending_hip = 0;                                          \
    if (e_ != hipSuccess) {                                        \
      ctx->last_hip = (int)e_;                                     \
      return VSF_ERR_HIP;                                          \
    }                                                              \
  } while (0)

namespace vsfi {

template <class T>
hipError_t upload(DevBuf<T>& dst, const std::vector<T>& v) {
  hipError_t e = dst.alloc(v.size() * sizeof(T));
  if (e != hipSuccess) return e;
  return hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

vsf_status alloc_devset(vsf_ctx* ctx, const Geometry& G, DevSet* ds, bool orb, int n_images);

// ---- scratch that follows the batch size of the *_dev calls ----
// Sized at vsf_create for max_images / 2 frames and as many pairs, or by vsf_reserve.  A call that needs more never waits
// for the GPU: grow_scratch() allocates anew and retires the old buffer (kernels already queued keep using it).
template <class T>
vsf_status grow_scratch(vsf_ctx* ctx, DevBuf<T>& buf, size_t bytes) {
  DevBuf<T> fresh;
  VSF_HIP(fresh.alloc(std::max<size_t>(bytes, 16)));
  if (buf) ctx->retired.emplace_back(buf.release());
  buf = std::move(fresh);
  return VSF_OK;
}
void free_retired(vsf_ctx* ctx);  // (callers have waited for every stream of the context)
// vsf_ingest.hip: the ONE way compressed files reach the device and are decoded there.  Files [0, n) of `kinds` (VSF_FILE_*;
// VSF_FILE_NONE: not a file, its image is left alone) are planned run by run of one format, `stage` and `scratch` are grown to
// the largest need without waiting for the GPU (a quarter of headroom; what is outgrown is retired), every run is filled at
// its offset of the staging pair, ONE upload goes out on `s` and each run's decoder is launched behind it: image i at
// d_dst + i * dst_image_stride, file i's damage in d_status[i * status_stride].  *n_runs (optional): the runs launched.
// Which staging pair is free is the caller's business (VsfStaging::uploaded).  The caller checks for launch errors.
// reduces (optional): width x height is the OUTPUT size and file i decodes at 1 / reduces[i] (vsf_plan_runs).
// out_format: VSF_OUT_GRAY (a byte a pixel: IMREAD_GRAYSCALE) or VSF_OUT_BGR (three, blue first: IMREAD_COLOR; dst_pitch is
// still bytes) -- what vsf_plan_runs takes in that format is what is decoded.
vsf_status decode_runs(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, const uint8_t* kinds, int n, int width,
                       int height, VsfStaging& stage, VsfDecodeScratch& scratch, uint8_t* d_dst, size_t dst_image_stride,
                       int dst_pitch, int32_t* d_status, int status_stride, hipStream_t s, int* n_runs = nullptr,
                       const uint8_t* reduces = nullptr, int out_format = VSF_OUT_GRAY);
vsf_status ensure_match_buffers(vsf_ctx* ctx, int pairs, int rows);
vsf_status ensure_match_host_staging(vsf_ctx* ctx, int rows);  // (host-pointer, synchronous entry points only)
vsf_status ensure_residual_buffers(vsf_ctx* ctx, int n_frames);
vsf_status ensure_temporal_buffers(vsf_ctx* ctx, int n_pairs);
vsf_status ensure_vision_buffers(vsf_ctx* ctx, int n_frames);
vsf_status ensure_pack_buffers(vsf_ctx* ctx, int n);
vsf_status reserve_scratch(vsf_ctx* ctx, int n_frames, int n_pairs);
vsf_status ensure_pipeline_buffers(vsf_ctx* ctx);
void free_observe(vsf_ctx* ctx);          // vsf_observe.hip: the queue's threads stop, then everything the queue owns goes
void stop_observe_threads(vsf_ctx* ctx);  // ... before anything waits for the context's streams to drain
void flush_observe(vsf_ctx* ctx);         // every frame that waits in the queue leaves for the GPU (the queue stays)
// vsf_observe_ingest.hip: how a batch's images reach its own buffer, and the buffers that takes -- each built by the first
// frame that needs it (a queue that only ever sees raw mono frames of the context's size owns none of them).
size_t compressed_cap(const vsf_ctx* ctx);    // bytes a compressed file may have: the submit's probe and the ring
vsf_status ensure_compressed(vsf_ctx* ctx);   // the pinned ring of files
vsf_status ensure_device_ring(vsf_ctx* ctx, bool big_slots);  // the events and the table of sources; !big_slots: the device ring
size_t mosaics_bytes(const vsf_ctx* ctx);     // the mosaics' buffer of own-size Bayer batches ...
vsf_status ensure_mosaics(vsf_ctx* ctx);      // ... its ONE allocation
enum { kInHostRing = 1, kInDeviceRing = 2, kInBatch = 4, kInBayer = 8 };  // the buffers of big slots (vsf_observe_plan.h)
vsf_status ensure_input(vsf_ctx* ctx, int what, size_t need = 0);
size_t input_bytes(const vsf_ctx* ctx);  // vsf_observe_stats: every byte the big slots take
// The copy stream's command sequence for frames [t0, t0 + n) as `plan` has it (observe_ingest_plan), up to ev_uploaded, which
// the context's stream waits for.
vsf_status ingest(vsf_ctx* ctx, vsf_ctx::ObserveBatch& b, int64_t t0, int n, const vsfi::ObserveIngestPlan& plan,
                  hipStream_t s_copy);

vsf_status check_status_word(vsf_ctx* ctx);
vsf_status validate_images(const vsf_ctx* ctx, const uint8_t* d_imgs, int n, size_t image_stride, size_t row_stride);
void prof_fold(vsf_ctx* ctx);         // stream must be idle
void sync_all_streams(vsf_ctx* ctx);  // every stream the context launches on

struct StageTimer {  // records an event pair around one stage when profiling is on
  vsf_ctx* ctx;
  size_t slot = 0;
  bool on;
  hipStream_t st;
  StageTimer(vsf_ctx* c, hipStream_t stream, int stage, int launches) : ctx(c), on(c->prof_on), st(stream) {
    if (!on) return;
    if (ctx->ev_used >= 2048) {
      sync_all_streams(ctx);
      prof_fold(ctx);
    }
    slot = ctx->ev_used++;
    while (ctx->ev_pool.size() < 2 * (slot + 1)) {
      ctx->ev_pool.emplace_back();
      vsf_note(ctx->ev_pool.back().alloc(hipEventDefault));
    }
    if (ctx->ev_stage.size() <= slot) {
      ctx->ev_stage.resize(slot + 1);
      ctx->ev_launches.resize(slot + 1);
    }
    ctx->ev_stage[slot] = stage;
    ctx->ev_launches[slot] = launches;
    vsf_note(hipEventRecord(ctx->ev_pool[2 * slot], st));
  }
  ~StageTimer() {
    if (on) vsf_note(hipEventRecord(ctx->ev_pool[2 * slot + 1], st));
  }
};

// The per-image work buffers of images [i0, i0 + n) seen as a batch of their own.
VsfDev shifted(const VsfDev& d, const VsfGeom& g, int i0);

// vsf_set_input_event: the batched call that follows waits for the caller's event on the context's stream (level 0 of the
// pyramid IS the input: FAST, Harris and the orientation read it there) -- the pipelined pyramid chain waits for it by
// itself in extract_on -- and the event is forgotten when the call returns (one-shot).
struct InputEventScope {
  vsf_ctx* ctx;
  // Built FIRST in the entry point (right behind the null check), so that every way out -- a refusal included -- forgets the
  // event: a handle left pending would be waited for by some later call, when the caller may long have destroyed or
  // re-recorded it.  wait() is issued once the arguments have been validated.
  explicit InputEventScope(vsf_ctx* c) : ctx(c) {}
  void wait() {
    if (ctx->input_event) vsf_note(hipStreamWaitEvent(ctx->stream, ctx->input_event, 0));
  }
  ~InputEventScope() { ctx->input_event = nullptr; }
};

// detectAndCompute for images [i0, i0 + n) of `im` on stream `st`.  `status`: the status word the kernels report capacity
// overflows into (the context's, or the word of the frame in flight that owns this extraction).
// `masks`: whose detection masks the images take; null: the context's (vsf_set_image_masks, image i0 + i by its parity).
void extract_on(vsf_ctx* ctx, hipStream_t st, const VsfImages& im_all, int i0, int n, vsf_keypoint* d_kp, uint8_t* d_desc,
                int32_t* d_counts, bool inputs_complete = false, const VsfSideStream* own_side = nullptr,
                int32_t* status = nullptr, int status_stride = 0, const VsfFastMask* masks = nullptr);
// vsf_mask.hip: the masks of vsf_set_image_masks for a launch whose first image is image `i0` of its call
VsfFastMask image_masks(const vsf_ctx* ctx, int i0);
// knnMatch(k = 2) + ratio test for pairs [p0, p0 + n) on stream `st`.
void match_on(vsf_ctx* ctx, hipStream_t st, const uint8_t* d_desc, const int32_t* d_counts, size_t set_stride,
              const int32_t* d_q_set, const int32_t* d_t_set, int p0, int n, int32_t* d_idx2, int32_t* d_dist2,
              vsf_dmatch* d_matches, int32_t* d_nmatches, int32_t* status = nullptr);
vsf_status fork_lane(vsf_ctx* ctx);
vsf_status join_lane(vsf_ctx* ctx);

// Runs body(stream, first, count) over `units` work items (images or stereo frames): all on the context's stream, or
// (vsf_set_lanes(ctx, 2)) as two halves on the two lanes.  Measured on MI355X: the stages are either VALU-bound
// (FAST, blur) or latency-bound, and a VALU-bound kernel at full occupancy leaves no registers for a second kernel's
// waves, so the second lane only fills launch gaps and tails (+5 % frames/s) while every kernel's own duration
// roughly doubles; one lane stays the default.
template <class Body>
vsf_status run_chunked(vsf_ctx* ctx, int units, Body body) {
  if (ctx->lanes < 2 || units < 2) {
    body(ctx->stream, 0, units);
    return VSF_OK;
  }
  vsf_status st = fork_lane(ctx);
  if (st != VSF_OK) return st;
  const int n0 = (units + 1) / 2;
  body(ctx->stream, 0, n0);
  body(ctx->aux_stream, n0, units - n0);
  return join_lane(ctx);
}

vsf_status extract_async(vsf_ctx* ctx, const VsfImages& im, vsf_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts,
                         bool inputs_complete = false);

}  // namespace vsfi

#endif  // VSF_CTX_H_
