// vsf_observe.hip -- Frontend::ObserveImage (slam_frontend.cc:400-472) as a QUEUE of stereo frames.
//
// vsf_observe_submit copies a frame's two images into pinned staging and returns a ticket; frames that wait are coalesced
// into ONE batched extraction + ONE batched tail:
//   upload      one copy command for the batch's images (a copy command costs ~180 us whatever it carries up to 10 MB)
//   extraction  ExtractFeatures x 2 and the stereo GetMatches of every frame of the batch (cc:411-416): the batched kernels
//   tail        RemoveAmbigStereo with the threshold chain in frame order (cc:417, 353, 392-394), every GetFeatureMatches of
//               the temporal loop (cc:424-434) and the right -> left match of Calculate3DPoints (cc:129-132) as ONE matcher
//               launch + one sort launch over the batch's pair list, the VisionFeature records (cc:437-443), one compact
//               result per frame written straight into pinned host memory.
// A frame's launch-bound chain of ~30 small kernels costs the host 5.4 us per launch and the GPU a launch-to-launch latency
// per kernel whatever the batch holds, so a batch of n frames costs little more than a batch of one until the chip is full.
// When a batch leaves (vsf_observe_queue.cc batch_to_launch): when a whole batch waits; when `min_batch` frames wait (a whole batch by default while the queue holds two, else half the queue) and
// fewer than `in_flight` batches are on the GPU; when the GPU is idle and no frame has arrived for 100 us; or when somebody
// collects a frame that still waits (a lone frame: the synchronous call is a batch of one).  While the GPU is busy, frames
// accumulate -- the batch size follows the caller's rate by itself.
// The kept frames' filtered descriptors live in a ring of descriptor sets in HBM (frame g in set g % ring); the pair list
// of a batch addresses them by set index, so a frame matches against frames of earlier batches and of its own alike.
// Results are those of one frame at a time, bit for bit (tests/test_gpu_observe.py).
// The host threads -- tickets, the lock, who launches and when, the staging copy's helper -- are plain C++ in
// vsf_observe_queue.cc; this file is what touches HIP: it builds the queue's buffers, launches a batch, and hands the queue
// that launch as a callable.
// STREAMS (vsf_observe_set_streams): the queue takes frames of several independent sequences -- several cameras on one GPU --
// and frames of different streams leave in the same batch.  Everything that crosses frames exists per stream: a threshold
// (thr_state[stream]), a ring of descriptor sets (frame k of stream s in set s ring + k % ring), the calibration (the batch's
// pinned block carries a table of its distinct calibrations and an index per frame).  vsf_observe_plan.cc does the arithmetic;
// each stream's results are those of a context of its own, byte for byte (tests/test_gpu_observe_streams.py).
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "vsf_ctx.h"
#include "vsf_glibc_random.h"

using namespace vsfi;

struct vsf_ctx::ObserveBatchMeta {
  int32_t n_frames, n_pairs;
  // followed by (offsets in int32 words from the start of the block, fixed by the queue's sizes):
  //   q_set[max_pairs] | t_set[max_pairs] | best_percent[max_pairs] (float) | out_sets[2 bmax] | frames[bmax] |
  //   params[bmax] | calibs[bmax] -- the last two are written and read only by a batch that holds more than one stream or
  //   more than one calibration -- | transforms[bmax]: M_f of every frame, written and read only with the point cloud on
  //   | (8-byte aligned) masks[2 bmax]: the detection mask block of every image, read only by a batch that has one
};

namespace {

struct MetaView {
  int32_t* q_set;
  int32_t* t_set;
  float* best_percent;
  int32_t* out_sets;
  VsfObserveFrame* frames;
  VsfObserveParam* params;
  vsf_calibration* calibs;
  vsfwp::Affine* transforms;
  const uint8_t** masks;
};

size_t meta_bytes(int max_pairs, int bmax) {
  return 16 + (size_t)max_pairs * 12 + (size_t)bmax * 8 +
         (size_t)bmax * (sizeof(VsfObserveFrame) + sizeof(VsfObserveParam) + sizeof(vsf_calibration) + sizeof(vsfwp::Affine)) +
         8 + (size_t)bmax * 2 * sizeof(const uint8_t*);
}

MetaView meta_view(vsf_ctx::ObserveBatchMeta* m, int max_pairs, int bmax) {
  uint8_t* b = reinterpret_cast<uint8_t*>(m) + 16;
  MetaView v;
  v.q_set = reinterpret_cast<int32_t*>(b);
  v.t_set = v.q_set + max_pairs;
  v.best_percent = reinterpret_cast<float*>(v.t_set + max_pairs);
  v.out_sets = reinterpret_cast<int32_t*>(v.best_percent + max_pairs);
  v.frames = reinterpret_cast<VsfObserveFrame*>(v.out_sets + 2 * bmax);
  v.params = reinterpret_cast<VsfObserveParam*>(v.frames + bmax);
  v.calibs = reinterpret_cast<vsf_calibration*>(v.params + bmax);
  v.transforms = reinterpret_cast<vsfwp::Affine*>(v.calibs + bmax);
  v.masks = reinterpret_cast<const uint8_t**>((reinterpret_cast<uintptr_t>(v.transforms + bmax) + 7) & ~(uintptr_t)7);
  return v;
}

// The tail's scratch o.floats: means [bmax] | thr [bmax + 1] | thr_state [n_streams] (cc:353, what crosses batches) ...
size_t tail_floats(const vsf_ctx::Observe& o) { return 2 * (size_t)o.bmax + 1 + (size_t)o.n_streams; }
float* tail_means(const vsf_ctx::Observe& o) { return o.floats.get(); }
float* tail_thr(const vsf_ctx::Observe& o) { return o.floats.get() + o.bmax; }
float* tail_thr_state(const vsf_ctx::Observe& o) { return o.floats.get() + 2 * o.bmax + 1; }
// ... and o.ints: counts_f [2 bmax] | nfeat [bmax] | npoints [bmax]
size_t tail_ints(const vsf_ctx::Observe& o) { return 4 * (size_t)o.bmax; }
int32_t* tail_counts_f(const vsf_ctx::Observe& o) { return o.ints.get(); }
int32_t* tail_nfeat(const vsf_ctx::Observe& o) { return o.ints.get() + 2 * o.bmax; }
int32_t* tail_npoints(const vsf_ctx::Observe& o) { return o.ints.get() + 3 * o.bmax; }

}  // namespace

namespace vsfi {

void stop_observe_threads(vsf_ctx* ctx) {
  vsf_ctx::Observe& o = ctx->ob;
  if (o.queue) o.queue->stop_thread();
  o.copy_helper.reset();
}

void flush_observe(vsf_ctx* ctx) {
  if (ctx->ob.ready && ctx->ob.queue) ctx->ob.queue->drain();
}

void free_observe(vsf_ctx* ctx) {
  vsf_ctx::Observe& o = ctx->ob;
  stop_observe_threads(ctx);
  // the device ring is written on the PRODUCERS' streams (vsf_observe_submit_dev), which sync_all_streams does not know: the
  // events recorded behind those launches say when they are done with it
  for (const Event& e : o.dev_ev)
    if (e) (void)hipEventSynchronize(e);
  // launch_batch publishes a batch slot's images as the context's last input (the vsf_debug_* level-0 reads): that view dies here
  for (const vsf_ctx::ObserveBatch& b : o.batch)
    if (b.d_img && ctx->last_images.base == b.d_img) ctx->last_valid = false;
  o = vsf_ctx::Observe();
}

}  // namespace vsfi

namespace {

ObserveGpu observe_gpu(vsf_ctx* ctx);

// The encode of a batch's n stereo canvases (which = 0: 2w x h) or match canvases (1: w x h) into the device slots: the ONE
// description the scratch is sized by and the tail launches with.
VsfEncodeJob debug_files_job(const vsf_ctx* ctx, int which, int n) {
  const vsf_ctx::Observe& o = ctx->ob;
  const int w = which ? ctx->p.width : 2 * ctx->p.width;
  return {o.files.form.kind, n, w, ctx->p.height, 3, o.dbg_stride, (size_t)3 * w, o.files.form.quality, o.files.slot, o.files.cap[which]};
}

// A slot of the ring of files: i32 stereo bytes, i32 match bytes, then (16-byte aligned) room for the encoder's bound of each.
void debug_files_slot_layout(vsf_ctx::Observe::DebugFiles& f, int w, int h) {
  for (int which = 0; which < 2; which++)
    f.cap[which] = (vsf_encode_capacity(f.form.kind, which ? w : 2 * w, h, 3) + 15) & ~(size_t)15;
  f.off[0] = 16;
  f.off[1] = 16 + f.cap[0];
  f.slot = (16 + f.cap[0] + f.cap[1] + 255) & ~(size_t)255;
}

// The files leave, not the canvases: device slots, the encoder's scratch and a pinned ring sized by the encoder's bound.
vsf_status alloc_debug_files(vsf_ctx* ctx) {
  vsf_ctx::Observe& o = ctx->ob;
  vsf_ctx::Observe::DebugFiles& f = o.files;
  const size_t B = (size_t)o.bmax;
  debug_files_slot_layout(f, ctx->p.width, ctx->p.height);
  if (f.cap[0] > 0x7FFFFFF0u) return VSF_ERR_UNSUPPORTED;
  VSF_HIP(f.d_slots.alloc(B * f.slot));
  // (+ the encoder's status word: a file that does not fit leaves its count at -1, which is what the view reports)
  VSF_HIP(f.d_bytes.alloc((2 * B + 1) * sizeof(int32_t)));
  VSF_HIP(hipMemset(f.d_bytes, 0, (2 * B + 1) * sizeof(int32_t)));
  VSF_HIP(f.d_scratch.alloc(std::max(vsf_encode_scratch_need(debug_files_job(ctx, 0, o.bmax)),
                                                   vsf_encode_scratch_need(debug_files_job(ctx, 1, o.bmax)))));
  VSF_HIP(f.h_ring.alloc((size_t)o.depth * f.slot, hipHostMallocMapped));
  return VSF_OK;
}

// vsf_observe_set_debug_seeds: streams [s0, s0 + n) start over -- srand(seed) -- in device memory.  (No kernel reads them: the
// queue is being built, or every frame of the stream has been collected.)
vsf_status upload_debug_generators(vsf_ctx* ctx, int s0, int n) {
  vsf_ctx::Observe& o = ctx->ob;
  std::vector<vsfrand::State> st((size_t)n);
  for (int s = 0; s < n; s++) vsfrand::seed(st[(size_t)s], o.seeds[(size_t)(s0 + s)]);
  VSF_HIP(hipMemcpy(o.dbg_rand + (size_t)s0 * 32, st.data(), (size_t)n * sizeof(vsfrand::State), hipMemcpyHostToDevice));
  return VSF_OK;
}

vsf_status ensure_observe(vsf_ctx* ctx, int frame_life) {
  vsf_ctx::Observe& o = ctx->ob;
  const vsf_ctx::DebugForm form = ctx->ob_debug ? ctx->ob_debug_form : vsf_ctx::DebugForm();
  const bool seeded = ctx->ob_debug && ctx->ob_seeded;  // (seeds without debug images: a queue as it always was)
  if (o.ready && o.frame_life == frame_life && o.debug == ctx->ob_debug && o.files.form == form && o.cloud == ctx->ob_cloud &&
      (!o.cloud || std::memcmp(o.cam_to_robot, ctx->ob_cam_to_robot, sizeof(o.cam_to_robot)) == 0) && o.seeded == seeded &&
      (!seeded || std::equal(o.seeds.begin(), o.seeds.end(), ctx->ob_seeds)))
    return VSF_OK;
  sync_all_streams(ctx);
  const int NS = ctx->ob_streams;
  std::vector<float> thr_state((size_t)NS, 10000.0f);  // cc:353, per stream
  if (o.floats)
    VSF_HIP(hipMemcpy(thr_state.data(), tail_thr_state(o), (size_t)std::min(NS, o.n_streams) * sizeof(float), hipMemcpyDeviceToHost));
  free_observe(ctx);
  o.n_streams = NS;
  o.streams.assign((size_t)NS, vsf_ctx::ObserveStream());
  const size_t K = (size_t)ctx->p.max_keypoints;
  const int frames_cap = std::max(1, ctx->p.max_images / 2);  // the extraction's own buffers hold max_images images
  o.depth = ctx->ob_depth > 0 ? ctx->ob_depth : frames_cap;
  o.bmax = std::min(o.depth, frames_cap);
  o.frame_life = frame_life;
  o.debug = ctx->ob_debug;
  o.files.form = form;
  o.ring = frame_life + o.bmax;
  o.max_pairs = o.bmax * (frame_life + 1);
  // (a batch may be one stream's frames alone: every stream's ring has room for frame_life + bmax sets)
  const size_t B = (size_t)o.bmax, P = (size_t)o.max_pairs, S = (size_t)NS * o.ring + B;
  VSF_HIP(o.sets.alloc(S * K * VSF_DESC_BYTES));
  VSF_HIP(o.set_counts.alloc(S * sizeof(int32_t)));
  VSF_HIP(hipMemset(o.set_counts, 0, S * sizeof(int32_t)));
  VSF_HIP(o.residual.alloc(B * K * sizeof(float)));
  VSF_HIP(o.floats.alloc(tail_floats(o) * sizeof(float)));
  VSF_HIP(hipMemset(o.floats, 0, tail_floats(o) * sizeof(float)));
  VSF_HIP(hipMemcpy(tail_thr_state(o), thr_state.data(), (size_t)NS * sizeof(float), hipMemcpyHostToDevice));
  VSF_HIP(o.kpf.alloc(2 * B * K * sizeof(vsf_keypoint)));
  VSF_HIP(o.ints.alloc(tail_ints(o) * sizeof(int32_t)));
  VSF_HIP(hipMemset(o.ints, 0, tail_ints(o) * sizeof(int32_t)));
  VSF_HIP(o.ex_idx2.alloc(B * K * 2 * sizeof(int32_t)));
  VSF_HIP(o.ex_dist2.alloc(B * K * 2 * sizeof(int32_t)));
  VSF_HIP(o.t_idx2.alloc(P * K * 2 * sizeof(int32_t)));
  VSF_HIP(o.t_dist2.alloc(P * K * 2 * sizeof(int32_t)));
  VSF_HIP(o.t_matches.alloc(P * K * sizeof(vsf_dmatch)));
  VSF_HIP(o.t_nmatches.alloc(P * sizeof(int32_t)));
  VSF_HIP(o.t_sortkeys.alloc(P * K * 8));
  VSF_HIP(o.pairs.alloc(P * K * 2 * sizeof(uint64_t)));
  VSF_HIP(o.npairs.alloc(P * sizeof(int32_t)));
  VSF_HIP(o.features.alloc(B * K * sizeof(vsf_vision_feature)));
  o.out_cap = vsf_observe_capacity(ctx, frame_life);
  o.out_stride = (o.out_cap + 255) & ~(size_t)255;
  VSF_HIP(o.h_img.alloc((size_t)o.depth * 2 * ctx->st_img_stride, hipHostMallocMapped));
  VSF_HIP(o.h_out.alloc((size_t)o.depth * o.out_stride, hipHostMallocMapped));
  if (o.debug) {  // vsf_observe_set_debug_images: canvases, winners, operations, the pinned debug ring and colour ring
    const size_t wh = (size_t)ctx->p.width * ctx->p.height;
    o.dbg_stride = (9 * wh + 255) & ~(size_t)255;  // stereo 2w x h x 3 | match w x h x 3
    o.col_ring = (int64_t)(o.depth + 1) * (int64_t)K;
    VSF_HIP(o.dbg_canvas.alloc(B * o.dbg_stride));
    VSF_HIP(o.dbg_win.alloc(B * 3 * wh * sizeof(uint64_t)));
    VSF_HIP(hipMemset(o.dbg_win, 0, B * 3 * wh * sizeof(uint64_t)));
    VSF_HIP(o.dbg_ops.alloc(B * 5 * K * sizeof(vsf_draw_op)));
    VSF_HIP(o.dbg_table.alloc(2 * B * 128));
    VSF_HIP(o.dbg_prev_kp.alloc((size_t)NS * K * sizeof(vsf_keypoint)));
    VSF_HIP(o.dbg_ints.alloc(8 + (((size_t)NS * sizeof(int32_t) + 7) & ~(size_t)7)));
    VSF_HIP(hipMemset(o.dbg_ints, 0, 8 + (((size_t)NS * sizeof(int32_t) + 7) & ~(size_t)7)));
    if (form.kind) {
      const vsf_status st = alloc_debug_files(ctx);
      if (st != VSF_OK) return st;
    } else {
      VSF_HIP(o.h_dbg.alloc((size_t)o.depth * o.dbg_stride, hipHostMallocMapped));
    }
    o.seeded = seeded;
    if (seeded) {  // a generator per stream on the device: no colour ring, no rand()
      o.seeds.assign(ctx->ob_seeds, ctx->ob_seeds + NS);
      VSF_HIP(o.dbg_rand.alloc((size_t)NS * sizeof(vsfrand::State)));
      VSF_HIP(o.dbg_stream_colours.alloc(B * K * sizeof(uint32_t)));
      const vsf_status st = upload_debug_generators(ctx, 0, NS);
      if (st != VSF_OK) return st;
    } else {
      VSF_HIP(o.h_col.alloc((size_t)o.col_ring * sizeof(uint32_t), hipHostMallocMapped));
    }
  }
  o.cloud = ctx->ob_cloud;
  if (o.cloud) {  // vsf_observe_set_world_points: the pinned ring of points and its counts, written by the tail's kernel
    std::memcpy(o.cam_to_robot, ctx->ob_cam_to_robot, sizeof(o.cam_to_robot));
    VSF_HIP(o.h_wp.alloc((size_t)o.depth * K * 3 * sizeof(double), hipHostMallocMapped));
    VSF_HIP(o.h_wp_n.alloc((size_t)o.depth * sizeof(int32_t), hipHostMallocMapped));
    std::memset(o.h_wp_n, 0, (size_t)o.depth * sizeof(int32_t));
  }
  for (vsf_ctx::ObserveBatch& b : o.batch) {
    VSF_HIP(b.d_img.alloc(2 * B * ctx->st_img_stride));
    VSF_HIP(b.kp_raw.alloc(2 * B * K * sizeof(vsf_keypoint)));
    VSF_HIP(b.desc_raw.alloc(2 * B * K * VSF_DESC_BYTES));
    VSF_HIP(b.counts_raw.alloc(2 * B * sizeof(int32_t)));
    VSF_HIP(b.matches.alloc(B * K * sizeof(vsf_dmatch)));
    VSF_HIP(b.nmatches.alloc(B * sizeof(int32_t)));
    VSF_HIP(b.status.alloc(2 * B * sizeof(int32_t)));
    VSF_HIP(hipMemset(b.status, 0, 2 * B * sizeof(int32_t)));
    VSF_HIP(b.h_meta.alloc(meta_bytes(o.max_pairs, o.bmax), hipHostMallocMapped));
    std::memset(b.h_meta, 0, meta_bytes(o.max_pairs, o.bmax));
    VSF_HIP(b.ev_uploaded.alloc(hipEventDisableTiming));
    VSF_HIP(b.ev_extracted.alloc(hipEventDisableTiming));
    VSF_HIP(b.ev_done.alloc(hipEventDisableTiming));
  }
  o.frames.assign((size_t)o.depth, vsf_ctx::ObserveFrame());
  // The tail rides a high-priority stream: it is short, latency-bound and what the host waits for; streams of different
  // priorities never share a hardware queue, so it runs beside the next batch's extraction instead of taking turns with it.
  int prio_lo = 0, prio_hi = 0;
  VSF_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  VSF_HIP(o.tail_stream.alloc(hipStreamNonBlocking, prio_hi));
  // ... and the uploads the LOWEST: with the default priority the copy stream may land on the hardware queue of the
  // context's stream (HIP hands its few queues out round-robin) and the next batch's upload then waits for this batch's
  // extraction instead of running beside it -- which it did or did not from one context to the next (17 k or 27 k frames/s)
  VSF_HIP(o.copy_stream.alloc(hipStreamNonBlocking, prio_lo));
  VSF_HIP(hipDeviceSynchronize());
  o.queue.reset(new (std::nothrow) ObserveQueue({o.depth, o.bmax, ctx->ob_min_batch, ctx->ob_in_flight}, observe_gpu(ctx)));
  if (!o.queue) return VSF_ERR_INVALID_ARG;
  o.ready = true;
  // the two host threads of a deep queue: VSF_OPT_OBSERVE_THREAD (without it the caller launches everything) and
  // VSF_OPT_OBSERVE_COPY_THREAD (without it the caller stages both images)
  if (o.depth >= 4 && ctx->tuning.observe_copy_thread) o.copy_helper.reset(new (std::nothrow) ObserveCopyHelper());
  if (o.depth >= 4 && ctx->tuning.observe_thread) o.queue->start_thread();
  return VSF_OK;
}

int batches_on_gpu(vsf_ctx* ctx) {  // launched and not finished (a query costs 0.1 us)
  int n = 0;
  for (vsf_ctx::ObserveBatch& b : ctx->ob.batch)
    if (b.used && hipEventQuery(b.ev_done) != hipSuccess) n++;
  (void)hipGetLastError();  // (hipErrorNotReady is not an error)
  return n;
}

// The debug images (slam_frontend.cc:74-115, 167-171, 458-466) of batch [t0, t0 + n), drawn in its tail from what it holds in HBM; then
// the canvases go into the frames' slots of the pinned debug ring (one copy, two when the slots wrap), or their files into the ring of files.
vsf_status launch_debug_images(vsf_ctx* ctx, const vsf_ctx::ObserveBatch& b, const MetaView& M, int64_t t0, int n, hipStream_t s_tail) {
  vsf_ctx::Observe& o = ctx->ob;
  vsf_ctx::Observe::DebugFiles& fl = o.files;
  // per canvas size (stereo, match): one copy command, or the encoder's launches + the kernel that carries the files home
  const int per_size = fl.form.kind ? vsf_encode_launches(fl.form.kind) + 1 : 1;
  StageTimer t(ctx, s_tail, VSF_STAGE_TAIL, 4 + (o.seeded ? 1 : 0) + 2 * per_size);  // (4: the drawing kernels; the colours')
  // (in the order of the struct's fields; o.ints: the filtered frames' counts, o.dbg_ints: the colour cursor, then the kept frame's count)
  const VsfObserveDebugArgs d{n, ctx->p.max_keypoints, ctx->p.width, ctx->p.height, b.d_img, ctx->st_img_stride, ctx->st_img_pitch,
                              o.kpf, o.ints, o.pairs, o.npairs, M.frames, o.dbg_prev_kp, reinterpret_cast<int32_t*>(o.dbg_ints + 1),
                              o.h_col, o.col_ring, o.dbg_ints, o.dbg_ops, o.dbg_table, o.dbg_canvas, o.dbg_stride, o.dbg_win,
                              o.h_out, o.out_stride, o.seeded ? M.params : nullptr, o.dbg_rand, o.dbg_stream_colours};
  vsf_launch_observe_debug(d, s_tail);
  if (o.seeded) {
    o.queue->stats.seeded_frames += n;
    o.queue->stats.colour_commands++;
  }
  const int slot0 = (int)(t0 % o.depth), first = std::min(n, o.depth - slot0);
  if (fl.form.kind) {
    // cv::imencode(".jpg") / (".png") of the canvases just drawn, stereo then match (two sizes: two encodes), into the batch's
    // device slots; then only the files' bytes cross to the pinned ring
    for (int which = 0; which < 2; which++) {
      int32_t* d_bytes = fl.d_bytes + (size_t)which * o.bmax;
      vsf_launch_encode(debug_files_job(ctx, which, n), o.dbg_canvas + (which ? (size_t)6 * d.width * d.height : 0), fl.d_scratch,
                        fl.d_slots + fl.off[which], d_bytes, fl.d_bytes + 2 * (size_t)o.bmax, s_tail);
      vsf_launch_files_home(fl.d_slots + fl.off[which], fl.slot, d_bytes, n, fl.h_ring, fl.slot, fl.off[which], which, slot0, o.depth,
                            M.frames, o.h_out, o.out_stride, s_tail);
    }
    o.queue->stats.file_commands += 2 * per_size;
  } else {
    VSF_HIP(hipMemcpyAsync(o.h_dbg + (size_t)slot0 * o.dbg_stride, o.dbg_canvas, (size_t)first * o.dbg_stride,
                           hipMemcpyDeviceToHost, s_tail));
    if (first < n)
      VSF_HIP(hipMemcpyAsync(o.h_dbg, o.dbg_canvas + (size_t)first * o.dbg_stride, (size_t)(n - first) * o.dbg_stride,
                             hipMemcpyDeviceToHost, s_tail));
  }
  return VSF_OK;
}

// Queues frames [t0, t0 + n) -- they wait in consecutive staging slots -- as one batch.  The caller holds the queue's baton.
vsf_status launch_batch(vsf_ctx* ctx, int64_t t0, int n, bool solo, int rows_hint) {
  vsf_ctx::Observe& o = ctx->ob;
  ObserveLaunchStats& stats = o.queue->stats;
  const int64_t t_begin = now_ns();
  const int bi = (int)(stats.batches % vsf_ctx::kObserveBatchSlots);
  vsf_ctx::ObserveBatch& b = o.batch[bi];
  // The slot's previous batch must have left the GPU: its kernels read the pinned parameter block that is rewritten below
  // (with `in_flight` batches on the GPU and four slots it has, long ago).
  if (b.used) {
    if (hipEventQuery(b.ev_done) != hipSuccess) stats.slot_waits++;
    (void)hipGetLastError();
    VSF_HIP(hipEventSynchronize(b.ev_done));
  }
  const size_t K = (size_t)ctx->p.max_keypoints;
  const int Kc = (int)K, life = o.frame_life;
  // ---- the batch's plan, before anything is enqueued: a refused batch leaves nothing on the streams ----
  // (vsf_observe_plan.cc: sets, pairs, the calibration table -- the submit has cut the list where a stream's parameters change --
  // and the ingest: what every frame is, the commands that bring its images into b.d_img)
  ObserveIngestPlan& I = o.ingest;
  o.plan_in.resize((size_t)n);
  I.in.resize((size_t)n);
  for (int f = 0; f < n; f++) {  // the ONE pass over the batch's frames that says what they are
    const vsf_ctx::ObserveFrame& fr = o.frames[(size_t)((t0 + f) % o.depth)];
    o.plan_in[(size_t)f] = {fr.stream, fr.k, &fr.calib, fr.best_percent};
    I.in[(size_t)f] = {fr.kind[0], fr.pix_new, fr.in_w, fr.in_h};
  }
  const ObservePlan& P = o.plan;
  if (!observe_plan(o.plan_in.data(), n, o.n_streams, o.ring, life, &o.plan) || !P.cuts.empty() || P.n_pairs > o.max_pairs)
    return VSF_ERR_INVALID_ARG;
  // (a batch has ONE pixel format: the submit has cut the list where it changes; in_half: the queue has seen a big-slot frame --
  // until then no record's declared size is looked at or written)
  if (!observe_ingest_plan(n, o.frames[(size_t)(t0 % o.depth)].pixfmt, t0, o.depth, o.in_half != 0,
                           observe_upload_max_gap(2 * o.in_half), &I))
    return VSF_ERR_INVALID_ARG;
  const int n_pairs = P.n_pairs, max_pairs_per_frame = P.max_pairs_per_frame;
  // one calibration: it rides in the kernel arguments; one stream: the chain of the lone sequence (both: today's launches)
  const bool table = P.calibs.size() > 1, chains = P.n_streams_present > 1;
  const vsf_calibration& calib0 = P.calibs[0];
  // solo: a lone frame with nothing else on the GPU runs on ONE stream from upload to result (no event hops in its chain);
  // otherwise copy, extraction and tail have a stream each, so that the next batch's upload and extraction run beside
  // this one's tail.
  // (compressed frames are decoded on the copy stream whatever else runs: the decoders' scratch exists once, for that stream)
  hipStream_t s_copy = solo && !I.files && !I.big_files ? ctx->stream : o.copy_stream, s_ex = ctx->stream,
              s_tail = solo ? ctx->stream : o.tail_stream;
  {
    const vsf_status st = ingest(ctx, b, t0, n, I, s_copy);
    if (st != VSF_OK) return st;
  }
  // ---- the batch's parameters, in pinned memory the kernels read directly ----
  const MetaView M = meta_view(b.h_meta, o.max_pairs, o.bmax);
  for (int f = 0; f < n; f++) {
    const ObservePlanFrame& pf = P.frames[(size_t)f];
    M.out_sets[2 * f] = pf.left_set;
    M.out_sets[2 * f + 1] = pf.right_set;
    M.frames[f] = {pf.left_set, pf.n_past, pf.tp0, (int32_t)((t0 + f) % o.depth)};
    if (table || chains || o.seeded) M.params[f] = {pf.stream, pf.calib, pf.best_percent, pf.prev, pf.tail};
  }
  std::memcpy(M.q_set, P.q_set.data(), (size_t)n_pairs * sizeof(int32_t));
  std::memcpy(M.t_set, P.t_set.data(), (size_t)n_pairs * sizeof(int32_t));
  std::memcpy(M.best_percent, P.best_percent.data(), (size_t)n_pairs * sizeof(float));
  if (table) std::memcpy(M.calibs, P.calibs.data(), P.calibs.size() * sizeof(vsf_calibration));
  if (o.cloud)  // M_f = (Translation(loc) * quat) * cam_to_robot of every frame, from the pose it was submitted with
    for (int f = 0; f < n; f++) {
      const vsf_ctx::ObserveFrame& fr = o.frames[(size_t)((t0 + f) % o.depth)];
      M.transforms[f] = vsfwp::camera_to_world(fr.pose.loc, fr.pose.quat_xyzw, fr.cam_to_robot);
    }
  b.h_meta->n_frames = n;
  b.h_meta->n_pairs = n_pairs;
  // ---- ExtractFeatures x 2 + GetMatches of every frame (cc:411-416) ----
  const VsfImages im{b.d_img, ctx->st_img_stride, ctx->st_img_pitch, 2 * n};
  // (Measured and left out: the pyramid of a batch on a side stream beside the previous batch's later stages, the
  // cross-call pipelining of vsf_set_pipeline -- 27.5 -> 23.4 k frames/s at 64 frames per batch, 31.9 -> 27.5 k at 128: the
  // single chain of 49 dependent launches is slower than the two chains + image-major kernel it replaces and takes the
  // vector ALU from the stages it runs beside.)
  // the images' detection masks (vsf_observe_set_stream_masks, as each frame's stream had them when it was submitted): a table
  // in the batch's pinned block; a batch without any takes the kernels without the predicate
  VsfFastMask masks;
  for (int f = 0; f < n; f++) {
    const vsf_ctx::ObserveFrame& fr = o.frames[(size_t)((t0 + f) % o.depth)];
    for (int side = 0; side < 2; side++) {
      const int slot = fr.mask_slot[side];
      M.masks[2 * f + side] = slot >= 0 && ctx->masks[slot].set ? ctx->masks[slot].block.get() : nullptr;
      if (M.masks[2 * f + side]) masks.table = M.masks;
    }
  }
  masks.bytes = ctx->orb.g.pyr_bytes;
  extract_on(ctx, s_ex, im, 0, 2 * n, b.kp_raw, b.desc_raw, b.counts_raw, false, nullptr, b.status, 1, &masks);
  ctx->last_images = im;
  ctx->last_valid = true;
  match_on(ctx, s_ex, b.desc_raw, b.counts_raw, K * VSF_DESC_BYTES, nullptr, nullptr, 0, n, o.ex_idx2, o.ex_dist2, b.matches,
           b.nmatches, b.status);
  if (s_tail != s_ex) {
    VSF_HIP(hipEventRecord(b.ev_extracted, s_ex));
    VSF_HIP(hipStreamWaitEvent(s_tail, b.ev_extracted, 0));
  }
  // the tails run in frame order: behind the previous batch's, whatever stream that ran on
  if (o.last_batch >= 0 && o.batch[o.last_batch].done_stream != s_tail)
    VSF_HIP(hipStreamWaitEvent(s_tail, o.batch[o.last_batch].ev_done, 0));
  // ---- RemoveAmbigStereo (cc:417): residuals, the threshold chain in frame order, the rebuilt frames ----
  float *means = tail_means(o), *thr = tail_thr(o), *thr_state = tail_thr_state(o);
  int32_t *counts_f = tail_counts_f(o), *nfeat = tail_nfeat(o), *npoints = tail_npoints(o);
  {
    StageTimer t(ctx, s_tail, VSF_STAGE_TAIL, 3);
    // (a lone frame: the three steps in one launch)
    float* thr_state0 = thr_state + P.frames[0].stream;
    if (n != 1 || !vsf_launch_stereo_one_frame(b.kp_raw, b.desc_raw, b.matches, b.nmatches, Kc, calib0.fundamental,
                                               ctx->p.residual_order, means, thr, thr_state0, o.kpf, o.sets, counts_f,
                                               M.out_sets, o.set_counts, s_tail)) {
      if (table)
        vsf_launch_stereo_residuals_table(b.kp_raw, b.matches, b.nmatches, n, Kc, M.params, M.calibs, ctx->p.residual_order,
                                          o.residual, means, s_tail);
      else
        vsf_launch_stereo_residuals(b.kp_raw, b.matches, b.nmatches, n, Kc, nullptr, calib0.fundamental, ctx->p.residual_order,
                                    o.residual, means, s_tail);
      if (chains)
        vsf_launch_stereo_thresholds_streams(means, n, M.params, thr_state, thr, s_tail);
      else
        vsf_launch_stereo_thresholds(means, n, thr_state0, thr, s_tail);
      vsf_launch_stereo_filter_only(b.kp_raw, b.desc_raw, b.matches, b.nmatches, n, Kc, o.residual, thr, o.kpf, o.sets,
                                    counts_f, s_tail, M.out_sets, o.set_counts);
    }
  }
  // ---- every GetFeatureMatches of the batch: one matcher launch, one sort launch (per-pair best_percent) ----
  {
    StageTimer t(ctx, s_tail, VSF_STAGE_KNN2, 1);
    // (rows_hint: what the caller's last collected frames held -- a filtered frame is a few hundred rows of the capacity)
    vsf_launch_knn2(o.sets, o.set_counts, K * VSF_DESC_BYTES, M.q_set, M.t_set, n_pairs, Kc, o.t_idx2, o.t_dist2, s_tail,
                    rows_hint);
  }
  {
    StageTimer t(ctx, s_tail, VSF_STAGE_RATIO, 1);
    vsf_launch_ratio_compact(o.set_counts, M.q_set, M.t_set, n_pairs, Kc, o.t_idx2, o.t_dist2, ctx->p.ratio_num,
                             ctx->p.ratio_shift, o.t_matches, o.t_nmatches, b.status, s_tail);
  }
  {
    StageTimer t(ctx, s_tail, VSF_STAGE_TAIL, 3);
    vsf_launch_sort_trim(o.t_matches, o.t_nmatches, n_pairs, Kc, P.frames[0].best_percent, M.best_percent, o.t_sortkeys, o.pairs,
                         o.npairs, s_tail, false, ctx->tuning.lds_limit);
    // ---- Calculate3DPoints + VisionFeature + UndistortFeaturePoints (cc:437-443): pairs [0, n) are the right -> left ones ----
    if (table)
      vsf_launch_vision_features_table(o.kpf, counts_f, o.pairs, o.npairs, n, Kc, M.params, M.calibs, o.features, nfeat, npoints,
                                       s_tail);
    else
      vsf_launch_vision_features(o.kpf, counts_f, o.pairs, o.npairs, n, Kc, calib0, o.features, nfeat, npoints, s_tail);
    // ---- one compact result per frame, into its slot of the pinned result ring ----
    VsfObserveArgs a;
    a.n_frames = n;
    a.max_rows = Kc;
    a.counts_raw = b.counts_raw;
    a.nmatches = b.nmatches;
    a.counts_f = counts_f;
    a.npoints = npoints;
    a.means = means;
    a.thr = thr;
    a.features = o.features;
    a.kp_f = o.kpf;
    a.desc_sets = o.sets;
    a.pairs = o.pairs;
    a.npairs = o.npairs;
    a.status = b.status;
    a.frames = M.frames;
    a.out = o.h_out;
    a.out_stride = o.out_stride;
    a.out_cap = (uint32_t)std::min<size_t>(o.out_cap, 0xFFFFFFF0u);
    vsf_launch_observe_pack(a, max_pairs_per_frame, s_tail);
  }
  if (o.cloud) {
    // ---- the point cloud (main.cc:155-173): ONE launch over the records just made; each frame's points and their count land
    // in its slot of the pinned rings, as the result does (no copy command) ----
    StageTimer t(ctx, s_tail, VSF_STAGE_TAIL, 1);
    vsf_launch_world_points_table(o.features, nfeat, n, Kc, M.transforms, M.frames, o.h_wp, o.h_wp_n, s_tail);
    stats.cloud_commands++;
    stats.cloud_frames += n;
  }
  if (o.debug) {
    const vsf_status st = launch_debug_images(ctx, b, M, t0, n, s_tail);
    if (st != VSF_OK) return st;
  }
  VSF_HIP(hipEventRecord(b.ev_done, s_tail));
  b.used = true;
  b.done_stream = s_tail;
  for (int f = 0; f < n; f++) o.frames[(size_t)((t0 + f) % o.depth)].batch = bi;
  o.last_batch = bi;
  if (chains) stats.multi++;
  stats.launch_ns += now_ns() - t_begin;
  VSF_STICKY();
  return VSF_OK;
}

// What the queue sees of the GPU (vsf_observe_queue.h).
ObserveGpu observe_gpu(vsf_ctx* ctx) {
  return {ctx,
          [](void* c, int64_t t0, int n, bool solo, int rows_hint) {
            return launch_batch(static_cast<vsf_ctx*>(c), t0, n, solo, rows_hint);
          },
          [](void* c) { return batches_on_gpu(static_cast<vsf_ctx*>(c)); },
          [](void* c) { return hipSetDevice(static_cast<vsf_ctx*>(c)->device) == hipSuccess; }};
}

vsf_pose identity_pose() { return {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 1.f}}; }

bool frames_in_queue(const vsf_ctx* ctx) { return ctx->ob.ready && ctx->ob.queue->next_collect != ctx->ob.queue->next_ticket; }

// What a queue is built with changes only before its window holds a frame: the next submit rebuilds the queue
// (ensure_observe carries the threshold).
vsf_status retire_unused_queue(vsf_ctx* ctx) {
  if (!ctx->ob.ready) return VSF_OK;
  if (ctx->ob.queue->next_ticket != 0) return VSF_ERR_INVALID_ARG;
  stop_observe_threads(ctx);
  return VSF_OK;
}

// The queue goes -- frames that still wait are dropped, the thresholds and the windows forgotten: the next submit builds another.
vsf_status drop_queue(vsf_ctx* ctx) {
  VSF_HIP(hipSetDevice(ctx->device));
  stop_observe_threads(ctx);
  sync_all_streams(ctx);
  free_observe(ctx);
  return VSF_OK;
}

// vsf_observe_set_debug_jpeg / _png: quality != 0 asks for files of `kind`, 0 takes that request back.
vsf_status set_debug_form(vsf_ctx* ctx, int kind, int quality) {
  vsf_ctx::DebugForm& f = ctx->ob_debug_form;
  // (debug images of several streams need a generator per stream: vsf_observe_set_debug_seeds)
  if (quality != 0 && ctx->ob_streams > 1 && !ctx->ob_seeded) return VSF_ERR_UNSUPPORTED;
  if (quality == (f.kind == kind ? f.quality : 0)) return VSF_OK;
  if (quality != 0 && !ctx->ob_debug) return VSF_ERR_INVALID_ARG;  // files of images nobody draws
  if (quality != 0 && f.kind != VSF_FILE_NONE && f.kind != kind) return VSF_ERR_INVALID_ARG;  // one form of file at a time
  const vsf_status st = retire_unused_queue(ctx);
  if (st != VSF_OK) return st;
  f.kind = quality ? kind : VSF_FILE_NONE;
  f.quality = quality;
  return VSF_OK;
}

// The slot of a frame whose results the views may hand out: collected, and its slot not yet handed to a later frame (valid
// until `depth` further frames have been submitted).  -1: `ticket` is no such frame, or there is no queue.
int collected_slot(const vsf_ctx::Observe& o, int64_t ticket) {
  if (!o.ready || ticket < 0 || ticket >= o.queue->next_collect || ticket < o.queue->next_ticket - o.depth) return -1;
  return (int)(ticket % o.depth);
}

// A collected frame's two files inside the pinned ring of files; kind: which form the caller asks for.
vsf_status debug_files_view(vsf_ctx* ctx, int kind, int64_t ticket, const uint8_t** stereo, size_t* stereo_bytes,
                            const uint8_t** match, size_t* match_bytes) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || !stereo || !stereo_bytes || !match || !match_bytes) return VSF_ERR_INVALID_ARG;
  *stereo = *match = nullptr;
  *stereo_bytes = *match_bytes = 0;
  const vsf_ctx::Observe& o = ctx->ob;
  const int slot = o.debug && o.files.form.kind == kind ? collected_slot(o, ticket) : -1;
  if (slot < 0) return VSF_ERR_INVALID_ARG;
  const uint32_t flags = reinterpret_cast<const uint32_t*>(o.h_out + (size_t)slot * o.out_stride)[14];
  const uint8_t* base = o.files.h_ring + (size_t)slot * o.files.slot;
  const int32_t* n = reinterpret_cast<const int32_t*>(base);
  // (cannot happen while vsf_encode_capacity is the bound it claims to be: a file that did not fit its slot)
  if (((flags & 1) && n[0] < 0) || ((flags & 2) && n[1] < 0)) return VSF_ERR_CAPACITY;
  if ((flags & 1) && n[0] > 0) {
    *stereo = base + o.files.off[0];
    *stereo_bytes = (size_t)n[0];
  }
  if ((flags & 2) && n[1] > 0) {
    *match = base + o.files.off[1];
    *match_bytes = (size_t)n[1];
  }
  return VSF_OK;
}

}  // namespace

// Every entry point of the context except the queue's own comes through here (VsfErrorScope): what waits in the queue
// leaves first and the launcher thread is idle afterwards -- it only wakes for frames that wait.
void vsf_ctx_enter(vsf_ctx* ctx) {
  vsf_ctx::Observe& o = ctx->ob;
  if (!o.ready || !o.queue->has_thread) return;
  if (hipSetDevice(ctx->device) != hipSuccess) return;
  o.queue->drain();
}

extern "C" {

size_t vsf_observe_capacity(const vsf_ctx* ctx, int frame_life) {
  if (!ctx || frame_life < 0 || frame_life + 1 > VSF_OBSERVE_MAX_PAIRS) return 0;
  const size_t K = (size_t)ctx->p.max_keypoints;
  return 64 + 4 * (size_t)((frame_life + 1 + 3) & ~3) + K * (28 + 28 + 32) + (size_t)(frame_life + 1) * K * 16;
}

vsf_status vsf_observe_set_debug_images(vsf_ctx* ctx, int on) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx) return VSF_ERR_INVALID_ARG;
  // several streams: rand()'s colour sequence must exist per stream (vsf_observe_set_debug_seeds); without it, refused
  if (on != 0 && ctx->ob_streams > 1 && !ctx->ob_seeded) return VSF_ERR_UNSUPPORTED;
  if ((on != 0) == ctx->ob_debug) return VSF_OK;
  const vsf_status st = retire_unused_queue(ctx);
  if (st == VSF_OK) ctx->ob_debug = on != 0;
  return st;
}

vsf_status vsf_observe_set_world_points(vsf_ctx* ctx, int on, const float* cam_to_robot) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || (on != 0 && !cam_to_robot)) return VSF_ERR_INVALID_ARG;
  if ((on != 0) == ctx->ob_cloud &&
      (on == 0 || std::memcmp(cam_to_robot, ctx->ob_cam_to_robot, sizeof(ctx->ob_cam_to_robot)) == 0))
    return VSF_OK;
  const vsf_status st = retire_unused_queue(ctx);
  if (st != VSF_OK) return st;
  ctx->ob_cloud = on != 0;
  if (on != 0) std::memcpy(ctx->ob_cam_to_robot, cam_to_robot, sizeof(ctx->ob_cam_to_robot));
  return VSF_OK;
}

vsf_status vsf_observe_set_stream_masks(vsf_ctx* ctx, int stream, int left_slot, int right_slot) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || stream < 0 || stream >= ctx->ob_streams || left_slot < -1 || left_slot >= VSF_MAX_MASKS || right_slot < -1 ||
      right_slot >= VSF_MAX_MASKS)
    return VSF_ERR_INVALID_ARG;
  ctx->ob_masks[stream].left = left_slot;
  ctx->ob_masks[stream].right = right_slot;
  return VSF_OK;
}

vsf_status vsf_observe_set_pose(vsf_ctx* ctx, int stream, const float* loc, const float* quat_xyzw) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || stream < 0 || stream >= ctx->ob_streams || !loc || !quat_xyzw) return VSF_ERR_INVALID_ARG;
  vsf_pose& p = ctx->ob_pose[stream];
  for (int i = 0; i < 3; i++) p.loc[i] = loc[i];
  for (int i = 0; i < 4; i++) p.quat_xyzw[i] = quat_xyzw[i];
  return VSF_OK;
}

vsf_status vsf_observe_world_points_view(vsf_ctx* ctx, int64_t ticket, const double** xyz, int32_t* n) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || !xyz || !n) return VSF_ERR_INVALID_ARG;
  *xyz = nullptr;
  *n = 0;
  const vsf_ctx::Observe& o = ctx->ob;
  const int slot = o.cloud ? collected_slot(o, ticket) : -1;
  if (slot < 0) return VSF_ERR_INVALID_ARG;
  const int32_t count = std::min(std::max(o.h_wp_n[slot], 0), ctx->p.max_keypoints);
  *n = count;
  if (count > 0) *xyz = o.h_wp + (size_t)slot * ctx->p.max_keypoints * 3;
  return VSF_OK;
}

vsf_status vsf_observe_debug_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** stereo, const uint8_t** match) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || !stereo || !match) return VSF_ERR_INVALID_ARG;
  *stereo = *match = nullptr;
  const vsf_ctx::Observe& o = ctx->ob;
  // (with vsf_observe_set_debug_jpeg / _png the raw canvases never leave the device)
  const int slot = o.debug && !o.files.form.kind ? collected_slot(o, ticket) : -1;
  if (slot < 0) return VSF_ERR_INVALID_ARG;
  const uint32_t flags = reinterpret_cast<const uint32_t*>(o.h_out + (size_t)slot * o.out_stride)[14];
  const uint8_t* base = o.h_dbg + (size_t)slot * o.dbg_stride;
  if (flags & 1) *stereo = base;
  if (flags & 2) *match = base + (size_t)6 * ctx->p.width * ctx->p.height;
  return VSF_OK;
}

vsf_status vsf_observe_set_debug_jpeg(vsf_ctx* ctx, int quality) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || quality < 0 || quality > 100) return VSF_ERR_INVALID_ARG;
  return set_debug_form(ctx, VSF_FILE_JPEG, quality);
}

vsf_status vsf_observe_debug_jpeg_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** stereo, size_t* stereo_bytes,
                                       const uint8_t** match, size_t* match_bytes) {
  return debug_files_view(ctx, VSF_FILE_JPEG, ticket, stereo, stereo_bytes, match, match_bytes);
}

vsf_status vsf_observe_set_debug_png(vsf_ctx* ctx, int on) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx) return VSF_ERR_INVALID_ARG;
  return set_debug_form(ctx, VSF_FILE_PNG, on != 0);
}

vsf_status vsf_observe_debug_png_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** stereo, size_t* stereo_bytes,
                                      const uint8_t** match, size_t* match_bytes) {
  return debug_files_view(ctx, VSF_FILE_PNG, ticket, stereo, stereo_bytes, match, match_bytes);
}

vsf_status vsf_observe_configure(vsf_ctx* ctx, int depth, int min_batch, int in_flight) {
  VsfErrorScope scope_(ctx);  // (sends what waits; the launcher thread is idle afterwards)
  if (!ctx || depth < 0 || depth > 1024 || min_batch < 0 || in_flight < 0 || in_flight > vsf_ctx::kObserveBatchSlots - 1)
    return VSF_ERR_INVALID_ARG;
  if (frames_in_queue(ctx)) return VSF_ERR_INVALID_ARG;
  if (ctx->ob.ready && depth != ctx->ob_depth) {  // the queue is rebuilt by the next submit; the threshold and the window go
    const vsf_status st = drop_queue(ctx);
    if (st != VSF_OK) return st;
  }
  ctx->ob_depth = depth;
  ctx->ob_min_batch = min_batch;
  ctx->ob_in_flight = in_flight > 0 ? in_flight : 2;
  if (ctx->ob.ready) {  // (a queue that stays follows at once)
    std::lock_guard<std::mutex> g(ctx->ob.queue->mu);
    ctx->ob.queue->sizes.min_batch = ctx->ob_min_batch;
    ctx->ob.queue->sizes.in_flight = ctx->ob_in_flight;
  }
  return VSF_OK;
}

vsf_status vsf_observe_set_streams(vsf_ctx* ctx, int n_streams) {
  VsfErrorScope scope_(ctx);  // (sends what waits; the launcher thread is idle afterwards)
  if (!ctx || n_streams < 1 || n_streams > VSF_OBSERVE_MAX_STREAMS) return VSF_ERR_INVALID_ARG;
  // (the seeds are one per stream: another count needs vsf_observe_set_debug_seeds first, with debug images off)
  if (ctx->ob_seeded && n_streams != ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  if (n_streams > 1 && ctx->ob_debug && !ctx->ob_seeded) return VSF_ERR_UNSUPPORTED;  // (one stream without seeds)
  if (frames_in_queue(ctx)) return VSF_ERR_INVALID_ARG;
  if (ctx->ob.ready && n_streams != ctx->ob_streams) {  // rebuilt by the next submit: every window and threshold starts over
    const vsf_status st = drop_queue(ctx);
    if (st != VSF_OK) return st;
  }
  if (n_streams != ctx->ob_streams)  // (vsf_observe_set_stream_cam_to_robot: the streams are other cameras now)
    for (bool& set : ctx->ob_stream_c2r_set) set = false;
  if (n_streams != ctx->ob_streams)  // (vsf_observe_set_input_size: ... of other sizes)
    for (int s = 0; s < VSF_OBSERVE_MAX_STREAMS; s++) ctx->ob_in_w[s] = ctx->ob_in_h[s] = ctx->ob_bayer_order[s] = 0;
  ctx->ob_streams = n_streams;
  return VSF_OK;
}

vsf_status vsf_observe_set_debug_seeds(vsf_ctx* ctx, const uint32_t* seeds, int n) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || n < 0 || (n > 0 && !seeds) || (n == 0 && seeds)) return VSF_ERR_INVALID_ARG;
  if (n != 0 && n != ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  if (ctx->ob_debug) return VSF_ERR_INVALID_ARG;  // the order of use: streams, seeds, switch
  // (before the queue's first frame or after vsf_observe_reset; a queue built without debug images holds nothing of this)
  if (ctx->ob.ready && ctx->ob.queue->next_ticket != 0) return VSF_ERR_INVALID_ARG;
  ctx->ob_seeded = n != 0;
  for (int s = 0; s < n; s++) ctx->ob_seeds[s] = seeds[s];
  return VSF_OK;
}

vsf_status vsf_observe_set_stream_cam_to_robot(vsf_ctx* ctx, int stream, const float* m) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  ctx->ob_stream_c2r_set[stream] = m != nullptr;
  if (m) std::memcpy(ctx->ob_stream_c2r[stream], m, sizeof(ctx->ob_stream_c2r[stream]));
  return VSF_OK;
}

vsf_status vsf_observe_set_input_size(vsf_ctx* ctx, int stream, int width, int height) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  if (!(width == 0 && height == 0) && !vsf_resize_size_ok(width, height)) return VSF_ERR_INVALID_ARG;
  // (the rule of vsf_observe_reset_stream: no frame of the stream submitted and not collected)
  if (ctx->ob.ready && ctx->ob.streams[(size_t)stream].uncollected != 0) return VSF_ERR_INVALID_ARG;
  ctx->ob_in_w[stream] = width;
  ctx->ob_in_h[stream] = height;
  return VSF_OK;
}

vsf_status vsf_observe_set_bayer_order(vsf_ctx* ctx, int stream, int pixfmt) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || stream < 0 || stream >= ctx->ob_streams || !observe_pix_is_bayer(pixfmt)) return VSF_ERR_INVALID_ARG;
  // (the rule of vsf_observe_reset_stream: no frame of the stream submitted and not collected)
  if (ctx->ob.ready && ctx->ob.streams[(size_t)stream].uncollected != 0) return VSF_ERR_INVALID_ARG;
  ctx->ob_bayer_order[stream] = pixfmt;
  return VSF_OK;
}

vsf_status vsf_observe_reset_stream(vsf_ctx* ctx, int stream) {
  VsfErrorScope scope_(ctx);  // (sends what waits; the launcher thread is idle afterwards)
  if (!ctx || stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  vsf_ctx::Observe& o = ctx->ob;
  if (o.ready && o.streams[(size_t)stream].uncollected != 0) return VSF_ERR_INVALID_ARG;
  ctx->ob_pose[stream] = identity_pose();  // (vsf_observe_set_pose: captured by the frames already submitted, all collected)
  if (!o.ready) return VSF_OK;  // (nothing else to forget)
  vsf_ctx::ObserveStream& st = o.streams[(size_t)stream];
  VSF_HIP(hipSetDevice(ctx->device));
  // Every frame of the stream has been collected: no kernel reads or writes its threshold any more (other streams' tails
  // may be running: they touch their own).  Its window is forgotten by counting its frames from 0 again -- the next frame
  // has no predecessor, and the sets fill in the same order as a fresh queue's.
  const float thr = 10000.0f;  // cc:353
  VSF_HIP(hipMemcpy(tail_thr_state(o) + stream, &thr, sizeof(float), hipMemcpyHostToDevice));
  if (o.debug && o.seeded) {  // its kept frame goes, its generator is seeded again
    VSF_HIP(hipMemset(reinterpret_cast<int32_t*>(o.dbg_ints + 1) + stream, 0, sizeof(int32_t)));
    const vsf_status sr = upload_debug_generators(ctx, stream, 1);
    if (sr != VSF_OK) return sr;
  }
  st.frames = 0;
  st.last_ticket = -1;
  return VSF_OK;
}

vsf_status vsf_observe_stats(const vsf_ctx* ctx, int64_t* out, int n) {
  if (!ctx || !out || n < 1) return VSF_ERR_INVALID_ARG;
  const vsf_ctx::Observe& o = ctx->ob;
  // (the launcher thread may be inside a batch: its counters and buffer sizes are read once it is out, under the queue's lock)
  std::unique_lock<std::mutex> lk;
  if (o.queue) lk = o.queue->lock_idle();
  const ObserveLaunchStats s = o.queue ? o.queue->stats : ObserveLaunchStats();
  // every byte the compressed path owns: 0 until the first compressed frame
  size_t cmp_bytes = o.h_cmp ? vsf_observe_compressed_ring_bytes(o.depth, o.cmp_cap) : 0;
  const size_t mosaics = o.d_bayer ? mosaics_bytes(ctx) : 0;
  cmp_bytes += mosaics;
  for (const vsf_ctx::ObserveBatch& b : o.batch) cmp_bytes += 2 * b.blob.cap;
  cmp_bytes += o.ing_scratch.bytes();
  // every buffer a frame of a new format made the queue build or enlarge (they are the compressed and resize paths' too:
  // the mosaics' buffer and the big slots, counted in [13] and [28] as well)
  const size_t pix_bytes = o.pix_seen ? input_bytes(ctx) + mosaics : 0;
  const int64_t v[33] = {s.frames, s.batches, s.max_batch, s.solo, s.forced, s.slot_waits,
                         (int64_t)o.depth, (int64_t)o.bmax, o.stat_copy_ns, s.launch_ns, o.stat_wait_ns,
                         s.compressed, s.ingest_commands, (int64_t)cmp_bytes,
                         s.file_commands, (int64_t)ctx->ob_streams, s.multi,
                         s.device_frames, s.device_commands + o.stat_dev_commands,
                         (int64_t)(o.d_ring ? vsf_observe_device_ring_bytes(ctx, o.depth) : 0),
                         s.cloud_frames, s.cloud_commands,
                         (int64_t)(o.h_wp ? (size_t)o.depth * ((size_t)ctx->p.max_keypoints * 3 * sizeof(double) + sizeof(int32_t)) : 0),
                         s.reduced, s.seeded_frames, s.colour_commands,
                         s.resized, s.resize_commands, (int64_t)input_bytes(ctx), s.multi_size,
                         s.pix_frames, s.pix_commands, (int64_t)pix_bytes};
  for (int i = 0; i < n && i < 33; i++) out[i] = v[i];
  return VSF_OK;
}

vsf_status vsf_observe_reset(vsf_ctx* ctx) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx) return VSF_ERR_INVALID_ARG;
  for (vsf_pose& p : ctx->ob_pose) p = identity_pose();
  return drop_queue(ctx);
}

// What a frame takes from its stream when it is submitted, for the point cloud: the sticky pose (vsf_observe_set_pose) and, with
// the cloud on, the stream's own left_cam_to_robot (vsf_observe_set_stream_cam_to_robot) or the one the queue was built with.
static void capture_placement(const vsf_ctx* ctx, int stream, vsf_ctx::ObserveFrame& fr) {
  fr.pose = ctx->ob_pose[stream];
  // ... and, for the extraction, its detection masks: its stream's -- or, as the frame of a synchronous vsf_observe_stereo*
  // call, the ones vsf_set_image_masks names for the calls outside the queue (image 0 the left, image 1 the right)
  fr.mask_slot[0] = ctx->ob_sync_call ? ctx->mask_even : ctx->ob_masks[stream].left;
  fr.mask_slot[1] = ctx->ob_sync_call ? ctx->mask_odd : ctx->ob_masks[stream].right;
  if (ctx->ob.cloud)
    std::memcpy(fr.cam_to_robot, ctx->ob_stream_c2r_set[stream] ? ctx->ob_stream_c2r[stream] : ctx->ob.cam_to_robot,
                sizeof(fr.cam_to_robot));
}

// ---- what every submit does: the refusal of its arguments, the size its stream's frames arrive at, the queue opened for its
// frames, the colours drawn ahead, the booking of a frame ----
// (a, b: the call's two images, or its array of frames twice)
static bool submit_args_ok(const vsf_ctx* ctx, const void* a, const void* b, const vsf_calibration* calib, const int64_t* tickets,
                           float best_percent, int frame_life) {
  return ctx && a && b && calib && tickets && best_percent >= 0.f && frame_life >= 0 && frame_life + 1 <= VSF_OBSERVE_MAX_PAIRS;
}

// The stream's declared size (vsf_observe_set_input_size), or the context's.
struct StreamInput {
  bool declared;
  int w, h;
};
static StreamInput stream_input(const vsf_ctx* ctx, int stream) {
  const bool declared = ctx->ob_in_w[stream] != 0;
  return {declared, declared ? ctx->ob_in_w[stream] : ctx->p.width, declared ? ctx->ob_in_h[stream] : ctx->p.height};
}

// Whether a big-slot frame needs the conversion's other buffer (kInBayer; also the batches' own big slots): a mosaic's gray
// image always, packed colour's unless it arrives at the context's size -- then it goes straight into the batch's images.
static bool gray_slots(const vsf_ctx* ctx, int pixfmt, int w, int h) {
  return observe_pix_is_bayer(pixfmt) || (vsf_pixfmt_bytes_per_pixel(pixfmt) > 1 && (w != ctx->p.width || h != ctx->p.height));
}

// Opens the queue -- built by the first submit of any kind -- for n consecutive frames of `stream`: their slots in *span.  What
// waits and may not share a batch with them leaves first: a stream's frames of one batch share one calibration and one
// best_percent, a batch's frames their pixel format, so frames that bring others than the waiting frame of THEIR stream in
// front of them send what waits.
static vsf_status open_queue(vsf_ctx* ctx, int stream, int pixfmt, const vsf_calibration* calib, float best_percent,
                             int frame_life, int n, ObserveSpan* span) {
  vsf_ctx::Observe& o = ctx->ob;
  if (o.ready && o.frame_life != frame_life) {  // (re-sizing the window drops nothing that is still in the queue)
    if (frames_in_queue(ctx)) return VSF_ERR_INVALID_ARG;
    stop_observe_threads(ctx);
  }
  const vsf_status st = ensure_observe(ctx, frame_life);
  if (st != VSF_OK) return st;
  ObserveQueue& q = *o.queue;
  // (next_ticket and next_collect are the caller's own: nobody else writes them; no room: collect the oldest frame first;
  // span == nullptr: ONE frame, whose slot is next_ticket % depth)
  if (span ? !observe_submit_span(q.next_ticket, q.next_collect, o.depth, n, span) : q.next_ticket - q.next_collect >= o.depth)
    return VSF_ERR_INVALID_ARG;
  std::unique_lock<std::mutex> lk(q.mu);
  if (q.status != VSF_OK) return q.status;
  if (q.next_launch >= q.next_ticket) return VSF_OK;  // (nothing waits)
  bool cut = o.frames[(size_t)((q.next_ticket - 1) % o.depth)].pixfmt != pixfmt;
  const int64_t mine = o.streams[(size_t)stream].last_ticket;
  if (!cut && mine >= q.next_launch) {
    const vsf_ctx::ObserveFrame& w0 = o.frames[(size_t)(mine % o.depth)];
    cut = observe_plan_must_cut(w0.calib, w0.best_percent, *calib, best_percent);
  }
  return cut ? q.caller_pump(lk, true) : VSF_OK;
}

// The stereo lines' colours, cv::Scalar(rand() % 255, rand() % 255, rand() % 255) (cc:95) in the reference's order -- GCC
// evaluates the three calls right to left: the first is channel 2 -- drawn ahead for the call's n frames: enough for every
// frame in the queue (a frame takes at most max_keypoints); the device takes them in frame order from its cursor.
static void draw_colours_ahead(vsf_ctx* ctx, int n) {
  vsf_ctx::Observe& o = ctx->ob;
  if (!o.debug || o.seeded) return;
  const ObserveQueue& q = *o.queue;
  const int64_t K = ctx->p.max_keypoints, want = o.col_retired + (q.next_ticket + n - q.next_collect) * K;
  for (; o.col_generated < want; o.col_generated++) {
    const uint32_t c2 = (uint32_t)(rand() % 255), c1 = (uint32_t)(rand() % 255), c0 = (uint32_t)(rand() % 255);
    o.h_col[o.col_generated % o.col_ring] = c0 | (c1 << 8) | (c2 << 16);
  }
}

// Books the frame of the queue's next ticket in `slot`: its record, its stream's counters, the ticket.  fr: what the submits'
// frames differ in -- where the two images are (kind, nbytes, reduce, dev_*) and what they are (pixfmt, pix_new, in_w x in_h;
// 0 x 0: an own-size frame, and all a queue that has seen no big-slot frame ever writes).
static vsf_status book_frame(vsf_ctx* ctx, int slot, int stream, vsf_ctx::ObserveFrame fr, const vsf_calibration* calib,
                             float best_percent, int64_t* ticket) {
  vsf_ctx::Observe& o = ctx->ob;
  vsf_ctx::ObserveStream& mine = o.streams[(size_t)stream];
  fr.calib = *calib;
  fr.best_percent = best_percent;
  capture_placement(ctx, stream, fr);
  fr.batch = -1;
  fr.stream = stream;
  fr.k = mine.frames++;
  mine.uncollected++;
  mine.last_ticket = o.queue->next_ticket;
  o.pix_seen |= fr.pix_new;
  o.frames[(size_t)slot] = fr;
  return o.queue->submit(ticket);
}

// The host submits.  kinds == nullptr: raw images of w x h at `stride`; else left / right are files of nbytes[0 / 1] bytes that
// have passed vsf_observe_probe_compressed_reduced as kinds[0 / 1] at 1 / reduce.
static vsf_status observe_submit(vsf_ctx* ctx, int stream, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride,
                                 const int* kinds, const size_t* nbytes, int pixfmt, const vsf_calibration* calib,
                                 float best_percent, int frame_life, int64_t* ticket, int reduce = 1, bool pix_call = false) {
  const bool bayer = observe_pix_is_bayer(pixfmt);
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (ctx->p.max_keypoints >= 65536) return VSF_ERR_UNSUPPORTED;
  if (stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  if (calib->triangulate_rows != 0 && calib->triangulate_rows != 4 && calib->triangulate_rows != 6)
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  vsf_ctx::Observe& o = ctx->ob;
  vsf_status st = open_queue(ctx, stream, pixfmt, calib, best_percent, frame_life, 1, nullptr);
  if (st != VSF_OK) return st;
  const ObserveQueue& q = *o.queue;
  const int slot = (int)(q.next_ticket % o.depth);
  draw_colours_ahead(ctx, 1);
  // (w x h is the stream's declared size then: the callers have checked; packed colour waits in the big slots whatever its size)
  const bool resized = ctx->ob_in_w[stream] != 0 || bpp > 1;
  if (resized) {
    if (bayer && w > 16384) return VSF_ERR_UNSUPPORTED;  // (the demosaic's limit)
    st = ensure_input(ctx, (kinds ? kInBatch : kInHostRing | kInBatch) | (gray_slots(ctx, pixfmt, w, h) ? kInBayer : 0),
                      bpp > 1 ? observe_pix_image_bytes(w, h, bpp) : 0);
    if (st != VSF_OK) return st;
  }
  const int64_t t_copy = now_ns();
  if (kinds) {
    // ---- the two files into the frame's slots of the compressed ring (built by the first such frame) ----
    st = ensure_compressed(ctx);
    if (st != VSF_OK) return st;
  }
  // (own-size mosaics go through the mosaics' buffer on their way in; a stream of compressed mosaics keeps one whatever its size)
  if (bayer && (kinds || !resized)) {
    st = ensure_mosaics(ctx);
    if (st != VSF_OK) return st;
  }
  if (kinds) {
    if (o.cmp_cap != compressed_cap(ctx) || nbytes[0] > o.cmp_cap || nbytes[1] > o.cmp_cap) return VSF_ERR_CAPACITY;
    uint8_t* h_cmp = o.h_cmp + (size_t)slot * 2 * o.cmp_slot;
    std::memcpy(h_cmp, left, nbytes[0]);
    std::memcpy(h_cmp + o.cmp_slot, right, nbytes[1]);
  } else {
    // ---- the two images into the frame's slot of the pinned staging ring, rows at the device pitch (the slot's previous
    // frame has been collected: its upload is long done); a big-slot frame: into its slot of the pinned ring of such slots,
    // rows at ITS width's pitch ----
    uint8_t* h_img = resized ? o.h_in + (size_t)slot * 2 * o.in_half : o.h_img + (size_t)slot * 2 * ctx->st_img_stride;
    const size_t h_stride = resized ? o.in_half : ctx->st_img_stride, h_pitch = resized ? observe_pix_pitch(w, bpp) : ctx->st_img_pitch;
    const size_t row = (size_t)w * (size_t)bpp;  // bytes
    const ObserveCopyHelper::Job jr{h_img + h_stride, right, h_pitch, stride, row, h};
    // frames are streaming in (the previous one is still in the queue): the helper thread takes the right image
    const bool helped = o.copy_helper && q.next_ticket > q.next_collect && o.copy_helper->post(jr);
    stage_image(h_img, h_pitch, left, stride, row, h);
    if (helped)
      o.copy_helper->wait();
    else
      stage_image(jr.dst, jr.dst_pitch, jr.src, jr.src_pitch, jr.width, jr.rows);
  }
  o.stat_copy_ns += now_ns() - t_copy;
  vsf_ctx::ObserveFrame fr{};
  for (int k = 0; k < 2; k++) {
    fr.kind[k] = kinds ? (uint8_t)kinds[k] : 0;
    fr.nbytes[k] = kinds ? (uint32_t)nbytes[k] : 0u;
  }
  fr.reduce = (uint8_t)reduce;
  fr.pixfmt = pixfmt;
  fr.pix_new = pix_call ? pixfmt != VSF_PIX_MONO8 : pixfmt >= VSF_PIX_BAYER_GRBG8;
  fr.in_w = resized ? w : 0;
  fr.in_h = resized ? h : 0;
  return book_frame(ctx, slot, stream, fr, calib, best_percent, ticket);
}

vsf_status vsf_observe_submit(vsf_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride,
                              const vsf_calibration* calib, float best_percent, int frame_life, int64_t* ticket) {
  return vsf_observe_submit_stream(ctx, 0, left, right, w, h, stride, calib, best_percent, frame_life, ticket);
}

vsf_status vsf_observe_submit_stream(vsf_ctx* ctx, int stream, const uint8_t* left, const uint8_t* right, int w, int h,
                                     size_t stride, const vsf_calibration* calib, float best_percent, int frame_life,
                                     int64_t* ticket) {
  VsfErrorScope scope_(ctx, false);
  if (!submit_args_ok(ctx, left, right, calib, ticket, best_percent, frame_life)) return VSF_ERR_INVALID_ARG;
  *ticket = -1;
  if (stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  const StreamInput in = stream_input(ctx, stream);
  if (w != in.w || h != in.h || stride < (size_t)w || ctx->p.max_images < 2) return VSF_ERR_INVALID_ARG;
  return observe_submit(ctx, stream, left, right, w, h, stride, nullptr, nullptr, VSF_PIX_MONO8, calib, best_percent, frame_life, ticket);
}

// Raw host frames of any pixel format.  MONO8 is the call above, byte for byte and launch for launch.
vsf_status vsf_observe_submit_stream_pix(vsf_ctx* ctx, int stream, const uint8_t* left, const uint8_t* right, int w, int h,
                                         size_t stride_bytes, int pixfmt, const vsf_calibration* calib, float best_percent,
                                         int frame_life, int64_t* ticket) {
  VsfErrorScope scope_(ctx, false);
  if (!submit_args_ok(ctx, left, right, calib, ticket, best_percent, frame_life)) return VSF_ERR_INVALID_ARG;
  *ticket = -1;
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (bpp == 0 || stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  const StreamInput in = stream_input(ctx, stream);
  if (w != in.w || h != in.h || stride_bytes < (size_t)w * (size_t)bpp || ctx->p.max_images < 2) return VSF_ERR_INVALID_ARG;
  if (observe_pix_is_bayer(pixfmt) && w > 16384) return VSF_ERR_UNSUPPORTED;  // (the demosaic's limit)
  if (bpp > 1 && observe_pix_image_bytes(w, h, bpp) == 0) return VSF_ERR_UNSUPPORTED;  // (2^31 bytes or more an image)
  return observe_submit(ctx, stream, left, right, w, h, stride_bytes, nullptr, nullptr, pixfmt, calib, best_percent, frame_life,
                        ticket, 1, true);
}

vsf_status vsf_observe_submit_compressed(vsf_ctx* ctx, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                         size_t right_bytes, int bayer, const vsf_calibration* calib, float best_percent,
                                         int frame_life, int64_t* ticket) {
  return vsf_observe_submit_compressed_stream(ctx, 0, left, left_bytes, right, right_bytes, bayer, calib, best_percent,
                                              frame_life, ticket);
}

// Both compressed submits: the decoders' host half at 1 / reduce for the two files, then the frame's booking.
static vsf_status observe_submit_files(vsf_ctx* ctx, int stream, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                       size_t right_bytes, int bayer, int reduce, const vsf_calibration* calib,
                                       float best_percent, int frame_life, int64_t* ticket);

vsf_status vsf_observe_submit_compressed_stream(vsf_ctx* ctx, int stream, const uint8_t* left, size_t left_bytes,
                                                const uint8_t* right, size_t right_bytes, int bayer,
                                                const vsf_calibration* calib, float best_percent, int frame_life,
                                                int64_t* ticket) {
  return observe_submit_files(ctx, stream, left, left_bytes, right, right_bytes, bayer, 1, calib, best_percent, frame_life, ticket);
}

// IMREAD_REDUCED_GRAYSCALE_<reduce> frames.  No `bayer`: a mosaic cannot be reduced in the DCT domain.
vsf_status vsf_observe_submit_compressed_reduced(vsf_ctx* ctx, int stream, const uint8_t* left, size_t left_bytes,
                                                 const uint8_t* right, size_t right_bytes, int reduce,
                                                 const vsf_calibration* calib, float best_percent, int frame_life,
                                                 int64_t* ticket) {
  if (ticket) *ticket = -1;
  if (!vsf_reduce_ok(reduce)) return VSF_ERR_INVALID_ARG;
  return observe_submit_files(ctx, stream, left, left_bytes, right, right_bytes, 0, reduce, calib, best_percent, frame_life, ticket);
}

static vsf_status observe_submit_files(vsf_ctx* ctx, int stream, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                       size_t right_bytes, int bayer, int reduce, const vsf_calibration* calib,
                                       float best_percent, int frame_life, int64_t* ticket) {
  VsfErrorScope scope_(ctx, false);
  if (!submit_args_ok(ctx, left, right, calib, ticket, best_percent, frame_life)) return VSF_ERR_INVALID_ARG;
  *ticket = -1;
  if (ctx->p.max_images < 2 || stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  // the decoders' host half, file by file: a refused file books nothing and leaves the queue as it was
  // a stream with a declared size (vsf_observe_set_input_size): the FILE's size must be that one -- it is decoded whole and
  // resized, cv::resize(DecodeImage(msg)); a reduced decode on top of that is not built
  const StreamInput in = stream_input(ctx, stream);
  if (in.declared && reduce != 1) return VSF_ERR_INVALID_ARG;
  const int w = in.w, h = in.h;
  const size_t cap = compressed_cap(ctx);
  const size_t nbytes[2] = {left_bytes, right_bytes};
  int kinds[2] = {0, 0};
  vsf_status st = vsf_observe_probe_compressed_reduced(left, left_bytes, reduce, w, h, cap, ctx->tuning.jpeg_serial, &kinds[0]);
  if (st == VSF_OK)
    st = vsf_observe_probe_compressed_reduced(right, right_bytes, reduce, w, h, cap, ctx->tuning.jpeg_serial, &kinds[1]);
  if (st != VSF_OK) return st;
  // (`bayer`: the order vsf_observe_set_bayer_order named for this stream, RGGB for a stream never told)
  const int order = ctx->ob_bayer_order[stream] ? ctx->ob_bayer_order[stream] : VSF_PIX_BAYER_RGGB8;
  return observe_submit(ctx, stream, left, right, w, h, 0, kinds, nbytes, bayer != 0 ? order : VSF_PIX_MONO8, calib, best_percent,
                        frame_life, ticket, reduce);
}

size_t vsf_observe_device_ring_bytes(const vsf_ctx* ctx, int depth) {
  if (!ctx || depth < 0 || depth > 1024) return 0;
  if (depth == 0) depth = ctx->ob_depth > 0 ? ctx->ob_depth : std::max(1, ctx->p.max_images / 2);
  return (size_t)depth * 2 * ctx->st_img_stride;
}

// Frames that are in device memory already.  The order of things: every refusal; the queue (built by the first submit of any
// kind); what waits and may not share a batch with these frames leaves; the ring; ONE launch on the producer's stream and
// the event behind it; only then the frames' records and their tickets, one by one -- a batch may leave between two of them,
// and takes the frames that have theirs.
vsf_status vsf_observe_submit_dev(vsf_ctx* ctx, int stream, const vsf_dev_frame* frames, int n, int pixfmt, void* producer_stream,
                                  const vsf_calibration* calib, float best_percent, int frame_life, int64_t* tickets) {
  VsfErrorScope scope_(ctx, false);
  if (!submit_args_ok(ctx, frames, frames, calib, tickets, best_percent, frame_life) || n < 1) return VSF_ERR_INVALID_ARG;
  for (int i = 0; i < n; i++) tickets[i] = -1;
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (bpp == 0) return VSF_ERR_INVALID_ARG;  // (2 .. 15 included)
  if (ctx->p.max_images < 2 || n > 1024) return VSF_ERR_INVALID_ARG;
  if (stream < 0 || stream >= ctx->ob_streams) return VSF_ERR_INVALID_ARG;
  const StreamInput in = stream_input(ctx, stream);
  const bool resized = in.declared || bpp > 1;  // (packed colour waits in the ring of big slots whatever its size)
  const size_t w = (size_t)in.w * (size_t)bpp;  // a row's bytes
  for (int i = 0; i < n; i++)
    if (!frames[i].left || !frames[i].right || frames[i].left_pitch < w || frames[i].right_pitch < w) return VSF_ERR_INVALID_ARG;
  if (ctx->p.max_keypoints >= 65536) return VSF_ERR_UNSUPPORTED;
  const bool bayer = observe_pix_is_bayer(pixfmt);
  if (resized && bayer && in.w > 16384) return VSF_ERR_UNSUPPORTED;  // (the demosaic's limit)
  if (bpp > 1 && observe_pix_image_bytes(in.w, in.h, bpp) == 0) return VSF_ERR_UNSUPPORTED;  // (2^31 bytes or more an image)
  if (calib->triangulate_rows != 0 && calib->triangulate_rows != 4 && calib->triangulate_rows != 6) return VSF_ERR_INVALID_ARG;
  hipStream_t producer = static_cast<hipStream_t>(producer_stream);
  VSF_HIP(hipSetDevice(ctx->device));
  vsf_ctx::Observe& o = ctx->ob;
  ObserveSpan span;  // (the cut rule once: the call's frames share everything it looks at)
  vsf_status st = open_queue(ctx, stream, pixfmt, calib, best_percent, frame_life, n, &span);
  if (st != VSF_OK) return st;
  st = ensure_device_ring(ctx, resized);
  if (st == VSF_OK && bayer && !resized) st = ensure_mosaics(ctx);
  if (st == VSF_OK && resized)
    st = ensure_input(ctx, kInDeviceRing | (gray_slots(ctx, pixfmt, in.w, in.h) ? kInBayer : 0),
                      bpp > 1 ? observe_pix_image_bytes(in.w, in.h, bpp) : 0);
  if (st != VSF_OK) return st;
  draw_colours_ahead(ctx, n);
  // ---- ONE launch on the producer's stream: the 2 n images into the frames' slots of the ring (the slots' previous frames
  // have been collected: the copies out of them are long done), and the event the batch's copy stream will wait for ----
  const int64_t t_copy = now_ns();
  VsfIngestSrc inl[VSF_INGEST_INLINE];
  const bool by_table = 2 * n > VSF_INGEST_INLINE;
  for (int i = 0; i < n; i++) {
    const int slot = (span.slot0 + i) % o.depth;
    VsfIngestSrc* e = by_table ? o.h_dev_src + 2 * (size_t)slot : inl + 2 * i;
    e[0] = {static_cast<const uint8_t*>(frames[i].left), frames[i].left_pitch};
    e[1] = {static_cast<const uint8_t*>(frames[i].right), frames[i].right_pitch};
  }
  if (resized)  // (into the ring of big slots, rows at the declared width's pitch: k_resize.hip reads them there)
    vsf_launch_ingest_ring(o.d_in_ring, o.in_half, (int)observe_pix_pitch(in.w, bpp), in.w * bpp, in.h, span.slot0, o.depth, n, inl,
                           by_table ? o.h_dev_src.get() : nullptr, producer);
  else
    vsf_launch_ingest_ring(o.d_ring, ctx->st_img_stride, (int)ctx->st_img_pitch, ctx->p.width, ctx->p.height, span.slot0, o.depth, n,
                           inl, by_table ? o.h_dev_src.get() : nullptr, producer);
  const int ev_slot = (span.slot0 + n - 1) % o.depth;
  VSF_HIP(hipEventRecord(o.dev_ev[(size_t)ev_slot], producer));
  VSF_STICKY();
  o.stat_dev_commands++;
  o.stat_copy_ns += now_ns() - t_copy;
  vsf_ctx::ObserveFrame fr{};
  fr.kind[0] = fr.kind[1] = kObserveKindDevice;
  fr.pixfmt = pixfmt;
  fr.pix_new = pixfmt >= VSF_PIX_BAYER_GRBG8;
  fr.in_w = resized ? in.w : 0;
  fr.in_h = resized ? in.h : 0;
  fr.dev_event = ev_slot;
  fr.dev_stream = producer;
  for (int i = 0; i < n; i++) {
    st = book_frame(ctx, (span.slot0 + i) % o.depth, stream, fr, calib, best_percent, &tickets[i]);
    if (st != VSF_OK) return st;
  }
  return VSF_OK;
}

vsf_status vsf_observe_set_compressed_cap(vsf_ctx* ctx, size_t cap_per_image) {
  VsfErrorScope scope_(ctx);  // (sends what waits; the launcher thread is idle afterwards)
  if (!ctx || (cap_per_image != 0 && vsf_observe_compressed_slot_bytes(cap_per_image) == 0)) return VSF_ERR_INVALID_ARG;
  vsf_ctx::Observe& o = ctx->ob;
  if (frames_in_queue(ctx)) return VSF_ERR_INVALID_ARG;
  if (o.h_cmp) {  // (every frame has been collected: no upload reads the ring; a pinned buffer is retired, not freed)
    ctx->retired_host.emplace_back(o.h_cmp.release());
    o.cmp_cap = o.cmp_slot = 0;
  }
  ctx->ob_cmp_cap = cap_per_image;
  return VSF_OK;
}

// Waits for the frame of `ticket` and points at its result inside the pinned result ring (valid until `depth` further
// frames have been submitted).
static vsf_status observe_wait(vsf_ctx* ctx, int64_t ticket, const uint8_t** view, size_t* bytes) {
  vsf_ctx::Observe& o = ctx->ob;
  *bytes = 0;
  // frames leave in the order they entered (the host's bookkeeping is sequential)
  if (!o.ready || ticket < 0 || ticket != o.queue->next_collect || ticket >= o.queue->next_ticket) return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  const int slot = (int)(ticket % o.depth);
  vsf_status st = o.queue->release(ticket);  // (if it still waits in staging, everything that waits leaves now)
  if (st != VSF_OK) return st;
  const vsf_ctx::ObserveBatch& b = o.batch[o.frames[(size_t)slot].batch];
  {
    const int64_t t_wait = now_ns();
    VSF_HIP(hipEventSynchronize(b.ev_done));
    o.stat_wait_ns += now_ns() - t_wait;
  }
  const uint8_t* res = o.h_out + (size_t)slot * o.out_stride;
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(res);
  const bool whole = hdr[0] == 0x4F465356u;
  o.streams[(size_t)o.frames[(size_t)slot].stream].uncollected--;
  if (o.debug && !o.seeded) o.col_retired += hdr[15];  // the colours this frame's stereo image took
  st = o.queue->collected(ticket, whole ? (int)hdr[2] : -1);  // (hdr[2]: the filtered frame's rows)
  if (!whole) return VSF_ERR_HIP;
  const_cast<uint32_t*>(hdr)[0] = 0;  // (the slot's next frame must write its own)
  *view = res;
  *bytes = hdr[3];
  if (st != VSF_OK) return st;
  if (hdr[11] != 0) return VSF_ERR_CAPACITY;  // the result does not fit its slot
  if (hdr[13] != 0) return VSF_ERR_INVALID_ARG;  // a file of this frame was refused on the device (extracted as zeros)
  return hdr[12] != 0 ? VSF_ERR_CAPACITY : VSF_OK;
}

vsf_status vsf_observe_poll(vsf_ctx* ctx, int64_t ticket, int* ready) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || !ready) return VSF_ERR_INVALID_ARG;
  *ready = 0;
  vsf_ctx::Observe& o = ctx->ob;
  if (!o.ready || ticket < o.queue->next_collect || ticket >= o.queue->next_ticket) return VSF_ERR_INVALID_ARG;
  const vsf_ctx::ObserveBatch* b = nullptr;
  {
    std::lock_guard<std::mutex> g(o.queue->mu);
    if (ticket >= o.queue->next_launch) return o.queue->status;  // it still waits in staging (nothing is forced)
    b = &o.batch[o.frames[(size_t)(ticket % o.depth)].batch];
  }
  VSF_HIP(hipSetDevice(ctx->device));
  const hipError_t e = hipEventQuery(b->ev_done);
  if (e == hipSuccess)
    *ready = 1;
  else if (e != hipErrorNotReady) {
    ctx->last_hip = (int)e;
    return VSF_ERR_HIP;
  }
  (void)hipGetLastError();
  return VSF_OK;
}

vsf_status vsf_observe_collect(vsf_ctx* ctx, int64_t ticket, uint8_t* out, size_t cap, size_t* out_bytes) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || !out || !out_bytes) return VSF_ERR_INVALID_ARG;
  const uint8_t* view = nullptr;
  const vsf_status st = observe_wait(ctx, ticket, &view, out_bytes);
  if (!view) return st;
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(view);
  if (hdr[11] != 0 || *out_bytes > cap) return VSF_ERR_CAPACITY;
  std::memcpy(out, view, *out_bytes);
  reinterpret_cast<uint32_t*>(out)[0] = 0x4F465356u;
  return st;
}

vsf_status vsf_observe_collect_view(vsf_ctx* ctx, int64_t ticket, const uint8_t** out, size_t* out_bytes) {
  VsfErrorScope scope_(ctx, false);
  if (!ctx || !out || !out_bytes) return VSF_ERR_INVALID_ARG;
  *out = nullptr;
  return observe_wait(ctx, ticket, out, out_bytes);
}

}  // extern "C"

// The synchronous calls: a submit and the collect of its ticket -- a batch of one.
template <class Submit>
static vsf_status stereo_call(vsf_ctx* ctx, uint8_t* out, size_t cap, size_t* out_bytes, Submit submit) {
  VsfErrorScope scope_(ctx, false);
  if (!out || !out_bytes) return VSF_ERR_INVALID_ARG;
  *out_bytes = 0;
  int64_t ticket = -1;
  struct SyncScope {  // (capture_placement: the frame this call submits takes vsf_set_image_masks' slots; every way out clears it)
    vsf_ctx* c;
    explicit SyncScope(vsf_ctx* ctx) : c(ctx) {
      if (c) c->ob_sync_call = true;
    }
    ~SyncScope() {
      if (c) c->ob_sync_call = false;
    }
  };
  vsf_status st;
  {
    SyncScope sync(ctx);
    st = submit(&ticket);
  }
  if (st != VSF_OK) return st;
  return vsf_observe_collect(ctx, ticket, out, cap, out_bytes);
}

extern "C" {

vsf_status vsf_observe_stereo(vsf_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride,
                              const vsf_calibration* calib, float best_percent, int frame_life, uint8_t* out,
                              size_t cap, size_t* out_bytes) {
  return stereo_call(ctx, out, cap, out_bytes, [&](int64_t* t) {
    return vsf_observe_submit(ctx, left, right, w, h, stride, calib, best_percent, frame_life, t);
  });
}

vsf_status vsf_observe_stereo_compressed(vsf_ctx* ctx, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                         size_t right_bytes, int bayer, const vsf_calibration* calib, float best_percent,
                                         int frame_life, uint8_t* out, size_t cap, size_t* out_bytes) {
  return stereo_call(ctx, out, cap, out_bytes, [&](int64_t* t) {
    return vsf_observe_submit_compressed(ctx, left, left_bytes, right, right_bytes, bayer, calib, best_percent, frame_life, t);
  });
}

vsf_status vsf_observe_stereo_compressed_reduced(vsf_ctx* ctx, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                                 size_t right_bytes, int reduce, const vsf_calibration* calib,
                                                 float best_percent, int frame_life, uint8_t* out, size_t cap,
                                                 size_t* out_bytes) {
  return stereo_call(ctx, out, cap, out_bytes, [&](int64_t* t) {
    return vsf_observe_submit_compressed_reduced(ctx, 0, left, left_bytes, right, right_bytes, reduce, calib, best_percent,
                                                 frame_life, t);
  });
}

}  // extern "C"
