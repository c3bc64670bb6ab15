// vsf_observe_ingest.hip -- the ingest of the ObserveImage queue (vsf_observe.hip): how the images of a batch's frames -- raw
// host frames, JPEG / PNG files, frames in device memory; mono, Bayer mosaics, packed colour; of the context's size or of a
// declared one -- get into the batch's own buffer b.d_img on the copy stream, and the buffers they wait in until then.
// What a batch's frames are and which commands that takes is plain C++ (vsf_observe_plan.cc observe_ingest_plan, run on the
// CPU by tests/cpp/test_observe_ingest_plan.cc); ingest() executes that plan and decides nothing again.  Every
// vsf_observe_stats counter of the ingest is incremented here, next to the command it counts.
#include <algorithm>
#include <mutex>
#include <vector>

#include "vsf_ctx.h"

namespace vsfi {

// ONE derivation, for the submit's probe and for the ring (vsf_observe_set_compressed_cap retires a ring built for another
// cap, so a ring that exists was built for this value).
size_t compressed_cap(const vsf_ctx* ctx) {
  return ctx->ob_cmp_cap ? ctx->ob_cmp_cap : vsf_observe_default_compressed_cap(ctx->p.width, ctx->p.height);
}

// The pinned ring the compressed files wait in: built by the first compressed submit.
vsf_status ensure_compressed(vsf_ctx* ctx) {
  vsf_ctx::Observe& o = ctx->ob;
  if (o.h_cmp) return VSF_OK;
  const size_t cap = compressed_cap(ctx);
  const size_t ring = vsf_observe_compressed_ring_bytes(o.depth, cap);
  if (ring == 0) return VSF_ERR_INVALID_ARG;
  VSF_HIP(o.h_cmp.alloc(ring, hipHostMallocDefault));
  o.cmp_cap = cap;
  o.cmp_slot = vsf_observe_compressed_slot_bytes(cap);
  return VSF_OK;
}

// The mosaics of an own-size Bayer batch -- raw host mosaics' upload, the decoders' output, the device ring's copies -- in the
// layout of the batch's images: its ONE demosaic reads them here.
size_t mosaics_bytes(const vsf_ctx* ctx) {
  const vsf_ctx::Observe& o = ctx->ob;
  return 2 * (size_t)o.bmax * ctx->st_img_stride;
}

vsf_status ensure_mosaics(vsf_ctx* ctx) {
  vsf_ctx::Observe& o = ctx->ob;
  if (!o.d_bayer) VSF_HIP(o.d_bayer.alloc(mosaics_bytes(ctx)));
  return VSF_OK;
}

// The events of device frames and the table of their sources; !big_slots: the device ring as well (frames in big slots wait
// in the ring of such slots, ensure_input).  Built by the first device frame (vsf_observe_device_ring_bytes says what it costs).
vsf_status ensure_device_ring(vsf_ctx* ctx, bool big_slots) {
  vsf_ctx::Observe& o = ctx->ob;
  if (o.dev_ev.empty()) {
    std::vector<Event> ev((size_t)o.depth);
    for (Event& e : ev) VSF_HIP(e.alloc(hipEventDisableTiming));
    VSF_HIP(o.h_dev_src.alloc((size_t)o.depth * 2 * sizeof(VsfIngestSrc), hipHostMallocMapped));
    o.dev_ev = std::move(ev);
  }
  if (big_slots || o.d_ring) return VSF_OK;
  const size_t bytes = vsf_observe_device_ring_bytes(ctx, o.depth);
  if (bytes == 0) return VSF_ERR_INVALID_ARG;
  VSF_HIP(o.d_ring.alloc(bytes));
  return VSF_OK;
}

// ---- the buffers of big slots (vsf_observe_plan.h), each built by the first frame that needs it: the pinned ring raw host
// frames wait in, the device ring, the batches' own big slots (a raw frame's upload, a compressed frame's decoded image), the
// mosaics (or the gray images of packed colour) of a batch ----
// need: bytes the arriving frame's image takes where that is more than every declared size's (a packed-colour frame,
// observe_pix_image_bytes: its rows are w * bpp bytes); the first frame that needs more room rebuilds, as a larger declared size does
vsf_status ensure_input(vsf_ctx* ctx, int what, size_t need) {
  vsf_ctx::Observe& o = ctx->ob;
  const size_t half = std::max(observe_input_half_bytes(ctx->ob_in_w, ctx->ob_in_h, ctx->ob_streams), need);
  if (half == 0) return VSF_ERR_INVALID_ARG;
  if (o.in_half != 0 && half > o.in_half) {
    // A larger size has been declared since these were built, and frames of other streams may wait in them or be on their
    // way out of them: what waits leaves, what left finishes, then they go (rare, and the one place the resize path waits).
    ObserveQueue& q = *o.queue;
    {
      std::unique_lock<std::mutex> lk(q.mu);
      if (q.status != VSF_OK) return q.status;
      if (q.next_launch < q.next_ticket) {
        const vsf_status st = q.caller_pump(lk, true);
        if (st != VSF_OK) return st;
      }
    }
    VSF_HIP(hipDeviceSynchronize());
    if (o.h_in) ctx->retired_host.emplace_back(o.h_in.release());
    o.d_in_ring = DevBuf<uint8_t>();
    o.d_bayer_in = DevBuf<uint8_t>();
    for (vsf_ctx::ObserveBatch& b : o.batch) b.d_in = DevBuf<uint8_t>();
  }
  o.in_half = std::max(o.in_half, half);
  const size_t slot = 2 * o.in_half;
  if ((what & kInHostRing) && !o.h_in) VSF_HIP(o.h_in.alloc((size_t)o.depth * slot, hipHostMallocDefault));
  if ((what & kInDeviceRing) && !o.d_in_ring) VSF_HIP(o.d_in_ring.alloc((size_t)o.depth * slot));
  if ((what & kInBayer) && !o.d_bayer_in) VSF_HIP(o.d_bayer_in.alloc((size_t)o.bmax * slot));
  if (what & (kInBatch | kInBayer))
    for (vsf_ctx::ObserveBatch& b : o.batch)
      if (!b.d_in) VSF_HIP(b.d_in.alloc((size_t)o.bmax * slot));
  return VSF_OK;
}

size_t input_bytes(const vsf_ctx* ctx) {
  const vsf_ctx::Observe& o = ctx->ob;
  const size_t slot = 2 * o.in_half;
  size_t bytes = (o.h_in ? (size_t)o.depth * slot : 0) + (o.d_in_ring ? (size_t)o.depth * slot : 0) +
                 (o.d_bayer_in ? (size_t)o.bmax * slot : 0);
  for (const vsf_ctx::ObserveBatch& b : o.batch) bytes += (b.d_in ? (size_t)o.bmax * slot : 0) + 2 * b.blob_in.cap;
  return bytes;
}

}  // namespace vsfi

using namespace vsfi;

namespace {

// The batch's 2 n images as decode_runs (vsf_ingest.hip) takes them: where their files lie in the ring of files and how long
// they are; every kind VSF_FILE_NONE (not a file: its image is left alone) until a decode names the frames it takes.
void batch_files(vsf_ctx::Observe& o, int64_t t0, int n) {
  o.dec_files.resize((size_t)(2 * n));
  o.dec_sizes.resize((size_t)(2 * n));
  o.dec_reduces.resize((size_t)(2 * n));
  o.dec_kinds.assign((size_t)(2 * n), (uint8_t)VSF_FILE_NONE);
  for (int i = 0; i < 2 * n; i++) {
    const int slot = (int)((t0 + i / 2) % o.depth);
    const vsf_ctx::ObserveFrame& fr = o.frames[(size_t)slot];
    o.dec_files[(size_t)i] = o.h_cmp + ((size_t)slot * 2 + (size_t)(i & 1)) * o.cmp_slot;
    o.dec_sizes[(size_t)i] = fr.nbytes[i & 1];
    o.dec_reduces[(size_t)i] = fr.reduce;
  }
}

// Own-size files: the batch's 2 n images go through decode_runs on `s` -- ONE upload for every run of one format among them, a
// status word per image (b.status: damage lands on its own image) -- into `dst`, the batch's images or the mosaics' buffer.
// (every file passed the decoders' host half at its submit; b.blob is free: the slot's previous batch has left the GPU)
vsf_status decode_own_files(vsf_ctx* ctx, vsf_ctx::ObserveBatch& b, int64_t t0, int n, const ObserveIngestPlan& P, uint8_t* dst,
                            hipStream_t s) {
  vsf_ctx::Observe& o = ctx->ob;
  ObserveLaunchStats& stats = o.queue->stats;
  batch_files(o, t0, n);
  // (frames of different denominators share the batch and its ONE upload: a run ends where the denominator changes)
  const bool any_reduced = std::any_of(o.dec_reduces.begin(), o.dec_reduces.end(), [](uint8_t r) { return r > 1; });
  for (int i = 0; i < 2 * n; i++)
    if (P.cls[(size_t)(i / 2)] == kObserveOwnFile) o.dec_kinds[(size_t)i] = o.frames[(size_t)((t0 + i / 2) % o.depth)].kind[i & 1];
  int runs = 0;
  const vsf_status st = decode_runs(ctx, o.dec_files.data(), o.dec_sizes.data(), o.dec_kinds.data(), 2 * n, ctx->p.width,
                                    ctx->p.height, b.blob, o.ing_scratch, dst, ctx->st_img_stride, (int)ctx->st_img_pitch, b.status,
                                    1, s, &runs, any_reduced ? o.dec_reduces.data() : nullptr);
  if (st != VSF_OK) return st;
  stats.ingest_commands += 1 + runs;  // (one copy command, each run's decode -- counted as one, whatever kernels it takes)
  for (int f = 0; f < n; f++) {
    stats.compressed += P.cls[(size_t)f] == kObserveOwnFile;
    stats.reduced += P.cls[(size_t)f] == kObserveOwnFile && o.dec_reduces[(size_t)(2 * f)] > 1;
  }
  return VSF_OK;
}

// Big-slot files: cv::imdecode, whole, at the size they have, into `dst`'s big slots at the index the frame has in the batch:
// a decode_runs per distinct size among them (a size is decoded at the first frame that has it).
vsf_status decode_big_files(vsf_ctx* ctx, vsf_ctx::ObserveBatch& b, int64_t t0, int n, const ObserveIngestPlan& P, uint8_t* dst,
                            hipStream_t s) {
  vsf_ctx::Observe& o = ctx->ob;
  batch_files(o, t0, n);
  int done[VSF_OBSERVE_MAX_STREAMS][2], n_done = 0;  // the sizes decoded so far: at most one per stream
  for (int f0 = 0; f0 < n; f0++) {
    const ObserveIngestIn& lead = P.in[(size_t)f0];
    bool seen = P.cls[(size_t)f0] != kObserveBigFile;
    for (int q = 0; q < n_done && !seen; q++) seen = done[q][0] == lead.in_w && done[q][1] == lead.in_h;
    if (seen || n_done == VSF_OBSERVE_MAX_STREAMS) continue;
    done[n_done][0] = lead.in_w, done[n_done++][1] = lead.in_h;
    for (int i = 0; i < 2 * n; i++) {
      const ObserveIngestIn& w = P.in[(size_t)(i / 2)];
      const bool mine = P.cls[(size_t)(i / 2)] == kObserveBigFile && w.in_w == lead.in_w && w.in_h == lead.in_h;
      o.dec_kinds[(size_t)i] = mine ? o.frames[(size_t)((t0 + i / 2) % o.depth)].kind[i & 1] : (uint8_t)VSF_FILE_NONE;
    }
    if (!b.blob_in.uploaded) VSF_HIP(b.blob_in.uploaded.alloc(hipEventDisableTiming));
    int runs = 0;
    const vsf_status st = decode_runs(ctx, o.dec_files.data(), o.dec_sizes.data(), o.dec_kinds.data(), 2 * n, lead.in_w, lead.in_h,
                                      b.blob_in, o.ing_scratch, dst, o.in_half, (int)observe_input_pitch(lead.in_w), b.status, 1, s,
                                      &runs);
    if (st != VSF_OK) return st;
    o.queue->stats.resize_commands += 1 + runs;  // (the upload, each run's decode)
  }
  return VSF_OK;
}

}  // namespace

namespace vsfi {

vsf_status ingest(vsf_ctx* ctx, vsf_ctx::ObserveBatch& b, int64_t t0, int n, const ObserveIngestPlan& P, hipStream_t s) {
  vsf_ctx::Observe& o = ctx->ob;
  ObserveLaunchStats& stats = o.queue->stats;
  const int cw = ctx->p.width, ch = ctx->p.height, img_pitch = (int)ctx->st_img_pitch;
  const size_t stride = ctx->st_img_stride, frame_bytes = 2 * stride;
  // own-size images land in the batch's images; the mosaics of a Bayer batch in the mosaics' buffer, whatever brings them
  uint8_t* own = P.mosaics ? o.d_bayer.get() : b.d_img.get();
  // ---- 1. raw host frames: ONE copy command (two when the frames wrap around the staging ring) for the batch's whole span of
  // the staging ring -- the steps below write over what the other frames' slots held ----
  if (P.raw) {
    const int slot0 = (int)(t0 % o.depth), first = std::min(n, o.depth - slot0);
    VSF_HIP(hipMemcpyAsync(own, o.h_img + (size_t)slot0 * frame_bytes, (size_t)first * frame_bytes, hipMemcpyHostToDevice, s));
    if (first < n)
      VSF_HIP(hipMemcpyAsync(own + (size_t)first * frame_bytes, o.h_img, (size_t)(n - first) * frame_bytes, hipMemcpyHostToDevice, s));
  }
  // ---- 2. device frames, own-size and big-slot alike: the copy stream waits for the launches that filled their slots -- for
  // the newest event of every stretch of frames that came over one producer stream: it is behind the others --, then ONE copy
  // command per run takes own-size frames out of the device ring ----
  const vsf_ctx::ObserveFrame* last = nullptr;
  for (int f = 0; (P.dev || P.big_dev) && f <= n; f++) {
    if (f < n && P.cls[(size_t)f] != kObserveOwnDevice && P.cls[(size_t)f] != kObserveBigDevice) continue;
    const vsf_ctx::ObserveFrame* fr = f < n ? &o.frames[(size_t)((t0 + f) % o.depth)] : nullptr;
    if (last && (!fr || fr->dev_stream != last->dev_stream)) VSF_HIP(hipStreamWaitEvent(s, o.dev_ev[(size_t)last->dev_event], 0));
    last = fr;
  }
  for (const ObserveRun& r : P.runs) {
    if (r.cls != kObserveRunDevice) continue;
    VSF_HIP(hipMemcpyAsync(own + (size_t)r.f0 * frame_bytes, o.d_ring + (size_t)r.slot0 * frame_bytes, (size_t)r.n * frame_bytes,
                           hipMemcpyDeviceToDevice, s));
    stats.device_commands++;
    stats.device_frames += r.n;
  }
  // ---- 3. own-size files: one more copy command for the files, the decoders ----
  if (P.files) {
    const vsf_status st = decode_own_files(ctx, b, t0, n, P, own, s);
    if (st != VSF_OK) return st;
  }
  // ---- 4. the ONE demosaic of an own-size Bayer batch, behind the last of the steps above that the batch has (a batch without
  // files has no step 3: the demosaic follows its device copies, or its upload); counted where that step's commands are ----
  if (P.demosaic != kObserveStepNone) {
    vsf_launch_to_gray(P.pixfmt, o.d_bayer, 2 * n, cw, ch, stride, img_pitch, b.d_img, stride, img_pitch, s);
    stats.device_commands += P.demosaic == kObserveAfterDeviceCopies;
    stats.ingest_commands += P.demosaic == kObserveAfterDecode;
    stats.pix_frames += P.own_pix_new;
    stats.pix_commands += P.own_pix_new != 0;
  }
  // ---- 5. big-slot frames, over whatever the steps above left in their places: raw host frames' uploads (ObserveUpload: one per
  // stretch of them, short gaps bridged) into the batch's big slots; the files decoded there, size by size; then per run gray
  // at the arriving size (mosaics, packed colour) and ONE resize launch into the batch's images ----
  const size_t half = o.in_half, slot = 2 * half;
  stats.multi_size += P.multi_size;
  for (const ObserveUpload& u : P.resize.uploads) {
    VSF_HIP(hipMemcpyAsync(b.d_in + (size_t)u.f0 * slot, o.h_in + (size_t)u.slot0 * slot, (size_t)u.n * slot, hipMemcpyHostToDevice, s));
    (P.bpp > 1 ? stats.pix_commands : stats.resize_commands)++;  // (packed colour is in the big slots whatever its size)
  }
  if (P.big_files) {
    const vsf_status st = decode_big_files(ctx, b, t0, n, P, P.mosaics ? o.d_bayer_in.get() : b.d_in.get(), s);
    if (st != VSF_OK) return st;
  }
  for (const ObserveResizeRun& r : P.resize.runs) {
    const int pitch = (int)observe_input_pitch(r.w);
    const bool ring = r.where == kObserveInDeviceRing;
    uint8_t* staged = b.d_in + (size_t)r.f0 * slot;
    uint8_t* images = b.d_img + (size_t)r.f0 * frame_bytes;
    const uint8_t* src = ring ? o.d_in_ring + (size_t)r.src0 * slot : staged;
    for (int f = r.f0; f < r.f0 + r.n; f++) {  // (what the frames also are)
      stats.device_frames += P.cls[(size_t)f] == kObserveBigDevice;
      stats.compressed += P.cls[(size_t)f] == kObserveBigFile;
    }
    if (P.mosaics) {  // the images are mosaics: where they lie -> gray in the batch's big slots
      // (a raw host mosaic was uploaded into the batch's big slot itself: it goes through the mosaics' buffer and back)
      uint8_t* mosaics = o.d_bayer_in + (size_t)r.f0 * slot;
      int n_new = 0;
      for (int f = r.f0; f < r.f0 + r.n; f++) {
        n_new += P.in[(size_t)f].pix_new;
        if (P.cls[(size_t)f] != kObserveBigRaw) continue;
        VSF_HIP(hipMemcpyAsync(mosaics + (size_t)(f - r.f0) * slot, staged + (size_t)(f - r.f0) * slot, slot, hipMemcpyDeviceToDevice, s));
        stats.pix_commands++;
      }
      vsf_launch_to_gray(P.pixfmt, ring ? src : mosaics, 2 * r.n, r.w, r.h, half, pitch, staged, half, pitch, s);
      stats.resize_commands++;
      stats.pix_commands += n_new != 0;
      stats.pix_frames += n_new;
      src = staged;
    } else if (P.bpp > 1) {  // packed colour, rows of w * bpp bytes: cv::resize(to_gray(frame)) -- gray at the arriving size first
      const int cpitch = (int)observe_pix_pitch(r.w, P.bpp);
      stats.pix_commands++;
      stats.pix_frames += r.n;
      if (r.w == cw && r.h == ch) {  // ... which is the context's: straight into the batch's images, nothing to resize
        vsf_launch_to_gray(P.pixfmt, src, 2 * r.n, r.w, r.h, half, cpitch, images, stride, img_pitch, s);
        continue;
      }
      uint8_t* gray = o.d_bayer_in + (size_t)r.f0 * slot;
      vsf_launch_to_gray(P.pixfmt, src, 2 * r.n, r.w, r.h, half, cpitch, gray, half, pitch, s);
      src = gray;
    }
    vsf_launch_resize_gray(src, 2 * r.n, r.w, r.h, half, (size_t)pitch, images, cw, ch, stride, ctx->st_img_pitch, s);
    stats.resize_commands++;
    stats.resized += r.n;
  }
  // ---- 6. the ONE ingest finish of a batch that holds files: an image its decoder refused becomes all zero; counted with the
  // last decode's commands ----
  if (P.finish != kObserveStepNone) {
    vsf_launch_ingest_finish(b.d_img, stride, img_pitch, ch, b.status, 2 * n, s);
    (P.finish == kObserveAfterBigDecode ? stats.resize_commands : stats.ingest_commands)++;
  }
  // ---- 7. the extraction, on the context's stream, waits for all of it ----
  if (s != ctx->stream) {
    VSF_HIP(hipEventRecord(b.ev_uploaded, s));
    VSF_HIP(hipStreamWaitEvent(ctx->stream, b.ev_uploaded, 0));
  }
  return VSF_OK;
}

}  // namespace vsfi
