// vsf_observe_plan.cc -- see vsf_observe_plan.h.  Plain C++: no device, no context.
#include "vsf_observe_plan.h"

#include <algorithm>
#include <cstring>

namespace vsfi {

bool observe_plan_must_cut(const vsf_calibration& a_calib, float a_best_percent, const vsf_calibration& b_calib,
                           float b_best_percent) {
  return a_best_percent != b_best_percent || std::memcmp(&a_calib, &b_calib, sizeof(vsf_calibration)) != 0;
}

bool observe_plan(const ObservePlanIn* in, int n, int n_streams, int ring, int life, ObservePlan* plan) {
  if (!in || !plan || n < 1 || n_streams < 1 || n_streams > VSF_OBSERVE_MAX_STREAMS || life < 0 || ring < life + 1) return false;
  if ((int64_t)n_streams * ring + n > INT32_MAX) return false;
  int last[VSF_OBSERVE_MAX_STREAMS];  // the stream's newest frame in the list so far, -1: none
  std::fill(last, last + n_streams, -1);
  plan->frames.resize((size_t)n);
  plan->q_set.clear();
  plan->t_set.clear();
  plan->best_percent.clear();
  plan->calibs.clear();
  plan->cuts.clear();
  plan->max_pairs_per_frame = 1;
  plan->n_streams_present = 0;
  for (int f = 0; f < n; f++) {
    const ObservePlanIn& w = in[f];
    if (w.stream < 0 || w.stream >= n_streams || w.k < 0 || !w.calib) return false;
    ObservePlanFrame& fm = plan->frames[(size_t)f];
    fm.left_set = w.stream * ring + (int32_t)(w.k % ring);
    fm.right_set = n_streams * ring + f;
    plan->q_set.push_back(fm.right_set);  // Calculate3DPoints: GetFeatureMatches(right, left) with best_percent_ 1.0 (cc:129-132)
    plan->t_set.push_back(fm.left_set);
    plan->best_percent.push_back(1.0f);
  }
  int n_pairs = n;
  for (int f = 0; f < n; f++) {
    const ObservePlanIn& w = in[f];
    ObservePlanFrame& fm = plan->frames[(size_t)f];
    fm.stream = w.stream;
    fm.best_percent = w.best_percent;
    fm.n_past = (int32_t)std::min<int64_t>(w.k, life);
    fm.tp0 = n_pairs;
    for (int p = 0; p < fm.n_past; p++) {  // oldest kept frame first: the order frame_list_ is walked in (cc:424)
      plan->q_set.push_back(w.stream * ring + (int32_t)((w.k - fm.n_past + p) % ring));
      plan->t_set.push_back(fm.left_set);
      plan->best_percent.push_back(w.best_percent);
      n_pairs++;
    }
    plan->max_pairs_per_frame = std::max(plan->max_pairs_per_frame, fm.n_past + 1);
    // the threshold chain: every stream's frames in batch order
    fm.prev = last[w.stream];
    fm.tail = -1;
    if (fm.prev < 0) {
      plan->n_streams_present++;
    } else {
      const ObservePlanIn& a = in[fm.prev];
      if (w.k != a.k + 1) return false;  // a stream's frames wait in the order they came
      if (observe_plan_must_cut(*a.calib, a.best_percent, *w.calib, w.best_percent)) plan->cuts.push_back(f);
    }
    last[w.stream] = f;
    // the calibration table: a stream's frames keep its entry; a stream's first frame searches the few there are
    auto same = [&](size_t i) { return std::memcmp(&plan->calibs[i], w.calib, sizeof(vsf_calibration)) == 0; };
    size_t c = fm.prev >= 0 ? (size_t)plan->frames[(size_t)fm.prev].calib : 0;
    if (fm.prev < 0 || !same(c))
      for (c = 0; c < plan->calibs.size() && !same(c);) c++;
    if (c == plan->calibs.size()) plan->calibs.push_back(*w.calib);
    fm.calib = (int32_t)c;
  }
  for (int f = 0; f < n; f++) {
    ObservePlanFrame& fm = plan->frames[(size_t)f];
    if (fm.prev < 0) fm.tail = last[fm.stream];
  }
  plan->n_pairs = n_pairs;
  return true;
}

bool observe_submit_span(int64_t next_ticket, int64_t next_collect, int depth, int n, ObserveSpan* span) {
  if (!span || depth < 1 || depth > 1024 || next_collect < 0 || next_ticket < next_collect || next_ticket - next_collect > depth)
    return false;
  const int free_slots = depth - (int)(next_ticket - next_collect);
  if (n < 1 || n > free_slots) return false;
  const int slot0 = (int)(next_ticket % depth), first = std::min(n, depth - slot0);
  *span = {slot0, first, n - first};
  return true;
}

bool observe_batch_runs(const uint8_t* kinds, int n, int64_t t0, int depth, std::vector<ObserveRun>* runs) {
  if (!kinds || !runs || depth < 1 || n < 1 || n > depth || t0 < 0) return false;
  runs->clear();
  int slot = (int)(t0 % depth);
  for (int f = 0; f < n; f++) {
    if (kinds[f] > kObserveKindDevice) return false;
    const int cls = kinds[f] == 0 ? kObserveRunRaw : kinds[f] == kObserveKindDevice ? kObserveRunDevice : kObserveRunCompressed;
    if (f == 0 || slot == 0 || runs->back().cls != cls)
      runs->push_back({cls, f, 1, slot});
    else
      runs->back().n++;
    if (++slot == depth) slot = 0;
  }
  return true;
}

size_t observe_input_pitch(int w) { return w >= 1 && w <= 32767 ? ((size_t)w + 63) & ~(size_t)63 : 0; }

size_t observe_input_image_bytes(int w, int h) {
  if (w < 1 || h < 1 || w > 32767 || h > 32767) return 0;
  return (observe_input_pitch(w) * (size_t)h + 255) & ~(size_t)255;
}

size_t observe_input_half_bytes(const int* in_w, const int* in_h, int n_streams) {
  if (!in_w || !in_h || n_streams < 1 || n_streams > VSF_OBSERVE_MAX_STREAMS) return 0;
  size_t half = 0;
  for (int s = 0; s < n_streams; s++)
    if (in_w[s] != 0 || in_h[s] != 0) half = std::max(half, observe_input_image_bytes(in_w[s], in_h[s]));
  return half;
}

size_t observe_pix_pitch(int w, int bpp) {
  if (w < 1 || w > 32767 || (bpp != 1 && bpp != 3 && bpp != 4)) return 0;
  return ((size_t)w * (size_t)bpp + 63) & ~(size_t)63;
}

size_t observe_pix_image_bytes(int w, int h, int bpp) {
  const size_t pitch = observe_pix_pitch(w, bpp);
  if (pitch == 0 || h < 1 || h > 32767) return 0;
  const size_t bytes = pitch * (size_t)h;
  return bytes <= 0x7FFFFFFFu ? (bytes + 255) & ~(size_t)255 : 0;
}

size_t observe_input_ring_bytes(int depth, size_t half) {
  if (depth < 1 || depth > 1024 || half == 0) return 0;
  return (size_t)depth * 2 * half;
}

int observe_upload_max_gap(size_t slot_bytes) {
  if (slot_bytes == 0) return 0;
  const size_t gap = (size_t)kObserveCopyCommandUs * kObserveLinkBytesPerUs / slot_bytes;
  return gap > 1024 ? 1024 : (int)gap;
}

bool observe_resize_plan(const ObserveResizeIn* in, int n, int64_t t0, int depth, int max_gap, ObserveResizePlan* plan) {
  if (!in || !plan || depth < 1 || n < 1 || n > depth || t0 < 0 || max_gap < 0) return false;
  plan->runs.clear();
  plan->uploads.clear();
  plan->n_resized = 0;
  int raw_last = -1;  // the last raw resized frame so far: the end of uploads.back()
  int slot = (int)(t0 % depth);
  bool open = false;  // the frame in front is the last of runs.back()
  for (int f = 0; f < n; f++, slot = slot + 1 == depth ? 0 : slot + 1) {
    const ObserveResizeIn& w = in[f];
    if (w.kind > kObserveKindDevice || w.w < 0 || w.h < 0 || (w.w == 0) != (w.h == 0)) return false;
    if (w.w == 0) {
      open = false;
      continue;
    }
    plan->n_resized++;
    const int where = w.kind == kObserveKindDevice ? kObserveInDeviceRing : kObserveInStaged;
    if (w.kind == 0) {
      // (the upload in front reaches this frame unless the gap is too long or the ring wrapped in between: slot <= gap then)
      if (raw_last >= 0 && f - raw_last - 1 <= max_gap && slot > f - raw_last - 1)
        plan->uploads.back().n = f - plan->uploads.back().f0 + 1;
      else
        plan->uploads.push_back({f, 1, slot});
      raw_last = f;
    }
    const bool wraps = where == kObserveInDeviceRing && slot == 0;
    if (open && !wraps && plan->runs.back().where == where && plan->runs.back().w == w.w && plan->runs.back().h == w.h)
      plan->runs.back().n++;
    else
      plan->runs.push_back({where, f, 1, where == kObserveInDeviceRing ? slot : f, w.w, w.h});
    open = true;
  }
  return true;
}

bool observe_pix_is_bayer(int pixfmt) {
  return pixfmt == VSF_PIX_BAYER_RGGB8 || pixfmt == VSF_PIX_BAYER_GRBG8 || pixfmt == VSF_PIX_BAYER_GBRG8 ||
         pixfmt == VSF_PIX_BAYER_BGGR8;
}

bool observe_ingest_plan(int n, int pixfmt, int64_t t0, int depth, bool may_resize, int max_gap, ObserveIngestPlan* plan) {
  if (!plan || depth < 1 || n < 1 || n > depth || t0 < 0 || max_gap < 0 || plan->in.size() < (size_t)n) return false;
  ObserveIngestPlan& p = *plan;
  p.pixfmt = pixfmt;
  p.bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (p.bpp == 0) return false;
  p.mosaics = observe_pix_is_bayer(pixfmt);
  p.raw = p.files = p.dev = p.big = p.big_files = p.big_dev = p.multi_size = false;
  p.own_pix_new = 0;
  p.cls.resize((size_t)n);
  p.run_kinds.resize((size_t)n);
  p.resize_in.resize((size_t)n);
  for (int f = 0; f < n; f++) {
    const ObserveIngestIn& w = p.in[(size_t)f];
    if (w.kind > kObserveKindDevice) return false;
    const bool big = may_resize && w.in_w != 0, dev = w.kind == kObserveKindDevice, file = w.kind != 0 && !dev;
    p.cls[(size_t)f] = (uint8_t)((big ? kObserveBigRaw : kObserveOwnRaw) + (file ? 1 : dev ? 2 : 0));
    p.raw |= !big && !file && !dev;
    p.files |= !big && file;
    p.dev |= !big && dev;
    p.big |= big;
    p.big_files |= big && file;
    p.big_dev |= big && dev;
    p.own_pix_new += p.mosaics && !big && w.pix_new;
    // (a device frame of a declared size is not copied: k_resize.hip reads it where it lies, in the ring of big slots)
    p.run_kinds[(size_t)f] = big ? (uint8_t)0 : w.kind;
    p.resize_in[(size_t)f] = {big ? w.in_w : 0, big ? w.in_h : 0, w.kind};
    p.multi_size |= p.resize_in[(size_t)f].w != p.resize_in[0].w || p.resize_in[(size_t)f].h != p.resize_in[0].h;
  }
  p.multi_size &= p.big;
  p.demosaic = !p.mosaics ? kObserveStepNone
               : p.files  ? kObserveAfterDecode
               : p.dev    ? kObserveAfterDeviceCopies
               : p.raw    ? kObserveAfterUpload
                          : kObserveStepNone;
  p.finish = p.big_files ? kObserveAfterBigDecode : p.files ? kObserveAfterDecode : kObserveStepNone;
  p.runs.clear();
  if (p.dev && !observe_batch_runs(p.run_kinds.data(), n, t0, depth, &p.runs)) return false;
  p.resize.runs.clear();
  p.resize.uploads.clear();
  p.resize.n_resized = 0;
  return !p.big || observe_resize_plan(p.resize_in.data(), n, t0, depth, max_gap, &p.resize);
}

}  // namespace vsfi

// ---- pixel formats (include/vsf.h): the table behind every call that takes a pixfmt ----
extern "C" {

int vsf_pixfmt_bytes_per_pixel(int pixfmt) {
  switch (pixfmt) {
    case VSF_PIX_MONO8:
    case VSF_PIX_BAYER_RGGB8:
    case VSF_PIX_BAYER_GRBG8:
    case VSF_PIX_BAYER_GBRG8:
    case VSF_PIX_BAYER_BGGR8:
      return 1;
    case VSF_PIX_BGR8:
    case VSF_PIX_RGB8:
      return 3;
    case VSF_PIX_BGRA8:
    case VSF_PIX_RGBA8:
      return 4;
    default:
      return 0;  // (2 .. 15 included: they stay unknown)
  }
}

vsf_status vsf_pixfmt_from_encoding(const char* ros_encoding, int* pixfmt) {
  static const struct {
    const char* name;
    int pixfmt;
  } kTable[] = {{"mono8", VSF_PIX_MONO8},           {"bayer_rggb8", VSF_PIX_BAYER_RGGB8}, {"bayer_grbg8", VSF_PIX_BAYER_GRBG8},
                {"bayer_gbrg8", VSF_PIX_BAYER_GBRG8}, {"bayer_bggr8", VSF_PIX_BAYER_BGGR8}, {"bgr8", VSF_PIX_BGR8},
                {"rgb8", VSF_PIX_RGB8},             {"bgra8", VSF_PIX_BGRA8},             {"rgba8", VSF_PIX_RGBA8}};
  if (!ros_encoding || !pixfmt) return VSF_ERR_INVALID_ARG;
  for (const auto& e : kTable)
    if (std::strcmp(ros_encoding, e.name) == 0) {
      *pixfmt = e.pixfmt;
      return VSF_OK;
    }
  return VSF_ERR_UNSUPPORTED;
}

}  // extern "C"
