// The ingest plan of a batch of the ObserveImage queue (csrc/vsf_observe_plan.cc observe_ingest_plan: what every frame is, the
// presence flags, the device ring's copies, the big-slot frames' uploads and resize runs, where the batch's one demosaic and
// its one ingest finish run) on the CPU: compiled together with that file, plainly and under AddressSanitizer + UBSan
// (tests/test_observe_ingest_plan.py).
//   randomised   depths 1 .. 1024, batches anywhere in the ring (wraps included), all four kinds, 0 .. 3 declared sizes, mono /
//                Bayer / packed colour, a queue that has seen a big-slot frame or not -- against a second spelling written
//                frame by frame here
//   fixed        the frame lists of two GPU tests with flags and run counts written out by hand; a batch of each class alone;
//                a device frame of a declared size alone (waits, no copy)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_observe_plan.h"

using namespace vsfi;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      if (++failures > 20) std::exit(1);                           \
    }                                                              \
  } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static int depth_of(int i) {  // 1 .. 1024: the small ones all, then a spread, then the largest
  static const int some[] = {17, 31, 32, 33, 63, 64, 100, 127, 128, 255, 256, 257, 500, 1000, 1023, 1024};
  return i < 16 ? i + 1 : some[i - 16];
}
constexpr int kDepths = 32;
constexpr uint8_t kRaw = 0, kJpeg = 1, kPng = 2, kDev = kObserveKindDevice;

struct Frame {
  uint8_t kind;
  bool pix_new;
  int w, h;  // declared size, 0 x 0: none
};

static bool plan(const std::vector<Frame>& fr, int pixfmt, int64_t t0, int depth, bool may_resize, int max_gap, ObserveIngestPlan* p) {
  p->in.resize(fr.size());
  for (size_t f = 0; f < fr.size(); f++) p->in[f] = {fr[f].kind, fr[f].pix_new, fr[f].w, fr[f].h};
  return observe_ingest_plan((int)fr.size(), pixfmt, t0, depth, may_resize, max_gap, p);
}

// Everything the plan says, against a second spelling: frame by frame, in the words the queue's launch used before it had a plan.
static void check(const std::vector<Frame>& fr, int pixfmt, int64_t t0, int depth, bool may_resize, int max_gap,
                  const ObserveIngestPlan& p) {
  const int n = (int)fr.size();
  const bool bayer = pixfmt == VSF_PIX_BAYER_RGGB8 || pixfmt == VSF_PIX_BAYER_GRBG8 || pixfmt == VSF_PIX_BAYER_GBRG8 ||
                     pixfmt == VSF_PIX_BAYER_BGGR8;
  CHECK(p.mosaics == bayer && p.pixfmt == pixfmt && p.bpp == vsf_pixfmt_bytes_per_pixel(pixfmt));
  CHECK((int)p.cls.size() >= n);
  // ---- the six flags: the expressions of the launch's flag loop ----
  bool any_raw = false, any_cmp = false, any_dev = false, rs_any = false, rs_cmp = false, rs_dev = false;
  int own_new = 0;
  std::vector<int> cover((size_t)n, 0), uploaded((size_t)n, 0);
  for (int f = 0; f < n; f++) {
    const uint8_t kind = fr[(size_t)f].kind;
    const bool rs = may_resize && fr[(size_t)f].w != 0, dev = kind == kObserveKindDevice, cmp = kind != 0 && !dev;
    any_raw |= !rs && kind == 0;
    any_dev |= !rs && dev;
    any_cmp |= !rs && cmp;
    rs_any |= rs;
    rs_dev |= rs && dev;
    rs_cmp |= rs && cmp;
    own_new += bayer && fr[(size_t)f].pix_new && !rs;
    // ---- exactly one class, the one the frame has ----
    int want = -1;
    if (!rs && kind == 0) want = kObserveOwnRaw;
    if (!rs && cmp) want = kObserveOwnFile;
    if (!rs && dev) want = kObserveOwnDevice;
    if (rs && kind == 0) want = kObserveBigRaw;
    if (rs && cmp) want = kObserveBigFile;
    if (rs && dev) want = kObserveBigDevice;
    CHECK(want >= 0 && p.cls[(size_t)f] == want);
  }
  CHECK(p.raw == any_raw && p.files == any_cmp && p.dev == any_dev);
  CHECK(p.big == rs_any && p.big_files == rs_cmp && p.big_dev == rs_dev);
  CHECK(p.own_pix_new == own_new);
  // ---- the device ring's copies and the resize runs cover every own-size device frame and every big-slot frame exactly once ----
  for (const ObserveRun& r : p.runs) {
    CHECK(r.n >= 1 && r.f0 >= 0 && r.f0 + r.n <= n && r.slot0 == (int)((t0 + r.f0) % depth) && r.slot0 + r.n <= depth);
    for (int f = r.f0; f < r.f0 + r.n && f < n; f++) {
      if (r.cls == kObserveRunDevice) cover[(size_t)f]++;
      CHECK((r.cls == kObserveRunDevice) == (p.cls[(size_t)f] == kObserveOwnDevice));  // (a big-slot device frame is no device run)
    }
  }
  CHECK(any_dev || p.runs.empty());
  for (const ObserveResizeRun& r : p.resize.runs) {
    CHECK(r.n >= 1 && r.f0 >= 0 && r.f0 + r.n <= n);
    const bool ring = r.where == kObserveInDeviceRing;
    CHECK(ring ? r.src0 == (int)((t0 + r.f0) % depth) && r.src0 + r.n <= depth : r.src0 == r.f0);
    for (int f = r.f0; f < r.f0 + r.n && f < n; f++) {
      cover[(size_t)f]++;
      CHECK(fr[(size_t)f].w == r.w && fr[(size_t)f].h == r.h && ring == (p.cls[(size_t)f] == kObserveBigDevice));
    }
  }
  int n_big = 0;
  for (int f = 0; f < n; f++) {
    const bool covered = p.cls[(size_t)f] == kObserveOwnDevice || p.cls[(size_t)f] >= kObserveBigRaw;
    CHECK(cover[(size_t)f] == (covered ? 1 : 0));
    n_big += p.cls[(size_t)f] >= kObserveBigRaw;
  }
  CHECK(p.resize.n_resized == n_big);
  // ---- raw big-slot frames are covered by the uploads: each once, every upload begins and ends with one, none across the ring's end ----
  for (const ObserveUpload& u : p.resize.uploads) {
    CHECK(u.n >= 1 && u.f0 >= 0 && u.f0 + u.n <= n && u.slot0 == (int)((t0 + u.f0) % depth) && u.slot0 + u.n <= depth);
    if (u.f0 + u.n > n) continue;
    CHECK(p.cls[(size_t)u.f0] == kObserveBigRaw && p.cls[(size_t)(u.f0 + u.n - 1)] == kObserveBigRaw);
    int gap = 0;
    for (int f = u.f0; f < u.f0 + u.n; f++) {
      uploaded[(size_t)f]++;
      gap = p.cls[(size_t)f] == kObserveBigRaw ? 0 : gap + 1;
      CHECK(gap <= max_gap);
    }
  }
  for (int f = 0; f < n; f++) CHECK(p.cls[(size_t)f] == kObserveBigRaw ? uploaded[(size_t)f] == 1 : uploaded[(size_t)f] <= 1);
  // ---- the one demosaic: behind the last step that wrote mosaics, in the order upload < device copies < decode ----
  int demosaic = kObserveStepNone;
  if (bayer && any_raw) demosaic = kObserveAfterUpload;
  if (bayer && any_dev) demosaic = kObserveAfterDeviceCopies;
  if (bayer && any_cmp) demosaic = kObserveAfterDecode;
  CHECK(p.demosaic == demosaic);
  CHECK((p.demosaic == kObserveStepNone) == !(bayer && (any_raw || any_dev || any_cmp)));
  // (the three conditions the launch had: in the device step, inline, in the decode step)
  CHECK((p.demosaic == kObserveAfterDeviceCopies) == (bayer && any_dev && !any_cmp));
  CHECK((p.demosaic == kObserveAfterUpload) == (bayer && any_raw && !any_dev && !any_cmp));
  CHECK((p.demosaic == kObserveAfterDecode) == (bayer && any_cmp));
  // ---- the one finish: owed exactly when a frame is a file, behind the last step that decodes files ----
  bool file = false;
  for (int f = 0; f < n; f++) file |= fr[(size_t)f].kind == kJpeg || fr[(size_t)f].kind == kPng;
  CHECK((p.finish != kObserveStepNone) == file);
  CHECK(p.finish == (rs_cmp ? kObserveAfterBigDecode : any_cmp ? kObserveAfterDecode : kObserveStepNone));
  // ---- more than one size: what the launch's scan over the resize plan's input found ----
  bool multi = false;
  for (int f = 1; f < n && rs_any; f++) {
    const int w0 = may_resize ? fr[0].w : 0, h0 = may_resize ? fr[0].h : 0;
    multi |= fr[(size_t)f].w != w0 || fr[(size_t)f].h != h0;
  }
  CHECK(p.multi_size == multi);
}

static long n_randomised = 0;
static void randomised() {
  static const int kFormats[] = {VSF_PIX_MONO8, VSF_PIX_BAYER_RGGB8, VSF_PIX_BAYER_GRBG8, VSF_PIX_BGR8, VSF_PIX_RGBA8};
  static const int kSizes[3][2] = {{640, 480}, {96, 80}, {1280, 722}};
  ObserveIngestPlan p;  // (one plan object for every case: it keeps its storage, and nothing of a case may reach the next)
  long checked = 0;
  for (int di = 0; di < kDepths; di++) {
    const int depth = depth_of(di);
    for (int rep = 0; rep < 120; rep++) {
      const int n = 1 + (int)(rnd() % (uint32_t)depth);
      // anywhere in the ring: every other batch reaches its end or wraps; tickets beyond 2^31 included
      const int64_t lap = (rep & 2) ? ((int64_t)1 << 33) / depth * depth : (int64_t)(rnd() % 100u) * depth;
      const int64_t t0 = lap + ((rep & 1) ? depth - 1 - (int)(rnd() % (uint32_t)n) : (int)(rnd() % (uint32_t)depth));
      const int pixfmt = kFormats[rnd() % 5u];
      const int declared = (int)(rnd() % 4u);  // streams [0, declared) of 4 have a declared size
      const bool may_resize = (rnd() % 4u) != 0;  // (false: the records' sizes mean nothing, whatever they hold)
      const int max_gap = (int)(rnd() % 8u);
      const uint32_t mix = rnd() % 16u;  // which kinds the batch draws from (0: all)
      std::vector<Frame> fr((size_t)n);
      for (Frame& f : fr) {
        do f.kind = (uint8_t)(rnd() % 4u);
        while (mix != 0 && !((mix >> f.kind) & 1u));
        const int s = (int)(rnd() % 4u);
        f.w = s < declared ? kSizes[s][0] : 0;
        f.h = s < declared ? kSizes[s][1] : 0;
        f.pix_new = (rnd() & 1u) != 0;
      }
      CHECK(plan(fr, pixfmt, t0, depth, may_resize, max_gap, &p));
      check(fr, pixfmt, t0, depth, may_resize, max_gap, p);
      checked++;
    }
  }
  n_randomised = checked;
}

// tests/test_gpu_observe_device.py test_raw_jpeg_png_and_device_frames_in_one_queue: depth 32, mono, no declared size.
static void fixed_mixed_kinds() {
  const uint8_t kinds[] = {kRaw, kJpeg, kPng, kDev, kDev, kPng, kRaw, kDev, kJpeg, kDev, kRaw};
  std::vector<Frame> fr;
  for (uint8_t k : kinds) fr.push_back({k, false, 0, 0});
  ObserveIngestPlan p;
  CHECK(plan(fr, VSF_PIX_MONO8, 0, 32, false, 0, &p));
  check(fr, VSF_PIX_MONO8, 0, 32, false, 0, p);
  CHECK(p.raw && p.files && p.dev && !p.big && !p.big_files && !p.big_dev && !p.mosaics && !p.multi_size);
  CHECK(p.demosaic == kObserveStepNone && p.finish == kObserveAfterDecode && p.own_pix_new == 0);
  // raw | jpeg png | dev dev | png | raw | dev | jpeg | dev | raw: nine runs, three of them the device ring's copies
  CHECK(p.runs.size() == 9);
  int copies = 0, copied = 0;
  for (const ObserveRun& r : p.runs)
    if (r.cls == kObserveRunDevice) copies++, copied += r.n;
  CHECK(copies == 3 && copied == 4);
  CHECK(p.runs[2].cls == kObserveRunDevice && p.runs[2].f0 == 3 && p.runs[2].n == 2 && p.runs[2].slot0 == 3);
  CHECK(p.resize.runs.empty() && p.resize.uploads.empty() && p.resize.n_resized == 0);
}

// tests/test_gpu_observe_resize.py test_streams_of_different_sizes_share_batches: stream 0 raw 640 x 480, 1 device 960 x 720,
// 2 PNG 200 x 150, 3 raw without a declared size, interleaved; depth 32, a batch of 16.
static void fixed_mixed_sizes() {
  std::vector<Frame> fr;
  for (int i = 0; i < 4; i++) {
    fr.push_back({kRaw, false, 640, 480});
    fr.push_back({kDev, false, 960, 720});
    fr.push_back({kPng, false, 200, 150});
    fr.push_back({kRaw, false, 0, 0});
  }
  const int in_w[4] = {640, 960, 200, 0}, in_h[4] = {480, 720, 150, 0};
  const size_t half = observe_input_half_bytes(in_w, in_h, 4);
  CHECK(half == (size_t)960 * 720);
  const int max_gap = observe_upload_max_gap(2 * half);
  CHECK(max_gap == 6);  // 180 us x 50 000 bytes / us over slots of 1 382 400 bytes
  ObserveIngestPlan p;
  CHECK(plan(fr, VSF_PIX_MONO8, 0, 32, true, max_gap, &p));
  check(fr, VSF_PIX_MONO8, 0, 32, true, max_gap, p);
  CHECK(p.raw && !p.files && !p.dev && p.big && p.big_files && p.big_dev && p.multi_size);
  CHECK(p.demosaic == kObserveStepNone && p.finish == kObserveAfterBigDecode);
  CHECK(p.runs.empty());  // (no own-size device frame: the device frames are waited for, none is copied)
  CHECK(p.resize.n_resized == 12 && p.resize.runs.size() == 12);  // (no two neighbours of one size: a launch per frame)
  // the four raw 640 x 480 frames lie three slots apart: the gaps are bridged, ONE upload of 13 slots
  CHECK(p.resize.uploads.size() == 1 && p.resize.uploads[0].f0 == 0 && p.resize.uploads[0].n == 13 && p.resize.uploads[0].slot0 == 0);
  // ... and the second batch, which wraps nothing at depth 32 but starts at slot 16
  CHECK(plan(fr, VSF_PIX_MONO8, 16, 32, true, max_gap, &p));
  check(fr, VSF_PIX_MONO8, 16, 32, true, max_gap, p);
  CHECK(p.resize.uploads.size() == 1 && p.resize.uploads[0].slot0 == 16 && p.resize.runs[1].src0 == 17);
}

// A batch that holds ONE class: every other class is empty, and so is every list that class has no part in.
static void fixed_one_class() {
  ObserveIngestPlan p;
  for (int big = 0; big < 2; big++)
    for (uint8_t kind : {kRaw, kPng, kDev})
      for (int pixfmt : {VSF_PIX_MONO8, VSF_PIX_BAYER_GBRG8}) {
        const std::vector<Frame> fr(3, Frame{kind, true, big ? 96 : 0, big ? 80 : 0});
        CHECK(plan(fr, pixfmt, 6, 8, true, 2, &p));  // (slots 6, 7, 0: the ring wraps inside the batch)
        check(fr, pixfmt, 6, 8, true, 2, p);
        CHECK(p.raw == (!big && kind == kRaw) && p.files == (!big && kind == kPng) && p.dev == (!big && kind == kDev));
        CHECK(p.big == (big != 0) && p.big_files == (big && kind == kPng) && p.big_dev == (big && kind == kDev) && !p.multi_size);
        CHECK(p.runs.size() == (!big && kind == kDev ? 2u : 0u));
        CHECK(p.resize.runs.size() == (!big ? 0u : kind == kDev ? 2u : 1u));  // (staged frames lie at their batch index: no wrap)
        CHECK(p.resize.uploads.size() == (big && kind == kRaw ? 2u : 0u));
        CHECK(p.own_pix_new == (pixfmt != VSF_PIX_MONO8 && !big ? 3 : 0));
        const bool bayer = pixfmt != VSF_PIX_MONO8;
        CHECK(p.demosaic == (!bayer || big ? kObserveStepNone
                                           : kind == kRaw ? kObserveAfterUpload
                                           : kind == kDev ? kObserveAfterDeviceCopies
                                                          : kObserveAfterDecode));
        CHECK(p.finish == (kind != kPng ? kObserveStepNone : big ? kObserveAfterBigDecode : kObserveAfterDecode));
      }
}

// A device frame of a declared size alone: its producer's event is waited for (big_dev), nothing is copied out of a ring (no
// run), one resize launch reads it where it lies.
static void fixed_declared_device_frame() {
  ObserveIngestPlan p;
  const std::vector<Frame> fr(1, Frame{kDev, false, 96, 80});
  CHECK(plan(fr, VSF_PIX_MONO8, 5, 4, true, 3, &p));
  check(fr, VSF_PIX_MONO8, 5, 4, true, 3, p);
  CHECK(p.big_dev && p.big && !p.dev && !p.raw && !p.files && !p.big_files && p.runs.empty() && p.resize.uploads.empty());
  CHECK(p.resize.runs.size() == 1 && p.resize.runs[0].where == kObserveInDeviceRing && p.resize.runs[0].src0 == 1);
  CHECK(p.cls[0] == kObserveBigDevice && p.demosaic == kObserveStepNone && p.finish == kObserveStepNone);
  // ... and before the queue has seen a big-slot frame the same record is an own-size device frame: one copy
  CHECK(plan(fr, VSF_PIX_MONO8, 5, 4, false, 0, &p));
  check(fr, VSF_PIX_MONO8, 5, 4, false, 0, p);
  CHECK(p.cls[0] == kObserveOwnDevice && p.dev && !p.big && p.runs.size() == 1 && p.runs[0].cls == kObserveRunDevice && p.resize.runs.empty());
}

static void refusals() {
  ObserveIngestPlan p;
  std::vector<Frame> fr(3, Frame{kRaw, false, 0, 0});
  CHECK(!plan(fr, VSF_PIX_MONO8, 0, 2, false, 0, &p));   // n > depth
  CHECK(!plan(fr, VSF_PIX_MONO8, -1, 4, false, 0, &p));  // t0 < 0
  CHECK(!plan(fr, VSF_PIX_MONO8, 0, 4, false, -1, &p));  // max_gap < 0
  CHECK(!plan(fr, 7, 0, 4, false, 0, &p));               // no pixel format
  fr[1].kind = 4;
  CHECK(!plan(fr, VSF_PIX_MONO8, 0, 4, false, 0, &p));   // no kind
  p.in.clear();
  CHECK(!observe_ingest_plan(3, VSF_PIX_MONO8, 0, 4, false, 0, &p));  // the caller filled nothing
  CHECK(!observe_ingest_plan(1, VSF_PIX_MONO8, 0, 4, false, 0, nullptr));
}

int main() {
  randomised();
  fixed_mixed_kinds();
  fixed_mixed_sizes();
  fixed_one_class();
  fixed_declared_device_frame();
  refusals();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok observe ingest plan: %ld randomised batches and the fixed cases\n", n_randomised);
  return 0;
}
