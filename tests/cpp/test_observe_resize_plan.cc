// The arithmetic of the ObserveImage queue's declared input sizes (vsf_observe_plan.cc: the big slots' layout, the runs one
// resize launch takes, the raw frames' upload span) and k_resize.hip's span rule (vsf_resize.h) as a stand-alone program on the
// CPU; tests/test_resize_plan.py builds it plainly and under AddressSanitizer + UBSan.  Every source address a resize launch
// would form is checked against the buffers' sizes for random batches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_observe_plan.h"
#include "../../vision_slam_frontend_amd/csrc/vsf_resize.h"

using namespace vsfi;

static int checks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    checks++;                                                     \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % n;
}

int main() {
  // ---- layout ----
  CHECK(observe_input_pitch(0) == 0 && observe_input_pitch(32768) == 0 && observe_input_pitch(1) == 64 && observe_input_pitch(64) == 64);
  CHECK(observe_input_pitch(65) == 128 && observe_input_pitch(1280) == 1280 && observe_input_pitch(32767) == 32768);
  CHECK(observe_input_image_bytes(1280, 960) == 1280u * 960u && observe_input_image_bytes(641, 481) == ((704u * 481u + 255u) & ~255u));
  CHECK(observe_input_image_bytes(0, 5) == 0 && observe_input_image_bytes(5, 32768) == 0);
  CHECK(observe_input_image_bytes(32767, 32767) == (size_t)32768 * 32767 + 0);  // (a multiple of 256 already; no overflow)
  {
    int w[4] = {0, 640, 0, 200}, h[4] = {0, 480, 0, 150};
    CHECK(observe_input_half_bytes(w, h, 4) == 640u * 480u);
    CHECK(observe_input_half_bytes(w, h, 1) == 0);  // (only stream 0 counts: none declared)
    w[2] = 960, h[2] = 720;
    CHECK(observe_input_half_bytes(w, h, 4) == 960u * 720u);
    CHECK(observe_input_half_bytes(w, h, 0) == 0 && observe_input_half_bytes(nullptr, h, 4) == 0);
    w[0] = 5, h[0] = 0;  // (a half-declared size is no size)
    CHECK(observe_input_image_bytes(5, 0) == 0 && observe_input_half_bytes(w, h, 4) == 960u * 720u);
    CHECK(observe_input_ring_bytes(256, 1280u * 960u) == (size_t)256 * 2 * 1280 * 960);
    CHECK(observe_input_ring_bytes(0, 64) == 0 && observe_input_ring_bytes(1025, 64) == 0 && observe_input_ring_bytes(4, 0) == 0);
  }
  // ---- runs ----
  ObserveResizePlan p;
  {
    // depth 8, t0 = 5: slots 5 6 7 0 1 2.  raw big | raw big | dev big | dev big (wraps at slot 0) | plain raw | png small-big
    const ObserveResizeIn in[6] = {{640, 480, 0}, {640, 480, 0}, {640, 480, 3}, {640, 480, 3}, {0, 0, 0}, {200, 150, 2}};
    CHECK(observe_resize_plan(in, 6, 5, 8, 0, &p));
    CHECK(p.runs.size() == 4 && p.n_resized == 5);
    CHECK(p.runs[0].where == kObserveInStaged && p.runs[0].f0 == 0 && p.runs[0].n == 2 && p.runs[0].src0 == 0);
    CHECK(p.runs[1].where == kObserveInDeviceRing && p.runs[1].f0 == 2 && p.runs[1].n == 1 && p.runs[1].src0 == 7);
    CHECK(p.runs[2].where == kObserveInDeviceRing && p.runs[2].f0 == 3 && p.runs[2].n == 1 && p.runs[2].src0 == 0);
    CHECK(p.runs[3].where == kObserveInStaged && p.runs[3].f0 == 5 && p.runs[3].n == 1 && p.runs[3].w == 200 && p.runs[3].h == 150);
    CHECK(p.uploads.size() == 1 && p.uploads[0].f0 == 0 && p.uploads[0].n == 2 && p.uploads[0].slot0 == 5);
  }
  {
    // the raw frames' span wraps the pinned ring; a raw and a compressed frame of one size share a run (both staged)
    const ObserveResizeIn in[4] = {{0, 0, 0}, {640, 480, 0}, {640, 480, 1}, {640, 480, 0}};
    CHECK(observe_resize_plan(in, 4, 6, 8, 1, &p));
    CHECK(p.runs.size() == 1 && p.runs[0].f0 == 1 && p.runs[0].n == 3 && p.runs[0].src0 == 1);
    // frame 1 in slot 7, frame 3 in slot 1: the gap of one could be bridged, but the ring wraps in it
    CHECK(p.uploads.size() == 2 && p.uploads[0].f0 == 1 && p.uploads[0].n == 1 && p.uploads[0].slot0 == 7);
    CHECK(p.uploads[1].f0 == 3 && p.uploads[1].n == 1 && p.uploads[1].slot0 == 1);
    // the same frames from ticket 0: one upload with the gap bridged, two without
    CHECK(observe_resize_plan(in, 4, 0, 8, 1, &p) && p.uploads.size() == 1 && p.uploads[0].f0 == 1 && p.uploads[0].n == 3 && p.uploads[0].slot0 == 1);
    CHECK(observe_resize_plan(in, 4, 0, 8, 0, &p) && p.uploads.size() == 2 && !observe_resize_plan(in, 4, 0, 8, -1, &p));
    // what a copy command's fixed cost is worth in slots: 9 MB over the slot
    CHECK(observe_upload_max_gap(2u * 1280u * 960u) == 3 && observe_upload_max_gap(2u * 256u * 150u) == 117 && observe_upload_max_gap(0) == 0);
    CHECK(observe_upload_max_gap(64) == 1024 && observe_upload_max_gap((size_t)20 << 20) == 0);
    const ObserveResizeIn none[2] = {{0, 0, 0}, {0, 0, 3}};
    CHECK(observe_resize_plan(none, 2, 0, 8, 3, &p) && p.runs.empty() && p.uploads.empty() && p.n_resized == 0);
    const ObserveResizeIn bad[1] = {{640, 0, 0}}, kind[1] = {{640, 480, 4}};
    CHECK(!observe_resize_plan(bad, 1, 0, 8, 0, &p) && !observe_resize_plan(kind, 1, 0, 8, 0, &p));
    CHECK(!observe_resize_plan(in, 4, 0, 3, 0, &p) && !observe_resize_plan(in, 0, 0, 8, 0, &p) && !observe_resize_plan(nullptr, 1, 0, 8, 0, &p));
    CHECK(!observe_resize_plan(in, 4, -1, 8, 0, &p));
  }
  // ---- random batches: every frame in exactly one run, every address a launch forms inside its buffer ----
  const int sizes[4][2] = {{640, 480}, {641, 481}, {200, 150}, {1280, 960}};
  for (int trial = 0; trial < 2000; trial++) {
    const int depth = 1 + (int)rnd(40), n = 1 + (int)rnd((uint32_t)depth), bmax = n;
    const int64_t t0 = (int64_t)rnd(1000);
    std::vector<ObserveResizeIn> in((size_t)n);
    int in_w[4], in_h[4];
    for (int s = 0; s < 4; s++) in_w[s] = sizes[s][0], in_h[s] = sizes[s][1];
    const size_t half = observe_input_half_bytes(in_w, in_h, 4), slot = 2 * half;
    for (ObserveResizeIn& w : in) {
      const int s = (int)rnd(6);
      w = s < 4 ? ObserveResizeIn{sizes[s][0], sizes[s][1], (uint8_t)rnd(4)} : ObserveResizeIn{0, 0, (uint8_t)rnd(4)};
    }
    const int max_gap = (int)rnd(5);
    CHECK(observe_resize_plan(in.data(), n, t0, depth, max_gap, &p));
    std::vector<int> covered((size_t)n, 0);
    for (const ObserveResizeRun& r : p.runs) {
      CHECK(r.n >= 1 && r.f0 >= 0 && r.f0 + r.n <= n);
      const size_t cap = (r.where == kObserveInDeviceRing ? (size_t)depth : (size_t)bmax) * slot;
      // the run's last image: base + (2 n - 1) half, its last row's last pixel
      const size_t last = (size_t)r.src0 * slot + (size_t)(2 * r.n - 1) * half + (size_t)(r.h - 1) * observe_input_pitch(r.w) + (size_t)r.w;
      CHECK(last <= cap);
      for (int f = r.f0; f < r.f0 + r.n; f++) {
        covered[(size_t)f]++;
        CHECK(in[(size_t)f].w == r.w && in[(size_t)f].h == r.h);
        CHECK((in[(size_t)f].kind == kObserveKindDevice) == (r.where == kObserveInDeviceRing));
        CHECK(r.where == kObserveInDeviceRing ? (r.src0 + (f - r.f0)) == (int)((t0 + f) % depth) : r.src0 + (f - r.f0) == f);
      }
    }
    int resized = 0;
    for (int f = 0; f < n; f++) {
      CHECK(covered[(size_t)f] == (in[(size_t)f].w != 0 ? 1 : 0));
      resized += in[(size_t)f].w != 0;
      if (in[(size_t)f].w != 0 && in[(size_t)f].kind == 0) {  // a raw resized frame lies inside exactly one upload, at its ring slot
        int inside = 0;
        for (const ObserveUpload& u : p.uploads)
          if (f >= u.f0 && f < u.f0 + u.n) {
            inside++;
            CHECK(u.slot0 + (f - u.f0) == (int)((t0 + f) % depth));
          }
        CHECK(inside == 1);
      }
    }
    CHECK(resized == p.n_resized);
    int prev_end = -1;
    for (const ObserveUpload& u : p.uploads) {  // in order, apart, inside the ring and the batch; ends are raw resized frames;
      CHECK(u.n >= 1 && u.f0 > prev_end && u.f0 + u.n <= n && u.slot0 >= 0 && u.slot0 + u.n <= depth);  // gaps inside <= max_gap
      const auto raw = [&](int f) { return in[(size_t)f].w != 0 && in[(size_t)f].kind == 0; };
      CHECK(raw(u.f0) && raw(u.f0 + u.n - 1));
      int gap = 0;
      for (int f = u.f0; f < u.f0 + u.n; f++) {
        gap = raw(f) ? 0 : gap + 1;
        CHECK(gap <= max_gap);
      }
      prev_end = u.f0 + u.n - 1;
    }
  }
  // ---- k_resize.hip's span rule: every tap of a wave's columns lies inside the window the launch sizes ----
  const int pairs[][2] = {{128, 64}, {129, 64}, {192, 64}, {512, 64}, {100, 64}, {40, 64}, {64, 64}, {131, 61}, {7, 3}, {7, 1},
                          {1300, 520}, {2600, 520}, {10400, 260}, {130, 523}, {1280, 640}, {1920, 640}, {32767, 1}, {1, 32767}};
  for (const auto& pr : pairs) {
    const int sw = pr[0], dw = pr[1], need = resize_span_dwords(sw, dw);
    const double scale = 1. / ((double)dw / sw);
    for (int xb = 0; xb < dw; xb += 256) {
      const int xe = xb + 255 < dw - 1 ? xb + 255 : dw - 1;
      const int lo = resize_xtap(xb, scale, sw).i0, hi = resize_xtap(xe, scale, sw).i1;
      for (int x = xb; x <= xe; x++) {
        const VsfTap t = resize_xtap(x, scale, sw);
        CHECK(t.i0 >= lo && t.i1 <= hi && t.i1 < sw && t.i0 <= t.i1);
        CHECK((t.i1 - lo) + 3 < 4 * need);  // (the byte index in the window at the largest skew)
      }
    }
  }
  CHECK(resize_span_dwords(1280, 640) <= 64 * 3 && resize_span_dwords(1920, 640) <= 64 * 10 && resize_span_dwords(1920, 640) > 64 * 3);
  std::printf("ok %d checks\n", checks);
  return 0;
}
