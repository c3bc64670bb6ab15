// The CPU oracle at the narrowest borders the C ABI accepts, as a stand-alone program for AddressSanitizer / UBSan
// (tests/test_oracle_border.py compiles it together with oracle/vsf_oracle.cc): the oracle does not materialise the borders
// of its levels, its comment argues for edgeThreshold 31 only, and the GPU tests at 22 .. 25 hold the kernels against it --
// so every read of Harris (reach 4), ICAngles (15) and the rotated pattern on the blurred level (19 + 3) must stay inside the
// level's own std::vector at 22 as well.  Levels and images live in exactly sized heap blocks: a read past a level is a
// heap-buffer-overflow report, not a neighbour's byte.
//
// Cases: uniform noise at 320x240, 203x151 and 515x322 (50 levels x 1.04, nfeatures 3000, FAST threshold 20 and 0), borders
// 22 and 25: keypoints on the border line of a level on all four sides; 45x45 (8 levels x 1.2, border 22): the one admissible
// pixel, as a dot and in noise -- IC angle, Harris and the descriptor's window at their closest to all four edges at once;
// 44x44: nothing admissible, zero keypoints.  Exit status 0 and a line "ok ..." when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../oracle/vsf_oracle.h"

static int fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (fails++ < 20) {                \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

struct Run {
  int total = 0, levels_used = 0;
  bool left = false, right = false, top = false, bottom = false;  // a keypoint on that border line of some level
  std::vector<vsfo_keypoint> kps;
};

static std::unique_ptr<uint8_t[]> noise(int w, int h, uint32_t seed) {
  std::unique_ptr<uint8_t[]> img(new uint8_t[(size_t)w * h]);  // exactly w * h bytes
  uint32_t s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < (size_t)w * h; i++) {
    s = s * 1664525u + 1013904223u;
    img[i] = (uint8_t)(s >> 24);
  }
  return img;
}

static Run run(const uint8_t* img, int w, int h, int border, int nfeatures, int nlevels, float scale, int fast_threshold) {
  vsfo_orb_params p;
  vsfo_orb_params_default(&p);
  p.edge_threshold = border;
  p.nfeatures = nfeatures;
  p.nlevels = nlevels;
  p.scale_factor = scale;
  p.fast_threshold = fast_threshold;
  vsfo_orb* o = vsfo_orb_create(&p);
  Run r;
  r.total = vsfo_orb_run(o, img, w, h, (size_t)w);
  CHECK(r.total >= 0, "%dx%d border %d: vsfo_orb_run %d", w, h, border, r.total);
  if (r.total < 0) {
    vsfo_orb_destroy(o);
    r.total = 0;
    return r;
  }
  for (int l = 0; l < vsfo_orb_nlevels(o); l++) {
    int lw, lh, nf;
    float sc;
    vsfo_orb_level_info(o, l, &lw, &lh, &sc, &nf);
    const int n = vsfo_orb_stage_keypoints(o, 4, l, nullptr, 0);
    std::vector<vsfo_keypoint> k((size_t)n + 1);
    vsfo_orb_stage_keypoints(o, 4, l, k.data(), n);
    r.levels_used += n > 0;
    CHECK(n == 0 || (lw > 2 * border && lh > 2 * border), "%dx%d border %d: level %d (%dx%d) should be empty", w, h, border, l, lw, lh);
    for (int i = 0; i < n; i++) {
      const int x = (int)std::lrintf(k[i].x), y = (int)std::lrintf(k[i].y);
      CHECK(x >= border && x < lw - border && y >= border && y < lh - border, "%dx%d border %d level %d: keypoint (%d, %d)", w, h,
            border, l, x, y);
      r.left |= x == border, r.right |= x == lw - border - 1, r.top |= y == border, r.bottom |= y == lh - border - 1;
    }
  }
  r.kps.resize((size_t)r.total + 1);
  std::vector<uint8_t> desc(((size_t)r.total + 1) * 32);
  CHECK(vsfo_orb_result(o, r.kps.data(), desc.data(), r.total) == r.total, "%dx%d border %d: vsfo_orb_result", w, h, border);
  r.kps.resize((size_t)r.total);
  vsfo_orb_destroy(o);
  return r;
}

int main() {
  int runs = 0;
  long kept = 0;
  const int sizes[3][2] = {{320, 240}, {203, 151}, {515, 322}};
  for (const auto& sz : sizes)
    for (int border : {22, 25})
      for (int thr : {20, 0}) {
        const int w = sz[0], h = sz[1];
        const std::unique_ptr<uint8_t[]> img = noise(w, h, (uint32_t)(w + border + thr));
        const Run r = run(img.get(), w, h, border, 3000, 50, 1.04f, thr);
        CHECK(r.total > 500, "%dx%d border %d threshold %d: %d keypoints", w, h, border, thr, r.total);
        CHECK(r.left && r.right && r.top && r.bottom, "%dx%d border %d threshold %d: no keypoint on a border line (%d %d %d %d)", w, h,
              border, thr, r.left, r.right, r.top, r.bottom);
        runs++, kept += r.total;
      }
  {
    // the one admissible pixel of a 45x45 image: (22, 22) of level 0; every other level is empty
    std::unique_ptr<uint8_t[]> dot(new uint8_t[45 * 45]);
    for (int i = 0; i < 45 * 45; i++) dot[i] = 30;
    dot[22 * 45 + 22] = 220;
    const Run d = run(dot.get(), 45, 45, 22, 500, 8, 1.2f, 20);
    CHECK(d.total == 1 && d.levels_used == 1, "dot: %d keypoints on %d levels", d.total, d.levels_used);
    if (d.total == 1) CHECK(d.kps[0].x == 22.f && d.kps[0].y == 22.f && d.kps[0].octave == 0, "dot at (%g, %g)", d.kps[0].x, d.kps[0].y);
    int found = 0;
    for (uint32_t seed = 1; seed <= 40; seed++) {  // (the centre must be a strict local maximum of FAST's score: some seeds give none)
      const std::unique_ptr<uint8_t[]> img = noise(45, 45, seed);
      const Run r = run(img.get(), 45, 45, 22, 500, 8, 1.2f, 20);
      CHECK(r.total <= 1, "45x45 noise %u: %d keypoints", seed, r.total);
      if (r.total == 1) CHECK(r.kps[0].x == 22.f && r.kps[0].y == 22.f, "45x45 noise %u at (%g, %g)", seed, r.kps[0].x, r.kps[0].y);
      found += r.total;
      runs++;
    }
    CHECK(found >= 1, "45x45 noise: none of 40 images gave a keypoint");
    const std::unique_ptr<uint8_t[]> none = noise(44, 44, 5);
    const Run z = run(none.get(), 44, 44, 22, 500, 8, 1.2f, 0);
    CHECK(z.total == 0 && z.levels_used == 0, "44x44: %d keypoints", z.total);
    runs += 2, kept += d.total + found;
    // below the reach the oracle refuses to run (it would read outside its levels)
    vsfo_orb_params p;
    vsfo_orb_params_default(&p);
    p.edge_threshold = 21;
    vsfo_orb* o = vsfo_orb_create(&p);
    CHECK(vsfo_orb_run(o, none.get(), 44, 44, 44) == -1, "edge_threshold 21 is not refused");
    vsfo_orb_destroy(o);
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok %d runs, %ld keypoints\n", runs, kept);
  return 0;
}
