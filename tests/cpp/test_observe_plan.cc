// The arithmetic of one batch of the ObserveImage queue (csrc/vsf_observe_plan.cc) on the CPU: compiled together with that
// file, plainly and under AddressSanitizer + UBSan (tests/test_observe_plan.py).
//   one stream      the closed forms the queue used before it had streams: frame g in set g % ring, right frames behind the
//                   ring, min(g, life) temporal pairs oldest first behind the batch's right -> left pairs
//   several streams every stream against a model of its own (a deque of the sets its kept frames went to), rings that wrap,
//                   frame_life 1 and the largest value the ring allows; no two live frames ever share a set
//   calibrations    duplicates collapse, distinct ones are kept in order of first use, every frame's index names its own
//   cuts            at a change inside a stream and nowhere else; the chain links (prev / tail) of the threshold kernel
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <set>
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

static vsf_calibration calibration(float tag) {
  vsf_calibration c;
  std::memset(&c, 0, sizeof(c));
  c.fundamental[5] = -1.f;
  c.fundamental[7] = 1.f;
  c.fundamental[8] = tag;
  c.projection_right[3] = -tag;
  return c;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// One stream: batches of every size cut out of one long sequence, against the closed forms.
static void one_stream() {
  const vsf_calibration c = calibration(0.f);
  for (int life : {0, 1, 3, 10})
    for (int bmax : {1, 4, 7}) {
      const int ring = life + bmax;
      ObservePlan plan;
      int64_t g0 = 0;
      while (g0 < 5 * ring + 3) {
        const int n = 1 + (int)(rnd() % (uint32_t)bmax);
        std::vector<ObservePlanIn> in;
        for (int f = 0; f < n; f++) in.push_back({0, g0 + f, &c, 0.3f});
        CHECK(observe_plan(in.data(), n, 1, ring, life, &plan));
        CHECK((int)plan.frames.size() == n && plan.cuts.empty() && plan.calibs.size() == 1 && plan.n_streams_present == 1);
        int n_pairs = n, widest = 1;
        for (int f = 0; f < n; f++) {
          const int64_t g = g0 + f;
          const int n_past = (int)(g < life ? g : life), left = (int)(g % ring), right = ring + f;
          const ObservePlanFrame& pf = plan.frames[(size_t)f];
          CHECK(pf.left_set == left && pf.right_set == right && pf.n_past == n_past && pf.tp0 == n_pairs);
          CHECK(pf.stream == 0 && pf.calib == 0 && pf.best_percent == 0.3f);
          CHECK(pf.prev == f - 1 && pf.tail == (f == 0 ? n - 1 : -1));
          CHECK(plan.q_set[(size_t)f] == right && plan.t_set[(size_t)f] == left && plan.best_percent[(size_t)f] == 1.0f);
          for (int p = 0; p < n_past; p++) {
            CHECK(plan.q_set[(size_t)n_pairs] == (int)((g - n_past + p) % ring));
            CHECK(plan.t_set[(size_t)n_pairs] == left && plan.best_percent[(size_t)n_pairs] == 0.3f);
            n_pairs++;
          }
          if (n_past + 1 > widest) widest = n_past + 1;
        }
        CHECK(plan.n_pairs == n_pairs && (int)plan.q_set.size() == n_pairs && plan.max_pairs_per_frame == widest);
        g0 += n;
      }
    }
}

// Several streams in random interleavings: a model per stream.
static void several_streams(int n_streams, int life, int bmax) {
  const int ring = life + bmax;
  std::vector<vsf_calibration> cal;
  for (int s = 0; s < n_streams; s++) cal.push_back(calibration((float)(s % 3)));  // three distinct ones, shared
  std::vector<int64_t> count((size_t)n_streams, 0);
  std::vector<std::deque<int>> window((size_t)n_streams);  // the sets of the stream's kept frames, oldest first
  ObservePlan plan;
  for (int batch = 0; batch < 60; batch++) {
    const int n = 1 + (int)(rnd() % (uint32_t)bmax);
    std::vector<ObservePlanIn> in;
    std::vector<int64_t> seen = count;
    for (int f = 0; f < n; f++) {
      // (runs of one stream, streams that start late: the low streams come far more often)
      const int s = (int)(rnd() % (uint32_t)(1 + rnd() % (uint32_t)n_streams));
      in.push_back({s, seen[(size_t)s]++, &cal[(size_t)s], 0.25f + 0.125f * (float)(s % 2)});
    }
    CHECK(observe_plan(in.data(), n, n_streams, ring, life, &plan));
    CHECK(plan.cuts.empty());
    std::set<int> present;
    std::map<int, int> last;
    std::set<int> written;
    int n_pairs = n;
    for (int f = 0; f < n; f++) {
      const int s = in[(size_t)f].stream;
      const ObservePlanFrame& pf = plan.frames[(size_t)f];
      std::deque<int>& w = window[(size_t)s];
      CHECK(pf.stream == s && pf.left_set >= s * ring && pf.left_set < (s + 1) * ring);
      CHECK(pf.left_set == s * ring + (int)(in[(size_t)f].k % ring));
      CHECK(pf.right_set == n_streams * ring + f);
      CHECK(pf.n_past == (int)w.size() && pf.tp0 == n_pairs);
      for (int set : w) CHECK(set != pf.left_set);  // a kept frame is never overwritten while it is still matched against
      for (size_t p = 0; p < w.size(); p++) {
        CHECK(plan.q_set[(size_t)n_pairs] == w[p] && plan.t_set[(size_t)n_pairs] == pf.left_set);
        CHECK(plan.best_percent[(size_t)n_pairs] == in[(size_t)f].best_percent);
        n_pairs++;
      }
      CHECK(plan.q_set[(size_t)f] == pf.right_set && plan.t_set[(size_t)f] == pf.left_set && plan.best_percent[(size_t)f] == 1.0f);
      CHECK(std::memcmp(&plan.calibs[(size_t)pf.calib], &cal[(size_t)s], sizeof(vsf_calibration)) == 0);
      CHECK(pf.prev == (last.count(s) ? last[s] : -1));
      last[s] = f;
      present.insert(s);
      CHECK(written.insert(pf.left_set).second);  // no two frames of a batch share a set
      w.push_back(pf.left_set);
      if ((int)w.size() > life) w.pop_front();
    }
    // a batch's writes never hit a set that a frame of ANOTHER position in the batch still reads as an older frame's
    for (int f = 0; f < n; f++) {
      const ObservePlanFrame& pf = plan.frames[(size_t)f];
      for (int p = 0; p < pf.n_past; p++) {
        const int q = plan.q_set[(size_t)(pf.tp0 + p)];
        if (written.count(q)) {  // written by this batch: then by an EARLIER frame of the same stream
          bool earlier = false;
          for (int e = 0; e < f; e++) earlier |= plan.frames[(size_t)e].left_set == q && plan.frames[(size_t)e].stream == pf.stream;
          CHECK(earlier);
        }
      }
      CHECK(pf.tail == (pf.prev < 0 ? last[pf.stream] : -1));
    }
    CHECK(plan.n_pairs == n_pairs && plan.n_streams_present == (int)present.size());
    std::set<int> tags;
    for (int s : present) tags.insert(s % 3);
    CHECK(plan.calibs.size() == tags.size());
    count = seen;
  }
}

static void calibration_table_and_cuts() {
  const vsf_calibration a = calibration(0.f), a2 = calibration(0.f), b = calibration(1.5f), c = calibration(2.f);
  ObservePlan plan;
  {  // duplicates (equal bytes at different addresses) collapse; distinct ones in order of first use
    const ObservePlanIn in[] = {{0, 0, &b, .3f}, {1, 0, &a, .3f}, {2, 0, &a2, .6f}, {0, 1, &b, .3f}, {3, 0, &c, .3f}, {1, 1, &a2, .3f}};
    CHECK(observe_plan(in, 6, 4, 8, 2, &plan));
    CHECK(plan.calibs.size() == 3 && plan.cuts.empty() && plan.n_streams_present == 4);
    CHECK(std::memcmp(&plan.calibs[0], &b, sizeof(b)) == 0 && std::memcmp(&plan.calibs[1], &a, sizeof(a)) == 0 &&
          std::memcmp(&plan.calibs[2], &c, sizeof(c)) == 0);
    const int want[] = {0, 1, 1, 0, 2, 1};
    for (int f = 0; f < 6; f++) CHECK(plan.frames[(size_t)f].calib == want[f]);
  }
  {  // frames of different streams differ in both parameters and share the batch; a change inside a stream cuts
    const ObservePlanIn in[] = {{0, 5, &a, .3f}, {1, 2, &b, .6f}, {0, 6, &a, .3f}, {1, 3, &c, .6f},   // stream 1: calibration
                                {0, 7, &a, .5f}, {1, 4, &c, .6f}, {2, 0, &b, .1f}, {0, 8, &a2, .5f}};  // stream 0: best_percent
    CHECK(observe_plan(in, 8, 3, 12, 3, &plan));
    CHECK(plan.cuts.size() == 2 && plan.cuts[0] == 3 && plan.cuts[1] == 4);
  }
  {  // one stream: the rule the queue had before (every change cuts)
    const ObservePlanIn in[] = {{0, 0, &a, .3f}, {0, 1, &a, .3f}, {0, 2, &b, .3f}, {0, 3, &b, .3f}, {0, 4, &b, .6f}};
    CHECK(observe_plan(in, 5, 1, 9, 3, &plan));
    CHECK(plan.cuts.size() == 2 && plan.cuts[0] == 2 && plan.cuts[1] == 4);
  }
  CHECK(observe_plan_must_cut(a, .3f, a2, .3f) == false && observe_plan_must_cut(a, .3f, a2, .31f) && observe_plan_must_cut(a, .3f, b, .3f));
  {  // refusals: a stream out of range, a frame out of order, a ring too small, no frames
    const ObservePlanIn bad_stream[] = {{2, 0, &a, .3f}}, neg[] = {{-1, 0, &a, .3f}}, order[] = {{0, 3, &a, .3f}, {0, 5, &a, .3f}},
                        one[] = {{0, 0, &a, .3f}}, nocal[] = {{0, 0, nullptr, .3f}};
    CHECK(!observe_plan(bad_stream, 1, 2, 8, 2, &plan) && !observe_plan(neg, 1, 2, 8, 2, &plan));
    CHECK(!observe_plan(order, 2, 1, 8, 2, &plan) && !observe_plan(nocal, 1, 1, 8, 2, &plan));
    CHECK(!observe_plan(one, 1, 1, 2, 2, &plan) && !observe_plan(one, 0, 1, 8, 2, &plan) && !observe_plan(one, 1, 0, 8, 2, &plan));
    CHECK(!observe_plan(one, 1, VSF_OBSERVE_MAX_STREAMS + 1, 8, 2, &plan) && observe_plan(one, 1, VSF_OBSERVE_MAX_STREAMS, 8, 2, &plan));
  }
}

int main() {
  one_stream();
  several_streams(3, 1, 4);
  several_streams(3, 2, 8);
  several_streams(5, 1, 1);
  several_streams(64, 63, 5);  // frame_life + 1 = VSF_OBSERVE_MAX_PAIRS: the largest window the queue takes
  several_streams(3, 63, 1);   // ... on the tightest ring (one frame per batch: ring = frame_life + 1)
  several_streams(7, 4, 32);
  calibration_table_and_cuts();
  if (failures) return 1;
  std::printf("ok observe plan\n");
  return 0;
}
