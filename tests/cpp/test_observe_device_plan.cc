// The slot arithmetic of device-resident frames in the ObserveImage queue (csrc/vsf_observe_plan.cc) on the CPU: compiled
// together with that file, plainly and under AddressSanitizer + UBSan (tests/test_observe_device_plan.py).
//   submit span   n consecutive frames into a ring of `depth` slots: refused unless 1 <= n <= depth - uncollected, else the
//                 slots [slot0, slot0 + first) and [0, second) -- against a frame-by-frame model, depths 1 .. 1024
//   batch runs    a batch's frames split into runs of raw / compressed / device frames that are contiguous in the ring:
//                 randomised kinds, every frame in exactly one run, runs in order, maximal, none across the ring's end
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

static void submit_spans() {
  long checked = 0;
  for (int di = 0; di < kDepths; di++) {
    const int depth = depth_of(di);
    for (int rep = 0; rep < 200; rep++) {
      // a queue somewhere in its life: tickets far beyond the first lap (and beyond 2^31) included
      const int uncollected = (int)(rnd() % (uint32_t)(depth + 1));
      const int64_t next_collect = (rep & 1) ? (int64_t)(rnd() % 5000u) : ((int64_t)1 << 33) + (int64_t)(rnd() % 5000u);
      const int64_t next_ticket = next_collect + uncollected;
      const int n = rep % 7 == 0 ? (int)(rnd() % 3u) - 1 + (rep % 14 == 0 ? depth - uncollected : 0)
                                 : 1 + (int)(rnd() % (uint32_t)(depth + 2));
      ObserveSpan sp{-1, -1, -1};
      const bool ok = observe_submit_span(next_ticket, next_collect, depth, n, &sp);
      const bool want = n >= 1 && n <= depth - uncollected;
      CHECK(ok == want);
      if (!ok) {
        CHECK(sp.slot0 == -1 && sp.first == -1 && sp.second == -1);  // a refusal writes nothing
        continue;
      }
      CHECK(sp.first >= 1 && sp.second >= 0 && sp.first + sp.second == n && sp.slot0 + sp.first <= depth);
      CHECK(sp.second == 0 || sp.slot0 + sp.first == depth);
      for (int f = 0; f < n; f++) {  // frame by frame
        const int slot = (int)((next_ticket + f) % depth);
        CHECK(slot == (f < sp.first ? sp.slot0 + f : f - sp.first));
        // ... and never a slot whose frame is still uncollected
        const int64_t back = (next_ticket + f) - depth;  // the ticket that used this slot last
        CHECK(back < next_collect);
      }
      checked++;
    }
  }
  CHECK(!observe_submit_span(0, 0, 0, 1, nullptr) && !observe_submit_span(0, 0, 4, 1, nullptr));
  ObserveSpan sp;
  CHECK(!observe_submit_span(3, 4, 4, 1, &sp));   // collected beyond issued
  CHECK(!observe_submit_span(-1, -1, 4, 1, &sp));
  CHECK(!observe_submit_span(0, 0, 1025, 1, &sp));
  CHECK(checked > 1000);
}

static int class_of(int kind) { return kind == 0 ? kObserveRunRaw : kind == kObserveKindDevice ? kObserveRunDevice : kObserveRunCompressed; }

static void batch_runs() {
  std::vector<uint8_t> kinds;
  std::vector<ObserveRun> runs;
  long wraps = 0, total = 0;
  for (int di = 0; di < kDepths; di++) {
    const int depth = depth_of(di);
    for (int rep = 0; rep < 150; rep++) {
      const int n = 1 + (int)(rnd() % (uint32_t)depth);
      const int64_t t0 = (rep & 1) ? (int64_t)(rnd() % 100000u) : ((int64_t)1 << 40) + (int64_t)(rnd() % 100000u);
      kinds.resize((size_t)n);
      const uint32_t flavour = rnd() % 4u;  // all one kind, long runs, short runs, anything
      for (int f = 0; f < n; f++) {
        if (flavour == 0)
          kinds[(size_t)f] = (uint8_t)(rep % 4);
        else if (f > 0 && flavour == 1 && rnd() % 8u)
          kinds[(size_t)f] = kinds[(size_t)f - 1];
        else
          kinds[(size_t)f] = (uint8_t)(rnd() % 4u);
      }
      CHECK(observe_batch_runs(kinds.data(), n, t0, depth, &runs));
      int f = 0;
      for (size_t r = 0; r < runs.size(); r++) {
        const ObserveRun& run = runs[r];
        CHECK(run.f0 == f && run.n >= 1 && run.f0 + run.n <= n);
        CHECK(run.slot0 == (int)((t0 + run.f0) % depth) && run.slot0 + run.n <= depth);
        for (int k = 0; k < run.n; k++) CHECK(class_of(kinds[(size_t)(run.f0 + k)]) == run.cls);
        if (r > 0) {  // maximal: a run ends where the class changes or the ring does
          const ObserveRun& prev = runs[r - 1];
          CHECK(prev.cls != run.cls || run.slot0 == 0);
          if (prev.cls == run.cls) wraps++;
        }
        f += run.n;
      }
      CHECK(f == n);
      // at most one wrap in a batch (n <= depth): runs <= class changes + 2
      int changes = 0;
      for (int k = 1; k < n; k++) changes += class_of(kinds[(size_t)k]) != class_of(kinds[(size_t)k - 1]);
      CHECK((int)runs.size() >= changes + 1 && (int)runs.size() <= changes + 2);
      total++;
    }
  }
  CHECK(wraps > 100 && total > 1000);
  // out of range: nothing is planned
  const uint8_t one[2] = {0, 9};
  CHECK(!observe_batch_runs(one, 2, 0, 4, &runs));      // an unknown kind
  CHECK(!observe_batch_runs(one, 1, 0, 0, &runs));      // no ring
  CHECK(!observe_batch_runs(one, 0, 0, 4, &runs));      // no frame
  CHECK(!observe_batch_runs(one, 1, -1, 4, &runs));     // no ticket
  CHECK(!observe_batch_runs(nullptr, 1, 0, 4, &runs));
  const uint8_t five[5] = {3, 3, 3, 3, 3};
  CHECK(!observe_batch_runs(five, 5, 0, 4, &runs));     // more frames than slots
  // depth 4, 4 device frames from ticket 6: slots 2 3 | 0 1
  CHECK(observe_batch_runs(five, 4, 6, 4, &runs) && runs.size() == 2);
  CHECK(runs[0].slot0 == 2 && runs[0].n == 2 && runs[1].slot0 == 0 && runs[1].n == 2 && runs[1].f0 == 2);
}

int main() {
  submit_spans();
  batch_runs();
  if (failures) return 1;
  std::printf("ok observe device plan\n");
  return 0;
}
