// The host threads of the ObserveImage queue (csrc/vsf_observe_queue.cc) on the CPU, with a fake GPU: compiled together with
// that file plainly, under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_observe_queue.py).
//   policy       batch_to_launch against an independent spelling of its four rules, exhaustively over small queues; the
//                GPU is not asked where the answer does not depend on it
//   copy helper  100 000 posts with pauses around its idle limit (a few microseconds here), so that thousands of them meet
//                it on its way to sleep: a posted job is always served; destroyed hot, asleep and unused
//   launcher     a caller that submits, and collects the oldest frame when the queue is full, with and without the launcher
//                thread: the batches tile the tickets in order, one launch at a time, a collected frame has left, drain
//                leaves nothing behind, a lone frame leaves by itself, a failed launch is sticky, stop joins, and a reader of
//                the statistics never sees one decrease.  The fake keeps its records WITHOUT a lock of its own: the baton
//                is what orders them, and ThreadSanitizer says so if it does not.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <thread>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_observe_queue.h"

using namespace vsfi;

static std::atomic<int> failures{0};
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      if (++failures > 20) std::exit(1);                           \
    }                                                              \
  } while (0)

static void spin_ns(int64_t ns) {
  for (const int64_t end = now_ns() + ns; now_ns() < end;) __builtin_ia32_pause();
}

struct Lcg {
  uint32_t s;
  uint32_t operator()() {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
  }
};

// ---- policy ----
static int busy_asked = 0, busy_value = 0;

static int policy_model(int pending, int depth, int bmax, int busy, int in_flight, int configured, int64_t quiet_ns, bool force) {
  if (pending == 0) return 0;
  if (force || pending >= bmax) return pending < bmax ? pending : bmax;  // forced, or a full batch
  int min_batch = configured > 0 ? configured : depth / 2;
  if (min_batch > bmax) min_batch = bmax;
  if (min_batch < 1) min_batch = 1;
  if (busy < in_flight && pending >= min_batch) return pending;  // busy below in_flight and min_batch waiting
  if (busy == 0 && quiet_ns > 100000) return pending;            // idle and quiet
  return 0;
}

static void policy() {
  const ObserveGpu gpu{nullptr, nullptr, [](void*) { return busy_asked++, busy_value; }, nullptr};
  long cases = 0;
  for (int depth = 1; depth <= 9; depth++)
    for (int bmax = 1; bmax <= depth; bmax++)
      for (int pending = 0; pending <= depth; pending++)
        for (int busy = 0; busy <= 3; busy++)
          for (int in_flight = 1; in_flight <= 3; in_flight++)
            for (int configured = 0; configured <= bmax + 1; configured++)
              for (int64_t quiet : {0, 100000, 100001})
                for (int force = 0; force < 2; force++, cases++) {
                  busy_asked = 0;
                  busy_value = busy;
                  const int got = batch_to_launch(pending, {depth, bmax, configured, in_flight}, force != 0, quiet, gpu);
                  CHECK(got == policy_model(pending, depth, bmax, busy, in_flight, configured, quiet, force != 0));
                  CHECK(busy_asked == (pending == 0 || force || pending >= bmax ? 0 : 1));
                }
  std::printf("policy: %ld cases\n", cases);
}

// ---- copy helper ----
static void copy_helper() {
  const std::chrono::microseconds idle(4);
  const int rows = 3, width = 64, src_pitch = 64, posts = 100000;
  std::vector<uint8_t> src((size_t)rows * src_pitch), dst((size_t)rows * 80);
  Lcg rnd{777u};
  int helped = 0;
  {
    ObserveCopyHelper h(idle);
    for (int i = 0; i < posts; i++) {
      for (size_t k = 0; k < src.size(); k++) src[k] = (uint8_t)(i * 31 + (int)k * 7 + (i >> 8));
      const size_t dst_pitch = i & 1 ? 80 : 64;
      std::memset(dst.data(), 0, dst.size());
      const ObserveCopyHelper::Job j{dst.data(), src.data(), dst_pitch, (size_t)src_pitch, (size_t)width, rows};
      if (h.post(j)) {
        h.wait();
        helped++;
      } else {
        stage_image(j.dst, j.dst_pitch, j.src, j.src_pitch, j.width, j.rows);
      }
      bool same = true;
      for (int y = 0; y < rows; y++) same &= std::memcmp(&dst[(size_t)y * dst_pitch], &src[(size_t)y * src_pitch], width) == 0;
      CHECK(same);
      spin_ns((int64_t)(rnd() % 16001u));  // 0 .. 4 idle limits
    }
  }
  CHECK(helped >= 1000 && helped <= posts - 1000);  // both branches of post() were taken, often
  uint8_t a[64] = {1, 2, 3}, b[64] = {0};
  const ObserveCopyHelper::Job j{b, a, 64, 64, 64, 1};
  {  // hot
    ObserveCopyHelper h(std::chrono::seconds(10));
    while (!h.post(j)) std::this_thread::yield();
    h.wait();
    CHECK(h.hot.load() && std::memcmp(a, b, 64) == 0);
  }
  {  // asleep
    ObserveCopyHelper h(idle);
    while (!h.post(j)) std::this_thread::yield();
    h.wait();
    while (h.hot.load()) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
  }
  { ObserveCopyHelper h(idle); }  // never had a job
  std::printf("copy helper: %d posts, %d taken by the helper\n", posts, helped);
}

// ---- launcher ----
struct FakeGpu {
  struct Batch {
    int64_t t0;
    int n;
    bool solo;
    int rows_hint;
    int64_t end_ns;
  };
  ObserveQueue* q = nullptr;
  std::vector<Batch> batches;  // (no lock: written inside launch, read by busy -- never at the same time, says the baton)
  std::atomic<bool> inside{false};
  Lcg rnd{4242u};
  int fail_at = -1;  // the batch that fails
  bool thread_ok = true;
  int busy() const {
    const int64_t now = now_ns();
    int n = 0;
    for (const Batch& b : batches) n += b.end_ns > now;
    return n;
  }
  vsf_status launch(int64_t t0, int n, bool solo, int rows_hint) {
    CHECK(!inside.exchange(true));
    vsf_status st = VSF_OK;
    if ((int)batches.size() == fail_at) {
      st = VSF_ERR_CAPACITY;
    } else {
      if (solo) CHECK(n == 1 && busy() == 0);
      const int64_t t = now_ns();
      spin_ns((int64_t)(rnd() % 50001u));
      batches.push_back({t0, n, solo, rows_hint, now_ns() + (int64_t)(rnd() % 200001u)});
      q->stats.launch_ns += now_ns() - t;  // (the baton holder's share of the statistics)
      q->stats.multi++;
    }
    inside.store(false);
    return st;
  }
  ObserveGpu callables() {
    return {this, [](void* s, int64_t t0, int n, bool solo, int rows) { return static_cast<FakeGpu*>(s)->launch(t0, n, solo, rows); },
            [](void* s) { return static_cast<FakeGpu*>(s)->busy(); }, [](void* s) { return static_cast<FakeGpu*>(s)->thread_ok; }};
  }
};

struct Rig {
  FakeGpu gpu;
  ObserveQueue q;
  Rig(int depth, int bmax, int min_batch, bool thread) : q({depth, bmax, min_batch, 2}, gpu.callables()) {
    gpu.q = &q;
    if (thread) q.start_thread();
  }
  int64_t next_launch() {
    std::lock_guard<std::mutex> g(q.mu);
    return q.next_launch;
  }
  vsf_status status() {
    std::lock_guard<std::mutex> g(q.mu);
    return q.status;
  }
  template <class F>
  bool within_5s(F done) {
    for (const int64_t end = now_ns() + 5000000000ll; now_ns() < end; std::this_thread::sleep_for(std::chrono::microseconds(100)))
      if (done()) return true;
    return false;
  }
};

static int rows_of(int64_t ticket) { return 50 + (int)(ticket % 7) * 30; }

static void stream_of_frames(int depth, int bmax, int min_batch, bool thread) {
  const int64_t tickets = 2000;
  Rig r(depth, bmax, min_batch, thread);
  ObserveQueue& q = r.q;
  std::atomic<bool> reading{true};
  std::thread reader([&] {  // vsf_observe_stats beside the launches
    ObserveLaunchStats last;
    while (reading.load()) {
      ObserveLaunchStats s;
      {
        const std::unique_lock<std::mutex> lk = q.lock_idle();
        CHECK(!q.launching);
        s = q.stats;
      }
      CHECK(s.frames >= last.frames && s.batches >= last.batches && s.max_batch >= last.max_batch && s.solo >= last.solo &&
            s.forced >= last.forced && s.launch_ns >= last.launch_ns && s.multi >= last.multi && s.multi == s.batches);
      last = s;
      std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  });
  std::set<int> hints{0};
  int hint = 0;
  auto collect_oldest = [&] {
    const int64_t c = q.next_collect;
    CHECK(q.release(c) == VSF_OK);
    CHECK(r.next_launch() > c);  // a collected frame has left, whoever launched it
    CHECK(q.collected(c, rows_of(c)) == VSF_OK);
    hint = std::max(rows_of(c) * 2 + 64, hint - hint / 8);
    hints.insert(hint);
  };
  for (int64_t t = 0; t < tickets; t++) {
    if (q.next_ticket - q.next_collect >= depth) collect_oldest();
    int64_t ticket = -1;
    CHECK(q.submit(&ticket) == VSF_OK && ticket == t);
    if (t % 500 == 250) {  // another entry point of the context comes by
      q.drain();
      std::lock_guard<std::mutex> g(q.mu);
      CHECK(q.next_launch == q.next_ticket && !q.launching);
    }
  }
  while (q.next_collect < q.next_ticket) collect_oldest();
  reading.store(false);
  reader.join();
  q.stop_thread();
  int64_t at = 0, solo = 0, widest = 0;
  for (const FakeGpu::Batch& b : r.gpu.batches) {
    CHECK(b.t0 == at && b.n >= 1 && b.n <= bmax && (!b.solo || b.n == 1) && hints.count(b.rows_hint) == 1);
    at += b.n;
    solo += b.solo;
    widest = std::max<int64_t>(widest, b.n);
  }
  CHECK(at == tickets && q.next_launch == tickets && q.status == VSF_OK);
  CHECK(q.stats.frames == tickets && q.stats.batches == (int64_t)r.gpu.batches.size() && q.stats.solo == solo &&
        q.stats.max_batch == widest && q.rows_hint == hint);
  std::printf("launcher: depth %d, %d per batch, min_batch %d, thread %d: %zu batches, %lld forced\n", depth, bmax, min_batch,
              (int)thread, r.gpu.batches.size(), (long long)q.stats.forced);
}

static void lone_frame() {
  Rig r(8, 8, 0, true);
  int64_t ticket = -1;
  CHECK(r.q.submit(&ticket) == VSF_OK && ticket == 0);
  CHECK(r.within_5s([&] { return r.next_launch() == 1; }));  // nobody collects: the thread sends it once the queue is quiet
  CHECK(r.gpu.batches.size() == 1 && r.gpu.batches[0].solo);
}

static void failed_launch(bool thread) {
  Rig r(4, 2, 0, thread);
  r.gpu.fail_at = 3;
  ObserveQueue& q = r.q;
  int64_t ticket = -1;
  for (int64_t t = 0; t < 3; t++)  // (submit, collect: batches of one)
    CHECK(q.submit(&ticket) == VSF_OK && q.release(t) == VSF_OK && q.collected(t, 10) == VSF_OK);
  CHECK(r.gpu.batches.size() == 3 && r.next_launch() == 3);
  CHECK(q.submit(&ticket) == VSF_OK && ticket == 3);  // (it waits for company)
  if (thread) CHECK(r.within_5s([&] { return r.status() == VSF_ERR_CAPACITY; }));  // the thread meets the failure by itself
  CHECK(q.release(3) == VSF_ERR_CAPACITY);
  r.gpu.fail_at = -1;  // (the GPU would take the next one: the queue does not offer it)
  CHECK(q.submit(&ticket) == (thread ? VSF_OK : VSF_ERR_CAPACITY) && ticket == 4);
  for (int i = 0; i < 3; i++) {
    CHECK(q.release(3) == VSF_ERR_CAPACITY);
    std::unique_lock<std::mutex> lk(q.mu);
    CHECK(q.caller_pump(lk, true) == VSF_ERR_CAPACITY && q.caller_pump(lk, false) == VSF_ERR_CAPACITY);
  }
  q.drain();
  CHECK(r.gpu.batches.size() == 3 && r.next_launch() == 3 && r.status() == VSF_ERR_CAPACITY && q.stats.batches == 3);
}

static void thread_cannot_begin() {
  Rig r(4, 4, 0, false);
  r.gpu.thread_ok = false;
  r.q.start_thread();
  CHECK(r.within_5s([&] { return r.status() == VSF_ERR_HIP; }));
  int64_t ticket = -1;
  CHECK(r.q.submit(&ticket) == VSF_OK && r.q.release(ticket) == VSF_ERR_HIP && r.gpu.batches.empty());
}

static void stop_with_frames_waiting() {
  for (int round = 0; round < 50; round++) {
    Rig r(32, 8, 0, true);
    int64_t ticket = -1;
    for (int t = 0; t < 20; t++) CHECK(r.q.submit(&ticket) == VSF_OK);
    spin_ns(round * 2000);  // (from "before its first launch" to "some launches in")
    if (round & 1) r.q.stop_thread();  // (else: the destructor's)
  }
}

int main() {
  policy();
  copy_helper();
  const int shapes[5][3] = {{1, 1, 0}, {4, 4, 0}, {32, 8, 0}, {32, 32, 12}, {7, 3, 3}};
  for (const auto& s : shapes)
    for (int thread = 0; thread < 2; thread++) stream_of_frames(s[0], s[1], s[2], thread != 0);
  lone_frame();
  failed_launch(false);
  failed_launch(true);
  thread_cannot_begin();
  stop_with_frames_waiting();
  if (failures) {
    std::printf("%d failures\n", failures.load());
    return 1;
  }
  std::printf("ok observe queue\n");
  return 0;
}
