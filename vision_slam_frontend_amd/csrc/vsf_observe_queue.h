// vsf_observe_queue.h -- the host threads of the ObserveImage queue (vsf_observe.hip), plain C++: who launches a batch and
// when, the tickets, and the helper that shares a frame's staging copy.  No HIP, no context: the queue sees the GPU through
// three callables (ObserveGpu), so tests/cpp/test_observe_queue.cc runs all of it on the CPU under ThreadSanitizer.
#ifndef VSF_OBSERVE_QUEUE_H_
#define VSF_OBSERVE_QUEUE_H_

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <thread>

#include "../../include/vsf.h"

namespace vsfi {

inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One row-wise copy of an image into the staging ring (rows at the device pitch): 5-12 us per 640x480 image on one core,
// depending on the host (its memory, its neighbours).
void stage_image(uint8_t* dst, size_t dst_pitch, const uint8_t* src, size_t src_pitch, size_t width, int rows);

// The staging copy is what a queued frame costs its caller once the launches have a thread of their own: 13 us per frame on
// one box, 23 us on another (the same run: 31.5 k and 28.9 k frames/s -- on the second the caller never waits for the GPU).
// While frames stream in (the previous one is still in the queue) a helper thread takes the right image: it spins for a job
// while it is hot and goes to sleep `idle` (300 us) after the last one, so a caller that submits and collects frame by frame
// never meets it (a wake-up costs more than the copy saves).  It touches host memory only.
// Going to sleep: the helper stores hot = false and then looks at `state` under `m`; post() stores state = 1 and then looks
// at `hot`.  All four are sequentially consistent, so at least one side sees the other: either the helper finds the job in
// its predicate, or post() finds hot == false and notifies under `m` -- which it gets only once the helper blocks.
struct ObserveCopyHelper {
  struct Job {
    uint8_t* dst;
    const uint8_t* src;
    size_t dst_pitch, src_pitch, width;
    int rows;
  };
  const std::chrono::nanoseconds idle;
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::atomic<int> state{0};  // 0 no job, 1 job posted, 2 job done
  std::atomic<bool> hot{false}, stop{false};
  bool wake = false;
  Job job{};
  explicit ObserveCopyHelper(std::chrono::nanoseconds idle_limit = std::chrono::microseconds(300));
  ~ObserveCopyHelper();
  void run();
  // true: the helper took `j` (wait() must follow); false: it sleeps -- woken for the frames behind this one -- and the
  // caller copies `j` itself.
  bool post(const Job& j);
  void wait() {
    while (state.load(std::memory_order_acquire) != 2) __builtin_ia32_pause();
    state.store(0, std::memory_order_relaxed);
  }
};

// What the queue sees of the GPU: vsf_observe.hip's launch_batch / batches_on_gpu / hipSetDevice, or a test's fake.
struct ObserveGpu {
  void* self;
  vsf_status (*launch)(void* self, int64_t t0, int n, bool solo, int rows_hint);  // frames [t0, t0 + n) as one batch
  int (*busy)(void* self);           // batches launched and not finished
  bool (*thread_begin)(void* self);  // the launcher thread's first step; false: it leaves with VSF_ERR_HIP
};

struct ObserveSizes {
  int depth, bmax;  // frames that may be submitted and not collected / per batch at most
  int min_batch;    // vsf_observe_configure: 0 = a whole batch while the queue holds two, else half the queue
  int in_flight;    // batches on the GPU at most before frames wait for company
};

// How many of `pending` waiting frames leave now (0: none); quiet_ns: since the last frame arrived.  gpu.busy is asked only
// where the answer depends on it.
int batch_to_launch(int pending, const ObserveSizes& s, bool force, int64_t quiet_ns, const ObserveGpu& gpu);

// vsf_observe_stats' share of the launches.  The queue counts the first five under `mu`; the rest is the launch callable's,
// written while it holds the baton.  Readers: ObserveQueue::lock_idle.
struct ObserveLaunchStats {
  int64_t frames = 0, batches = 0, max_batch = 0, solo = 0, forced = 0;
  int64_t slot_waits = 0, launch_ns = 0, multi = 0, compressed = 0, ingest_commands = 0, file_commands = 0;
  int64_t device_frames = 0, device_commands = 0;  // vsf_observe_submit_dev: frames launched, the batches' copies and kernels
  int64_t cloud_frames = 0, cloud_commands = 0;    // vsf_observe_set_world_points: frames launched, the batches' one kernel each
  int64_t reduced = 0;                             // vsf_observe_submit_compressed_reduced: frames launched with reduce > 1
  int64_t pix_frames = 0, pix_commands = 0;  // new pixel formats: frames converted, the batches' launches and copies for them
  int64_t resized = 0, resize_commands = 0, multi_size = 0;        // vsf_observe_set_input_size: frames resized, the batches' launches and copies for them
  int64_t seeded_frames = 0, colour_commands = 0;  // vsf_observe_set_debug_seeds: frames coloured by a stream's generator, the kernel's launches
};

// Who launches.  A batch costs the host 0.1 ms (a lone frame) to 0.4 ms (the batched pyramid alone is 50-100 launches).
// By default the caller launches, between two submits (4-5 us per frame at 64-128 frames per batch).  With
// VSF_OPT_OBSERVE_THREAD a queue of depth >= 4 has a LAUNCHER thread instead: the caller stages frames and the thread sends
// whatever the policy releases, polling the GPU's state while frames wait (measured slower wherever depth == batch size, the
// same elsewhere: off by default).  The caller still launches by itself where waiting for the thread would cost more than it
// saves: when it collects a frame that still waits (the synchronous call: submit, collect), and for every other entry
// point of the context, which first sends everything that waits (VsfErrorScope -> vsf_ctx_enter -> drain), so that nothing
// else ever runs beside the thread.  `launching` is the baton: whoever holds it is alone inside gpu.launch.
struct ObserveQueue {
  const ObserveGpu gpu;
  mutable std::mutex mu;  // guards everything below
  mutable std::condition_variable cv_caller;
  std::condition_variable cv_thread;
  bool launching = false, stop = false, has_thread = false;
  vsf_status status = VSF_OK;  // first failure of a launch: sticky until the queue is rebuilt
  std::thread th;
  int64_t next_ticket = 0;     // tickets issued (written by the caller alone, as next_collect)
  int64_t next_launch = 0;     // first frame still waiting in staging
  int64_t next_collect = 0;    // oldest frame not collected
  int64_t last_submit_ns = 0;  // when the last frame arrived
  ObserveSizes sizes;
  int rows_hint = 0;  // expected rows of a filtered frame (from the collected results; 0: unknown)
  ObserveLaunchStats stats;

  ObserveQueue(const ObserveSizes& s, const ObserveGpu& g) : gpu(g), sizes(s) {}
  ~ObserveQueue() { stop_thread(); }
  void start_thread();
  void stop_thread();  // frames that still wait stay where they are
  // One batch, by whoever holds the lock: takes the baton, launches outside the lock, publishes next_launch.
  vsf_status launch_one(std::unique_lock<std::mutex>& lk, int n);
  // The caller's side.  force: everything that waits leaves now (somebody collects one of them, the parameters change, or
  // another entry point of the context is about to run); otherwise whatever the policy releases.  mu held on entry and exit.
  vsf_status caller_pump(std::unique_lock<std::mutex>& lk, bool force);
  // A staged frame gets its ticket: the thread hears of it, or the caller launches what the policy releases.
  vsf_status submit(int64_t* ticket);
  // Before `ticket` is waited for: if it still waits in staging, everything that waits leaves now.
  vsf_status release(int64_t ticket);
  // `ticket` has been collected; rows >= 0: what its filtered frame held, for rows_hint.
  vsf_status collected(int64_t ticket, int rows);
  void drain();  // everything that waits leaves and nobody launches afterwards
  std::unique_lock<std::mutex> lock_idle() const;  // mu, taken while nobody holds the baton (forces nothing out)

 private:
  void thread_loop();
};

}  // namespace vsfi

#endif  // VSF_OBSERVE_QUEUE_H_
