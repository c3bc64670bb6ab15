// vsf_observe_queue.cc -- see vsf_observe_queue.h.
#include "vsf_observe_queue.h"

#include <algorithm>
#include <cstring>

namespace vsfi {

void stage_image(uint8_t* dst, size_t dst_pitch, const uint8_t* src, size_t src_pitch, size_t width, int rows) {
  if (dst_pitch == src_pitch) {
    std::memcpy(dst, src, (size_t)(rows - 1) * src_pitch + width);
  } else {
    for (int y = 0; y < rows; y++) std::memcpy(dst + (size_t)y * dst_pitch, src + (size_t)y * src_pitch, width);
  }
}

ObserveCopyHelper::ObserveCopyHelper(std::chrono::nanoseconds idle_limit) : idle(idle_limit) {
  th = std::thread([this] { run(); });
}

ObserveCopyHelper::~ObserveCopyHelper() {
  {
    std::lock_guard<std::mutex> g(m);
    stop.store(true);
  }
  cv.notify_all();
  th.join();
}

void ObserveCopyHelper::run() {
  using Clock = std::chrono::steady_clock;
  while (!stop.load(std::memory_order_acquire)) {
    hot.store(true, std::memory_order_release);
    Clock::time_point last = Clock::now();
    while (!stop.load(std::memory_order_relaxed)) {
      if (state.load(std::memory_order_acquire) == 1) {
        stage_image(job.dst, job.dst_pitch, job.src, job.src_pitch, job.width, job.rows);
        state.store(2, std::memory_order_release);
        last = Clock::now();
      } else {
        __builtin_ia32_pause();
        if (Clock::now() - last > idle) break;
      }
    }
    hot.store(false);
    std::unique_lock<std::mutex> g(m);
    // (a job posted between the last look and `hot = false` is still served: the wait's predicate sees it)
    cv.wait(g, [this] { return stop.load() || wake || state.load() == 1; });
    wake = false;
  }
}

bool ObserveCopyHelper::post(const Job& j) {
  if (!hot.load(std::memory_order_acquire)) {
    {
      std::lock_guard<std::mutex> g(m);
      wake = true;
    }
    cv.notify_one();
    return false;
  }
  job = j;
  state.store(1);
  if (!hot.load()) {  // it was on its way to sleep: once it blocks -- it holds `m` until then -- the predicate serves the job
    std::lock_guard<std::mutex> g(m);
    cv.notify_one();
  }
  return true;
}

int batch_to_launch(int pending, const ObserveSizes& s, bool force, int64_t quiet_ns, const ObserveGpu& gpu) {
  if (pending <= 0) return 0;
  if (force || pending >= s.bmax) return std::min(pending, s.bmax);
  // An idle GPU takes whatever waits.  A busy one is in no hurry: frames wait for company because a batch costs ~50-100
  // launches whatever it carries (measured on the caller's thread: batches of 1-8 frames 14 k frames/s, of 32-64 frames
  // 27 k).  How much company: in steady state a batch leaves the moment `min_batch` frames wait, so min_batch IS the batch
  // size -- by default a whole batch when the queue is deep enough for the caller to fill the next one meanwhile (depth >= 2
  // batches), else half the queue, so that staging and the GPU still overlap (tools/exp/min_batch.sh: depth 64 / 32 per
  // batch 19.8 -> 25.0 k frames/s against half a batch, 128 / 64 27.9 -> 28.8 k, 256 / 128 32.0 -> 32.4 k; at depth =
  // batch size half the queue is what it was).
  // ... and "idle" must not be mistaken for "nobody is coming": while frames stream in (the last one arrived less than
  // 100 us ago) even an idle GPU waits for min_batch of them.  Without that a GPU that once ran dry keeps being fed batches of
  // a few frames, each gone before the next has gathered (measured: the same queue at 15 k or 32 k frames/s).
  const int busy = gpu.busy(gpu.self);
  const int min_batch = s.min_batch > 0 ? std::min(s.min_batch, s.bmax) : std::max(1, std::min(s.bmax, s.depth / 2));
  if (busy < s.in_flight && pending >= min_batch) return pending;
  return (busy == 0 && quiet_ns > 100000) ? pending : 0;
}

void ObserveQueue::start_thread() {
  has_thread = true;
  th = std::thread([this] { thread_loop(); });
}

void ObserveQueue::stop_thread() {
  if (!has_thread) return;
  {
    std::lock_guard<std::mutex> g(mu);
    stop = true;
  }
  cv_thread.notify_all();
  th.join();
  has_thread = false;
}

vsf_status ObserveQueue::launch_one(std::unique_lock<std::mutex>& lk, int n) {
  const int64_t t0 = next_launch;
  const bool solo = n == 1 && gpu.busy(gpu.self) == 0;
  const int rows = rows_hint;  // (the caller writes it under mu: collected())
  launching = true;
  lk.unlock();
  const vsf_status st = gpu.launch(gpu.self, t0, n, solo, rows);
  lk.lock();
  launching = false;
  if (st == VSF_OK) {
    next_launch = t0 + n;
    stats.batches++;
    stats.frames += n;
    stats.max_batch = std::max<int64_t>(stats.max_batch, n);
    if (solo) stats.solo++;
  } else if (status == VSF_OK) {
    status = st;
  }
  cv_caller.notify_all();
  if (has_thread) cv_thread.notify_one();
  return st;
}

vsf_status ObserveQueue::caller_pump(std::unique_lock<std::mutex>& lk, bool force) {
  while (true) {
    if (launching) {  // the thread is at it
      if (!force) return VSF_OK;
      cv_caller.wait(lk);
      continue;
    }
    if (status != VSF_OK) return status;
    const int n = batch_to_launch((int)(next_ticket - next_launch), sizes, force, now_ns() - last_submit_ns, gpu);
    if (n == 0) return VSF_OK;
    if (force) stats.forced++;
    const vsf_status st = launch_one(lk, n);
    if (st != VSF_OK) return st;
  }
}

void ObserveQueue::thread_loop() {
  if (!gpu.thread_begin(gpu.self)) {
    std::lock_guard<std::mutex> g(mu);
    status = VSF_ERR_HIP;
    return;
  }
  std::unique_lock<std::mutex> lk(mu);
  while (!stop) {
    if (launching || status != VSF_OK || next_launch >= next_ticket) {
      cv_thread.wait(lk);  // (a submit into an empty queue, the end of a launch and stop notify)
      continue;
    }
    const int n = batch_to_launch((int)(next_ticket - next_launch), sizes, false, now_ns() - last_submit_ns, gpu);
    if (n == 0) {  // frames wait for company or for the GPU: its state changes without a notification
      cv_thread.wait_for(lk, std::chrono::microseconds(40));
      continue;
    }
    (void)launch_one(lk, n);
  }
}

vsf_status ObserveQueue::submit(int64_t* ticket) {
  std::unique_lock<std::mutex> lk(mu);
  const bool was_empty = next_launch == next_ticket;
  *ticket = next_ticket++;
  last_submit_ns = now_ns();
  if (has_thread) {
    // the thread launches: it sleeps while nothing waits and polls while something does.  (A caller that collects right
    // away launches the frame itself there -- waking the thread would cost more than the launch.)
    if (was_empty) cv_thread.notify_one();
    return VSF_OK;
  }
  return caller_pump(lk, false);
}

vsf_status ObserveQueue::release(int64_t ticket) {
  std::unique_lock<std::mutex> lk(mu);
  if (ticket >= next_launch) {
    const vsf_status st = caller_pump(lk, true);
    if (st != VSF_OK) return st;
  }
  if (ticket >= next_launch) return status != VSF_OK ? status : VSF_ERR_HIP;
  return VSF_OK;
}

vsf_status ObserveQueue::collected(int64_t ticket, int rows) {
  std::unique_lock<std::mutex> lk(mu);
  next_collect = ticket + 1;
  const vsf_status st = has_thread ? VSF_OK : caller_pump(lk, false);  // (the GPU may have room again)
  // the filtered frames' size, for the matcher's launch choice: the largest of the last few frames with room to grow
  if (rows >= 0) rows_hint = std::max(rows * 2 + 64, rows_hint - rows_hint / 8);
  return st;
}

void ObserveQueue::drain() {
  std::unique_lock<std::mutex> lk(mu);
  (void)caller_pump(lk, true);
  while (launching) cv_caller.wait(lk);
}

std::unique_lock<std::mutex> ObserveQueue::lock_idle() const {
  std::unique_lock<std::mutex> lk(mu);
  while (launching) cv_caller.wait(lk);
  return lk;
}

}  // namespace vsfi
