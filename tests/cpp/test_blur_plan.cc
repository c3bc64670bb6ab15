// csrc/vsf_blur_plan.h on the CPU: which blurred pyramid a call's blur writes, which release it waits for and records.
// The program issues call sequences the way extract_on (csrc/vsf_api.hip) does, onto a model of the context's streams in
// which an operation knows every operation that is ordered in front of it (stream order, and what a waited event had seen
// when it was recorded), and checks at every call:
//   * the blur writes no buffer that descriptors queued earlier still read, or an earlier blur still writes, without being
//     ordered behind them;
//   * the descriptors read the buffer their own call's blur wrote, behind that blur;
//   * the state names the buffer the last call wrote (what vsf_debug_level_image reads).
// Sequences: early throughout; the fork beside FAST throughout; the option as 1, 0, 1, 1, 0 and toggled every call; a small
// call (blur in line) in between; calls on a stream of their own in between; two-lane calls between the waits vsf_set_lanes
// makes; every sequence of up to 7 calls over the five one-stream kinds; random ones of 64.  A planner that is wrong on
// purpose (the early blur into the buffer the previous call reads) must be caught, or the model checks nothing.
// Exit status 0 and a line "ok ..." when everything holds.
#include <bitset>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_blur_plan.h"

static const int kMaxOps = 1024;
typedef std::bitset<kMaxOps> Seen;

enum StreamId { S_MAIN, S_PIPE, S_BLUR, S_AUX, S_OWN, S_COUNT };
// what a call is, as the walker issues it
enum CallKind { C_EARLY, C_MAIN_BESIDE, C_MAIN_INLINE, C_OWN_BESIDE, C_OWN_INLINE, C_TWO_LANES, C_COUNT };

struct Op {
  bool write;
  int call, buf, lo, hi;  // images [lo, hi) of the buffer
  Seen before;
};

typedef VsfBlurPlan (*Planner)(VsfBlurState*, VsfBlurKind, bool);

static VsfBlurPlan wrong_planner(VsfBlurState* s, VsfBlurKind kind, bool events) {
  const int flip = s->flip;
  VsfBlurPlan p = vsf_blur_plan(s, kind, events);
  if (kind == VSF_BLUR_EARLY) {  // the buffer the previous call's descriptors read, without waiting for them
    p.buf = flip;
    p.wait_free = false;
    s->flip = flip;
  }
  return p;
}

struct Model {
  Planner planner;
  VsfBlurState state;
  Seen seen[S_COUNT];
  Seen ev_free[2], ev_blur_done, ev_blur_fork, ev_pyr_done, ev_lane;
  std::vector<Op> ops;
  int calls = 0;
  long violations = 0;
  const char* first = nullptr;
  int first_call = -1;

  explicit Model(Planner p) : planner(p) {}

  void fail(const char* what, int call) {
    if (!violations++) {
      first = what;
      first_call = call;
    }
  }
  int issue(StreamId s, bool write, int call, int buf, int lo, int hi) {
    const int id = (int)ops.size();
    if (id >= kMaxOps) return -1;
    ops.push_back(Op{write, call, buf, lo, hi, seen[s]});
    if (write)  // every earlier reader and writer of these images of this buffer is ordered in front
      for (int i = 0; i < id; i++) {
        const Op& o = ops[(size_t)i];
        if (o.buf == buf && o.lo < hi && lo < o.hi && !seen[s].test((size_t)i))
          fail(o.write ? "a blur writes beside an earlier blur of the same buffer" : "a blur writes a buffer queued descriptors still read", call);
      }
    seen[s].set((size_t)id);
    return id;
  }
  void host_waits_for(StreamId s) {  // hipStreamSynchronize: what the stream has seen is over before anything issued later
    for (Seen& x : seen) x |= seen[s];
  }
  // one extraction of images [lo, hi) on stream `st`, as extract_on issues it
  void extract(VsfBlurKind kind, StreamId st, bool beside, int lo, int hi) {
    const int call = calls;
    const VsfBlurPlan p = planner(&state, kind, true);
    int blur = -1;
    auto launch_blur = [&](StreamId bs) {
      if (p.wait_free) seen[bs] |= ev_free[p.buf];
      blur = issue(bs, true, call, p.buf, lo, hi);
    };
    if (kind == VSF_BLUR_EARLY) {
      (void)issue(S_PIPE, false, call, -1, 0, 0);  // the pyramid chain (no blurred pyramid involved)
      ev_pyr_done = seen[S_PIPE];
      seen[st] |= ev_pyr_done;
      launch_blur(S_PIPE);
      ev_blur_done = seen[S_PIPE];
    } else if (beside) {
      ev_blur_fork = seen[st];
      seen[S_BLUR] |= ev_blur_fork;
      launch_blur(S_BLUR);
      ev_blur_done = seen[S_BLUR];
    }
    (void)issue(st, false, call, -1, 0, 0);  // FAST, selection
    if (kind == VSF_BLUR_EARLY || beside)
      seen[st] |= ev_blur_done;
    else
      launch_blur(st);
    const int desc = issue(st, false, call, p.buf, lo, hi);
    if (p.record_free) ev_free[p.buf] = seen[st];
    if (blur < 0 || desc < 0) {
      fail("the model ran out of operations", call);
      return;
    }
    if (ops[(size_t)blur].buf != ops[(size_t)desc].buf) fail("the descriptors read another buffer than their blur wrote", call);
    if (!ops[(size_t)desc].before.test((size_t)blur)) fail("the descriptors are not ordered behind their blur", call);
    if (kind != VSF_BLUR_LANE && state.flip != p.buf) fail("the state does not name the buffer the last call wrote", call);
    if (kind != VSF_BLUR_EARLY && p.buf != 0) fail("a call off the early path left buffer 0", call);
  }
  void call(CallKind c) {
    switch (c) {
      case C_EARLY: extract(VSF_BLUR_EARLY, S_MAIN, true, 0, 64); break;
      case C_MAIN_BESIDE: extract(VSF_BLUR_MAIN, S_MAIN, true, 0, 64); break;
      case C_MAIN_INLINE: extract(VSF_BLUR_MAIN, S_MAIN, false, 0, 16); break;
      case C_OWN_BESIDE: extract(VSF_BLUR_OWN, S_OWN, true, 0, 64); break;
      case C_OWN_INLINE: extract(VSF_BLUR_OWN, S_OWN, false, 0, 16); break;
      case C_TWO_LANES:
        host_waits_for(S_MAIN);  // vsf_set_lanes(ctx, 2)
        ev_lane = seen[S_MAIN];  // fork_lane
        seen[S_AUX] |= ev_lane;
        extract(VSF_BLUR_MAIN, S_MAIN, false, 0, 8);
        extract(VSF_BLUR_LANE, S_AUX, false, 8, 16);
        seen[S_MAIN] |= seen[S_AUX];  // join_lane
        host_waits_for(S_MAIN);       // vsf_set_lanes(ctx, 1)
        break;
      default: break;
    }
    calls++;
  }
};

static int fails = 0;
static long walked = 0;

static long walk(const std::vector<int>& seq, Planner planner, bool expect_clean, const char* name) {
  Model m(planner);
  for (int c : seq) m.call((CallKind)c);
  walked++;
  if (expect_clean && m.violations && fails++ < 20) {
    std::printf("FAIL %s: call %d: %s (sequence", name, m.first_call, m.first);
    for (int c : seq) std::printf(" %d", c);
    std::printf(")\n");
  }
  return m.violations;
}

int main() {
  const int E = C_EARLY, M = C_MAIN_BESIDE, I = C_MAIN_INLINE, O = C_OWN_BESIDE, L = C_TWO_LANES;
  walk({E, E, E, E, E, E, E, E}, vsf_blur_plan, true, "early throughout");
  walk({M, M, M, M, M, M}, vsf_blur_plan, true, "beside FAST throughout");
  walk({E, M, E, E, M}, vsf_blur_plan, true, "1 0 1 1 0");
  walk({E, M, E, M, E, M, E, M, E}, vsf_blur_plan, true, "toggled every call");
  walk({E, E, I, E, E, I, I, E}, vsf_blur_plan, true, "a small call in between");
  walk({E, E, O, E, E, C_OWN_INLINE, M, E, O, I, E}, vsf_blur_plan, true, "a stream of its own in between");
  walk({E, E, L, E, E, L, M, L, L, E}, vsf_blur_plan, true, "two lanes in between");
  // every sequence of up to 7 calls over the one-stream kinds
  for (int len = 1; len <= 7; len++) {
    std::vector<int> seq((size_t)len, 0);
    for (;;) {
      walk(seq, vsf_blur_plan, true, "exhaustive");
      int i = 0;
      while (i < len && ++seq[(size_t)i] == C_TWO_LANES) seq[(size_t)i++] = 0;
      if (i == len) break;
    }
  }
  // random sequences of 64 calls, two-lane episodes included
  uint32_t r = 12345u;
  for (int n = 0; n < 2000; n++) {
    std::vector<int> seq(64);
    for (int& c : seq) {
      r = r * 1664525u + 1013904223u;
      c = (int)((r >> 16) % C_COUNT);
    }
    walk(seq, vsf_blur_plan, true, "random");
  }
  // the model has teeth: the early blur into the buffer the previous call's descriptors read is caught
  if (walk({E, E, E}, wrong_planner, false, "wrong planner") == 0) {
    std::printf("FAIL the model accepts an early blur into the previous call's buffer\n");
    fails++;
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok %ld sequences\n", walked);
  return 0;
}
