// csrc/vsf_extract_plan.h on the CPU: the books, the decisions and the ORDER of an extraction, walked over call sequences.
// The backend below is a model of the context's streams in which an operation knows every operation that is ordered in
// front of it (stream order, what a waited event had seen when it was recorded, what the host waited for); the waits,
// records and launches it receives come from vsf_extract_issue() itself, the function extract_on (csrc/vsf_api.hip) issues
// onto the GPU.  Around an extraction the walker makes the host and stream waits the entry points make (vsf_set_lanes,
// vsf_set_option, vsf_set_pipeline, vsf_tune_fast_resident, launch_batch of the ObserveImage queue).  Checked at every call:
//   * no writer of a pyramid, candidate or blurred-pyramid buffer runs beside an earlier reader or writer of the same images
//     of that buffer (pyramid: written by the chain, read by both FAST parts, selection, blur, descriptors; candidate pair:
//     written by both FAST parts, read by the selection; blurred pyramid: written by the blur, read by the descriptors);
//   * every reader reads the buffer its own call's writer wrote, behind that writer;
//   * the state names the buffers the last call wrote (what the debug hooks read).
// Sequences: early throughout; the fork beside FAST throughout; VSF_OPT_BLUR_EARLY as 1, 0, 1, 1, 0 and toggled every call; a
// small call (blur in line) in between; calls on a stream of their own in between; two-lane calls; every sequence of up to 7
// calls over the five one-stream kinds, under each setting of the early FAST part and VSF_OPT_PIPE_AFTER_FAST; every sequence
// of up to 3 calls over every kind and option value; random ones of 64, the options changing from call to call, pipelining
// switched off and on and the tune call included; batches of the ObserveImage queue among themselves and among calls that
// do not pipeline (between pipelined calls the walk shows a hazard in the schedule as it is: main(), "finding").  Every one
// of these is walked with the wait for the context's stream that vsf_set_option makes where the options change, and
// WITHOUT it, nothing between the calls but stream and event order: the schedule must not lean on that wait.  Planners
// that are wrong on purpose -- one per resource -- must be caught, or the model checks nothing.
// Exit status 0 and a line "ok ..." when everything holds.
#include <bitset>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_extract_plan.h"

static const int kMaxOps = 4096;
typedef std::bitset<kMaxOps> Seen;

enum StreamId { S_MAIN, S_PIPE, S_BLUR, S_AUX, S_OWN, S_COPY, S_TAIL, S_COUNT };
enum Res { R_PYR, R_CAND, R_BLUR, R_COUNT };
// What a call is.  C_QUEUE: a batch of the ObserveImage queue (launch_batch: on the context's stream, inputs not promised
// complete); C_TUNE: vsf_tune_fast_resident; C_PIPELINE_OFF / _ON: vsf_set_pipeline, no extraction.
enum CallKind { C_MAIN64, C_MAIN16, C_OWN64, C_OWN16, C_TWO_LANES, C_QUEUE, C_TUNE, C_PIPELINE_OFF, C_PIPELINE_ON, C_COUNT };
// a sequence element: kind | options << 4
enum { O_FAST_EARLY = 1, O_BLUR_EARLY = 2, O_PIPE_AFTER_FAST = 4, O_COUNT = 8, O_ALL = 7 };
static int code(int kind, int options = O_ALL) { return kind | options << 4; }

struct Op {
  bool write;
  int call, res, buf, lo, hi;  // images [lo, hi) of buffer `buf` of resource `res`
  int parts;                   // pyramid: 1 = the levels the early FAST part reads, 2 = the rest; candidates: 1 = the early
                               // part's cells, 2 = the rest
};

typedef VsfExtractPlan (*Planner)(VsfExtractState*, const VsfExtractFacts&);

// the wrong planners: a chain that does not wait for the pyramid's release ...
static VsfExtractPlan wrong_pyramid(VsfExtractState* s, const VsfExtractFacts& f) {
  VsfExtractPlan p = vsf_extract_plan(s, f);
  p.wait_pyr_free = false;
  return p;
}
// ... an early FAST part that does not wait for the release of its candidate pair ...
static VsfExtractPlan wrong_candidates(VsfExtractState* s, const VsfExtractFacts& f) {
  VsfExtractPlan p = vsf_extract_plan(s, f);
  p.wait_cand_free = false;
  return p;
}
// ... and with neither wait
static VsfExtractPlan wrong_pyramid_and_candidates(VsfExtractState* s, const VsfExtractFacts& f) {
  VsfExtractPlan p = wrong_pyramid(s, f);
  p.wait_cand_free = false;
  return p;
}
// ... the blur behind the chain into the buffer the previous call's descriptors read, without waiting for them
static VsfExtractPlan wrong_blur(VsfExtractState* s, const VsfExtractFacts& f) {
  const int flip = s->blur.flip;
  VsfExtractPlan p = vsf_extract_plan(s, f);
  if (p.blur_where == VSF_BLUR_BEHIND_CHAIN) {
    p.blur_buf = flip;
    p.wait_blur_free = false;
    s->blur.flip = flip;
  }
  return p;
}

struct Model {
  Planner planner;
  bool pipe_is_aux;  // no VSF_OPT_PIPE_PRIORITY: the pipelined chain runs on the aux stream
  // vsf_set_option waits for the context's stream.  Without: the options change with nothing between the calls but stream and
  // event order -- no entry point does that, and the schedule must hold all the same (it may not come to lean on that wait)
  bool option_wait;
  VsfExtractState state;
  bool pipeline = true;  // (vsf_set_pipeline(ctx, 1) has been called: the buffers and events of a pipelined context exist)
  int options = -1;      // what vsf_set_option last set
  Seen seen[S_COUNT];
  Seen ev[VSF_XE_COUNT], ev_lane, ev_uploaded, ev_extracted, ev_batch_done[4];
  long batches = 0;
  std::vector<Op> ops;
  int calls = 0;
  long violations[R_COUNT] = {0, 0, 0}, other = 0;
  const char* first = nullptr;
  int first_call = -1;

  Model(Planner p, bool aux, bool wait) : planner(p), pipe_is_aux(aux), option_wait(wait) {}

  long total() const { return violations[R_PYR] + violations[R_CAND] + violations[R_BLUR] + other; }
  void fail(const char* what, int call, int res = -1) {
    if (!total()) {
      first = what;
      first_call = call;
    }
    (res < 0 ? other : violations[res])++;
  }

  // ---- the backend vsf_extract_issue() runs on ----
  struct Backend {
    Model& m;
    const VsfExtractPlan& p;
    StreamId st;
    int lo, hi;
    StreamId stream(VsfXStream s) const { return s == VSF_XS_CALL ? st : s == VSF_XS_BLUR ? S_BLUR : m.pipe_is_aux ? S_AUX : S_PIPE; }
    void wait(VsfXStream s, VsfXEvent e) { m.seen[stream(s)] |= m.ev[e]; }
    void record(VsfXEvent e, VsfXStream s) { m.ev[e] = m.seen[stream(s)]; }
    // (A call on a stream that is not ordered with the context's has a release for its blurred pyramid only, VSF_BLUR_OWN; no
    // entry point makes such a call today -- the queue's batches run on the context's stream -- and were one to, the pyramid
    // and the candidates it shares with the context's calls would need releases too.  Its blurred pyramid is what is checked.)
    bool checked(int res) const { return st != S_OWN || res == R_BLUR; }
    void read(StreamId s, int res, int buf, int parts = 3) {
      if (checked(res)) m.issue(s, false, res, buf, lo, hi, parts);
    }
    void write(StreamId s, int res, int buf, int parts = 3) {
      if (checked(res)) m.issue(s, true, res, buf, lo, hi, parts);
    }
    void launch(VsfXStage stage, VsfXStream xs) {
      const StreamId s = stream(xs);
      switch (stage) {
        case VSF_XG_PYRAMID:
          if (xs == VSF_XS_PIPE && p.n_early > 0) {  // the chain up to level early_levels - 1, the hook, the rest
            write(s, R_PYR, p.pyr_buf, 1);
            vsf_extract_issue_early(p, *this, xs);
            write(s, R_PYR, p.pyr_buf, 2);
          } else {
            write(s, R_PYR, p.pyr_buf);
          }
          break;
        case VSF_XG_FAST_EARLY:
          read(s, R_PYR, p.pyr_buf, 1);
          write(s, R_CAND, p.cand_buf, 1);
          break;
        case VSF_XG_FAST:
          read(s, R_PYR, p.pyr_buf);
          write(s, R_CAND, p.cand_buf, p.n_early > 0 ? 2 : 3);
          break;
        case VSF_XG_SELECT:
          read(s, R_PYR, p.pyr_buf);
          read(s, R_CAND, p.cand_buf);
          break;
        case VSF_XG_BLUR:
          read(s, R_PYR, p.pyr_buf);
          write(s, R_BLUR, p.blur_buf);
          break;
        case VSF_XG_DESCRIBE:
          read(s, R_PYR, p.pyr_buf);
          read(s, R_BLUR, p.blur_buf);
          break;
      }
    }
  };

  void issue(StreamId s, bool write, int res, int buf, int lo, int hi, int parts) {
    const int id = (int)ops.size();
    if (id >= kMaxOps) {
      fail("the model ran out of operations", calls);
      return;
    }
    bool own_writer = false;
    for (int i = 0; i < id; i++) {
      const Op& o = ops[(size_t)i];
      if (o.res != res || !(o.lo < hi && lo < o.hi) || !(o.parts & parts)) continue;
      const bool ordered = seen[s].test((size_t)i);
      if (write) {  // every earlier reader and writer of these images of this buffer is ordered in front
        if (o.buf == buf && !ordered)
          fail(o.write ? "a writer runs beside an earlier writer of the same buffer" : "a writer runs beside a queued reader of its buffer",
               calls, res);
      } else if (o.write && o.call == calls) {  // the reader's own call wrote what it reads, and is through
        own_writer = true;
        if (o.buf != buf) fail("a reader reads another buffer than its call wrote", calls, res);
        if (!ordered) fail("a reader is not ordered behind its call's writer", calls, res);
      }
    }
    if (!write && !own_writer) fail("a reader's call wrote nothing for it", calls, res);
    ops.push_back(Op{write, calls, res, buf, lo, hi, parts});
    seen[s].set((size_t)id);
  }
  void host_waits_for(StreamId s) {  // hipStreamSynchronize: what the stream has seen is over before anything issued later
    for (Seen& x : seen) x |= seen[s];
  }
  void host_waits_for_event(const Seen& e) {  // hipEventSynchronize
    for (Seen& x : seen) x |= e;
  }

  // one extract_on of images [lo, hi) on stream `st`
  void extract(StreamId st, int lo, int hi, bool inputs_complete, int lanes, int fast_force = -1) {
    VsfExtractFacts f{};
    f.pipeline = pipeline;
    f.inputs_complete = inputs_complete;
    f.lanes = lanes;
    f.on_main = st == S_MAIN;
    f.on_aux = st == S_AUX;
    f.first_image = lo == 0;
    f.own_side = false;
    f.n = hi - lo;
    f.blur_overlap = true;
    f.blur_stream = f.cand_alt = f.blur_alt = true;
    f.pipe_after_fast = (options & O_PIPE_AFTER_FAST) != 0;
    f.blur_early = (options & O_BLUR_EARLY) != 0;
    f.early_levels = options & O_FAST_EARLY ? 2 : 0;
    f.n_early = options & O_FAST_EARLY ? 40 : 0;
    f.fast_force = fast_force;
    f.fast_resident = -1;
    f.tune_n = 0;
    f.tune_choice = -1;
    f.ingest_pending = f.input_pending = false;
    const VsfExtractPlan p = planner(&state, f);
    Backend b{*this, p, st, lo, hi};
    vsf_extract_issue(p, b);
    if (fast_force >= 0 && (p.n_early > 0 || p.pipe || p.resident != fast_force)) fail("the tune call does not run the form it times", calls);
    if (!p.blur_lane && state.blur.flip != p.blur_buf) fail("the state does not name the blurred pyramid the last call wrote", calls);
    if (p.blur_where != VSF_BLUR_BEHIND_CHAIN && p.blur_buf != 0) fail("a call off the early path left blurred pyramid 0", calls);
    if (state.cand_flip != p.cand_buf) fail("the state does not name the candidate pair the last call used", calls);
    if (p.pipe ? state.pyr_flip != (p.pyr_buf ^ 1) : p.pyr_buf != 0) fail("a pipelined call does not alternate the pyramids, or another call left pyramid 0", calls);
  }
  void set_options(int o) {
    if (o == options) return;
    if (option_wait) host_waits_for(S_MAIN);
    options = o;
  }
  void set_pipeline(bool on) {  // vsf_set_pipeline: waits for the main, the aux and the pipe stream, resets the books
    host_waits_for(S_MAIN);
    host_waits_for(S_AUX);
    if (!pipe_is_aux) host_waits_for(S_PIPE);
    pipeline = on;
    state.reset_pipeline();
  }
  void call(int c) {
    const int kind = c & 15;
    if (kind < C_PIPELINE_OFF) set_options(c >> 4);
    switch (kind) {
      case C_MAIN64: extract(S_MAIN, 0, 64, true, 1); break;
      case C_MAIN16: extract(S_MAIN, 0, 16, true, 1); break;
      case C_OWN64: extract(S_OWN, 0, 64, true, 1); break;
      case C_OWN16: extract(S_OWN, 0, 16, true, 1); break;
      case C_TWO_LANES:
        host_waits_for(S_MAIN);  // vsf_set_lanes(ctx, 2)
        ev_lane = seen[S_MAIN];  // fork_lane
        seen[S_AUX] |= ev_lane;
        extract(S_MAIN, 0, 8, true, 2);
        extract(S_AUX, 8, 16, true, 2);
        seen[S_MAIN] |= seen[S_AUX];  // join_lane
        host_waits_for(S_MAIN);       // vsf_set_lanes(ctx, 1)
        break;
      case C_QUEUE: {  // launch_batch (vsf_observe.hip), a batch that is not solo
        Seen& done = ev_batch_done[batches++ % 4];
        host_waits_for_event(done);     // the slot's previous batch has left the GPU
        ev_uploaded = seen[S_COPY];     // ingest(): the upload on the copy stream, the context's stream waits for it
        seen[S_MAIN] |= ev_uploaded;
        extract(S_MAIN, 0, 64, false, 1);
        ev_extracted = seen[S_MAIN];    // the tail on its own stream behind the extraction and the previous batch's tail
        seen[S_TAIL] |= ev_extracted;
        done = seen[S_TAIL];
        break;
      }
      case C_TUNE:  // vsf_tune_fast_resident: every stream idle, then the two forms in turn, each waited for
        for (int s = 0; s < S_COUNT; s++)
          if (s != S_OWN) host_waits_for((StreamId)s);
        for (int run = 0; run < 3; run++) {
          extract(S_MAIN, 0, 64, false, 1, run & 1 ? 3 : 0);
          host_waits_for(S_MAIN);
          calls++;  // (each run is a call of its own to the checks)
        }
        calls--;
        break;
      case C_PIPELINE_OFF: set_pipeline(false); break;
      case C_PIPELINE_ON: set_pipeline(true); break;
      default: break;
    }
    calls++;
  }
};

static int fails = 0;
static long walked = 0;

struct Walked {
  long total, res[R_COUNT];
};

static Walked walk(const std::vector<int>& seq, Planner planner, bool expect_clean, const char* name, bool pipe_is_aux = false,
                   bool option_wait = true) {
  Model m(planner, pipe_is_aux, option_wait);
  for (int c : seq) m.call(c);
  walked++;
  if (expect_clean && m.total() && fails++ < 20) {
    std::printf("FAIL %s: call %d: %s (sequence", name, m.first_call, m.first);
    for (int c : seq) std::printf(" %d/%d", c & 15, c >> 4);
    std::printf(")%s%s\n", pipe_is_aux ? " chain on the aux stream" : "", option_wait ? "" : " no wait in vsf_set_option");
  }
  return Walked{m.total(), {m.violations[R_PYR], m.violations[R_CAND], m.violations[R_BLUR]}};
}

// ... the chain on a stream of its own and on the aux stream, with and without the wait in vsf_set_option
static void walk_both(const std::vector<int>& seq, const char* name) {
  for (int v = 0; v < 4; v++) walk(seq, vsf_extract_plan, true, name, (v & 1) != 0, (v & 2) != 0);
}

// every sequence of 1 .. max_len elements of `alphabet`
static void exhaustive(const std::vector<int>& alphabet, int max_len, const char* name) {
  const int n = (int)alphabet.size();
  for (int len = 1; len <= max_len; len++) {
    std::vector<int> idx((size_t)len, 0), seq((size_t)len);
    for (;;) {
      for (int i = 0; i < len; i++) seq[(size_t)i] = alphabet[(size_t)idx[(size_t)i]];
      walk(seq, vsf_extract_plan, true, name, false, true);
      walk(seq, vsf_extract_plan, true, name, false, false);
      int i = 0;
      while (i < len && ++idx[(size_t)i] == n) idx[(size_t)i++] = 0;
      if (i == len) break;
    }
  }
}

int main() {
  // (the names of the sequences the blur's plan has always been walked over: E the blur behind the chain, M forked beside FAST)
  const int E = code(C_MAIN64), M = code(C_MAIN64, O_ALL & ~O_BLUR_EARLY), I = code(C_MAIN16), O = code(C_OWN64),
            OI = code(C_OWN16), L = code(C_TWO_LANES);
  walk_both({E, E, E, E, E, E, E, E}, "early throughout");
  walk_both({M, M, M, M, M, M}, "beside FAST throughout");
  walk_both({E, M, E, E, M}, "1 0 1 1 0");
  walk_both({E, M, E, M, E, M, E, M, E}, "toggled every call");
  walk_both({E, E, I, E, E, I, I, E}, "a small call in between");
  walk_both({E, E, O, E, E, OI, M, E, O, I, E}, "a stream of its own in between");
  walk_both({E, E, L, E, E, L, M, L, L, E}, "two lanes in between");
  // the early FAST part 0 / > 0 independently of the blur, VSF_OPT_PIPE_AFTER_FAST 0 / 1, changing from call to call
  {
    std::vector<int> seq;
    for (int k = 0; k < 24; k++) seq.push_back(code(C_MAIN64, (k * 5 + k / 3) % O_COUNT));
    walk_both(seq, "the options changing from call to call");
  }
  // pipelining off and on again, the tune call, in the middle of early calls
  walk_both({E, E, code(C_PIPELINE_OFF), E, code(C_PIPELINE_ON), E, E, E}, "pipelining off for a call");
  walk_both({E, E, code(C_TUNE), E, E, code(C_TUNE), M, E}, "the tune call in between");
  walk_both({E, E, I, L, code(C_TUNE), code(C_MAIN64, O_PIPE_AFTER_FAST), code(C_PIPELINE_OFF), E, code(C_PIPELINE_ON), E, E},
            "the sequence of tests/test_gpu_extract_sequence.py");
  // every sequence of up to 7 calls over the one-stream kinds, under each setting of the early FAST part and PIPE_AFTER_FAST
  // (VSF_OPT_BLUR_EARLY as the kinds have always had it: 64-image calls on the context's stream with and without)
  for (int fixed = 0; fixed < 4; fixed++) {
    const int o = (fixed & 1 ? O_FAST_EARLY : 0) | (fixed & 2 ? O_PIPE_AFTER_FAST : 0);
    exhaustive({code(C_MAIN64, o | O_BLUR_EARLY), code(C_MAIN64, o), code(C_MAIN16, o | O_BLUR_EARLY), code(C_OWN64, o | O_BLUR_EARLY),
                code(C_OWN16, o | O_BLUR_EARLY)},
               7, "exhaustive, one-stream kinds");
  }
  // every sequence of up to 3 calls over every kind but the queue's (below) and every option value
  {
    std::vector<int> all;
    for (int k = 0; k < C_COUNT; k++)
      if (k != C_QUEUE)
        for (int o = 0; o < (k < C_PIPELINE_OFF ? O_COUNT : 1); o++) all.push_back(code(k, o));
    exhaustive(all, 3, "exhaustive, every kind and option");
  }
  // random sequences of 64 calls over everything but the queue's batches
  uint32_t r = 12345u;
  auto next = [&r](uint32_t n) {
    r = r * 1664525u + 1013904223u;
    return (int)((r >> 16) % n);
  };
  for (int n = 0; n < 2000; n++) {
    std::vector<int> seq(64);
    for (int& c : seq) {
      int k = next(C_COUNT);
      if (k == C_QUEUE) k = C_MAIN64;
      c = code(k, k < C_PIPELINE_OFF ? next(O_COUNT) : 0);
    }
    walk(seq, vsf_extract_plan, true, "random", (n & 1) != 0, true);
    walk(seq, vsf_extract_plan, true, "random", (n & 1) != 0, false);
  }
  // Batches of the ObserveImage queue: clean among themselves and among calls that do not pipeline ...
  const int Q = code(C_QUEUE);
  walk_both({Q, Q, Q, Q, Q, Q, Q, Q, Q, Q}, "batches of the queue");
  walk_both({code(C_PIPELINE_OFF), Q, E, Q, Q, M, I, Q, L, Q, code(C_TUNE), Q}, "batches of the queue among unpipelined calls");
  for (int n = 0; n < 500; n++) {
    std::vector<int> seq(64);
    seq[0] = code(C_PIPELINE_OFF);
    for (size_t i = 1; i < seq.size(); i++) {
      int k = next(C_PIPELINE_OFF);
      seq[i] = code(k, next(O_COUNT));
    }
    walk(seq, vsf_extract_plan, true, "random, the queue among unpipelined calls", (n & 1) != 0, true);
    walk(seq, vsf_extract_plan, true, "random, the queue among unpipelined calls", (n & 1) != 0, false);
  }
  // ... and a FINDING between pipelined calls, kept as the schedule has it: the batch reads pyramid 0 on the context's stream,
  // nothing makes the host wait behind it, and the next pipelined chain but one writes pyramid 0 behind the release its last
  // PIPELINED user recorded -- which is in front of the batch.  (A context runs the queue or pipelined batched calls; the
  // model says what mixing them would need.)
  if (walk({E, E, Q, E}, vsf_extract_plan, false, "finding").res[R_PYR] == 0) {
    std::printf("FAIL the model no longer sees the chain beside a queue batch's readers: update the finding\n");
    fails++;
  }
  // the model has teeth: one wrong planner per resource
  const int EN = code(C_MAIN64, O_FAST_EARLY | O_BLUR_EARLY);  // (VSF_OPT_PIPE_AFTER_FAST 0: ev_pyr_free is the chain's only order)
  if (walk({EN, EN, EN}, wrong_pyramid, false, "wrong pyramid planner").res[R_PYR] == 0) {
    std::printf("FAIL the model accepts a chain that does not wait for its pyramid's release\n");
    fails++;
  }
  // (the early FAST part starts behind the chain's first launches, and the chain has waited for the pyramid the call before
  // the last released behind ITS selection: while that wait is made it implies this one in every sequence.  So: the wait for
  // the candidates alone keeps them safe under a chain that does not wait, and without it they are not.)
  {
    const Walked a = walk({EN, EN, EN}, wrong_pyramid, false, "wrong pyramid planner"),
                 b = walk({EN, EN, EN}, wrong_pyramid_and_candidates, false, "wrong candidate planner");
    if (a.res[R_CAND] != 0 || b.res[R_CAND] == 0) {
      std::printf("FAIL the model accepts an early FAST part that does not wait for its candidate pair's release\n");
      fails++;
    }
    if (walk({EN, EN, EN, EN, EN}, wrong_candidates, false, "wrong candidate planner alone").total != 0) {
      std::printf("FAIL ev_cand_free is no longer implied by ev_pyr_free: make the check above the plain one\n");
      fails++;
    }
  }
  if (walk({E, E, E}, wrong_blur, false, "wrong blur planner").res[R_BLUR] == 0) {
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
