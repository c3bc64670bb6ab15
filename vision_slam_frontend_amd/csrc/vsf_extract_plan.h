// vsf_extract_plan.h -- the schedule of one extraction (pyramid -> FAST -> selection -> blur -> descriptors), stated once:
// the books the calls of a context leave to one another, the decisions a call makes from them, and the order in which its
// waits, records and launches are queued.  Plain C++, no HIP: vsf_api.hip extract_on issues vsf_extract_issue() onto the
// context's streams and events, tests/cpp/test_extract_plan.cc onto a model of them that knows which operation is ordered
// behind which, and walks call sequences over it.
//
// Three resources come in pairs, because a pipelined call writes them on a stream that is not ordered behind the previous
// call's readers (NOTES.md "The extraction's schedule" has the measurements behind each):
//   the pyramid          written by the resize chain; read by both FAST parts, selection, blur and descriptors.  A pipelined
//                        call's chain runs on the pipe stream into the buffer the previous call does not use.
//   the candidate pair   (candidates + row starts) written by both FAST parts, read by the selection.  A call with an early
//                        FAST part takes the other pair: that part runs on the blur stream beside the previous selection.
//   the blurred pyramid  written by the blur, read by the descriptors.  A call whose blur follows its chain on the pipe
//                        stream takes the other buffer (vsf_blur_plan below).
// ev_*_free[i] is recorded behind the last reader of buffer i; a writer that stream order does not put behind that reader
// waits for it.
#ifndef VSF_EXTRACT_PLAN_H_
#define VSF_EXTRACT_PLAN_H_

// ---- the blurred pyramid ----
// Buffer 0 is the context's own (`dorb.blur`), buffer 1 `blur_alt` of a pipelined context.  ev_blur_free[i] is recorded
// behind the descriptors that read buffer i -- the only reader of a blurred level.
//   VSF_BLUR_EARLY  a pipelined call with VSF_OPT_BLUR_EARLY: the blur is queued on the pipe stream behind the call's pyramid
//                   chain, not ordered behind the PREVIOUS call's descriptors, which may still read the buffer the last blur
//                   wrote -- so it takes the other one, once the descriptors that last read THAT one are through.
//   VSF_BLUR_MAIN   every other call on the context's stream (the blur on it, or forked from it onto the blur stream; the
//                   first of two lanes): the blur follows all earlier work of that stream and writes buffer 0.  The stream
//                   has waited for every earlier blur in front of its descriptors, and those descriptors are on it: stream
//                   order covers readers and writers alike, unless the release of buffer 0 was last recorded somewhere else.
//   VSF_BLUR_LANE   the second half of a two-lane call, between fork_lane and join_lane: other images of buffer 0, as a whole
//                   in the main stream's order; the first half kept the books, and what it waited for this half waits for.
//                   (vsf_set_lanes waits for the stream before the number of lanes changes.)
//   VSF_BLUR_OWN    a call on a stream that is not ordered with the context's: buffer 0, behind its last release, and it
//                   records the next one.
enum VsfBlurKind { VSF_BLUR_EARLY = 0, VSF_BLUR_MAIN = 1, VSF_BLUR_LANE = 2, VSF_BLUR_OWN = 3 };

struct VsfBlurState {
  int flip = 0;                           // the buffer the last call's blur wrote
  bool free_valid[2] = {false, false};    // ev_blur_free[i] has been recorded
  bool free_on_main[2] = {false, false};  // ... on the context's stream
  bool lane_wait = false;                 // the last VSF_BLUR_MAIN call waited for a release
};

struct VsfBlurPlan {
  int buf;           // the blur writes it, the descriptors read it
  bool wait_free;    // the stream the blur runs on waits for ev_blur_free[buf] in front of it
  bool record_free;  // the call's stream records ev_blur_free[buf] behind the descriptors
};

// `events`: the context has ev_blur_free (a pipelined context; without them no call was ever VSF_BLUR_EARLY).
inline VsfBlurPlan vsf_blur_plan(VsfBlurState* s, VsfBlurKind kind, bool events) {
  VsfBlurPlan p{0, false, false};
  if (!events) return p;
  if (kind == VSF_BLUR_LANE) {
    p.wait_free = s->lane_wait;  // (re-recorded by the first half since: behind that half's descriptors, and so behind what it waited for)
    return p;
  }
  if (kind == VSF_BLUR_EARLY) {
    p.buf = s->flip ^ 1;
    p.wait_free = s->free_valid[p.buf];
  } else {
    p.wait_free = s->free_valid[0] && !(kind == VSF_BLUR_MAIN && s->free_on_main[0]);
    if (kind == VSF_BLUR_MAIN) s->lane_wait = p.wait_free;
  }
  p.record_free = true;
  s->flip = p.buf;
  s->free_valid[p.buf] = true;
  s->free_on_main[p.buf] = kind != VSF_BLUR_OWN;
  return p;
}

// ---- the books ----
struct VsfExtractState {
  int pyr_flip = 0;                          // the pyramid buffer the next pipelined call's chain writes
  bool pyr_free_valid[2] = {false, false};   // ev_pyr_free[i] has been recorded
  int cand_flip = 0;                         // the candidate pair the last call used (what the debug hooks read)
  bool cand_free_valid[2] = {false, false};  // ev_cand_free[i] has been recorded
  bool fast_done_valid = false;              // ev_fast_done has been recorded
  VsfBlurState blur;

  // vsf_set_pipeline, which has waited for the main, the aux and the pipe stream: what was recorded on them is over.  The
  // blur keeps its releases: a reader of buffer 0 may sit on a stream that was not waited for.
  void reset_pipeline() {
    pyr_free_valid[0] = pyr_free_valid[1] = false;
    cand_free_valid[0] = cand_free_valid[1] = false;
    fast_done_valid = false;
  }
};

// ---- what a call is ----
struct VsfExtractFacts {
  // vsf_set_pipeline is on, and the caller promised the images are complete: the chain need not follow the stream's earlier work
  bool pipeline, inputs_complete;
  int lanes;                                  // vsf_set_lanes
  bool on_main, on_aux;                       // the call's stream is the context's / its aux stream
  bool first_image, own_side;                 // i0 == 0; the caller brought side streams of its own
  int n;                                      // images
  bool blur_overlap;                          // vsf_set_blur_overlap
  bool blur_stream, cand_alt, blur_alt;       // the context has them
  bool pipe_after_fast, blur_early;           // VSF_OPT_PIPE_AFTER_FAST, VSF_OPT_BLUR_EARLY
  // VSF_OPT_FAST_EARLY_LEVELS clamped to the levels that have a full cell, and vsf_fast_n_early() of it (vsf_fast_split.h)
  int early_levels, n_early;
  // the form vsf_tune_fast_resident is timing, vsf_set_fast_resident, the batch size the tune call measured and what it found
  int fast_force, fast_resident, tune_n, tune_choice;
  bool ingest_pending, input_pending;         // ev_ingest_done / the caller's input event is to be waited for
};

enum VsfBlurWhere { VSF_BLUR_INLINE = 0, VSF_BLUR_FORKED = 1, VSF_BLUR_BEHIND_CHAIN = 2 };

struct VsfExtractPlan {
  bool pipe;  // the chain on the pipe stream, not ordered behind the call's stream
  // the early FAST part starts behind the launch that makes level early_levels - 1, on the head [0, n_early) of the full
  // cells; n_early 0: one FAST pass
  int early_levels, n_early;
  int pyr_buf, cand_buf, blur_buf;
  VsfBlurWhere blur_where;
  bool blur_lane;  // the second half of a two-lane call: the first half kept the books (and named the last buffer)
  int resident;    // FAST's waves per SIMD as one resident workgroup per CU; 0: a grid
  bool wait_pyr_free, wait_fast_done, wait_ingest, wait_input;  // the chain, in front of its first launch
  bool wait_cand_free, wait_blur_free;                          // the early FAST part; the blur
  bool record_cand_free, record_blur_free;
};

// ---- the decisions ----
inline VsfExtractPlan vsf_extract_plan(VsfExtractState* s, const VsfExtractFacts& f) {
  VsfExtractPlan p{};
  // The pyramid depends on the input images only: where the caller promised they are complete, the chain goes onto the pipe
  // stream and overlaps the previous call's later stages.  One lane, the context's stream, whole batches only.
  p.pipe = f.pipeline && f.inputs_complete && f.lanes == 1 && f.on_main && f.first_image;
  const bool tune_call = f.fast_force >= 0;
  // VSF_OPT_FAST_EARLY_LEVELS: the full cells of the first levels are scored by a launch of their own on the blur stream,
  // beside the PREVIOUS call's selection and descriptors, which wait on latency.  Pipelined calls only; never the tune call.
  p.early_levels = p.pipe && f.cand_alt && f.blur_stream && !tune_call ? f.early_levels : 0;
  p.n_early = p.early_levels > 0 ? f.n_early : 0;
  // Such a call takes the other candidate pair; a call without an early part stays on the pair the last call used: its FAST
  // follows that call's selection on this stream.  Every pipelined call records the release of the pair it read, so the
  // option may change from call to call.
  if (p.n_early > 0) s->cand_flip ^= 1;
  p.cand_buf = s->cand_flip;
  p.wait_cand_free = p.n_early > 0 && s->cand_free_valid[p.cand_buf];
  p.record_cand_free = p.pipe && f.cand_alt;
  if (p.record_cand_free) s->cand_free_valid[p.cand_buf] = true;
  // The blur runs beside other stages in batches of 32 images or more: forked behind the pyramid beside FAST (matrix cores
  // and memory beside the vector ALU), or -- VSF_OPT_BLUR_EARLY, a pipelined call -- behind the chain on the pipe stream.
  // The tune call, smaller batches, two lanes and own_side extractions keep the fork and buffer 0.
  const bool beside = f.blur_overlap && f.n >= 32 && f.blur_stream;
  const bool early_blur = p.pipe && beside && f.blur_early && f.blur_alt && !tune_call && !f.own_side;
  p.blur_where = early_blur ? VSF_BLUR_BEHIND_CHAIN : beside ? VSF_BLUR_FORKED : VSF_BLUR_INLINE;
  const VsfBlurKind kind = early_blur                  ? VSF_BLUR_EARLY
                           : f.on_main                 ? VSF_BLUR_MAIN
                           : f.lanes == 2 && f.on_aux ? VSF_BLUR_LANE
                                                       : VSF_BLUR_OWN;
  const VsfBlurPlan bp = vsf_blur_plan(&s->blur, kind, f.blur_alt);
  p.blur_buf = bp.buf;
  p.blur_lane = kind == VSF_BLUR_LANE;
  p.wait_blur_free = bp.wait_free;
  p.record_blur_free = bp.record_free;
  // With the blur beside it FAST may run as ONE resident workgroup per CU, which leaves registers to the blur.  Whether
  // that pays depends on the batch: the tune call forces each form in turn, vsf_set_fast_resident overrides, otherwise what
  // the tune call found for this batch size -- the grid for a size nobody measured.
  if (beside && f.lanes == 1 && f.on_main && f.first_image && !f.own_side)
    p.resident = tune_call                                  ? f.fast_force
                 : f.fast_resident >= 0                     ? f.fast_resident
                 : f.tune_n == f.n && f.tune_choice > 0 ? f.tune_choice
                                                            : 0;
  if (p.pipe) {
    // the chain writes the buffer the previous call does not use, once the call before that has released it, and not
    // before the previous call's FAST has finished (FAST fills every register; the stages behind it leave room)
    p.pyr_buf = s->pyr_flip;
    p.wait_pyr_free = s->pyr_free_valid[p.pyr_buf];
    p.wait_fast_done = s->fast_done_valid && f.pipe_after_fast;
    p.wait_ingest = f.ingest_pending;
    p.wait_input = f.input_pending;
    s->pyr_free_valid[p.pyr_buf] = true;
    s->pyr_flip ^= 1;
    s->fast_done_valid = true;
  }
  return p;
}

// ---- the order ----
enum VsfXStream { VSF_XS_CALL = 0, VSF_XS_PIPE, VSF_XS_BLUR, VSF_XS_COUNT };  // the call's stream, the chain's, the blur stream
// (the releases: + buffer or pair)
enum VsfXEvent { VSF_XE_PYR_FREE = 0, VSF_XE_CAND_FREE = 2, VSF_XE_BLUR_FREE = 4, VSF_XE_FAST_DONE = 6, VSF_XE_INGEST_DONE,
                 VSF_XE_INPUT, VSF_XE_EARLY_GO, VSF_XE_EARLY_DONE, VSF_XE_PYR_DONE, VSF_XE_BLUR_FORK, VSF_XE_BLUR_DONE, VSF_XE_COUNT };
enum VsfXStage { VSF_XG_PYRAMID = 0, VSF_XG_FAST_EARLY, VSF_XG_FAST, VSF_XG_SELECT, VSF_XG_BLUR, VSF_XG_DESCRIBE };

inline VsfXEvent vsf_xe(VsfXEvent base, int buf) { return (VsfXEvent)(base + buf); }

// The early FAST part.  A backend calls this from inside launch(VSF_XG_PYRAMID, chain) of a call with n_early > 0, right
// behind the chain's launch that makes level early_levels - 1 (behind the whole chain if no launch of its own makes it).
template <class Backend>
inline void vsf_extract_issue_early(const VsfExtractPlan& p, Backend& b, VsfXStream chain) {
  b.record(VSF_XE_EARLY_GO, chain);
  b.wait(VSF_XS_BLUR, VSF_XE_EARLY_GO);
  // ... and not before the selection that last read this pair is through
  if (p.wait_cand_free) b.wait(VSF_XS_BLUR, vsf_xe(VSF_XE_CAND_FREE, p.cand_buf));
  b.launch(VSF_XG_FAST_EARLY, VSF_XS_BLUR);
  b.record(VSF_XE_EARLY_DONE, VSF_XS_BLUR);
}

template <class Backend>
inline void vsf_extract_issue_blur(const VsfExtractPlan& p, Backend& b, VsfXStream s) {
  // ... not before the descriptors that last read this buffer are through, where stream order does not say so already
  if (p.wait_blur_free) b.wait(s, vsf_xe(VSF_XE_BLUR_FREE, p.blur_buf));
  b.launch(VSF_XG_BLUR, s);
}

template <class Backend>
inline void vsf_extract_issue(const VsfExtractPlan& p, Backend& b) {
  if (p.pipe) {
    if (p.wait_pyr_free) b.wait(VSF_XS_PIPE, vsf_xe(VSF_XE_PYR_FREE, p.pyr_buf));
    if (p.wait_fast_done) b.wait(VSF_XS_PIPE, VSF_XE_FAST_DONE);
    // ... nor before images this library itself is still producing on the context's stream are complete, nor before the
    // caller's own producer has finished them (vsf_set_input_event)
    if (p.wait_ingest) b.wait(VSF_XS_PIPE, VSF_XE_INGEST_DONE);
    if (p.wait_input) b.wait(VSF_XS_PIPE, VSF_XE_INPUT);
    b.launch(VSF_XG_PYRAMID, VSF_XS_PIPE);  // (the early FAST part from inside it)
    b.record(VSF_XE_PYR_DONE, VSF_XS_PIPE);
    b.wait(VSF_XS_CALL, VSF_XE_PYR_DONE);
    // Not on the blur stream: the early FAST part lives there and the blur would wait behind it.  The next call's chain
    // waits for this call's FAST anyway, so the blur in front of it delays nothing.
    if (p.blur_where == VSF_BLUR_BEHIND_CHAIN) {
      vsf_extract_issue_blur(p, b, VSF_XS_PIPE);
      b.record(VSF_XE_BLUR_DONE, VSF_XS_PIPE);
    }
  } else {
    b.launch(VSF_XG_PYRAMID, VSF_XS_CALL);
  }
  if (p.blur_where == VSF_BLUR_FORKED) {  // (on the blur stream behind an early FAST part: stream order)
    b.record(VSF_XE_BLUR_FORK, VSF_XS_CALL);
    b.wait(VSF_XS_BLUR, VSF_XE_BLUR_FORK);
    vsf_extract_issue_blur(p, b, VSF_XS_BLUR);
    b.record(VSF_XE_BLUR_DONE, VSF_XS_BLUR);
  }
  if (p.n_early > 0) b.wait(VSF_XS_CALL, VSF_XE_EARLY_DONE);
  b.launch(VSF_XG_FAST, VSF_XS_CALL);
  if (p.pipe) b.record(VSF_XE_FAST_DONE, VSF_XS_CALL);
  b.launch(VSF_XG_SELECT, VSF_XS_CALL);
  if (p.record_cand_free) b.record(vsf_xe(VSF_XE_CAND_FREE, p.cand_buf), VSF_XS_CALL);  // the last reader of this pair is queued
  if (p.blur_where == VSF_BLUR_INLINE)
    vsf_extract_issue_blur(p, b, VSF_XS_CALL);
  else
    b.wait(VSF_XS_CALL, VSF_XE_BLUR_DONE);
  b.launch(VSF_XG_DESCRIBE, VSF_XS_CALL);
  if (p.record_blur_free) b.record(vsf_xe(VSF_XE_BLUR_FREE, p.blur_buf), VSF_XS_CALL);  // the only reader of this blurred pyramid is queued
  // every reader of this pyramid buffer is queued: the call after the next may overwrite it
  if (p.pipe) b.record(vsf_xe(VSF_XE_PYR_FREE, p.pyr_buf), VSF_XS_CALL);
}

#endif  // VSF_EXTRACT_PLAN_H_
