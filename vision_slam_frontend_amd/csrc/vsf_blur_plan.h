// vsf_blur_plan.h -- which of the two blurred-pyramid buffers a call's blur writes (and its descriptors read), and which
// release event the blur waits for and the call records: a function of what the calls before it left behind and of the
// call's kind.  Plain C++ (tests/cpp/test_blur_plan.cc compiles it with g++ and walks call sequences over a model of the
// streams); vsf_api.hip extract_on issues what the plan says.
//
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
//   VSF_BLUR_OWN    a call on a stream that is not ordered with the context's (a batch of the ObserveImage queue on a slot's
//                   stream): buffer 0, behind its last release, and it records the next one.
#ifndef VSF_BLUR_PLAN_H_
#define VSF_BLUR_PLAN_H_

enum VsfBlurKind { VSF_BLUR_EARLY = 0, VSF_BLUR_MAIN = 1, VSF_BLUR_LANE = 2, VSF_BLUR_OWN = 3 };

struct VsfBlurState {
  int flip = 0;                           // the buffer the last call's blur wrote (vsf_ctx: blur_flip)
  bool free_valid[2] = {false, false};    // ev_blur_free[i] has been recorded (vsf_ctx: blur_free_valid)
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

#endif  // VSF_BLUR_PLAN_H_
