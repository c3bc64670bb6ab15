// vsf_observe_plan.h -- the arithmetic of one batch of the ObserveImage queue (vsf_observe.hip launch_batch), plain C++: which
// descriptor set every frame's filtered left / right frame goes to, which earlier sets it is matched against, the pair list
// the ONE matcher launch and the ONE sort launch of the tail walk, the batch's distinct calibrations, and where a run of
// waiting frames must be cut into batches.  No device, no context: tests/cpp/test_observe_plan.cc runs it on the CPU.
//
// The queue takes frames of n_streams independent sequences (vsf_observe_set_streams).  Frame k of stream s -- k counts that
// stream's frames since the queue was built or the stream was reset -- keeps its filtered left frame in set
// s * ring + k % ring; its temporal pairs are that stream's min(k, life) predecessors, oldest first (the order frame_list_ is
// walked in, slam_frontend.cc:424); its right frame lives for the length of the tail in set n_streams * ring + (index in the
// batch).  ring >= life + (frames of one stream a batch may hold), so a batch never overwrites a set it still reads.
#ifndef VSF_OBSERVE_PLAN_H_
#define VSF_OBSERVE_PLAN_H_

#include <cstdint>
#include <vector>

#include "../../include/vsf.h"

namespace vsfi {

struct ObservePlanIn {  // a waiting frame
  int32_t stream;
  int64_t k;  // frames of its stream in front of it
  const vsf_calibration* calib;
  float best_percent;
};

struct ObservePlanFrame {
  int32_t left_set, right_set;
  int32_t n_past;  // temporal pairs
  int32_t tp0;     // index of its first temporal pair in the pair list (its right -> left pair is pair f)
  int32_t stream;
  int32_t calib;  // index into ObservePlan::calibs
  float best_percent;
  int32_t prev;  // the frame of its stream in front of it IN THIS BATCH, -1: none (its threshold is the stream's state)
  int32_t tail;  // where prev < 0: the last frame of its stream in this batch (whose mean the stream's state takes)
};

struct ObservePlan {
  std::vector<ObservePlanFrame> frames;  // [n]
  // pairs [0, n): Calculate3DPoints' right -> left match of frame f with best_percent 1 (cc:129-132); then every frame's
  // temporal pairs, frame after frame
  std::vector<int32_t> q_set, t_set;
  std::vector<float> best_percent;
  std::vector<vsf_calibration> calibs;  // the batch's calibrations, each once, in order of first use
  // Indices i in (0, n) where frame i brings another calibration or best_percent than the frame of ITS OWN stream in front
  // of it in the list: frame i starts a new batch.  Frames of different streams may differ in both and share one.
  std::vector<int32_t> cuts;
  int n_pairs = 0;
  int max_pairs_per_frame = 1;
  int n_streams_present = 0;  // distinct streams among the frames
};

// Whether `b`, waiting behind frame `a` of the same stream, may not share a's batch.
bool observe_plan_must_cut(const vsf_calibration& a_calib, float a_best_percent, const vsf_calibration& b_calib,
                           float b_best_percent);

// Plans frames in[0, n) as ONE batch (the sets, the pairs, the calibration table) and notes in `cuts` where the list would
// have to be cut; the caller launches a list without cuts.  `plan` is reused from batch to batch (its vectors keep their
// storage).  false: an argument is out of range (a stream outside [0, n_streams), k < 0, ring < life + 1, ...).
bool observe_plan(const ObservePlanIn* in, int n, int n_streams, int ring, int life, ObservePlan* plan);

}  // namespace vsfi

#endif  // VSF_OBSERVE_PLAN_H_
