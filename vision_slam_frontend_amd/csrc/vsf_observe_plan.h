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

// ---- frames that already live in device memory (vsf_observe_submit_dev) ----
// Such frames wait in a DEVICE ring of `depth` slots in the staging ring's layout (ticket t in slot t % depth), beside the
// raw frames' pinned ring and the compressed frames' ring of files.

// ObserveFrame::kind of a device frame (0 raw, VSF_FILE_JPEG = 1, VSF_FILE_PNG = 2 are the others).
enum { kObserveKindDevice = 3 };

// One call's n consecutive frames: slots [slot0, slot0 + first), then [0, second) when they wrap the ring.
struct ObserveSpan {
  int slot0, first, second;
};
// false -- and *span untouched -- unless 1 <= n <= depth - (next_ticket - next_collect): a call never takes a slot whose
// frame has not been collected.
bool observe_submit_span(int64_t next_ticket, int64_t next_collect, int depth, int n, ObserveSpan* span);

// A batch's frames [t0, t0 + n) by where their images come from: a run is a stretch of frames of one class whose slots are
// contiguous in the rings -- what ONE copy command can carry.
enum { kObserveRunRaw = 0, kObserveRunCompressed = 1, kObserveRunDevice = 2 };
struct ObserveRun {
  int cls;    // kObserveRun*
  int f0, n;  // frames [f0, f0 + n) of the batch
  int slot0;  // the ring slot of frame f0; slot0 + n <= depth
};
// kinds[f]: ObserveFrame::kind of the batch's frame f.  Runs come in frame order and are maximal: a new one starts where the
// class changes or the ring wraps (at most once: n <= depth).  false: an argument is out of range; `runs` keeps its storage
// from batch to batch.
bool observe_batch_runs(const uint8_t* kinds, int n, int64_t t0, int depth, std::vector<ObserveRun>* runs);

// ---- frames of another size than the context's (vsf_observe_set_input_size) ----
// A stream with a declared size W x H hands in frames of that size; k_resize.hip brings them to the context's size inside the
// batch.  Until then they wait in rings of their own, whose slots hold a frame of ANY declared size:
//   an image of W x H has its rows observe_input_pitch(W) apart (W rounded up to 64, the staging rule) and takes
//   observe_input_image_bytes(W, H) = pitch * H rounded up to 256 bytes;
//   `half`, the place of one image, is the largest of these over the declared sizes; a slot is 2 * half: the left image at
//   its start, the right one `half` behind it -- so the 2 n images of n consecutive slots lie `half` apart, whatever their
//   size, and one resize launch takes them.
size_t observe_input_pitch(int w);               // 0: w outside 1 .. 32767
size_t observe_input_image_bytes(int w, int h);  // 0: a size outside 1 .. 32767
// in_w[s], in_h[s]: stream s's declared size, 0 x 0: none.  0: no stream has one (or an argument is out of range).
size_t observe_input_half_bytes(const int* in_w, const int* in_h, int n_streams);
// A frame of packed colour (VSF_PIX_BGR8 ..., bpp = 3 or 4 bytes per pixel; bpp = 1: the functions above) waits in the same
// big slots, whether its stream has a declared size or not: its rows are w * bpp bytes, observe_pix_pitch apart (rounded
// up to 64, the same rule in bytes), and `half` is at least observe_pix_image_bytes of the largest such frame seen.
// 0: w or h outside 1 .. 32767, another bpp, or an image of 2^31 bytes or more (the conversion kernel addresses an image
// with 32-bit offsets).
size_t observe_pix_pitch(int w, int bpp);
size_t observe_pix_image_bytes(int w, int h, int bpp);
// A ring of `depth` such slots, 0 where there is none.
size_t observe_input_ring_bytes(int depth, size_t half);

// Where a batch's resized frames lie and what takes them to the batch's images.  A frame waits either STAGED -- raw host
// frames in the pinned ring of big slots, uploaded into the batch's own buffer of big slots; compressed frames decoded into
// that buffer: both at the index the frame has in the batch -- or in the DEVICE ring of big slots, at its ring slot.
enum { kObserveInStaged = 0, kObserveInDeviceRing = 1 };
struct ObserveResizeIn {  // a frame of the batch
  int w, h;               // its declared size, 0 x 0: it is not resized
  uint8_t kind;           // ObserveFrame::kind
};
struct ObserveResizeRun {  // ONE resize launch: 2 n images of w x h, `half` apart, from slot `src0` on
  int where;               // kObserveIn*
  int f0, n;               // frames [f0, f0 + n) of the batch
  int src0;                // staged: f0; device ring: the ring slot of frame f0 (src0 + n <= depth)
  int w, h;
};
struct ObserveUpload {  // ONE copy command out of the pinned ring of big slots: batch frames [f0, f0 + n), ring slots
  int f0, n, slot0;     // [slot0, slot0 + n) (slot0 + n <= depth), into the batch's big slots [f0, f0 + n)
};
struct ObserveResizePlan {
  std::vector<ObserveResizeRun> runs;  // in frame order, maximal: a run ends where the size or the place changes, or the ring wraps
  // The raw host frames among them, as copy commands.  A copy command has a fixed cost whatever it carries, so slots that hold
  // nothing of the raw resized frames are carried along where that is cheaper than a command of their own: a gap of up to
  // `max_gap` such slots between two raw resized frames is bridged, a longer one ends the upload (max_gap = 0: nothing is
  // carried along).  An upload also ends where the ring wraps.  Every upload begins and ends with a raw resized frame.
  std::vector<ObserveUpload> uploads;
  int n_resized = 0;
};
// The gap worth bridging for slots of `slot_bytes`: what a link of kObserveLinkBytesPerUs carries in the kObserveCopyCommandUs a
// copy command costs by itself (NOTES.md: 180 us whatever it carries; 50 GB/s: 9 MB).  BOTH constants come from this
// repository's earlier notes on the queue's first upload; neither was measured for this path.
enum { kObserveCopyCommandUs = 180, kObserveLinkBytesPerUs = 50000 };
int observe_upload_max_gap(size_t slot_bytes);
// false: an argument is out of range (n > depth, a size with one side 0, a kind that does not exist, max_gap < 0); `plan`
// keeps its storage.
bool observe_resize_plan(const ObserveResizeIn* in, int n, int64_t t0, int depth, int max_gap, ObserveResizePlan* plan);

// ---- the ingest of a batch: what every frame is, and which commands take the batch's images to its own buffer ----
// (vsf_observe_ingest.hip ingest() executes this and decides nothing of it again)
bool observe_pix_is_bayer(int pixfmt);  // VSF_PIX_BAYER_*

// What a frame is.  OWN-size frames have the context's size and lie where the staging ring's layout puts them (raw: the
// pinned staging ring, file: the ring of files, device: the device ring); BIG-slot frames have a declared size or packed
// colour and wait in the rings of big slots (a file: in the ring of files all the same) until k_resize.hip / the gray
// conversion brings them to the batch's images.
enum ObserveFrameClass : uint8_t {
  kObserveOwnRaw = 0, kObserveOwnFile, kObserveOwnDevice, kObserveBigRaw, kObserveBigFile, kObserveBigDevice
};
// The step of the copy stream's sequence (raw upload, device copies, decode of own-size files, ..., decode of big-slot files)
// behind which a command that exists ONCE per batch runs.
enum { kObserveStepNone = 0, kObserveAfterUpload, kObserveAfterDeviceCopies, kObserveAfterDecode, kObserveAfterBigDecode };

struct ObserveIngestIn {  // a frame of the batch: ObserveFrame::kind[0], its declared size (0 x 0: none), ObserveFrame::pix_new
  uint8_t kind;
  bool pix_new;
  int in_w, in_h;
};
struct ObserveIngestPlan {
  std::vector<ObserveIngestIn> in;  // [n] the caller fills it in its ONE pass over the batch's frames
  std::vector<uint8_t> cls;         // [n] ObserveFrameClass
  bool raw = false, files = false, dev = false;  // an own-size frame of that kind is there
  bool big = false, big_files = false, big_dev = false;  // a big-slot frame; one that is a file / a device frame
  int pixfmt = 0, bpp = 1;  // the batch's ONE pixel format and its bytes per pixel
  bool mosaics = false;     // ... is a Bayer order: own-size images go through the mosaics' buffer
  // An own-size Bayer batch is demosaiced ONCE, behind the last step that wrote mosaics: kObserveAfterUpload / AfterDeviceCopies /
  // AfterDecode; kObserveStepNone: not mosaics, or no own-size frame.
  int demosaic = kObserveStepNone;
  // The ingest finish (an image its decoder refused becomes all zero) is owed when a frame is a file, and runs ONCE, behind the
  // last step that decodes files: kObserveAfterDecode / AfterBigDecode; kObserveStepNone: no file.
  int finish = kObserveStepNone;
  int own_pix_new = 0;      // own-size frames with pix_new of a mosaics batch (vsf_observe_stats [30], [31])
  bool multi_size = false;  // big-slot frames are there and the batch's frames came in at more than one size
  std::vector<ObserveRun> runs;  // own-size frames: the device ring's copies (big-slot device frames are read where they lie:
                                 // they are no device run).  Empty without an own-size device frame.
  ObserveResizePlan resize;      // big-slot frames.  Empty without one.
  std::vector<uint8_t> run_kinds;          // (scratch: the batch as observe_batch_runs ...
  std::vector<ObserveResizeIn> resize_in;  //  ... and observe_resize_plan take it)
};
// Classifies plan->in[0, n) -- the frames of tickets [t0, t0 + n) in rings of `depth` slots -- and plans their ingest.
// may_resize: the queue has seen a big-slot frame (until then no record's declared size means anything); max_gap:
// observe_upload_max_gap of a big slot.  `plan` keeps its storage from batch to batch.  false: an argument is out of range.
bool observe_ingest_plan(int n, int pixfmt, int64_t t0, int depth, bool may_resize, int max_gap, ObserveIngestPlan* plan);

}  // namespace vsfi

#endif  // VSF_OBSERVE_PLAN_H_
