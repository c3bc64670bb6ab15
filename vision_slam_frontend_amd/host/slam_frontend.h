// slam_frontend.h -- host-side mirror of the reference's slam::Frontend (src/slam_frontend.h:117-142) on top of
// the C ABI of include/vsf.h.  Same public method names and semantics:
//   ObserveImage (cc:400-472), ObserveOdometry (cc:250-263), GetSLAMProblem (cc:498-503), GetNumPoses (cc:505),
//   GetConfig (h:142), the debug-image getters (cc:474-495; drawn on the GPU by vsf_draw_canvases, csrc/k_draw.hip).
// cv::Mat is replaced by slam::Image (a non-owning view) and Eigen types by the PODs of slam_types.h; both swaps
// are mechanical for a maintainer who has OpenCV / Eigen.  The two private methods that call
// OpenCV in the reference -- ExtractFeatures (cc:266) and GetMatches (cc:521) -- call vsf_extract /
// vsf_get_matches here; everything else is the reference's own host logic restated.
#ifndef VSF_HOST_SLAM_FRONTEND_H_
#define VSF_HOST_SLAM_FRONTEND_H_

#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vsf.h"
#include "../csrc/vsf_glibc_random.h"  // glibc's rand(), shared with the queue's colour kernel
#include "slam_types.h"
#include "slam_visualization.h"

namespace slam {

using slam_types::Quaternionf;
using slam_types::Vector2f;
using slam_types::Vector3f;

// Non-owning 8-bit image view (stands in for `const cv::Mat&`): single-channel unless `channels` says otherwise (the debug
// images are 3-channel, bytes in OpenCV's B, G, R order).
struct Image {
  const uint8_t* data = nullptr;
  int rows = 0, cols = 0;
  size_t step = 0;
  int channels = 1;
  Image() {}
  Image(const uint8_t* d, int r, int c, size_t s, int ch = 1) : data(d), rows(r), cols(c), step(s), channels(ch) {}
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
};

// src/slam_frontend.h:42-56
struct CameraIntrinsics {
  float k1, k2, k3;
  float p1, p2;
  float fx, fy, cx, cy;
};

struct Matrix3f {
  float m[9];  // row-major
  float operator()(int r, int c) const { return m[3 * r + c]; }
  float& operator()(int r, int c) { return m[3 * r + c]; }
};

// Eigen::Affine3f as the reference uses it (h:96, cc:613-618, slam_frontend_main.cc:341-344): a rotation and a
// translation, `Translation3f(XT) * RT`.
struct Affine3f {
  Matrix3f linear_;  // row-major
  Vector3f translation_;
  Affine3f() : linear_{{1, 0, 0, 0, 1, 0, 0, 0, 1}} {}
  Affine3f(const Matrix3f& rotation, const Vector3f& translation) : linear_(rotation), translation_(translation) {}
  Vector3f translation() const { return translation_; }
  // (Eigen's Transform::rotation() of an affine transform takes the closest rotation of the linear part by SVD; the linear
  // part IS a rotation here -- cc:614-617 -- so it is returned as it is: equal to float rounding)
  Matrix3f rotation() const { return linear_; }
  Matrix3f linear() const { return linear_; }
  Vector3f operator*(const Vector3f& p) const {
    return Vector3f((linear_(0, 0) * p.x() + linear_(0, 1) * p.y()) + linear_(0, 2) * p.z() + translation_.x(),
                    (linear_(1, 0) * p.x() + linear_(1, 1) * p.y()) + linear_(1, 2) * p.z() + translation_.y(),
                    (linear_(2, 0) * p.x() + linear_(2, 1) * p.y()) + linear_(2, 2) * p.z() + translation_.z());
  }
};

// src/slam_frontend.h:58-97; defaults are the reference's (cc:550-652) except where noted in the .cc.
struct FrontendConfig {
  enum class DescriptorExtractorType { AKAZE, ORB, BRISK, SURF, SIFT, FREAK };
  FrontendConfig();
  bool debug_images_;
  // An addition the reference does not have: 1 .. 100 makes the queued modes keep the debug images as JPEG files of that quality
  // (what cv::imencode(".jpg") writes for them; vsf_observe_set_debug_jpeg) INSTEAD of the raw images -- the raw getters below
  // then return nothing.  0 (the default): raw images.  Ignored in per-call mode.
  int debug_jpeg_quality_;
  // The same, lossless: the queued modes keep the debug images as PNG files (what cv::imencode(".png") writes for them;
  // vsf_observe_set_debug_png).  Off by default; ignored in per-call mode; not together with debug_jpeg_quality_ (the second of
  // the two to be asked for is refused with VSF_ERR_INVALID_ARG).
  bool debug_png_;
  // An addition: where the stereo lines' colours (cc:95) come from.  false (the default): the process's rand(), as in the
  // reference.  true: a generator the OBJECT owns -- srand(debug_colour_seed_), rand(), rand(), ... as glibc computes them
  // (csrc/vsf_glibc_random.h) -- on the device in the queued modes (vsf_observe_set_debug_seeds), on the host in per-call mode;
  // the process's rand() is then never called.  Seed 1 is what a fresh process draws.  A context that is replaced in the
  // middle of a sequence (another image size, pipelining switched on) starts the sequence over, in every mode.  What a FrontendGroup's members need
  // to have debug images at all: one sequence shared by several cameras would not be any camera's own.
  bool debug_colour_seeded_;
  uint32_t debug_colour_seed_;
  // An addition: the object also builds what the reference's driver publishes to RViz after every pose (PublishVisualization,
  // slam_frontend_main.cc:194-225) -- the point cloud on the GPU, inside the queue's batches, the pose graph while nodes and
  // factors are booked -- for Frontend::GetVisualization.  Off by default: nothing is launched, copied or kept for it.
  bool visualization_;
  // An addition: which of cv::imdecode's flags ObserveCompressedImage mirrors.  1 (the default): IMREAD_GRAYSCALE, the
  // reference's (slam_frontend_main.cc:100).  2, 4, 8: IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8 -- a JPEG payload of W x H is
  // decoded by libjpeg's reduced inverse DCTs straight to ceil(W / N) x ceil(H / N) pixels (vsf_observe_submit_compressed_reduced),
  // which is then the image size of the object.  The calibration in this configuration is the caller's, FOR THE REDUCED
  // IMAGE: nothing is scaled.  PNG payloads are refused at N > 1 (VSF_ERR_UNSUPPORTED), and so are bayer_rggb8 frames
  // (VSF_ERR_INVALID_ARG: a mosaic cannot be reduced in the DCT domain).  In a FrontendGroup it is per member: a 1280 x 960
  // camera at 2 and a 640 x 480 camera at 1 share one 640 x 480 context.
  int imdecode_reduce_;
  // The Bayer order of compressed topics (ObserveCompressedImage with bayer_rggb8 set): one of VSF_PIX_BAYER_RGGB8 (the
  // default: the reference's PointGrey pair), _GRBG8, _GBRG8, _BGGR8 -- vsf_observe_set_bayer_order.
  int bayer_order_;
  // An addition: cv::resize(img, Size(resize_width_, resize_height_)) in front of everything (0 x 0, the default: off).  When
  // set, the object's context has THAT size and ObserveImage / ObserveDeviceImage / ObserveCompressedImage take frames of the
  // camera's own size, whatever it is: the queue declares it to the object's stream (vsf_observe_set_input_size) and resizes
  // on the device inside the batch; per-call mode resizes through vsf_resize_gray.  A frame of another size than the one
  // before books what is in flight, then re-declares.  The calibration is the caller's, for the RESIZED image.  Device frames
  // have no size of their own: image_width x image_height states the camera's.  With imdecode_reduce_ > 1 as well, compressed
  // frames are refused (VSF_ERR_INVALID_ARG: the two are not combined).  In a FrontendGroup the field is per member; the
  // resized size -- the context's -- is what the members must agree on.
  int resize_width_, resize_height_;
  // An addition: cv::ORB::detectAndCompute's (and FastFeatureDetector::detect's) mask argument, which the reference leaves at
  // cv::noArray() (cc:274-277): 8-bit views of the CONTEXT's size (the resized size where resize_width_ is set), non-zero where
  // a corner may sit -- the hood, the other eye's housing, a rectification wedge, a time stamp are zero.  Empty (the default):
  // no mask.  The object copies the masks when it is built (and in set_masks), and sets them when its context is created
  // (vsf_mask_set; include/vsf.h "Detection masks" states OpenCV's rule): in every mode the left image takes mask_left_ and
  // the right image mask_right_.  A mask of another size than the context's is refused with VSF_ERR_INVALID_ARG.  In a
  // FrontendGroup the pair is per member.
  Image mask_left_, mask_right_;
  // An addition: bytes one compressed payload may have (vsf_observe_set_compressed_cap), applied when the context is created.
  // 0 (the default): the library's, width x height + 64 KB OF THE CONTEXT'S SIZE -- with imdecode_reduce_ > 1 that is the
  // REDUCED size, and a camera's files of N times the side are usually larger: set this (vsf_observe_default_compressed_cap of
  // the camera's own size is a good value), or the payloads are refused with VSF_ERR_CAPACITY.  One value per context: a
  // FrontendGroup takes member 0's, and set_compressed_cap on any member sets the group's.
  size_t compressed_cap_;
  DescriptorExtractorType descriptor_extract_type_;
  float best_percent_;
  float nn_match_ratio_;
  float min_odom_translation;
  float min_odom_rotation;
  uint32_t min_vision_matches;
  uint32_t frame_life_;
  CameraIntrinsics intrinsics_left, intrinsics_right;
  float projection_left[12], projection_right[12];  // 3x4 row-major (cv::Mat CV_32F in the reference)
  Matrix3f fundamental;
  // Affine transform from the frame of the left camera to the robot (h:96; literals cc:613-618; the reference's caller
  // reads it through GetConfig() for the CameraExtrinsics message and the point cloud, slam_frontend_main.cc:158, 342).
  Affine3f left_cam_to_robot;
  // ORB parameters the reference hard-codes in cv::ORB::create (cc:205-213); exposed so BASELINE configs can set
  // nfeatures = 2000 / 8000.
  int orb_nfeatures;
  // cv::ORB::create's scoreType (vsf_params::score_type): VSF_SCORE_HARRIS (0, the reference's literal, the default) or
  // VSF_SCORE_FAST (1: one cut per level on the FAST score, no Harris responses; a frame can hold more than orb_nfeatures
  // keypoints, see include/vsf.h).  Honoured in per-call, synchronous and pipelined mode alike -- the mode belongs to the
  // context; the members of a FrontendGroup share one context and must agree on it.
  int orb_score_type_;
  // How RemoveAmbigStereo's three-term dot products are summed (vsf_params::residual_order): 0 = as Eigen 3.3 does,
  // a0 b0 + (a1 b1 + a2 b2) (default); 1 = left to right.
  int residual_order;
  // Image geometry the GPU context is created for (the reference takes it from the first cv::Mat).
  int image_width, image_height;
};

// FrontendConfig's stereo calibration in the layout of the C ABI (include/vsf.h vsf_calibration).
vsf_calibration MakeCalibration(const FrontendConfig& config);
// The size of the context a configuration asks for: resize_width_ x resize_height_ where set, else image_width x image_height.
int ContextWidth(const FrontendConfig& config);
int ContextHeight(const FrontendConfig& config);
// config.left_cam_to_robot as the 3 x 4 row-major matrix the point cloud's calls take, and such a matrix as the transform.
void CamToRobot(const FrontendConfig& config, float out[12]);
Affine3f AffineFromRowMajor(const float m[12]);

using slam_visualization::Visualization;
// The driver's AddFeaturePoints with its own signature (slam_frontend_main.cc:155-157): the CPU restatement of the cloud.
inline void AddFeaturePoints(const FrontendConfig& config, const slam_types::SLAMProblem& problem,
                             slam_visualization::Marker* marker_ptr) {
  float c[12];
  CamToRobot(config, c);
  slam_visualization::AddFeaturePoints(c, problem, marker_ptr);
}

// src/slam_frontend.h:100-114
class Frame {
 public:
  Frame(const std::vector<vsf_keypoint>& keypoints, const std::vector<uint8_t>& descriptors, uint64_t frame_ID);
  Frame() : frame_ID_(0) {}
  uint64_t frame_ID_;
  std::vector<vsf_keypoint> keypoints_;
  std::vector<bool> is_initial_;
  std::vector<int64_t> initial_ids_;
  std::vector<uint8_t> descriptors_;  // keypoints_.size() x 32, row-major (cv::Mat CV_8U in the reference)
};

class FrontendGroup;

class Frontend {
 public:
  // config_path is ignored exactly as in the reference (quirk Q1: FrontendConfig::Load is never defined).
  explicit Frontend(const std::string& config_path);
  Frontend(const std::string& config_path, const FrontendConfig& config, int device = 0);
  ~Frontend();
  Frontend(const Frontend&) = delete;
  Frontend& operator=(const Frontend&) = delete;

  // True iff a new SLAM node was added.  Never throws; a failing GPU call is reported by last_status().
  bool ObserveImage(const Image& left_image, const Image& right_image, double time);
  // The same for raw frames of any pixel format (VSF_PIX_*, include/vsf.h: sensor_msgs/Image as the driver publishes it --
  // mono8, the four bayer_*8 orders, bgr8 / rgb8 / bgra8 / rgba8): cols x rows PIXELS, `step` in BYTES.  The frame becomes
  // gray on the device (inside the queue's batch; in per-call mode by one vsf_to_gray call in front of the steps) and is
  // observed exactly as ObserveImage observes that gray image: the problem is the same, byte for byte.  VSF_PIX_MONO8 is the
  // call above.  An unknown code or a step below cols x bytes per pixel: false, last_status() == VSF_ERR_INVALID_ARG, nothing booked.
  bool ObserveImage(const Image& left_image, const Image& right_image, double time, int pixfmt);
  // The reference's CompressedImageCallback in one call (slam_frontend_main.cc:98-133): the two messages' payloads -- JPEG
  // (baseline or progressive) or PNG -- are decoded on the GPU inside the queue (cv::imdecode IMREAD_GRAYSCALE; with
  // bayer_rggb8 also COLOR_BayerBG2BGR + COLOR_BGR2GRAY) and observed exactly as ObserveImage observes the decoded images,
  // synchronous or pipelined.  OdomCheck comes first: a gated frame is not parsed.  A file the host refuses (malformed or
  // unsupported header, another size, above the queue's byte cap) books nothing: false, last_status() says why.  A file
  // the DEVICE refuses (broken PNG data, a JPEG stream that breaks off at a missing restart marker) is observed as an
  // all-zero image -- a node without features (defined deviation, include/vsf.h).  refused_frames() counts such frames
  // as they are booked and never goes back; last_status() reads VSF_ERR_INVALID_ARG right after that booking only, i.e. in
  // synchronous mode -- a pipelined Frontend books frames inside later calls, whose own status follows at once, so there
  // the counter is the way to learn of it.  The host keeps no copy of such a frame's pixels: with debug_images_ on,
  // getDebugImages() / getDebugStereoImages() hold canvases drawn on the GPU from the DECODED (and demosaiced) images.
  bool ObserveCompressedImage(const uint8_t* left, size_t left_bytes, const uint8_t* right, size_t right_bytes,
                              bool bayer_rggb8, double time);
  // The same frame when it ALREADY LIVES IN DEVICE MEMORY (a tensor, a decoder's or camera SDK's buffer, the caller's own
  // kernel's output): two images of the context's size (config.image_width x image_height, or whatever earlier frames
  // were) on the context's device, any base address, any pitch >= width, stream-ordered on `hip_stream` (a hipStream_t;
  // NULL: the default stream) like hipMemcpyAsync -- the images may still be being produced by work queued on that stream
  // and may be overwritten by work queued on it after the call (vsf_observe_submit_dev).  bayer_rggb8: the images are
  // mosaics (COLOR_BayerBG2BGR + COLOR_BGR2GRAY on the device).  OdomCheck and the bookkeeping are ObserveImage's;
  // synchronous or pipelined; the problem is the one ObserveImage builds from the same pixels, byte for byte.
  bool ObserveDeviceImage(const void* left, size_t left_pitch, const void* right, size_t right_pitch, void* hip_stream,
                          double time, bool bayer_rggb8 = false);
  // ... of any pixel format (VSF_PIX_*): a pitch is >= width x bytes per pixel.
  bool ObserveDeviceImage(const void* left, size_t left_pitch, const void* right, size_t right_pitch, void* hip_stream,
                          double time, int pixfmt);
  // config.bayer_order_ (one of the four VSF_PIX_BAYER_* codes; anything else: VSF_ERR_INVALID_ARG and no change).  Legal
  // at any time: it is read by the next ObserveCompressedImage with bayer_rggb8 set, which books the frames in flight
  // before the queue is told (vsf_observe_set_bayer_order).
  void set_bayer_order(int pixfmt);
  void ObserveOdometry(const Vector3f& translation, const Quaternionf& rotation, double timestamp);
  void GetSLAMProblem(slam_types::SLAMProblem* problem) const;
  int GetNumPoses();
  FrontendConfig GetConfig() { return config_; }
  // The four markers of the driver's PublishVisualization (slam_frontend_main.cc:194-225) for the frames BOOKED SO FAR, with
  // config.visualization_ on (else false and VSF_ERR_INVALID_ARG): nodes (id 0, POINTS), odometry factors (1, LINE_LIST),
  // vision factors (2, LINE_LIST), the point cloud (3, POINTS, colours (1, 1, 1, 0.2)), frame "map".
  //   Unlike GetSLAMProblem and the accessors below this call does NOT flush the queue: it first books the frames whose
  // results are already there -- it never waits for the GPU and sends nothing early -- and reports those, so a driver that asks
  // after every node keeps the queue's batches whole.  After Flush() it is complete: every observed frame is in it, and the
  // markers are, byte for byte, those of the synchronous modes and of slam_visualization::BuildVisualization on the problem.
  //   The pose graph is host bookkeeping made while nodes and factors are booked; the cloud is the concatenation of the
  // booked frames' device-made points (vsf_observe_set_world_points; per-call mode: one vsf_world_points per node).  A node's
  // pose never changes once booked, so everything here only grows: handing the SAME Visualization object in again appends
  // what is new (its markers must not have been edited in between); any other object is filled from scratch.
  bool GetVisualization(Visualization* out);
  void set_visualization(bool on);  // config.visualization_, under the rule of set_debug_images
  // config.left_cam_to_robot as a 3 x 4 row-major matrix, under the same rule (a group's member: its stream's own)
  void set_left_cam_to_robot(const float m[12]);
  // config.projection_left / projection_right (3 x 4 row-major) after construction, under the same rule: a stereo rig other than
  // the reference's hard-coded one (cc:595-611) -- what Calculate3DPoints triangulates with.
  void set_projections(const float left[12], const float right[12]);
  // The cloud as the object keeps it: three doubles per point, booked frames in order (valid until the next call that books).
  const std::vector<double>& visualization_cloud() const { return cloud_; }
  // cc:474-495.  With config.debug_images_ on, every node keeps a match image (CreateMatchDebugImage, cc:100-115; from the
  // second node on) and a stereo image (CreateStereoDebugImage, cc:74-98; unless the node has no stereo match, cc:131-133)
  // for the object's lifetime.  Like GetNumPoses these book the frames still in flight first; the views point into memory
  // the object owns and stay valid while it lives.
  std::vector<Image> getDebugImages();
  Image GetLastDebugImage();
  Image GetLastDebugStereoImage();
  std::vector<Image> getDebugStereoImages();
  // The newest match / stereo image as a JPEG file (config.debug_jpeg_quality_ > 0) or a PNG file (config.debug_png_), queued
  // modes: the payload of a sensor_msgs/CompressedImage whose format string is `format` ("jpeg" / "png", slam_to_ros.h).
  // {nullptr, 0, nullptr} when there is none.  Valid while the object lives.
  struct CompressedView {
    const uint8_t* data = nullptr;
    size_t size = 0;
    const char* format = nullptr;
  };
  CompressedView GetLastDebugImageCompressed();
  CompressedView GetLastDebugStereoImageCompressed();

  // Additions (not in the reference): error reporting instead of abort, and read access for tests.
  vsf_status last_status() const { return last_status_; }
  // Frames booked so far whose compressed file the DEVICE refused (observed as an all-zero image); sticky.
  uint64_t refused_frames() const { return refused_frames_; }
  // true (default): ObserveImage is one GPU submission (vsf_observe_stereo); false: one C-ABI call per reference call
  // (vsf_extract_pair, vsf_get_matches, ...) with the reference's host steps in between.  Same results; choose before
  // the first ObserveImage.
  void set_fused(bool on);
  // ObserveImage's return value is OdomCheck's decision (cc:404-409): nothing in the reference's control flow needs a
  // frame's features before the next frame arrives.  With pipelining on (fused mode; choose before the first
  // ObserveImage) a call copies its frame into the GPU context's queue (vsf_observe_submit) and returns; frames that wait
  // there leave for the GPU as ONE batched extraction + tail, and a frame's result is collected and booked -- in frame
  // order, with the odometry of ITS call -- as soon as a later call finds it finished, at the latest when the queue is full
  // (queue_depth() frames later) or when anything reads the problem (GetSLAMProblem, GetNumPoses, the accessors below,
  // Flush).  Same nodes, factors and bytes as the
  // synchronous mode; a GPU failure then surfaces in last_status() some calls late.
  void set_pipelined(bool on);
  // config.debug_images_ after construction (before the first ObserveImage; later calls fail with VSF_ERR_INVALID_ARG).
  void set_debug_images(bool on);
  void set_debug_jpeg_quality(int quality);  // config.debug_jpeg_quality_, under the same rule
  void set_debug_png(bool on);               // config.debug_png_, under the same rule
  // config.debug_colour_seeded_ / debug_colour_seed_, under the same rule; the generator starts over.  (A group's member: the
  // seeds are the queue's and go in when the group is built -- VSF_ERR_INVALID_ARG.)
  void set_debug_colour_seed(bool seeded, uint32_t seed);
  // config.imdecode_reduce_ (1, 2, 4, 8; anything else: VSF_ERR_INVALID_ARG and no change).  Legal at any time: it is read by
  // each ObserveCompressedImage; the image size stays what the first frame made it.
  void set_imdecode_reduce(int reduce);
  // config.resize_width_ / resize_height_ (0, 0: off; one side 0 or a side above 32767: VSF_ERR_INVALID_ARG and no change);
  // camera_width x camera_height > 0: config.image_width / image_height as well (what device frames are taken to be).
  // Before the first frame, or at any time: the next frame sizes the context and declares its own size.
  void set_resize(int width, int height, int camera_width = 0, int camera_height = 0);
  // config.mask_left_ / mask_right_ (an empty view: no mask for that eye); the object keeps copies.  At any time: a context
  // that exists takes them at once (vsf_mask_set sends every frame still waiting in the queue first, so frames observed before
  // the call keep the masks they were observed with); otherwise the next context does.
  void set_masks(const Image& left, const Image& right);
  // config.compressed_cap_.  Before the first compressed frame, or while no frame is in flight (vsf_observe_set_compressed_cap's
  // rule; otherwise last_status() says VSF_ERR_INVALID_ARG and nothing changes on the device).
  void set_compressed_cap(size_t cap_per_image);
  // Frames ObserveImage may leave in the queue when pipelined (1..1024, default 256) and the most frames one batch carries
  // (default 128; the context's extraction buffers are sized for it: ~25 MB of HBM per 640x480 frame; the queue's staging
  // and result rings are pinned host memory: depth x (two images + vsf_observe_capacity)).  Measured on an MI355X at
  // 640x480 / 2000 features: depth 32 19 k frames/s, 64 25 k, 128 (64 per batch) 28 k, 256 (128 per batch) 32 k.
  void set_queue_depth(int n);
  void set_frames_in_flight(int n) { set_queue_depth(n); }  // (the name of rounds 3-5)
  void set_batch_frames(int n);
  // While the GPU is busy, fewer waiting frames than this stay in the queue (0: a whole batch, or half the queue's depth
  // when that is less; 1: whatever waits leaves as soon as fewer than two batches are on the GPU).
  void set_min_batch(int n);
  // The queue's host threads: the staging-copy helper (VSF_OPT_OBSERVE_COPY_THREAD, on by default) and the launcher
  // (VSF_OPT_OBSERVE_THREAD, off by default: with frames gathering into batches it only pays on a host whose launches
  // are what bounds the caller, and costs where depth = batch).
  void set_queue_thread(bool on);
  void set_copy_thread(bool on) { copy_thread_ = on; }
  // Any vsf_option of the context (applied when it is created): launch choices only, results never depend on them.
  void set_context_option(int option, int value) { ctx_options_.push_back({option, value}); }
  // The GPU context behind the object (nullptr before the first image / without image_width): for tools that read its
  // per-stage timers or queue statistics; whoever calls an entry point on it shares the object's single-caller rule.
  vsf_ctx* context() const { return ctx_; }
  // vsf_observe_stats of the context (frames, batches, largest batch, ...): how the queue coalesced.
  void queue_stats(int64_t out[11]) const { for (int i = 0; i < 11; i++) out[i] = 0; if (ctx_) vsf_observe_stats(ctx_, out, 11); }
  int queue_depth() const { return pipelined_ ? depth_ : 1; }
  int frames_in_flight() const { return queue_depth(); }
  int batch_frames() const { return pipelined_ ? (depth_ < batch_frames_ ? depth_ : batch_frames_) : 1; }
  bool Flush();  // collects and books every frame still in flight; false (and last_status()) if one of them failed
  float stereo_ambig_constraint() const { Sync(); return stereo_ambig_constraint_; }
  const std::vector<Frame>& frame_list() const { Sync(); return frame_list_; }
  const std::vector<slam_types::SLAMNode>& nodes() const { Sync(); return nodes_; }
  const std::vector<slam_types::VisionFactor>& vision_factors() const { Sync(); return vision_factors_; }
  const std::vector<slam_types::OdometryFactor>& odometry_factors() const { Sync(); return odometry_factors_; }

 private:
  friend class FrontendGroup;
  // A member of a FrontendGroup: stream `stream` of the group's one context and queue.
  Frontend(const FrontendConfig& config, int device, FrontendGroup* group, int stream);
  bool OdomCheck();
  bool ExtractFeatures(const Image& image, Frame* curr_frame, int eye = 0);  // eye: 0 the left image, 1 the right one
  // The two ExtractFeatures calls of ObserveImage (cc:411-412) as one batch of two images (vsf_extract_pair).
  bool ExtractFeaturesPair(const Image& left, const Image& right, Frame* left_frame, Frame* right_frame);
  // The temporal loop of ObserveImage (cc:424-434): GetFeatureMatches of every past frame against the new one, with
  // the matcher run once for all of them (vsf_get_matches_multi); same factors, same order, same bookkeeping.
  void GetFeatureMatchesAll(std::vector<Frame>* past_frames, Frame* curr_frame,
                            std::vector<slam_types::VisionFactor>* out);
  slam_types::VisionFactor GetFeatureMatches(Frame* past_frame_ptr, Frame* curr_frame_ptr);
  std::vector<vsf_dmatch> GetMatches(const Frame& frame_query, const Frame& frame_train, double nn_match_ratio);
  void RemoveAmbigStereo(Frame* left, Frame* right, const std::vector<vsf_dmatch>& stereo_matches);
  void AddOdometryFactor();
  void UndistortFeaturePoints(std::vector<slam_types::VisionFeature>* features);
  void Calculate3DPoints(Frame* left_frame, Frame* right_frame, std::vector<Vector3f>* points,
                         slam_types::VisionFactor* matches_out = nullptr);
  bool EnsureContext(int width, int height);  // (a group member: the group's)
  bool EnsureOwnContext(int width, int height, int n_streams);
  // config_.mask_left_ / mask_right_ into slots 2 stream_ and 2 stream_ + 1 of `ctx` (an empty view clears its slot), named to
  // the object's stream of the queue and -- an object with a context of its own -- to the calls outside the queue.
  vsf_status ApplyMasks(vsf_ctx* ctx);
  int mask_slot(int eye) const;  // the slot of that eye's mask, -1: none
  // Per-call mode: the context's pair becomes (eye `first`, right) -- (right, right) around the one call that extracts a right
  // image on its own, (left, right), what ApplyMasks left, behind it.
  void SelectImageMasks(int first);
  void OwnMasks();  // config_'s views into copies the object owns
  std::vector<uint8_t> mask_store_[2];
  // What the configuration asks of the queue's debug images, in the order the context takes it: everything off, the seeds
  // (one per stream: a group's lead hands in every member's), the switch, the form of file.
  vsf_status ApplyDebugConfig(int n_streams);
  // The form the queue's debug images leave in, as config_.debug_jpeg_quality_ / debug_png_ ask for it: raw images, or the bit of
  // the one form of file (both bits only in a configuration the context refuses).  The ONE place that reads the pair.
  enum { kFormRaw = 0, kFormJpeg = 1, kFormPng = 2 };
  int debug_file_form() const { return (config_.debug_jpeg_quality_ > 0 ? kFormJpeg : 0) | (config_.debug_png_ ? kFormPng : 0); }
  const char* debug_file_format() const { return (debug_file_form() & kFormPng) ? "png" : "jpeg"; }  // CompressedView::format
  bool ObserveImageFused(const Image& left_image, const Image& right_image, int pixfmt = VSF_PIX_MONO8);
  bool DeclareBayerOrder();  // the queue learns config.bayer_order_ (frames in flight are booked first)
  int told_bayer_order_ = 0;  // what it was told last (0: nothing: RGGB)
  std::vector<uint8_t> gray_[2];  // per-call mode: the gray images of a frame of another pixel format
  struct FramePayload {  // what a frame brings to the queue: two raw images at `step`, two compressed files, or two
                         // images in device memory at left_bytes / right_bytes per row, ordered on `hip_stream`
    const uint8_t* left = nullptr;
    const uint8_t* right = nullptr;
    size_t step = 0, left_bytes = 0, right_bytes = 0;
    bool compressed = false, bayer = false, device = false;
    int pixfmt = -1;  // raw and device frames: a VSF_PIX_* code; -1: `bayer` says it (MONO8 or BAYER_RGGB8)
    int reduce = 1;  // compressed: config.imdecode_reduce_ at the call
    void* hip_stream = nullptr;
  };
  // (width x height: the frame's own size -- the context's, or the camera's with config.resize_width_ / resize_height_ set)
  bool ObserveFused(int width, int height, const FramePayload& fp);
  bool resizing() const { return config_.resize_width_ > 0 && config_.resize_height_ > 0; }
  // What the object's stream has been told its frames' size is (0 x 0: the context's): vsf_observe_set_input_size, with what
  // is in flight booked first.  (A new context starts at 0 x 0.)
  bool DeclareInput(int width, int height);
  int declared_w_ = 0, declared_h_ = 0;
  std::vector<uint8_t> resized_[2];  // per-call mode: the two resized images
  void FinishNode(const Frame& curr_frame, const std::vector<slam_types::VisionFeature>& features);
  // visualization_: the newest node and the factors booked with it (vision factors from index `first_vision_factor`) join the
  // pose-graph lists; points [xyz, xyz + 3 n) -- the node's, made on the device -- join the cloud.
  void BookVisualization(size_t first_vision_factor, const double* xyz, int n);
  bool SetQueuePose();  // the pose the next node will carry, handed to the queue before its frame is submitted
  bool BookFinished();  // books the frames whose results are already there: never waits, sends nothing early
  // A frame the GPU is still working on, with the odometry its ObserveImage call saw (cc:444-458 reads it at the END of
  // the call; between submit and collect the driver may already have delivered the next pose).
  struct PendingFrame {
    int64_t ticket;
    Vector3f odom_translation, prev_odom_translation;
    Quaternionf odom_rotation, prev_odom_rotation;
    double odom_timestamp;
  };
  // An image the object owns (one entry of debug_images_ / debug_stereo_images_).
  struct OwnedImage {
    std::vector<uint8_t> data;
    int rows = 0, cols = 0;
    Image view() const { return Image(data.data(), rows, cols, (size_t)cols * 3, 3); }
  };
  // Per-call mode: CreateStereoDebugImage (cc:74-98, when `stereo` is given) and CreateMatchDebugImage (cc:100-115, when
  // `temporal` is) of one node, drawn on the GPU in one vsf_draw_canvases call (the queue draws its own in the batch's tail) and appended to the lists in that order.  stereo pairs are
  // (right index, left index), temporal pairs (past index, current index), as booked.
  void DrawDebugImages(const uint8_t* left, const uint8_t* right, int w, int h, size_t pitch, const Frame& curr_frame,
                       const std::vector<vsf_keypoint>& right_keypoints, const std::vector<slam_types::FeatureMatch>* stereo,
                       const Frame* past_frame, const std::vector<slam_types::FeatureMatch>* temporal);
  bool RetireOldest();
  void Sync() const { const_cast<Frontend*>(this)->Flush(); }

  bool odom_initialized_;
  Vector3f init_odom_translation_;
  Quaternionf init_odom_rotation_;
  Vector3f prev_odom_translation_;
  Quaternionf prev_odom_rotation_;
  Vector3f odom_translation_;
  Quaternionf odom_rotation_;
  double odom_timestamp_;
  FrontendConfig config_;
  uint64_t curr_frame_ID_;
  std::vector<Frame> frame_list_;
  std::vector<slam_types::VisionFactor> vision_factors_;
  std::vector<slam_types::SLAMNode> nodes_;
  std::vector<slam_types::OdometryFactor> odometry_factors_;
  // The reference keeps this in a file-static shared by all instances (cc:353, quirk Q3); here it is per object.
  float stereo_ambig_constraint_;
  std::vector<OwnedImage> debug_images_, debug_stereo_images_;  // cc h:202-203: kept for the object's lifetime
  vsfrand::State colour_rng_;  // per-call mode with config_.debug_colour_seeded_: the object's own rand()
  std::vector<std::vector<uint8_t>> debug_files_, debug_stereo_files_;  // ... or their JPEG / PNG files (debug_jpeg_quality_ / debug_png_)
  // visualization_: the pose graph as points (one per node; two per factor) and the cloud (three doubles per point)
  std::vector<slam_visualization::Point> viz_nodes_, viz_odometry_, viz_vision_;
  std::vector<double> cloud_;
  bool fused_;
  bool pipelined_;
  int depth_ = 256, batch_frames_ = 128, min_batch_ = 0;
  bool queue_thread_ = false, copy_thread_ = true;
  std::vector<std::pair<int, int>> ctx_options_;
  std::vector<PendingFrame> pending_;  // a ring: pending_head_ is the oldest, pending_count_ frames wait
  size_t pending_head_ = 0, pending_count_ = 0;
  int ctx_depth_ = 0;
  int ctx_generation_ = 0;  // contexts created so far (a replaced context may come back at the same address)
  vsf_ctx* ctx_;
  FrontendGroup* group_ = nullptr;  // the group this object is a member of: ctx_ is then the group's (its first member owns it)
  int stream_ = 0;                  // ... and this is its stream of the context's queue
  bool owns_ctx_ = true;
  int device_;
  vsf_status last_status_;
  uint64_t refused_frames_ = 0;
};

// Several cameras, one GPU: N Frontend objects on ONE context and ONE ObserveImage queue, member i on stream i
// (vsf_observe_set_streams).  Frames of different members wait in the same queue and leave for the GPU in the same batch, so
// the members share the extraction buffers (~25 MB of HBM per frame of a batch) and a batch's ~45 launches.  Every member's
// nodes, factors and bytes are those of a Frontend of its own fed the same calls (tests/test_gpu_frontend_group.py).
//   The members' configurations may differ in everything a frame brings to the queue -- the calibration (intrinsics,
// projections, fundamental), best_percent_, the odometry gates -- and must agree in what the context is built with:
// orb_nfeatures, nn_match_ratio_, residual_order, frame_life_, visualization_, the image size and -- the queue draws for every
// stream or for none, in one form -- debug_images_, debug_jpeg_quality_, debug_png_ (else last_status() of the group reads
// VSF_ERR_INVALID_ARG and nothing is observed).  left_cam_to_robot is per member: the group hands each member's matrix to its
// stream (vsf_observe_set_stream_cam_to_robot), so two cameras on one robot keep two clouds.  Members observe in fused mode
// (a member's set_fused does nothing).
//   Debug images in a group of more than one member need debug_colour_seeded_ on EVERY member (each stream then draws its
// colours from a generator of its own, vsf_observe_set_debug_seeds); a configuration that asks for debug images without it is
// refused by the constructor with VSF_ERR_UNSUPPORTED.  With it every member's getDebugImages / getDebugStereoImages /
// GetLast... / ...Compressed are those of a Frontend of its own (tests/test_gpu_frontend_group_debug.py).
//   The queue is the group's: set_pipelined / set_queue / set_queue_thread below set every member alike, and the same
// setters called on one member (set_pipelined, set_queue_depth, set_batch_frames, set_min_batch, set_queue_thread) are
// handed to the group, so the members never disagree.  Context options and the copy thread are read from member(0).
//   Tickets are retired in the order they were issued, whichever member they belong to, and each result is booked by the
// member that submitted it with the odometry of ITS call.  Reading one member's problem books everything in flight.
class FrontendGroup {
 public:
  explicit FrontendGroup(const std::vector<FrontendConfig>& configs, int device = 0);
  ~FrontendGroup();
  FrontendGroup(const FrontendGroup&) = delete;
  FrontendGroup& operator=(const FrontendGroup&) = delete;

  int size() const { return (int)members_.size(); }
  Frontend& member(int i) { return *members_[(size_t)i]; }
  void ObserveOdometry(int i, const Vector3f& translation, const Quaternionf& rotation, double timestamp) {
    member(i).ObserveOdometry(translation, rotation, timestamp);
  }
  bool ObserveImage(int i, const Image& left_image, const Image& right_image, double time) {
    return member(i).ObserveImage(left_image, right_image, time);
  }
  bool ObserveDeviceImage(int i, const void* left, size_t left_pitch, const void* right, size_t right_pitch, void* hip_stream,
                          double time, bool bayer_rggb8 = false) {
    return member(i).ObserveDeviceImage(left, left_pitch, right, right_pitch, hip_stream, time, bayer_rggb8);
  }
  bool ObserveImage(int i, const Image& left_image, const Image& right_image, double time, int pixfmt) {
    return member(i).ObserveImage(left_image, right_image, time, pixfmt);
  }
  bool ObserveDeviceImage(int i, const void* left, size_t left_pitch, const void* right, size_t right_pitch, void* hip_stream,
                          double time, int pixfmt) {
    return member(i).ObserveDeviceImage(left, left_pitch, right, right_pitch, hip_stream, time, pixfmt);
  }
  bool ObserveCompressedImage(int i, const uint8_t* left, size_t left_bytes, const uint8_t* right, size_t right_bytes,
                              bool bayer_rggb8, double time) {
    return member(i).ObserveCompressedImage(left, left_bytes, right, right_bytes, bayer_rggb8, time);
  }
  void GetSLAMProblem(int i, slam_types::SLAMProblem* problem) { member(i).GetSLAMProblem(problem); }
  bool Flush();  // collects and books every frame still in flight, in ticket order; false if one of them failed
  // As the Frontend's own (before the first image): the one queue of the group.
  void set_pipelined(bool on);
  void set_queue(int depth, int batch_frames, int min_batch);  // depth / batch_frames 0, min_batch < 0: as it is
  void set_queue_thread(bool on);
  void set_compressed_cap(size_t cap_per_image);
  vsf_status last_status() const { return last_status_; }
  vsf_ctx* context() const { return members_.empty() ? nullptr : members_[0]->ctx_; }

 private:
  friend class Frontend;
  bool EnsureContext(int width, int height);
  bool RetireOldest();  // the oldest ticket, by the member it belongs to
  size_t in_flight() const { return order_.size(); }
  int64_t oldest_ticket() const;
  void submitted(int stream) { order_.push_back(stream); }

  std::vector<Frontend*> members_;
  std::deque<int> order_;  // the members of the frames in flight, in ticket order
  bool ready_ = false;  // every member is constructed
  vsf_status last_status_ = VSF_OK;
};

}  // namespace slam

#endif  // VSF_HOST_SLAM_FRONTEND_H_
