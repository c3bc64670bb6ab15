// frontend_capi.cc -- flat C view of slam::Frontend so tests (ctypes) and foreign callers can drive the host
// class: same call sequence as the reference's driver (slam_frontend_main.cc:132,147,321).
#include <chrono>
#include <vector>
#include <cstring>

#include "bag_extract.h"
#include "slam_frontend.h"
#include "slam_to_ros.h"

using slam::Frontend;
using slam::FrontendConfig;

extern "C" {

// score_type: FrontendConfig::orb_score_type_ (VSF_SCORE_HARRIS / VSF_SCORE_FAST)
void* vsfh_frontend_create_score(int nfeatures, int width, int height, int device, const float* fundamental9,
                                 float best_percent, int frame_life, int score_type) {
  FrontendConfig cfg;
  cfg.orb_nfeatures = nfeatures;
  cfg.orb_score_type_ = score_type;
  cfg.image_width = width;
  cfg.image_height = height;
  if (fundamental9) std::memcpy(cfg.fundamental.m, fundamental9, 9 * sizeof(float));
  if (best_percent > 0) cfg.best_percent_ = best_percent;
  if (frame_life > 0) cfg.frame_life_ = (uint32_t)frame_life;
  return new Frontend("", cfg, device);
}
// (the call as it was before the score type: the reference's HARRIS_SCORE)
void* vsfh_frontend_create(int nfeatures, int width, int height, int device, const float* fundamental9,
                           float best_percent, int frame_life) {
  return vsfh_frontend_create_score(nfeatures, width, height, device, fundamental9, best_percent, frame_life, VSF_SCORE_HARRIS);
}

// The stereo calibration of a default-constructed FrontendConfig (the reference's hard-coded constants,
// slam_frontend.cc:565-644) in the layout the C ABI takes -- the one place tests, bench.py and the multi-GPU path get it.
void vsfh_default_calibration(vsf_calibration* out) { *out = slam::MakeCalibration(FrontendConfig()); }

void vsfh_set_fused(void* f, int on) { static_cast<Frontend*>(f)->set_fused(on != 0); }
void vsfh_set_pipelined(void* f, int on) { static_cast<Frontend*>(f)->set_pipelined(on != 0); }
void vsfh_set_frames_in_flight(void* f, int n) { static_cast<Frontend*>(f)->set_queue_depth(n); }
void vsfh_set_queue(void* f, int depth, int batch_frames, int min_batch) {
  Frontend* fe = static_cast<Frontend*>(f);
  if (depth > 0) fe->set_queue_depth(depth);
  if (batch_frames > 0) fe->set_batch_frames(batch_frames);
  fe->set_min_batch(min_batch);
}

void vsfh_set_queue_threads(void* f, int launcher, int copy) {
  static_cast<Frontend*>(f)->set_queue_thread(launcher != 0);
  static_cast<Frontend*>(f)->set_copy_thread(copy != 0);
}

// The reference's driver loop (slam_frontend_main.cc:271-328) for n_frames stereo frames taken in turn from `frames`
// (n_src x 2 x h x w bytes): ObserveOdometry (a pose 0.3 m further on: OdomCheck accepts every frame) + ObserveImage per
// frame, no Python between the calls.  The clock starts at frame `warm` (after a Flush) and stops behind the final Flush.
// read_every > 0: GetSLAMProblem after every read_every-th new node, as the reference's driver does after every one
// (main.cc:320-321) -- that read waits for every frame still in the queue.
// Returns the steady frames per second; *mean_call_ms / *max_call_ms: time inside ObserveImage; < 0 on failure.
double vsfh_time_sequence(void* f, const uint8_t* frames, int n_src, int w, int h, int n_frames, int warm, int read_every,
                          double* mean_call_ms, double* max_call_ms) {
  using Clock = std::chrono::steady_clock;
  Frontend* fe = static_cast<Frontend*>(f);
  const slam::Quaternionf q(1, 0, 0, 0);
  const int first = fe->GetNumPoses();
  if (first == 0) fe->ObserveOdometry(slam::Vector3f(0, 0, 0), q, 0.0);
  Clock::time_point t0 = Clock::now();
  double sum = 0, worst = 0;
  for (int k = 0; k < n_frames; k++) {
    if (k == warm) {
      fe->Flush();
      t0 = Clock::now();
    }
    const uint8_t* l = frames + (size_t)(k % n_src) * 2 * w * h;
    fe->ObserveOdometry(slam::Vector3f(0.3f * (first + k + 1), 0, 0), q, 1.0 + first + k);
    const Clock::time_point a = Clock::now();
    const bool added = fe->ObserveImage(slam::Image(l, h, w, (size_t)w), slam::Image(l + (size_t)w * h, h, w, (size_t)w),
                                        1.0 + first + k);
    const double dt = std::chrono::duration<double>(Clock::now() - a).count();
    if (!added || fe->last_status() != VSF_OK) return -1.0;
    if (read_every > 0 && (k + 1) % read_every == 0) {
      slam_types::SLAMProblem problem;
      fe->GetSLAMProblem(&problem);
      if (problem.nodes.empty()) return -1.0;
    }
    if (k >= warm) {
      sum += dt;
      if (dt > worst) worst = dt;
    }
  }
  if (!fe->Flush()) return -1.0;
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  const int n = n_frames - warm;
  if (mean_call_ms) *mean_call_ms = n > 0 ? 1e3 * sum / n : 0;
  if (max_call_ms) *max_call_ms = 1e3 * worst;
  return n > 0 && wall > 0 ? n / wall : 0.0;
}
// The same loop fed from compressed payloads in host memory (n_src stereo frames: file 2i is frame i's left, 2i + 1 its right;
// file j is blob[offsets[j], offsets[j + 1])), as the reference's CompressedImageCallback is (slam_frontend_main.cc:98-133).
// decode == NULL: ObserveCompressedImage (the GPU decodes inside the queue).  Otherwise decode-then-observe on the host:
// decode(file, bytes, w, h, dst, pitch, &w_out, &h_out) -- a libjpeg driven as cv::imdecode drives it -- fills two w x h
// images per frame and ObserveImage takes them.  Returns the steady frames per second; *mean_call_ms / *max_call_ms: time inside the
// frame's calls (decode included); < 0 on failure.
typedef int (*vsfh_decode_fn)(const char* file, size_t bytes, int w, int h, void* dst, size_t pitch, int* w_out, int* h_out);
double vsfh_time_compressed_sequence(void* f, const uint8_t* blob, const uint64_t* offsets, int n_src, int bayer, int w, int h,
                                     int n_frames, int warm, vsfh_decode_fn decode, double* mean_call_ms, double* max_call_ms) {
  using Clock = std::chrono::steady_clock;
  Frontend* fe = static_cast<Frontend*>(f);
  const slam::Quaternionf q(1, 0, 0, 0);
  const int first = fe->GetNumPoses();
  if (first == 0) fe->ObserveOdometry(slam::Vector3f(0, 0, 0), q, 0.0);
  std::vector<uint8_t> scratch(decode ? (size_t)2 * w * h : 0);
  Clock::time_point t0 = Clock::now();
  double sum = 0, worst = 0;
  for (int k = 0; k < n_frames; k++) {
    if (k == warm) {
      fe->Flush();
      t0 = Clock::now();
    }
    const int i = k % n_src;
    const uint8_t *l = blob + offsets[2 * i], *r = blob + offsets[2 * i + 1];
    const size_t nl = (size_t)(offsets[2 * i + 1] - offsets[2 * i]), nr = (size_t)(offsets[2 * i + 2] - offsets[2 * i + 1]);
    fe->ObserveOdometry(slam::Vector3f(0.3f * (first + k + 1), 0, 0), q, 1.0 + first + k);
    const Clock::time_point a = Clock::now();
    bool added;
    if (decode) {
      int ww = 0, hh = 0;
      uint8_t *dl = scratch.data(), *dr = scratch.data() + (size_t)w * h;
      if (decode(reinterpret_cast<const char*>(l), nl, w, h, dl, (size_t)w, &ww, &hh) != 0 ||
          decode(reinterpret_cast<const char*>(r), nr, w, h, dr, (size_t)w, &ww, &hh) != 0)
        return -1.0;
      added = fe->ObserveImage(slam::Image(dl, h, w, (size_t)w), slam::Image(dr, h, w, (size_t)w), 1.0 + first + k);
    } else {
      added = fe->ObserveCompressedImage(l, nl, r, nr, bayer != 0, 1.0 + first + k);
    }
    const double dt = std::chrono::duration<double>(Clock::now() - a).count();
    if (!added || fe->last_status() != VSF_OK) return -1.0;
    if (k >= warm) {
      sum += dt;
      if (dt > worst) worst = dt;
    }
  }
  if (!fe->Flush()) return -1.0;
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  const int n = n_frames - warm;
  if (mean_call_ms) *mean_call_ms = n > 0 ? 1e3 * sum / n : 0;
  if (max_call_ms) *max_call_ms = 1e3 * worst;
  return n > 0 && wall > 0 ? n / wall : 0.0;
}
int vsfh_flush(void* f) { return static_cast<Frontend*>(f)->Flush() ? 1 : 0; }

// Debug images (slam_frontend.cc:474-495).  stereo = 0: getDebugImages / GetLastDebugImage; 1: the stereo ones.
void vsfh_set_debug_images(void* f, int on) { static_cast<Frontend*>(f)->set_debug_images(on != 0); }
int vsfh_num_debug_images(void* f, int stereo) {
  Frontend* fe = static_cast<Frontend*>(f);
  return (int)(stereo ? fe->getDebugStereoImages() : fe->getDebugImages()).size();
}
// Image i (i = -1: GetLastDebugImage / GetLastDebugStereoImage): its shape into rows_cols_ch[3], min(size, cap) bytes
// (rows packed) into out.  Returns 1, or 0 when there is no such image (the getter's empty cv::Mat).
int vsfh_debug_image(void* f, int stereo, int i, uint8_t* out, size_t cap, int rows_cols_ch[3]) {
  Frontend* fe = static_cast<Frontend*>(f);
  slam::Image im;
  if (i < 0) {
    im = stereo ? fe->GetLastDebugStereoImage() : fe->GetLastDebugImage();
  } else {
    const std::vector<slam::Image> all = stereo ? fe->getDebugStereoImages() : fe->getDebugImages();
    if (i < (int)all.size()) im = all[i];
  }
  rows_cols_ch[0] = rows_cols_ch[1] = rows_cols_ch[2] = 0;
  if (im.empty()) return 0;
  rows_cols_ch[0] = im.rows, rows_cols_ch[1] = im.cols, rows_cols_ch[2] = im.channels;
  const size_t row = (size_t)im.cols * im.channels;
  for (int y = 0; y < im.rows && out && (size_t)(y + 1) * row <= cap; y++) std::memcpy(out + y * row, im.data + y * im.step, row);
  return 1;
}

void vsfh_set_debug_jpeg_quality(void* f, int quality) { static_cast<Frontend*>(f)->set_debug_jpeg_quality(quality); }
void vsfh_set_debug_png(void* f, int on) { static_cast<Frontend*>(f)->set_debug_png(on != 0); }
// FrontendConfig::debug_colour_seeded_ / debug_colour_seed_: the stereo lines' colours from a generator the object owns
void vsfh_set_debug_colour_seed(void* f, int seeded, uint32_t seed) {
  static_cast<Frontend*>(f)->set_debug_colour_seed(seeded != 0, seed);
}
// FrontendConfig::imdecode_reduce_ (a group's member: the pointer vsfh_group_member returns)
void vsfh_set_imdecode_reduce(void* f, int reduce) { static_cast<Frontend*>(f)->set_imdecode_reduce(reduce); }
// FrontendConfig::resize_width_ / resize_height_ (a group's member: the pointer vsfh_group_member returns); camera_width x
// camera_height > 0: image_width / image_height too, what device frames are taken to be
void vsfh_set_resize(void* f, int width, int height, int camera_width, int camera_height) {
  static_cast<Frontend*>(f)->set_resize(width, height, camera_width, camera_height);
}
// FrontendConfig::mask_left_ / mask_right_ (a group's member: the pointer vsfh_group_member returns): two masks of w x h at
// `step` (NULL: no mask for that eye); the object keeps copies.
void vsfh_set_masks(void* f, const uint8_t* left, const uint8_t* right, int w, int h, size_t step) {
  static_cast<Frontend*>(f)->set_masks(left ? slam::Image(left, h, w, step) : slam::Image(),
                                       right ? slam::Image(right, h, w, step) : slam::Image());
}
// FrontendConfig::compressed_cap_ (a group's member: the group's)
void vsfh_set_compressed_cap(void* f, size_t cap_per_image) { static_cast<Frontend*>(f)->set_compressed_cap(cap_per_image); }
// The format of what vsfh_debug_image_compressed returns: 0 none, 1 "jpeg", 2 "png".
int vsfh_debug_image_compressed_format(void* f, int stereo) {
  Frontend* fe = static_cast<Frontend*>(f);
  const Frontend::CompressedView v = stereo ? fe->GetLastDebugStereoImageCompressed() : fe->GetLastDebugImageCompressed();
  return !v.format ? 0 : v.format[0] == 'p' ? 2 : 1;
}
// GetLastDebugImageCompressed / GetLastDebugStereoImageCompressed: the file's size (0: none); min(size, cap) bytes into out.
size_t vsfh_debug_image_compressed(void* f, int stereo, uint8_t* out, size_t cap) {
  Frontend* fe = static_cast<Frontend*>(f);
  const Frontend::CompressedView v = stereo ? fe->GetLastDebugStereoImageCompressed() : fe->GetLastDebugImageCompressed();
  if (out && v.size) std::memcpy(out, v.data, v.size < cap ? v.size : cap);
  return v.size;
}

// ---- what the driver publishes to RViz (slam_visualization.h, Frontend::GetVisualization) ----
void vsfh_set_projections(void* f, const float left12[12], const float right12[12]) {
  static_cast<Frontend*>(f)->set_projections(left12, right12);
}
void vsfh_set_visualization(void* f, int on) { static_cast<Frontend*>(f)->set_visualization(on != 0); }
void vsfh_set_left_cam_to_robot(void* f, const float m12[12]) { static_cast<Frontend*>(f)->set_left_cam_to_robot(m12); }
void vsfh_group_set_visualization(void* g, int on) {
  slam::FrontendGroup* gr = static_cast<slam::FrontendGroup*>(g);
  for (int i = 0; i < gr->size(); i++) gr->member(i).set_visualization(on != 0);
}

namespace {
// host != 0: PublishVisualization's markers computed on the CPU from the whole problem, as the reference's driver does
// (GetSLAMProblem -- which flushes -- then AddFeaturePoints / AddPoseGraph); else Frontend::GetVisualization.
bool get_visualization(Frontend* fe, int host, slam::Visualization* v) {
  if (!host) return fe->GetVisualization(v);
  slam_types::SLAMProblem problem;
  fe->GetSLAMProblem(&problem);
  float cam_to_robot[12];
  slam::CamToRobot(fe->GetConfig(), cam_to_robot);
  slam_visualization::BuildVisualization(cam_to_robot, problem, v);
  return true;
}
const slam_visualization::Marker& marker_of(const slam::Visualization& v, int which) {
  return which == 0 ? v.nodes : which == 1 ? v.odometry : which == 2 ? v.vision : v.vision_points;
}
}  // namespace

// Points of marker `which` (0 nodes, 1 odometry lines, 2 vision lines, 3 the cloud): the count, or -1; min(count, cap) points
// of three doubles into out.
long long vsfh_visualization_points(void* f, int host, int which, double* out, size_t cap) {
  slam::Visualization v;
  if (which < 0 || which > 3 || !get_visualization(static_cast<Frontend*>(f), host, &v)) return -1;
  const slam_visualization::Marker& m = marker_of(v, which);
  const size_t n = m.points.size() < cap ? m.points.size() : cap;
  if (out && n) std::memcpy(out, m.points.data(), n * sizeof(slam_visualization::Point));
  return (long long)m.points.size();
}
// ROS-1 wire bytes of what the driver publishes: which = 0 the MarkerArray of slam_frontend/pose_graph (nodes, odometry, vision),
// 1 the Marker of slam_frontend/points (the cloud).  The payload size (0 on failure); min(size, cap) bytes into out.
size_t vsfh_serialize_visualization(void* f, int host, int which, uint8_t* out, size_t cap) {
  slam::Visualization v;
  if (!get_visualization(static_cast<Frontend*>(f), host, &v)) return 0;
  std::vector<uint8_t> bytes;
  if (which == 0)
    slam_to_ros::SerializeMarkerArray(v.PoseGraph(), &bytes);
  else
    slam_to_ros::SerializeMarker(v.vision_points, &bytes);
  if (out && cap) std::memcpy(out, bytes.data(), bytes.size() < cap ? bytes.size() : cap);
  return bytes.size();
}
// The CPU restatement alone, no Frontend and no GPU: slam_visualization::AddFeaturePoints on a problem of ONE node with pose
// (loc xyz, quaternion xyzw) and n features whose point3d are point3d[3 i ..].  Returns the points kept; out holds 3 n doubles.
int vsfh_add_feature_points(const float cam_to_robot[12], const float loc[3], const float quat_xyzw[4], const float* point3d, int n,
                            double* out) {
  slam_types::SLAMProblem problem;
  problem.nodes.resize(1);
  slam_types::SLAMNode& node = problem.nodes[0];
  node.pose = slam_types::RobotPose(slam::Vector3f(loc[0], loc[1], loc[2]),
                                    slam::Quaternionf(quat_xyzw[3], quat_xyzw[0], quat_xyzw[1], quat_xyzw[2]));
  for (int i = 0; i < n; i++)
    node.features.push_back(slam_types::VisionFeature((uint64_t)i, slam::Vector2f(),
                                                      slam::Vector3f(point3d[3 * i], point3d[3 * i + 1], point3d[3 * i + 2])));
  slam_visualization::Marker m;
  slam_visualization::InitializeMarker(slam_visualization::Marker::POINTS, slam_visualization::Color4f::kWhite(), 0.025f, 0.025f,
                                       0.025f, &m);
  slam_visualization::AddFeaturePoints(cam_to_robot, problem, &m);
  if (!m.points.empty()) std::memcpy(out, m.points.data(), m.points.size() * sizeof(slam_visualization::Point));
  return (int)m.points.size();
}

// The driver's loop of vsfh_time_sequence with the visualization asked for after EVERY node (slam_frontend_main.cc:319-325).
// host == 0: Frontend::GetVisualization into one Visualization object kept across the loop (it only appends; the queue is not
// flushed); host != 0: GetSLAMProblem + AddFeaturePoints / AddPoseGraph over the whole problem per node, as the reference does.
// Either way the two messages are serialised every `publish_every`-th node (0: never).  Returns the steady frames per second;
// *points: the cloud's size at the end; < 0 on failure.
double vsfh_time_visualization(void* f, const uint8_t* frames, int n_src, int w, int h, int n_frames, int warm, int host,
                               int publish_every, long long* points) {
  using Clock = std::chrono::steady_clock;
  Frontend* fe = static_cast<Frontend*>(f);
  const slam::Quaternionf q(1, 0, 0, 0);
  const int first = fe->GetNumPoses();
  if (first == 0) fe->ObserveOdometry(slam::Vector3f(0, 0, 0), q, 0.0);
  slam::Visualization v;
  std::vector<uint8_t> bytes;
  Clock::time_point t0 = Clock::now();
  for (int k = 0; k < n_frames; k++) {
    if (k == warm) {
      fe->Flush();
      t0 = Clock::now();
    }
    const uint8_t* l = frames + (size_t)(k % n_src) * 2 * w * h;
    fe->ObserveOdometry(slam::Vector3f(0.3f * (first + k + 1), 0, 0), q, 1.0 + first + k);
    const bool added = fe->ObserveImage(slam::Image(l, h, w, (size_t)w), slam::Image(l + (size_t)w * h, h, w, (size_t)w),
                                        1.0 + first + k);
    if (!added || fe->last_status() != VSF_OK) return -1.0;
    if (!get_visualization(fe, host, &v)) return -1.0;
    if (publish_every > 0 && (k + 1) % publish_every == 0) {
      slam_to_ros::SerializeMarkerArray(v.PoseGraph(), &bytes);
      slam_to_ros::SerializeMarker(v.vision_points, &bytes);
    }
  }
  if (!fe->Flush() || !get_visualization(fe, host, &v)) return -1.0;
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  if (points) *points = (long long)v.vision_points.points.size();
  const int n = n_frames - warm;
  return n > 0 && wall > 0 ? n / wall : 0.0;
}

void vsfh_frontend_destroy(void* f) { delete static_cast<Frontend*>(f); }

// slam::FrontendGroup: n members on one context.  Member i takes fundamental9[9 i ..] and best_percent[i] (<= 0: the
// default); the rest as vsfh_frontend_create.  vsfh_group_member hands out
// member i as a Frontend every vsfh_* call above takes (the group owns it: never vsfh_frontend_destroy).
// A group of n members: per member a fundamental matrix and (optional, > 0) a best_percent; then what a group must be BUILT
// with: the debug images' switch and form (0 / 0 / 0: none), a colour seed per member (NULL: the process's rand() -- refused with
// more than one member and debug images), a left_cam_to_robot per member (n x 12 floats, 3 x 4 row-major; NULL: the
// reference's) and visualization_.
// ... and score_type: every member's FrontendConfig::orb_score_type_ (one context, one mode).
void* vsfh_group_create_score(int n, int nfeatures, int width, int height, int device, const float* fundamental9,
                              const float* best_percent, int frame_life, int debug_images, int debug_jpeg_quality, int debug_png,
                              const uint32_t* colour_seeds, const float* cam_to_robots, int visualization, int score_type) {
  std::vector<FrontendConfig> cfgs((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) {
    FrontendConfig& cfg = cfgs[(size_t)i];
    cfg.orb_nfeatures = nfeatures;
    cfg.orb_score_type_ = score_type;
    cfg.image_width = width;
    cfg.image_height = height;
    if (fundamental9) std::memcpy(cfg.fundamental.m, fundamental9 + 9 * i, 9 * sizeof(float));
    if (best_percent && best_percent[i] > 0) cfg.best_percent_ = best_percent[i];
    if (frame_life > 0) cfg.frame_life_ = (uint32_t)frame_life;
    cfg.debug_images_ = debug_images != 0;
    cfg.debug_jpeg_quality_ = debug_jpeg_quality;
    cfg.debug_png_ = debug_png != 0;
    cfg.debug_colour_seeded_ = colour_seeds != nullptr;
    if (colour_seeds) cfg.debug_colour_seed_ = colour_seeds[i];
    cfg.visualization_ = visualization != 0;
    if (cam_to_robots) cfg.left_cam_to_robot = slam::AffineFromRowMajor(cam_to_robots + 12 * i);
  }
  return new slam::FrontendGroup(cfgs, device);
}
// (the call as it was before the score type)
void* vsfh_group_create_ex(int n, int nfeatures, int width, int height, int device, const float* fundamental9,
                           const float* best_percent, int frame_life, int debug_images, int debug_jpeg_quality, int debug_png,
                           const uint32_t* colour_seeds, const float* cam_to_robots, int visualization) {
  return vsfh_group_create_score(n, nfeatures, width, height, device, fundamental9, best_percent, frame_life, debug_images,
                                 debug_jpeg_quality, debug_png, colour_seeds, cam_to_robots, visualization, VSF_SCORE_HARRIS);
}
// (the call as it was before the group took debug images and extrinsics)
void* vsfh_group_create(int n, int nfeatures, int width, int height, int device, const float* fundamental9,
                        const float* best_percent, int frame_life) {
  return vsfh_group_create_ex(n, nfeatures, width, height, device, fundamental9, best_percent, frame_life, 0, 0, 0, nullptr, nullptr, 0);
}
void vsfh_group_destroy(void* g) { delete static_cast<slam::FrontendGroup*>(g); }
int vsfh_group_size(void* g) { return static_cast<slam::FrontendGroup*>(g)->size(); }
void* vsfh_group_member(void* g, int i) {
  slam::FrontendGroup* gr = static_cast<slam::FrontendGroup*>(g);
  return i >= 0 && i < gr->size() ? &gr->member(i) : nullptr;
}
int vsfh_group_last_status(void* g) { return (int)static_cast<slam::FrontendGroup*>(g)->last_status(); }
void vsfh_group_set_pipelined(void* g, int on) { static_cast<slam::FrontendGroup*>(g)->set_pipelined(on != 0); }
void vsfh_group_set_queue(void* g, int depth, int batch_frames, int min_batch) {
  static_cast<slam::FrontendGroup*>(g)->set_queue(depth, batch_frames, min_batch);
}
void vsfh_group_set_queue_thread(void* g, int on) { static_cast<slam::FrontendGroup*>(g)->set_queue_thread(on != 0); }
int vsfh_group_flush(void* g) { return static_cast<slam::FrontendGroup*>(g)->Flush() ? 1 : 0; }
void vsfh_group_observe_odometry(void* g, int i, const float t[3], const float q_wxyz[4], double ts) {
  static_cast<slam::FrontendGroup*>(g)->ObserveOdometry(i, slam::Vector3f(t[0], t[1], t[2]),
                                                        slam::Quaternionf(q_wxyz[0], q_wxyz[1], q_wxyz[2], q_wxyz[3]), ts);
}
int vsfh_group_observe_image(void* g, int i, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, double time) {
  return static_cast<slam::FrontendGroup*>(g)->ObserveImage(i, slam::Image(left, h, w, stride), slam::Image(right, h, w, stride), time)
             ? 1
             : 0;
}
int vsfh_group_observe_compressed_image(void* g, int i, const uint8_t* left, size_t left_bytes, const uint8_t* right,
                                        size_t right_bytes, int bayer_rggb8, double time) {
  return static_cast<slam::FrontendGroup*>(g)->ObserveCompressedImage(i, left, left_bytes, right, right_bytes, bayer_rggb8 != 0, time)
             ? 1
             : 0;
}
int vsfh_group_observe_device_image(void* g, int i, const void* left, size_t left_pitch, const void* right, size_t right_pitch,
                                    void* hip_stream, double time, int bayer_rggb8) {
  return static_cast<slam::FrontendGroup*>(g)->ObserveDeviceImage(i, left, left_pitch, right, right_pitch, hip_stream, time,
                                                                   bayer_rggb8 != 0)
             ? 1
             : 0;
}
// vsf_observe_stats of a Frontend's context (out[0..n)).
int vsfh_queue_stats(void* f, int64_t* out, int n) {
  vsf_ctx* c = static_cast<Frontend*>(f)->context();
  return c ? (int)vsf_observe_stats(c, out, n) : (int)VSF_ERR_INVALID_ARG;
}
// vsf_observe_stats of the group's context (out[0..n)).
int vsfh_group_queue_stats(void* g, int64_t* out, int n) {
  vsf_ctx* c = static_cast<slam::FrontendGroup*>(g)->context();
  return c ? (int)vsf_observe_stats(c, out, n) : (int)VSF_ERR_INVALID_ARG;
}

void vsfh_observe_odometry(void* f, const float t[3], const float q_wxyz[4], double ts) {
  static_cast<Frontend*>(f)->ObserveOdometry(slam::Vector3f(t[0], t[1], t[2]),
                                             slam::Quaternionf(q_wxyz[0], q_wxyz[1], q_wxyz[2], q_wxyz[3]), ts);
}

int vsfh_observe_image(void* f, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, double time) {
  return static_cast<Frontend*>(f)->ObserveImage(slam::Image(left, h, w, stride), slam::Image(right, h, w, stride), time)
             ? 1
             : 0;
}

int vsfh_observe_compressed_image(void* f, const uint8_t* left, size_t left_bytes, const uint8_t* right, size_t right_bytes,
                                  int bayer_rggb8, double time) {
  return static_cast<Frontend*>(f)->ObserveCompressedImage(left, left_bytes, right, right_bytes, bayer_rggb8 != 0, time) ? 1 : 0;
}

int vsfh_observe_device_image(void* f, const void* left, size_t left_pitch, const void* right, size_t right_pitch,
                              void* hip_stream, double time, int bayer_rggb8) {
  return static_cast<Frontend*>(f)->ObserveDeviceImage(left, left_pitch, right, right_pitch, hip_stream, time, bayer_rggb8 != 0) ? 1 : 0;
}

// ... of any pixel format (VSF_PIX_*): w x h pixels, stride / pitches in bytes
int vsfh_observe_image_pix(void* f, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, int pixfmt, double time) {
  return static_cast<Frontend*>(f)->ObserveImage(slam::Image(left, h, w, stride), slam::Image(right, h, w, stride), time, pixfmt) ? 1 : 0;
}
int vsfh_observe_device_image_pix(void* f, const void* left, size_t left_pitch, const void* right, size_t right_pitch,
                                  void* hip_stream, double time, int pixfmt) {
  return static_cast<Frontend*>(f)->ObserveDeviceImage(left, left_pitch, right, right_pitch, hip_stream, time, pixfmt) ? 1 : 0;
}
int vsfh_group_observe_image_pix(void* g, int i, const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, int pixfmt,
                                 double time) {
  return static_cast<slam::FrontendGroup*>(g)->ObserveImage(i, slam::Image(left, h, w, stride), slam::Image(right, h, w, stride), time,
                                                            pixfmt)
             ? 1
             : 0;
}
int vsfh_group_observe_device_image_pix(void* g, int i, const void* left, size_t left_pitch, const void* right, size_t right_pitch,
                                        void* hip_stream, double time, int pixfmt) {
  return static_cast<slam::FrontendGroup*>(g)->ObserveDeviceImage(i, left, left_pitch, right, right_pitch, hip_stream, time, pixfmt)
             ? 1
             : 0;
}
// FrontendConfig::bayer_order_ (a group's member: the pointer vsfh_group_member returns)
void vsfh_set_bayer_order(void* f, int pixfmt) { static_cast<Frontend*>(f)->set_bayer_order(pixfmt); }

unsigned long long vsfh_refused_frames(void* f) { return static_cast<Frontend*>(f)->refused_frames(); }
int vsfh_last_status(void* f) { return (int)static_cast<Frontend*>(f)->last_status(); }
int vsfh_num_poses(void* f) { return static_cast<Frontend*>(f)->GetNumPoses(); }
float vsfh_stereo_ambig_constraint(void* f) { return static_cast<Frontend*>(f)->stereo_ambig_constraint(); }

void vsfh_get_fundamental(void* f, float out9[9]) {
  const FrontendConfig c = static_cast<Frontend*>(f)->GetConfig();
  std::memcpy(out9, c.fundamental.m, 9 * sizeof(float));
}

int vsfh_num_vision_factors(void* f) {
  slam_types::SLAMProblem p;
  static_cast<Frontend*>(f)->GetSLAMProblem(&p);
  return (int)p.vision_factors.size();
}

int vsfh_vision_factor(void* f, int i, uint64_t* pose_initial, uint64_t* pose_current, uint64_t* pairs, int cap) {
  const auto& vf = static_cast<Frontend*>(f)->vision_factors();
  if (i < 0 || i >= (int)vf.size()) return -1;
  *pose_initial = vf[i].pose_idx_initial;
  *pose_current = vf[i].pose_idx_current;
  const int n = (int)vf[i].feature_matches.size();
  for (int k = 0; k < n && k < cap; k++) {
    pairs[2 * k] = vf[i].feature_matches[k].feature_idx_initial;
    pairs[2 * k + 1] = vf[i].feature_matches[k].feature_idx_current;
  }
  return n;
}

// pose7 = loc xyz + angle wxyz; feat = cap x 6: feature_idx, pixel x, pixel y, point3d xyz
int vsfh_node(void* f, int i, uint64_t* node_idx, double* timestamp, float pose7[7], float* feat, int cap) {
  const auto& nodes = static_cast<Frontend*>(f)->nodes();
  if (i < 0 || i >= (int)nodes.size()) return -1;
  const slam_types::SLAMNode& n = nodes[i];
  *node_idx = n.node_idx;
  *timestamp = n.timestamp;
  const float p[7] = {n.pose.loc.x(),   n.pose.loc.y(),   n.pose.loc.z(),  n.pose.angle.w(),
                      n.pose.angle.x(), n.pose.angle.y(), n.pose.angle.z()};
  std::memcpy(pose7, p, sizeof(p));
  const int m = (int)n.features.size();
  for (int k = 0; k < m && k < cap; k++) {
    const slam_types::VisionFeature& v = n.features[k];
    const float r[6] = {(float)v.feature_idx, v.pixel.x(), v.pixel.y(), v.point3d.x(), v.point3d.y(), v.point3d.z()};
    std::memcpy(feat + 6 * k, r, sizeof(r));
  }
  return m;
}

int vsfh_num_odometry_factors(void* f) { return (int)static_cast<Frontend*>(f)->odometry_factors().size(); }

int vsfh_odometry_factor(void* f, int i, uint64_t ij[2], float tq[7]) {
  const auto& of = static_cast<Frontend*>(f)->odometry_factors();
  if (i < 0 || i >= (int)of.size()) return -1;
  ij[0] = of[i].pose_i;
  ij[1] = of[i].pose_j;
  const float r[7] = {of[i].translation.x(), of[i].translation.y(), of[i].translation.z(), of[i].rotation.w(),
                      of[i].rotation.x(),    of[i].rotation.y(),    of[i].rotation.z()};
  std::memcpy(tq, r, sizeof(r));
  return 0;
}

// Keypoints / descriptors of the i-th retained frame (after RemoveAmbigStereo re-indexing).
int vsfh_frame(void* f, int i, uint64_t* frame_id, vsf_keypoint* kp, uint8_t* desc, int cap) {
  const auto& fl = static_cast<Frontend*>(f)->frame_list();
  if (i < 0 || i >= (int)fl.size()) return -1;
  *frame_id = fl[i].frame_ID_;
  const int n = (int)fl[i].keypoints_.size();
  const int m = n < cap ? n : cap;
  if (m > 0 && kp) std::memcpy(kp, fl[i].keypoints_.data(), (size_t)m * sizeof(vsf_keypoint));
  if (m > 0 && desc && fl[i].descriptors_.size() >= (size_t)m * VSF_DESC_BYTES)
    std::memcpy(desc, fl[i].descriptors_.data(), (size_t)m * VSF_DESC_BYTES);
  return n;
}


// FrontendConfig::left_cam_to_robot (h:96, cc:613-618) as the reference's caller reads it through GetConfig(): rotation
// (row-major 3 x 3) and translation; and the two calibration messages that caller writes into its bag from it
// (slam_frontend_main.cc:341-365): CameraExtrinsics (48 B) and CameraIntrinsics (32 B) payloads.
void vsfh_left_cam_to_robot(void* f, float rotation9[9], float translation3[3]) {
  const FrontendConfig c = static_cast<Frontend*>(f)->GetConfig();
  std::memcpy(rotation9, c.left_cam_to_robot.rotation().m, 9 * sizeof(float));
  const slam::Vector3f t = c.left_cam_to_robot.translation();
  translation3[0] = t.x(), translation3[1] = t.y(), translation3[2] = t.z();
}

void vsfh_serialize_calibration(void* f, uint8_t extrinsics48[48], uint8_t intrinsics32[32]) {
  const FrontendConfig c = static_cast<Frontend*>(f)->GetConfig();
  const slam::Vector3f rT = c.left_cam_to_robot.translation();
  const float t[3] = {rT.x(), rT.y(), rT.z()};
  const slam_types::CameraExtrinsics a = slam_to_ros::ExtrinsicsFromAffine(c.left_cam_to_robot.rotation().m, t);
  slam_types::CameraIntrinsics k;
  k.fx = c.intrinsics_left.fx;
  k.cx = c.intrinsics_left.cx;
  k.fy = c.intrinsics_left.fy;
  k.cy = c.intrinsics_left.cy;
  std::vector<uint8_t> b;
  slam_to_ros::SerializeExtrinsics(a, &b);
  std::memcpy(extrinsics48, b.data(), 48);
  slam_to_ros::SerializeIntrinsics(k, &b);
  std::memcpy(intrinsics32, b.data(), 32);
}

// ROS-1 wire bytes of the current SLAMProblem (slam_to_ros.h; what the reference writes into its output bag,
// slam_frontend_main.cc:341-374).  Returns the payload size; copies min(size, cap) bytes.
size_t vsfh_serialize_problem(void* f, uint8_t* out, size_t cap) {
  slam_types::SLAMProblem p;
  static_cast<Frontend*>(f)->GetSLAMProblem(&p);
  std::vector<uint8_t> bytes;
  slam_to_ros::SerializeSLAMProblem(p, &bytes);
  if (out && cap) std::memcpy(out, bytes.data(), bytes.size() < cap ? bytes.size() : cap);
  return bytes.size();
}

// FrontendGroup::GetSLAMProblem(i) as ROS-1 wire bytes (vsfh_serialize_problem's rules).
size_t vsfh_group_serialize_problem(void* g, int i, uint8_t* out, size_t cap) {
  slam_types::SLAMProblem p;
  static_cast<slam::FrontendGroup*>(g)->GetSLAMProblem(i, &p);
  std::vector<uint8_t> bytes;
  slam_to_ros::SerializeSLAMProblem(p, &bytes);
  if (out && cap) std::memcpy(out, bytes.data(), bytes.size() < cap ? bytes.size() : cap);
  return bytes.size();
}

// slam::BagExtract (bag_extract.h: src/test/bag_extract.cc without the bag).  quality 0 = 95; max_per_call < 1 = 512.
void* vsfh_bag_extract_create(int device, int quality, int max_per_call) {
  return new slam::BagExtract(device, quality, max_per_call < 1 ? 512 : (size_t)max_per_call);
}
void vsfh_bag_extract_destroy(void* b) { delete static_cast<slam::BagExtract*>(b); }
// n serialized sensor_msgs/CompressedImage messages, message j = blob[offsets[j], offsets[j + 1]).  The paths in message order,
// each followed by '\n' (an empty line: no file for that message), into `paths`: returns their total size and copies
// min(size, cap) bytes.  *status: BagExtract::last_status(); *calls: vsf_bag_extract_batch calls made.
size_t vsfh_bag_extract_run(void* b, const uint8_t* blob, const size_t* offsets, int n, const char* output, char* paths, size_t cap,
                            int* status, int* calls) {
  slam::BagExtract* be = static_cast<slam::BagExtract*>(b);
  std::vector<std::pair<const uint8_t*, size_t>> msgs;
  for (int j = 0; j < n; j++) msgs.emplace_back(blob + offsets[j], offsets[j + 1] - offsets[j]);
  std::string all;
  for (const std::string& p : be->Run(msgs, output ? output : "")) all += p + "\n";
  if (status) *status = (int)be->last_status();
  if (calls) *calls = (int)be->calls();
  if (paths && cap) std::memcpy(paths, all.data(), all.size() < cap ? all.size() : cap);
  return all.size();
}
// slam::BagExtractPath: returns the path's size and copies min(size, cap) bytes.
size_t vsfh_bag_extract_path(const char* output, uint64_t count, uint64_t index, char* out, size_t cap) {
  const std::string p = slam::BagExtractPath(output ? output : "", count, index);
  if (out && cap) std::memcpy(out, p.data(), p.size() < cap ? p.size() : cap);
  return p.size();
}

}  // extern "C"
