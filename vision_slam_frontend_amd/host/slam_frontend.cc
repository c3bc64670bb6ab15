// slam_frontend.cc -- host orchestration of one stereo frame, mirroring the reference's
// src/slam_frontend.cc:117-538 with the OpenCV calls replaced by the C ABI (include/vsf.h).
#include "slam_frontend.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace slam {

using slam_types::FeatureMatch;
using slam_types::OdometryFactor;
using slam_types::RobotPose;
using slam_types::SLAMNode;
using slam_types::SLAMProblem;
using slam_types::VisionFactor;
using slam_types::VisionFeature;

namespace {

Matrix3f Mul(const Matrix3f& a, const Matrix3f& b) {
  Matrix3f r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r(i, j) = (a(i, 0) * b(0, j) + a(i, 1) * b(1, j)) + a(i, 2) * b(2, j);
  return r;
}

Matrix3f Transpose(const Matrix3f& a) {
  Matrix3f r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r(i, j) = a(j, i);
  return r;
}

Matrix3f Inverse(const Matrix3f& a) {
  Matrix3f r;
  const float c00 = a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1), c01 = a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2),
              c02 = a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0);
  const float det = a(0, 0) * c00 + a(0, 1) * c01 + a(0, 2) * c02;
  const float id = 1.0f / det;
  r(0, 0) = c00 * id;
  r(0, 1) = (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) * id;
  r(0, 2) = (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) * id;
  r(1, 0) = c01 * id;
  r(1, 1) = (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) * id;
  r(1, 2) = (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) * id;
  r(2, 0) = c02 * id;
  r(2, 1) = (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) * id;
  r(2, 2) = (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) * id;
  return r;
}

Matrix3f CameraMatrix(const CameraIntrinsics& I) {  // cc:542-548
  Matrix3f M;
  const float v[9] = {I.fx, 0, I.cx, 0, I.fy, I.cy, 0, 0, 1};
  std::memcpy(M.m, v, sizeof(v));
  return M;
}

// Right singular vector of the smallest singular value of the M x 4 system whose columns are At[0..3] (M <= 6):
// one-sided (Hestenes) Jacobi in double as cv::SVD::compute runs it for cv::triangulatePoints (core/src/lapack.cpp
// JacobiSVDImpl_: rotate column pairs until every pair is orthogonal to 10 * DBL_EPSILON, at most 30 sweeps).
void SmallestRightSingularVector(double At[4][6], int M, double out[4]) {
  const double eps = 2.220446049250313e-16 * 10;
  double W[4], Vt[4][4];
  for (int i = 0; i < 4; i++) {
    W[i] = 0;
    for (int k = 0; k < M; k++) W[i] += At[i][k] * At[i][k];
    for (int k = 0; k < 4; k++) Vt[i][k] = i == k;
  }
  auto hyp = [](double a, double b) {
    a = std::fabs(a), b = std::fabs(b);
    if (a > b) return a * std::sqrt(1 + (b / a) * (b / a));
    return b > 0 ? b * std::sqrt(1 + (a / b) * (a / b)) : 0.0;
  };
  for (int iter = 0; iter < 30; iter++) {
    bool changed = false;
    for (int i = 0; i < 3; i++)
      for (int j = i + 1; j < 4; j++) {
        double a = W[i], b = W[j], p = 0;
        for (int k = 0; k < M; k++) p += At[i][k] * At[j][k];
        if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = hyp(p, beta);
        double c, s;
        if (beta < 0) {
          s = std::sqrt((gamma - beta) * 0.5 / gamma);
          c = p / (gamma * s * 2);
        } else {
          c = std::sqrt((gamma + beta) / (gamma * 2));
          s = p / (gamma * c * 2);
        }
        a = b = 0;
        for (int k = 0; k < M; k++) {
          const double t0 = c * At[i][k] + s * At[j][k], t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0, At[j][k] = t1;
          a += t0 * t0, b += t1 * t1;
        }
        W[i] = a, W[j] = b;
        changed = true;
        for (int k = 0; k < 4; k++) {
          const double t0 = c * Vt[i][k] + s * Vt[j][k], t1 = -s * Vt[i][k] + c * Vt[j][k];
          Vt[i][k] = t0, Vt[j][k] = t1;
        }
      }
    if (!changed) break;
  }
  int best = 0;
  for (int i = 0; i < 4; i++) {
    W[i] = 0;
    for (int k = 0; k < M; k++) W[i] += At[i][k] * At[i][k];
    if (W[i] < W[best]) best = i;
  }
  for (int k = 0; k < 4; k++) out[k] = Vt[best][k];
}

}  // namespace

// ---- configuration: the reference's hard-coded defaults (cc:550-652) ----
FrontendConfig::FrontendConfig() {
  // reference: true (cc:552; quirk Q10: it retains every image forever).  Off here so that nothing is drawn or kept unless
  // asked for; on, the images are the reference's byte for byte (drawn on the GPU, csrc/k_draw.hip).
  debug_images_ = false;
  debug_jpeg_quality_ = 0;
  debug_png_ = false;
  debug_colour_seeded_ = false;
  debug_colour_seed_ = 1;
  visualization_ = false;
  imdecode_reduce_ = 1;  // IMREAD_GRAYSCALE, the reference's flag
  bayer_order_ = VSF_PIX_BAYER_RGGB8;  // COLOR_BayerBG2BGR, the reference's
  resize_width_ = resize_height_ = 0;  // no cv::resize in front
  compressed_cap_ = 0;   // the library's default: the context's width x height + 64 KB
  // reference: AKAZE (cc:553, quirk Q1); ORB is the north-star path and the only extractor built here
  descriptor_extract_type_ = DescriptorExtractorType::ORB;
  best_percent_ = 0.3f;
  nn_match_ratio_ = 0.6f;
  frame_life_ = 10;
  min_odom_rotation = (float)(10.0 / 180.0 * M_PI);
  min_odom_translation = 0.2f;
  min_vision_matches = 10;
  orb_nfeatures = 10000;  // cc:205
  orb_score_type_ = VSF_SCORE_HARRIS;  // cc:211 (cv::ORB::HARRIS_SCORE)
  residual_order = 0;     // Eigen 3.3's reduction order of a fixed-size-3 lazy product (cc:381-383)
  image_width = 0;        // 0: taken from the first observed image
  image_height = 0;

  intrinsics_left.fx = 527.873518f;
  intrinsics_left.cx = 482.823413f;
  intrinsics_left.fy = 527.276819f;
  intrinsics_left.cy = 298.033945f;
  intrinsics_left.k1 = -0.153137f;
  intrinsics_left.k2 = 0.075666f;
  intrinsics_left.p1 = -0.000227f;
  intrinsics_left.p2 = -0.000320f;
  intrinsics_left.k3 = 0;
  intrinsics_right.fx = 530.158021f;
  intrinsics_right.cx = 475.540633f;
  intrinsics_right.fy = 529.682234f;
  intrinsics_right.cy = 299.995465f;
  intrinsics_right.k1 = -0.156833f;
  intrinsics_right.k2 = 0.081841f;
  intrinsics_right.p1 = -0.000779f;
  intrinsics_right.p2 = -0.000356f;
  intrinsics_right.k3 = -0.000779f;

  const Matrix3f K_left = CameraMatrix(intrinsics_left), K_right = CameraMatrix(intrinsics_right);
  const float A_right[12] = {0.999593617649873f,  0.021411909431148f,  -0.018818333830411f, -0.131707087331978f,
                             -0.021140534893290f, 0.999671312094879f,  0.014503294761121f,  0.003232397463343f,
                             0.019122691705565f,  -0.014099571235136f, 0.999717722536176f,  -0.001146108483477f};
  const float A_left[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      float l = 0, r = 0;
      for (int k = 0; k < 3; k++) {
        l += K_left(i, k) * A_left[4 * k + j];
        r += K_right(i, k) * A_right[4 * k + j];
      }
      projection_left[4 * i + j] = l;
      projection_right[4 * i + j] = r;
    }
  {  // cc:613-618: left_cam_to_robot = Eigen::Translation3f(XT) * RT
    Matrix3f RT;
    const float rt[9] = {0.009916590468f, -0.2835522866f, 0.9589055021f,  -0.9998698619f, -0.01501486552f,
                         0.005900269087f, 0.01272480238f, -0.9588392225f, -0.2836642819f};
    std::memcpy(RT.m, rt, sizeof(rt));
    left_cam_to_robot = Affine3f(RT, Vector3f(-0.01f, 0.06f, 0.5299999713897705f));
  }
  // Fundamental matrix (cc:635-644).  The reference builds the cross-product matrix from A[1], A[2], A[3] of a
  // 3-vector (out-of-range read, quirk Q2); the well-formed skew matrix of A is used here instead.
  Matrix3f rotation;
  float translation[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) rotation(i, j) = A_right[4 * i + j];
    translation[i] = A_right[4 * i + 3];
  }
  const Matrix3f KRt = Mul(K_left, Transpose(rotation));
  float A[3];
  for (int i = 0; i < 3; i++) A[i] = (KRt(i, 0) * translation[0] + KRt(i, 1) * translation[1]) + KRt(i, 2) * translation[2];
  Matrix3f C;
  const float c[9] = {0.0f, -A[2], A[1], A[2], 0.0f, -A[0], -A[1], A[0], 0.0f};
  std::memcpy(C.m, c, sizeof(c));
  fundamental = Mul(Mul(Mul(Transpose(Inverse(K_right)), rotation), Transpose(K_left)), C);
}

void CamToRobot(const FrontendConfig& config, float out[12]) {
  const Affine3f& a = config.left_cam_to_robot;
  const float t[3] = {a.translation_.x(), a.translation_.y(), a.translation_.z()};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) out[4 * r + c] = a.linear_(r, c);
    out[4 * r + 3] = t[r];
  }
}

Affine3f AffineFromRowMajor(const float m[12]) {
  Matrix3f R;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R(r, c) = m[4 * r + c];
  return Affine3f(R, Vector3f(m[3], m[7], m[11]));
}

vsf_calibration MakeCalibration(const FrontendConfig& config) {
  vsf_calibration c;
  std::memset(&c, 0, sizeof(c));
  std::memcpy(c.projection_left, config.projection_left, sizeof(c.projection_left));
  std::memcpy(c.projection_right, config.projection_right, sizeof(c.projection_right));
  const Matrix3f K = CameraMatrix(config.intrinsics_left);  // camera_matrix_left, cc:575-578
  std::memcpy(c.camera_matrix_left, K.m, sizeof(c.camera_matrix_left));
  const CameraIntrinsics& I = config.intrinsics_left;       // distortion_coeffs_left, cc:623-628
  const float d[5] = {I.k1, I.k2, I.p1, I.p2, I.k3};
  std::memcpy(c.distortion_left, d, sizeof(d));
  std::memcpy(c.fundamental, config.fundamental.m, sizeof(c.fundamental));
  c.triangulate_rows = 6;  // OpenCV 3.2.0's cvTriangulatePoints (CMakeLists.txt:20 pins that version)
  return c;
}

// ---- Frame (cc:511-519) ----
Frame::Frame(const std::vector<vsf_keypoint>& keypoints, const std::vector<uint8_t>& descriptors, uint64_t frame_ID) {
  keypoints_ = keypoints;
  descriptors_ = descriptors;
  frame_ID_ = frame_ID;
  is_initial_ = std::vector<bool>(keypoints_.size(), true);
  initial_ids_ = std::vector<int64_t>(keypoints_.size(), -1);
}

// ---- Frontend ----
Frontend::Frontend(const std::string& config_path) : Frontend(config_path, FrontendConfig(), 0) {}

Frontend::Frontend(const std::string& /*config_path*/, const FrontendConfig& config, int device)
    : Frontend(config, device, nullptr, 0) {
  if (ContextWidth(config_) > 0 && ContextHeight(config_) > 0) EnsureContext(ContextWidth(config_), ContextHeight(config_));
}

// Everything but the context: a Frontend of its own builds it right away (above), a group builds ONE for all its members.
Frontend::Frontend(const FrontendConfig& config, int device, FrontendGroup* group, int stream)
    : odom_initialized_(false),
      odom_timestamp_(0),
      config_(config),
      curr_frame_ID_(0),
      stereo_ambig_constraint_(10000),  // cc:353
      fused_(true),
      pipelined_(false),
      ctx_(nullptr),
      group_(group),
      stream_(stream),
      owns_ctx_(stream == 0),
      device_(device),
      last_status_(VSF_OK) {
  vsfrand::seed(colour_rng_, config_.debug_colour_seed_);
  OwnMasks();
  if (config_.descriptor_extract_type_ != FrontendConfig::DescriptorExtractorType::ORB &&
      config_.descriptor_extract_type_ != FrontendConfig::DescriptorExtractorType::FREAK)
    last_status_ = VSF_ERR_UNSUPPORTED;  // the reference would build AKAZE / BRISK / SURF / SIFT here (cc:193-232)
}

// Frames still in flight (pipelined mode) are dropped, not booked: nobody can read the problem any more.  vsf_destroy
// waits for every stream of the context -- the slots' included -- before it frees what their kernels write.
Frontend::~Frontend() {
  pending_count_ = 0;
  if (owns_ctx_) vsf_destroy(ctx_);
}

bool Frontend::EnsureContext(int width, int height) {
  return group_ ? group_->EnsureContext(width, height) : EnsureOwnContext(width, height, 1);
}

bool Frontend::EnsureOwnContext(int width, int height, int n_streams) {
  if (ctx_) {
    vsf_params p;
    vsf_get_params(ctx_, &p);
    if (p.width == width && p.height == height && p.max_images >= 2 * batch_frames() && ctx_depth_ == queue_depth())
      return true;
    // the context is replaced (another image size, or pipelining switched on): the frames still in the queue belong to
    // the old one and are booked first, in order; whatever that returns, their tickets die with the context
    Flush();
    pending_count_ = 0;
    vsf_destroy(ctx_);
    ctx_ = nullptr;
  }
  vsf_params p;
  vsf_params_default(&p, width, height, 2 * batch_frames());  // extraction buffers for one batch of stereo frames
  p.nfeatures = config_.orb_nfeatures;
  p.score_type = config_.orb_score_type_;
  p.residual_order = config_.residual_order;
  last_status_ = vsf_params_set_ratio(&p, config_.nn_match_ratio_);
  if (last_status_ != VSF_OK) return false;
  last_status_ = vsf_create(&p, device_, &ctx_);
  if (last_status_ != VSF_OK) return false;
  ctx_generation_++;
  declared_w_ = declared_h_ = 0;  // (a new context's streams have no declared input size)
  told_bayer_order_ = 0;          // (... and have been told no Bayer order)
  ctx_depth_ = queue_depth();
  last_status_ = vsf_set_option(ctx_, VSF_OPT_OBSERVE_THREAD, queue_thread_ ? 1 : 0);
  if (last_status_ == VSF_OK) last_status_ = vsf_set_option(ctx_, VSF_OPT_OBSERVE_COPY_THREAD, copy_thread_ ? 1 : 0);
  for (const auto& ov : ctx_options_)
    if (last_status_ == VSF_OK) last_status_ = vsf_set_option(ctx_, ov.first, ov.second);
  if (last_status_ == VSF_OK) last_status_ = vsf_observe_configure(ctx_, ctx_depth_, min_batch_, 0);
  if (last_status_ == VSF_OK && n_streams > 1) last_status_ = vsf_observe_set_streams(ctx_, n_streams);
  if (last_status_ == VSF_OK && config_.compressed_cap_ > 0) last_status_ = vsf_observe_set_compressed_cap(ctx_, config_.compressed_cap_);
  if (last_status_ == VSF_OK) last_status_ = ApplyDebugConfig(n_streams);
  // the point cloud of GetVisualization: one more launch in every batch's tail (vsf_observe_set_world_points)
  if (last_status_ == VSF_OK && config_.visualization_) {
    float cam_to_robot[12];
    CamToRobot(config_, cam_to_robot);
    last_status_ = vsf_observe_set_world_points(ctx_, 1, cam_to_robot);
  }
  // the detection masks: each member's pair into its own slots, named to its stream
  for (int i = 0; last_status_ == VSF_OK && i < n_streams; i++)
    last_status_ = group_ ? group_->members_[(size_t)i]->ApplyMasks(ctx_) : ApplyMasks(ctx_);
  // ... placed with each camera's own left_cam_to_robot: a group's members are streams of this one queue
  for (int i = 0; group_ && last_status_ == VSF_OK && i < n_streams; i++) {
    float cam_to_robot[12];
    CamToRobot(group_->members_[(size_t)i]->config_, cam_to_robot);
    last_status_ = vsf_observe_set_stream_cam_to_robot(ctx_, i, cam_to_robot);
  }
  pending_.assign((size_t)ctx_depth_, PendingFrame());
  pending_head_ = pending_count_ = 0;
  return last_status_ == VSF_OK;
}

vsf_status Frontend::ApplyDebugConfig(int n_streams) {
  // (the seeds go in while the switch is off; the forms of file need it on: off in reverse order first -- all three are
  // accepted without effect where nothing was on)
  vsf_status st = vsf_observe_set_debug_png(ctx_, 0);
  if (st == VSF_OK) st = vsf_observe_set_debug_jpeg(ctx_, 0);
  if (st == VSF_OK) st = vsf_observe_set_debug_images(ctx_, 0);
  if (st == VSF_OK) {
    std::vector<uint32_t> seeds;
    if (config_.debug_colour_seeded_)
      for (int i = 0; i < n_streams; i++) seeds.push_back(group_ ? group_->members_[(size_t)i]->config_.debug_colour_seed_ : config_.debug_colour_seed_);
    st = vsf_observe_set_debug_seeds(ctx_, seeds.empty() ? nullptr : seeds.data(), (int)seeds.size());
    // (the queue's generators start at their seeds here: so does the object's own, which per-call mode draws from -- the modes
    // agree across a replaced context too)
    vsfrand::seed(colour_rng_, config_.debug_colour_seed_);
  }
  // the queue's results carry the right frame's filtered keypoints too (the stereo debug image draws them)
  if (st == VSF_OK && config_.debug_images_) st = vsf_observe_set_debug_images(ctx_, 1);
  // ... and leave as files when the configuration asks for one form of them (both: the second request is refused)
  const int form = debug_file_form();
  if (st == VSF_OK && config_.debug_images_ && (form & kFormJpeg)) st = vsf_observe_set_debug_jpeg(ctx_, config_.debug_jpeg_quality_);
  if (st == VSF_OK && config_.debug_images_ && (form & kFormPng)) st = vsf_observe_set_debug_png(ctx_, 1);
  return st;
}

// cc:250-263.  The reference copies the still-uninitialised odom_*_ into prev_odom_*_ on the first call (quirk
// Q11); here prev_* starts at the first observed pose.
void Frontend::ObserveOdometry(const Vector3f& translation, const Quaternionf& rotation, double timestamp) {
  if (!odom_initialized_) {
    init_odom_rotation_ = rotation;
    init_odom_translation_ = translation;
    prev_odom_rotation_ = rotation;
    prev_odom_translation_ = translation;
    odom_initialized_ = true;
  }
  odom_translation_ = translation;
  odom_rotation_ = rotation;
  odom_timestamp_ = timestamp;
}

// cc:175-186
bool Frontend::OdomCheck() {
  if (!odom_initialized_) return false;
  if ((prev_odom_translation_ - odom_translation_).norm() > config_.min_odom_translation) return true;
  if (prev_odom_rotation_.angularDistance(odom_rotation_) > config_.min_odom_rotation) return true;
  return false;
}

// cc:266-280: detectAndCompute (ORB) or FAST detect (+ FREAK compute, which is not built: keypoints only).
void Frontend::OwnMasks() {
  Image* views[2] = {&config_.mask_left_, &config_.mask_right_};
  for (int eye = 0; eye < 2; eye++) {
    Image& v = *views[eye];
    if (v.empty()) {
      mask_store_[eye].clear();
      v = Image();
      continue;
    }
    std::vector<uint8_t> copy((size_t)v.rows * (size_t)v.cols);
    for (int y = 0; y < v.rows; y++) std::memcpy(copy.data() + (size_t)y * v.cols, v.data + (size_t)y * v.step, (size_t)v.cols);
    mask_store_[eye].swap(copy);
    v = Image(mask_store_[eye].data(), v.rows, v.cols, (size_t)v.cols);
  }
}

int Frontend::mask_slot(int eye) const {
  return (eye ? config_.mask_right_ : config_.mask_left_).empty() ? -1 : 2 * stream_ + eye;
}

vsf_status Frontend::ApplyMasks(vsf_ctx* ctx) {
  const Image* views[2] = {&config_.mask_left_, &config_.mask_right_};
  for (int eye = 0; eye < 2; eye++) {
    const Image& v = *views[eye];
    const vsf_status st = v.empty() ? vsf_mask_clear(ctx, 2 * stream_ + eye)
                                    : vsf_mask_set(ctx, 2 * stream_ + eye, v.data, v.cols, v.rows, v.step);
    if (st != VSF_OK) return st;
  }
  vsf_status st = vsf_observe_set_stream_masks(ctx, stream_, mask_slot(0), mask_slot(1));
  if (st == VSF_OK && !group_) st = vsf_set_image_masks(ctx, mask_slot(0), mask_slot(1));
  return st;
}

void Frontend::set_masks(const Image& left, const Image& right) {
  config_.mask_left_ = left;
  config_.mask_right_ = right;
  OwnMasks();
  if (ctx_) last_status_ = ApplyMasks(ctx_);  // (no context yet: the next one takes them, and an earlier status stays)
}

void Frontend::SelectImageMasks(int first) {
  // (the context's pair is (left, right) since ApplyMasks; an object without masks never asks)
  if (mask_slot(0) >= 0 || mask_slot(1) >= 0) vsf_set_image_masks(ctx_, mask_slot(first), mask_slot(1));
}

bool Frontend::ExtractFeatures(const Image& image, Frame* frame, int eye) {
  if (image.empty() || !EnsureContext(image.cols, image.rows)) {
    if (last_status_ == VSF_OK) last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  // the right image extracted on its own is image 0 of its call: the pair is (right, right) for that call alone
  struct EyeScope {
    Frontend* f;
    int eye;
    EyeScope(Frontend* fe, int e) : f(fe), eye(e) {
      if (eye) f->SelectImageMasks(1);
    }
    ~EyeScope() {
      if (eye) f->SelectImageMasks(0);
    }
  } eye_scope(this, eye);
  vsf_params p;
  vsf_get_params(ctx_, &p);
  int n = 0;
  std::vector<vsf_keypoint> kps;
  std::vector<uint8_t> desc;
  if (config_.descriptor_extract_type_ == FrontendConfig::DescriptorExtractorType::FREAK) {
    int cap = 1 << 16;
    kps.resize(cap);
    last_status_ = vsf_fast_detect(ctx_, image.data, image.cols, image.rows, image.step, -1, 1, kps.data(), cap, &n);
    if (last_status_ == VSF_ERR_CAPACITY) {
      cap = n;
      kps.resize(cap);
      last_status_ = vsf_fast_detect(ctx_, image.data, image.cols, image.rows, image.step, -1, 1, kps.data(), cap, &n);
    }
    if (last_status_ != VSF_OK) return false;
    kps.resize(n);
  } else {
    const int cap = p.max_keypoints;
    kps.resize(cap);
    desc.resize((size_t)cap * VSF_DESC_BYTES);
    last_status_ = vsf_extract(ctx_, image.data, image.cols, image.rows, image.step, kps.data(), desc.data(), cap, &n);
    if (last_status_ != VSF_OK) return false;
    kps.resize(n);
    desc.resize((size_t)n * VSF_DESC_BYTES);
  }
  *frame = Frame(kps, desc, curr_frame_ID_);
  return true;
}

bool Frontend::ExtractFeaturesPair(const Image& left, const Image& right, Frame* left_frame, Frame* right_frame) {
  const bool orb = config_.descriptor_extract_type_ != FrontendConfig::DescriptorExtractorType::FREAK;
  if (!orb || left.empty() || right.empty() || left.cols != right.cols || left.rows != right.rows ||
      left.step != right.step)
    return ExtractFeatures(left, left_frame, 0) && ExtractFeatures(right, right_frame, 1);
  if (!EnsureContext(left.cols, left.rows)) {
    if (last_status_ == VSF_OK) last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  vsf_params p;
  vsf_get_params(ctx_, &p);
  const int cap = p.max_keypoints;
  std::vector<vsf_keypoint> kl(cap), kr(cap);
  std::vector<uint8_t> dl((size_t)cap * VSF_DESC_BYTES), dr((size_t)cap * VSF_DESC_BYTES);
  int nl = 0, nr = 0;
  last_status_ = vsf_extract_pair(ctx_, left.data, right.data, left.cols, left.rows, left.step, kl.data(), dl.data(), &nl,
                                  kr.data(), dr.data(), &nr, cap);
  if (last_status_ != VSF_OK) return false;
  kl.resize(nl);
  dl.resize((size_t)nl * VSF_DESC_BYTES);
  kr.resize(nr);
  dr.resize((size_t)nr * VSF_DESC_BYTES);
  *left_frame = Frame(kl, dl, curr_frame_ID_);
  *right_frame = Frame(kr, dr, curr_frame_ID_);
  return true;
}

// cc:521-538
std::vector<vsf_dmatch> Frontend::GetMatches(const Frame& frame_query, const Frame& frame_train, double nn_match_ratio) {
  std::vector<vsf_dmatch> best_matches;
  if (nn_match_ratio != (double)config_.nn_match_ratio_ || !ctx_) {
    last_status_ = VSF_ERR_UNSUPPORTED;  // the context carries the configured ratio
    return best_matches;
  }
  const int nq = (int)frame_query.keypoints_.size(), nt = (int)frame_train.keypoints_.size();
  if (frame_query.descriptors_.size() != (size_t)nq * VSF_DESC_BYTES ||
      frame_train.descriptors_.size() != (size_t)nt * VSF_DESC_BYTES)
    return best_matches;  // no descriptors (FREAK branch)
  best_matches.resize(nq);
  int n = 0;
  last_status_ = vsf_get_matches(ctx_, frame_query.descriptors_.data(), nq, frame_train.descriptors_.data(), nt,
                                 best_matches.data(), nq, &n);
  best_matches.resize(last_status_ == VSF_OK ? n : 0);
  return best_matches;
}

// cc:282-309
VisionFactor Frontend::GetFeatureMatches(Frame* past_frame_ptr, Frame* curr_frame_ptr) {
  Frame& past_frame = *past_frame_ptr;
  Frame& curr_frame = *curr_frame_ptr;
  std::vector<FeatureMatch> pairs;
  std::vector<vsf_dmatch> matches = GetMatches(past_frame, curr_frame, config_.nn_match_ratio_);
  // cv::DMatch::operator< compares distance only; std::sort is unstable and its tie order decides who survives.
  std::sort(matches.begin(), matches.end(),
            [](const vsf_dmatch& a, const vsf_dmatch& b) { return a.distance < b.distance; });
  const int num_good_matches = (int)(matches.size() * config_.best_percent_);  // size_t * float -> float -> int
  matches.erase(matches.begin() + std::min<size_t>(std::max(num_good_matches, 0), matches.size()), matches.end());
  for (const vsf_dmatch& match : matches) {
    pairs.push_back(FeatureMatch(match.queryIdx, match.trainIdx));
    if (curr_frame.is_initial_[match.trainIdx]) {
      curr_frame.is_initial_[match.trainIdx] = false;
      curr_frame.initial_ids_[match.trainIdx] = past_frame.is_initial_[match.queryIdx]
                                                    ? (int64_t)past_frame.frame_ID_
                                                    : past_frame.initial_ids_[match.queryIdx];
    }
  }
  return VisionFactor(past_frame.frame_ID_, curr_frame.frame_ID_, pairs);
}

void Frontend::GetFeatureMatchesAll(std::vector<Frame>* past_frames, Frame* curr_frame_ptr,
                                    std::vector<VisionFactor>* out) {
  Frame& curr_frame = *curr_frame_ptr;
  const int S = (int)past_frames->size();
  if (S == 0) return;
  const int nt = (int)curr_frame.keypoints_.size();
  bool batched = ctx_ != nullptr && curr_frame.descriptors_.size() == (size_t)nt * VSF_DESC_BYTES;
  std::vector<const uint8_t*> q(S);
  std::vector<int> nq(S), nm(S, 0);
  int cap = 1;
  for (int s = 0; s < S && batched; s++) {
    const Frame& f = (*past_frames)[s];
    nq[s] = (int)f.keypoints_.size();
    if (f.descriptors_.size() != (size_t)nq[s] * VSF_DESC_BYTES) batched = false;
    q[s] = f.descriptors_.data();
    cap = std::max(cap, nq[s]);
  }
  if (!batched) {  // (FREAK branch: no descriptors) one call per past frame, as the reference
    for (Frame& past : *past_frames) out->push_back(GetFeatureMatches(&past, &curr_frame));
    return;
  }
  std::vector<vsf_dmatch> all((size_t)S * cap);
  last_status_ = vsf_get_matches_multi(ctx_, q.data(), nq.data(), S, curr_frame.descriptors_.data(), nt, all.data(), cap,
                                       nm.data());
  if (last_status_ != VSF_OK) std::fill(nm.begin(), nm.end(), 0);
  for (int s = 0; s < S; s++) {  // cc:289-308 for every past frame, in list order
    Frame& past_frame = (*past_frames)[s];
    std::vector<vsf_dmatch> matches(all.begin() + (size_t)s * cap, all.begin() + (size_t)s * cap + nm[s]);
    std::sort(matches.begin(), matches.end(),
              [](const vsf_dmatch& a, const vsf_dmatch& b) { return a.distance < b.distance; });
    const int num_good_matches = (int)(matches.size() * config_.best_percent_);
    matches.erase(matches.begin() + std::min<size_t>(std::max(num_good_matches, 0), matches.size()), matches.end());
    std::vector<FeatureMatch> pairs;
    for (const vsf_dmatch& match : matches) {
      pairs.push_back(FeatureMatch(match.queryIdx, match.trainIdx));
      if (curr_frame.is_initial_[match.trainIdx]) {
        curr_frame.is_initial_[match.trainIdx] = false;
        curr_frame.initial_ids_[match.trainIdx] = past_frame.is_initial_[match.queryIdx]
                                                      ? (int64_t)past_frame.frame_ID_
                                                      : past_frame.initial_ids_[match.queryIdx];
      }
    }
    out->push_back(VisionFactor(past_frame.frame_ID_, curr_frame.frame_ID_, pairs));
  }
}

// cc:311-321
void Frontend::AddOdometryFactor() {
  const Vector3f translation = prev_odom_rotation_.inverse() * (odom_translation_ - prev_odom_translation_);
  const Quaternionf rotation(odom_rotation_ * prev_odom_rotation_.inverse());
  odometry_factors_.push_back(OdometryFactor(curr_frame_ID_ - 1, curr_frame_ID_, translation, rotation));
}

// cc:353-398.  |l^T F r| per stereo match; survivors re-index both frames; the next frame's threshold is this frame's
// mean residual + 2.  The reference's `(left_ph.transpose() * F * right_ph).norm()` is two rounds of three-term dot
// products; Eigen 3.3 evaluates a fixed-size-3 lazy product coefficient as cwiseProduct().sum() with the unrolled
// reduction redux_novec_unroller<.., 0, 3>, which splits 1 + 2: a0 b0 + (a1 b1 + a2 b2) (config_.residual_order 0);
// .norm() of the 1 x 1 result is sqrt(x * x) == |x| barring under- / overflow of the square.
namespace {
inline float Dot3(int order, float a0, float b0, float a1, float b1, float a2, float b2) {
  const float p0 = a0 * b0, p1 = a1 * b1, p2 = a2 * b2;
  return order ? (p0 + p1) + p2 : p0 + (p1 + p2);
}
}  // namespace

void Frontend::RemoveAmbigStereo(Frame* left, Frame* right, const std::vector<vsf_dmatch>& stereo_matches) {
  std::vector<vsf_keypoint> left_keypoints, right_keypoints;
  std::vector<uint8_t> left_descs, right_descs;
  const Matrix3f& F = config_.fundamental;
  float avg_constraint = 0.0f;
  for (size_t m = 0; m < stereo_matches.size(); m++) {
    const vsf_dmatch& match = stereo_matches[m];
    const vsf_keypoint& lk = left->keypoints_[match.queryIdx];
    const vsf_keypoint& rk = right->keypoints_[match.trainIdx];
    const float l[3] = {lk.x, lk.y, 1.0f}, r[3] = {rk.x, rk.y, 1.0f};
    float t[3];
    const int order = config_.residual_order;
    for (int j = 0; j < 3; j++) t[j] = Dot3(order, l[0], F(0, j), l[1], F(1, j), l[2], F(2, j));
    const float constraint = std::fabs(Dot3(order, t[0], r[0], t[1], r[1], t[2], r[2]));
    avg_constraint += constraint;
    if (constraint <= stereo_ambig_constraint_) {
      left_keypoints.push_back(lk);
      right_keypoints.push_back(rk);
      const uint8_t* ld = left->descriptors_.data() + (size_t)match.queryIdx * VSF_DESC_BYTES;
      const uint8_t* rd = right->descriptors_.data() + (size_t)match.trainIdx * VSF_DESC_BYTES;
      left_descs.insert(left_descs.end(), ld, ld + VSF_DESC_BYTES);
      right_descs.insert(right_descs.end(), rd, rd + VSF_DESC_BYTES);
    }
  }
  // cc:392-394.  Without a match this is 0/0 + 2 = NaN (quirk Q3): the next frame keeps no feature (`c <= NaN` is
  // false) but updates the threshold from its own matches, so the frame after it is filtered normally again.
  stereo_ambig_constraint_ = avg_constraint / (float)stereo_matches.size() + 2.0f;
  *left = Frame(left_keypoints, left_descs, left->frame_ID_);
  *right = Frame(right_keypoints, right_descs, right->frame_ID_);
}

// cc:117-173: right->left matches with best_percent forced to 1, then cv::triangulatePoints (per point the right
// singular vector of the smallest singular value of the 6 x 4 system OpenCV 3.2 builds: x*P2-P0, y*P2-P1, x*P1-y*P0 per
// view, in double) and the homogeneous divide in float.  Same arithmetic as the device kernel (csrc/k_points.hip);
// against real OpenCV the values agree to rounding (its SVD may run through LAPACK), not bit for bit.
void Frontend::Calculate3DPoints(Frame* left_frame, Frame* right_frame, std::vector<Vector3f>* points,
                                 VisionFactor* matches_out) {
  const float best_percent = config_.best_percent_;
  config_.best_percent_ = 1.0f;
  const VisionFactor matches = GetFeatureMatches(right_frame, left_frame);
  config_.best_percent_ = best_percent;
  if (matches_out) *matches_out = matches;
  if (matches.feature_matches.empty()) return;
  const float* P[2] = {config_.projection_left, config_.projection_right};
  for (const FeatureMatch& match : matches.feature_matches) {
    const vsf_keypoint& left_pt = left_frame->keypoints_[match.feature_idx_current];
    const vsf_keypoint& right_pt = right_frame->keypoints_[match.feature_idx_initial];
    const double xy[2][2] = {{left_pt.x, left_pt.y}, {right_pt.x, right_pt.y}};
    double At[4][6];
    for (int j = 0; j < 2; j++)
      for (int k = 0; k < 4; k++) {
        const double p0 = P[j][k], p1 = P[j][4 + k], p2 = P[j][8 + k];
        At[k][3 * j + 0] = xy[j][0] * p2 - p0;
        At[k][3 * j + 1] = xy[j][1] * p2 - p1;
        At[k][3 * j + 2] = xy[j][0] * p1 - xy[j][1] * p0;
      }
    double X[4];
    SmallestRightSingularVector(At, 6, X);
    const float xf = (float)X[0], yf = (float)X[1], zf = (float)X[2], wf = (float)X[3];
    points->push_back(Vector3f(xf, yf, zf) / wf);
  }
}

// cc:323-351: cv::undistortPoints(distorted, out, K_left, dist_left, noArray(), K_left): 5 fixed-point
// iterations in double per point, then re-projection with the same camera matrix (row f2 of SURVEY section 8(f)).
void Frontend::UndistortFeaturePoints(std::vector<VisionFeature>* features_ptr) {
  std::vector<VisionFeature>& features = *features_ptr;
  const CameraIntrinsics& I = config_.intrinsics_left;
  const double k[5] = {I.k1, I.k2, I.p1, I.p2, I.k3};
  const double fx = I.fx, fy = I.fy, cx = I.cx, cy = I.cy, ifx = 1. / fx, ify = 1. / fy;
  for (VisionFeature& f : features) {
    double x = (f.pixel.x() - cx) * ifx, y = (f.pixel.y() - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
      const double r2 = x * x + y * y;
      const double icdist = 1. / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
      const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
      const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
      x = (x0 - deltaX) * icdist;
      y = (y0 - deltaY) * icdist;
    }
    f.pixel = Vector2f((float)(x * fx + cx), (float)(y * fy + cy));
  }
}

// cc:400-472 through ONE submission to the GPU (vsf_observe_stereo): upload, both ExtractFeatures, GetMatches,
// RemoveAmbigStereo, every GetFeatureMatches of the temporal loop, Calculate3DPoints, the VisionFeature records and
// UndistortFeaturePoints run on the device back to back and come home in one compact buffer; the kept frames'
// descriptors never leave HBM.  What stays here is the reference's bookkeeping (is_initial_ / initial_ids_, nodes,
// factors, the sliding window), in the reference's order.
bool Frontend::ObserveImageFused(const Image& left_image, const Image& right_image, int pixfmt) {
  FramePayload fp;
  fp.left = left_image.data;
  fp.right = right_image.data;
  fp.step = left_image.step;
  if (pixfmt != VSF_PIX_MONO8) fp.pixfmt = pixfmt;  // (MONO8: the call the queue has always had)
  return ObserveFused(left_image.cols, left_image.rows, fp);
}

bool Frontend::DeclareBayerOrder() {
  const int order = config_.bayer_order_;
  if (order == (told_bayer_order_ ? told_bayer_order_ : (int)VSF_PIX_BAYER_RGGB8)) return true;
  // (the library takes a new order only while no frame of the stream is in flight: the rule of DeclareInput)
  if (!(group_ ? group_->Flush() : Flush())) return false;
  last_status_ = vsf_observe_set_bayer_order(ctx_, stream_, order);
  if (last_status_ != VSF_OK) return false;
  told_bayer_order_ = order;
  return true;
}

bool Frontend::DeclareInput(int width, int height) {
  if (width == declared_w_ && height == declared_h_) return true;
  // a frame of another size than the one before: the library takes a new size only while no frame of the stream is in
  // flight, so those are booked first (a group's in its order)
  if (!(group_ ? group_->Flush() : Flush())) return false;
  last_status_ = vsf_observe_set_input_size(ctx_, stream_, width, height);
  if (last_status_ != VSF_OK) return false;
  declared_w_ = width;
  declared_h_ = height;
  return true;
}

bool Frontend::ObserveFused(int width, int height, const FramePayload& fp) {
  // config.resize_width_ / resize_height_: the context has the resized size, the frame its own
  const int cw = resizing() ? config_.resize_width_ : width, ch = resizing() ? config_.resize_height_ : height;
  if (!EnsureContext(cw, ch)) {
    if (last_status_ == VSF_OK) last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  // (a frame that has the context's size already is a frame like any other: no declared size, no resize launch)
  const bool other = width != cw || height != ch;
  if (!DeclareInput(other ? width : 0, other ? height : 0)) return false;
  if (fp.compressed && fp.bayer && !DeclareBayerOrder()) return false;
  const vsf_calibration calib = MakeCalibration(config_);
  // the queue must have room: when it is full, the oldest frame is collected and booked first
  // (a group member: the queue is the group's, and so is the order its frames are retired in)
  auto in_flight = [this] { return group_ ? group_->in_flight() : pending_count_; };
  auto retire = [this] { return group_ ? group_->RetireOldest() : RetireOldest(); };
  while ((int)in_flight() >= queue_depth())
    if (!retire()) return false;
  PendingFrame& pf = pending_[(pending_head_ + pending_count_) % pending_.size()];
  if (config_.visualization_ && !SetQueuePose()) return false;
  if (fp.device) {  // (already in HBM: one launch on the producer's stream, no staging copy, no upload)
    const vsf_dev_frame df{fp.left, fp.right, fp.left_bytes, fp.right_bytes};
    const int pixfmt = fp.pixfmt >= 0 ? fp.pixfmt : fp.bayer ? (int)VSF_PIX_BAYER_RGGB8 : (int)VSF_PIX_MONO8;
    last_status_ = vsf_observe_submit_dev(ctx_, stream_, &df, 1, pixfmt, fp.hip_stream, &calib, config_.best_percent_,
                                          (int)config_.frame_life_, &pf.ticket);
  } else if (fp.compressed && fp.reduce > 1)  // IMREAD_REDUCED_GRAYSCALE_N (refusals as below)
    last_status_ = vsf_observe_submit_compressed_reduced(ctx_, stream_, fp.left, fp.left_bytes, fp.right, fp.right_bytes, fp.reduce,
                                                         &calib, config_.best_percent_, (int)config_.frame_life_, &pf.ticket);
  else if (fp.compressed)  // (a file the host half of the decoders refuses: no ticket, nothing booked, the queue as it was)
    last_status_ = vsf_observe_submit_compressed_stream(ctx_, stream_, fp.left, fp.left_bytes, fp.right, fp.right_bytes,
                                                        fp.bayer ? 1 : 0, &calib, config_.best_percent_,
                                                        (int)config_.frame_life_, &pf.ticket);
  else if (fp.pixfmt >= 0)  // sensor_msgs/Image as published: gray on the device, inside the batch
    last_status_ = vsf_observe_submit_stream_pix(ctx_, stream_, fp.left, fp.right, width, height, fp.step, fp.pixfmt, &calib,
                                                 config_.best_percent_, (int)config_.frame_life_, &pf.ticket);
  else
    last_status_ = vsf_observe_submit_stream(ctx_, stream_, fp.left, fp.right, width, height, fp.step, &calib,
                                             config_.best_percent_, (int)config_.frame_life_, &pf.ticket);
  if (last_status_ != VSF_OK) return false;
  pf.odom_translation = odom_translation_;
  pf.odom_rotation = odom_rotation_;
  pf.prev_odom_translation = prev_odom_translation_;
  pf.prev_odom_rotation = prev_odom_rotation_;
  pf.odom_timestamp = odom_timestamp_;
  pending_count_++;
  if (group_) group_->submitted(stream_);
  // cc:457-458: the pose of this frame is what the NEXT call's OdomCheck compares with
  prev_odom_rotation_ = odom_rotation_;
  prev_odom_translation_ = odom_translation_;
  if (!pipelined_) return retire();
  // results that are already there are booked now (no waiting, nothing sent early): at a camera's rate the problem stays a
  // frame or two behind instead of a queue's depth; when frames stream in faster than the GPU serves them this finds nothing
  // and the queue fills as before
  return BookFinished();
}

// Books, oldest first, the frames whose results are already there (vsf_observe_poll: no wait, nothing sent early); the newest
// frame always stays in flight.  What ObserveFused does behind every submit, and all GetVisualization does to the queue.
bool Frontend::BookFinished() {
  auto in_flight = [this] { return group_ ? group_->in_flight() : pending_count_; };
  while (ctx_ && in_flight() > 1) {
    int ready = 0;
    const int64_t oldest = group_ ? group_->oldest_ticket() : pending_[pending_head_].ticket;
    if (vsf_observe_poll(ctx_, oldest, &ready) != VSF_OK || !ready) break;
    if (!(group_ ? group_->RetireOldest() : RetireOldest())) return false;
  }
  return true;
}

// The pose of the node this frame becomes (cc:444-447, the expressions of RetireOldest / FinishNode on the odometry this call
// sees), handed to the queue so that the batch's tail can place the frame's points in the world.
bool Frontend::SetQueuePose() {
  const Vector3f loc = init_odom_rotation_.inverse() * (odom_translation_ - init_odom_translation_);
  const Quaternionf angle = odom_rotation_ * init_odom_rotation_.inverse();
  const float l[3] = {loc.x(), loc.y(), loc.z()}, q[4] = {angle.x(), angle.y(), angle.z(), angle.w()};
  last_status_ = vsf_observe_set_pose(ctx_, stream_, l, q);
  return last_status_ == VSF_OK;
}

void Frontend::BookVisualization(size_t first_vision_factor, const double* xyz, int n) {
  const SLAMNode& node = nodes_.back();
  viz_nodes_.push_back(slam_visualization::StdPoint(node.pose.loc));
  if (node.node_idx > 0 && !odometry_factors_.empty()) {  // (the factor booked with this node: pose_i = node_idx - 1)
    const OdometryFactor& f = odometry_factors_.back();
    viz_odometry_.push_back(slam_visualization::StdPoint(nodes_[f.pose_i].pose.loc));
    viz_odometry_.push_back(slam_visualization::StdPoint(nodes_[f.pose_j].pose.loc));
  }
  for (size_t i = first_vision_factor; i < vision_factors_.size(); i++) {
    const VisionFactor& f = vision_factors_[i];
    viz_vision_.push_back(slam_visualization::StdPoint(nodes_[f.pose_idx_initial].pose.loc));
    viz_vision_.push_back(slam_visualization::StdPoint(nodes_[f.pose_idx_current].pose.loc));
  }
  if (n > 0) cloud_.insert(cloud_.end(), xyz, xyz + (size_t)3 * n);
}

bool Frontend::GetVisualization(Visualization* out) {
  if (!out || !config_.visualization_) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  if (pipelined_ && !BookFinished()) return false;
  using slam_visualization::ColorRGBA;
  using slam_visualization::Marker;
  using slam_visualization::Point;
  const size_t n_cloud = cloud_.size() / 3;
  if (out->source != this || out->nodes.points.size() > viz_nodes_.size() || out->odometry.points.size() > viz_odometry_.size() ||
      out->vision.points.size() > viz_vision_.size() || out->vision_points.points.size() > n_cloud) {
    slam_visualization::InitializeVisualization(out);
    out->source = this;
  }
  auto append = [](Marker* m, const Point* all, size_t n, const slam_visualization::Color4f& colour) {
    const size_t have = m->points.size();
    if (have == n) return;
    m->points.insert(m->points.end(), all + have, all + n);
    m->colors.resize(n, slam_visualization::StdColor(colour));
  };
  append(&out->nodes, viz_nodes_.data(), viz_nodes_.size(), slam_visualization::Color4f::kRed());
  append(&out->odometry, viz_odometry_.data(), viz_odometry_.size(), slam_visualization::Color4f::kGreen());
  append(&out->vision, viz_vision_.data(), viz_vision_.size(), slam_visualization::Color4f::kBlue());
  // (Point is three doubles without padding: the cloud's doubles ARE its points)
  static_assert(sizeof(Point) == 3 * sizeof(double), "the cloud is appended as Points");
  {
    Marker* m = &out->vision_points;
    const size_t have = m->points.size();
    if (have < n_cloud) {
      m->points.resize(n_cloud);
      std::memcpy(static_cast<void*>(m->points.data() + have), cloud_.data() + 3 * have, (n_cloud - have) * sizeof(Point));
      m->colors.resize(n_cloud, slam_visualization::StdColor(slam_visualization::CloudColor()));
    }
  }
  return true;
}

void Frontend::set_projections(const float left[12], const float right[12]) {
  if (!left || !right || !nodes_.empty() || pending_count_ > 0) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  std::memcpy(config_.projection_left, left, sizeof(config_.projection_left));
  std::memcpy(config_.projection_right, right, sizeof(config_.projection_right));
}

void Frontend::set_visualization(bool on) {
  // (before the first ObserveImage, like set_debug_images: the cloud and the nodes must start together)
  if (!nodes_.empty() || pending_count_ > 0) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  config_.visualization_ = on;
  if (ctx_) {
    float cam_to_robot[12];
    CamToRobot(config_, cam_to_robot);
    last_status_ = vsf_observe_set_world_points(ctx_, on ? 1 : 0, cam_to_robot);
    // (a group's member: the switch is the queue's, the matrix its stream's own)
    if (group_ && last_status_ == VSF_OK) last_status_ = vsf_observe_set_stream_cam_to_robot(ctx_, stream_, cam_to_robot);
  }
}

void Frontend::set_left_cam_to_robot(const float m[12]) {
  if (!nodes_.empty() || pending_count_ > 0) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  config_.left_cam_to_robot = AffineFromRowMajor(m);
  if (ctx_ && group_) last_status_ = vsf_observe_set_stream_cam_to_robot(ctx_, stream_, m);
  if (ctx_ && !group_ && config_.visualization_) last_status_ = vsf_observe_set_world_points(ctx_, 1, m);
}

bool Frontend::Flush() {
  if (group_) return group_->Flush();  // (tickets leave in the order they were issued, whichever member they belong to)
  while (pending_count_ > 0)
    if (!RetireOldest()) return false;
  return true;
}

// The second half of ObserveImageFused for the oldest frame in flight: wait for its result, decode it, and do the
// reference's bookkeeping (cc:424-470) with the odometry that frame's call saw.
bool Frontend::RetireOldest() {
  const PendingFrame pf = pending_[pending_head_];
  pending_head_ = (pending_head_ + 1) % pending_.size();
  pending_count_--;
  size_t bytes = 0;
  const uint8_t* b = nullptr;  // the result, read where the GPU wrote it (the context's pinned result ring)
  last_status_ = vsf_observe_collect_view(ctx_, pf.ticket, &b, &bytes);
  // A compressed frame whose file the DEVICE refused (header word 13) is still a frame: it was extracted as an all-zero image
  // and is booked like any other -- a node without features -- so that the queue's window and frame_list_ stay in step;
  // refused_frames() counts it; last_status() keeps the VSF_ERR_INVALID_ARG of its collect until the next call's status.
  const bool refused = last_status_ == VSF_ERR_INVALID_ARG && b && bytes >= 64 && reinterpret_cast<const uint32_t*>(b)[13] != 0;
  if (last_status_ != VSF_OK && !refused) return false;
  if (refused) refused_frames_++;
  uint32_t hdr[16];
  std::memcpy(hdr, b, sizeof(hdr));
  const int n_pairs = (int)hdr[1], nfeat = (int)hdr[2];
  std::memcpy(&stereo_ambig_constraint_, &hdr[10], sizeof(float));  // the static's value after this frame (cc:392-394)
  if (n_pairs != (int)frame_list_.size() + 1) {  // the context's window and frame_list_ went out of step
    last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  std::vector<uint32_t> npairs((size_t)n_pairs);
  std::memcpy(npairs.data(), b + 64, (size_t)n_pairs * 4);
  size_t off = 64 + 4 * (size_t)((n_pairs + 3) & ~3);
  const uint8_t* feat_bytes = b + off;
  off += (size_t)nfeat * sizeof(vsf_vision_feature);
  std::vector<const uint8_t*> pair_bytes((size_t)n_pairs);
  for (int p = 0; p < n_pairs; p++) {
    pair_bytes[p] = b + off;
    off += (size_t)npairs[p] * sizeof(vsf_feature_match);
  }
  Frame curr_frame;  // Frame(kps, desc, curr_frame_ID_), built in place (cc:511-519)
  curr_frame.frame_ID_ = curr_frame_ID_;
  curr_frame.keypoints_.resize((size_t)nfeat);
  curr_frame.descriptors_.resize((size_t)nfeat * VSF_DESC_BYTES);
  if (nfeat > 0) {
    std::memcpy(curr_frame.keypoints_.data(), b + off, (size_t)nfeat * sizeof(vsf_keypoint));
    std::memcpy(curr_frame.descriptors_.data(), b + off + (size_t)nfeat * sizeof(vsf_keypoint), curr_frame.descriptors_.size());
  }
  curr_frame.is_initial_.assign((size_t)nfeat, true);
  curr_frame.initial_ids_.assign((size_t)nfeat, -1);
  auto book = [](const Frame& past_frame, Frame* curr, const uint8_t* bytes, uint32_t n, std::vector<FeatureMatch>* pairs) {
    if (pairs) pairs->reserve(n);
    for (uint32_t k = 0; k < n; k++) {  // cc:294-306
      vsf_feature_match m;
      std::memcpy(&m, bytes + (size_t)k * sizeof(m), sizeof(m));
      if (pairs) pairs->push_back(FeatureMatch(m.feature_idx_initial, m.feature_idx_current));
      if (m.feature_idx_current < curr->is_initial_.size() && curr->is_initial_[m.feature_idx_current]) {
        curr->is_initial_[m.feature_idx_current] = false;
        curr->initial_ids_[m.feature_idx_current] =
            m.feature_idx_initial < past_frame.is_initial_.size() && !past_frame.is_initial_[m.feature_idx_initial]
                ? past_frame.initial_ids_[m.feature_idx_initial]
                : (int64_t)past_frame.frame_ID_;
      }
    }
  };
  const size_t first_vision_factor = vision_factors_.size();
  for (int p = 0; p + 1 < n_pairs; p++) {  // the temporal loop, cc:424-434
    std::vector<FeatureMatch> pairs;
    book(frame_list_[p], &curr_frame, pair_bytes[p], npairs[p], &pairs);
    vision_factors_.emplace_back(frame_list_[p].frame_ID_, curr_frame.frame_ID_, std::move(pairs));
  }
  {  // Calculate3DPoints' GetFeatureMatches(right, left) (cc:131): every row of the right frame is still `initial`
    Frame right_temp_frame;
    right_temp_frame.frame_ID_ = curr_frame_ID_;
    book(right_temp_frame, &curr_frame, pair_bytes[n_pairs - 1], npairs[n_pairs - 1], nullptr);
  }
  if (config_.debug_images_ && debug_file_form() != kFormRaw) {
    // encoded in the batch's tail (vsf_observe_set_debug_jpeg / vsf_observe_set_debug_png)
    const uint8_t *stereo = nullptr, *match = nullptr;
    size_t stereo_bytes = 0, match_bytes = 0;
    const vsf_status ds = (debug_file_form() & kFormPng)
                              ? vsf_observe_debug_png_view(ctx_, pf.ticket, &stereo, &stereo_bytes, &match, &match_bytes)
                              : vsf_observe_debug_jpeg_view(ctx_, pf.ticket, &stereo, &stereo_bytes, &match, &match_bytes);
    if (ds != VSF_OK) {
      last_status_ = ds;
      return false;
    }
    if (stereo) debug_stereo_files_.emplace_back(stereo, stereo + stereo_bytes);
    if (match) debug_files_.emplace_back(match, match + match_bytes);
  } else if (config_.debug_images_) {  // drawn in the batch's tail (vsf_observe_set_debug_images); kept, as the reference keeps them
    const uint8_t *stereo = nullptr, *match = nullptr;
    const vsf_status ds = vsf_observe_debug_view(ctx_, pf.ticket, &stereo, &match);
    if (ds != VSF_OK) {
      last_status_ = ds;
      return false;
    }
    vsf_params p;
    vsf_get_params(ctx_, &p);
    if (stereo) debug_stereo_images_.push_back(OwnedImage{std::vector<uint8_t>(stereo, stereo + (size_t)6 * p.width * p.height),
                                                          p.height, 2 * p.width});
    if (match) debug_images_.push_back(OwnedImage{std::vector<uint8_t>(match, match + (size_t)3 * p.width * p.height),
                                                  p.height, p.width});
  }
  std::vector<VisionFeature> features;
  features.reserve((size_t)nfeat);
  for (int i = 0; i < nfeat; i++) {  // cc:438-443, computed on the device
    vsf_vision_feature f;
    std::memcpy(&f, feat_bytes + (size_t)i * sizeof(f), sizeof(f));
    features.push_back(VisionFeature((uint64_t)f.feature_idx_lo | ((uint64_t)f.feature_idx_hi << 32),
                                     Vector2f(f.pixel[0], f.pixel[1]), Vector3f(f.point3d[0], f.point3d[1], f.point3d[2])));
  }
  // cc:444-470 with the odometry of this frame's call
  const Vector3f loc = init_odom_rotation_.inverse() * (pf.odom_translation - init_odom_translation_);
  const Quaternionf angle = pf.odom_rotation * init_odom_rotation_.inverse();
  nodes_.emplace_back(curr_frame_ID_, pf.odom_timestamp, RobotPose(loc, angle), std::move(features));
  if (curr_frame_ID_ > 0) {  // AddOdometryFactor, cc:311-321
    const Vector3f translation = pf.prev_odom_rotation.inverse() * (pf.odom_translation - pf.prev_odom_translation);
    const Quaternionf rotation(pf.odom_rotation * pf.prev_odom_rotation.inverse());
    odometry_factors_.push_back(OdometryFactor(curr_frame_ID_ - 1, curr_frame_ID_, translation, rotation));
  }
  if (config_.visualization_) {  // the node's points, made in the batch's tail (vsf_observe_set_world_points)
    const double* xyz = nullptr;
    int32_t n_points = 0;
    const vsf_status vs = vsf_observe_world_points_view(ctx_, pf.ticket, &xyz, &n_points);
    if (vs != VSF_OK) {
      last_status_ = vs;
      return false;
    }
    BookVisualization(first_vision_factor, xyz, n_points);
  }
  curr_frame_ID_++;
  if (frame_list_.size() >= config_.frame_life_ && !frame_list_.empty()) frame_list_.erase(frame_list_.begin());
  frame_list_.push_back(std::move(curr_frame));
  return true;
}

// cc:444-470: node, odometry factor, sliding window.
void Frontend::FinishNode(const Frame& curr_frame, const std::vector<VisionFeature>& features) {
  const Vector3f loc = init_odom_rotation_.inverse() * (odom_translation_ - init_odom_translation_);
  const Quaternionf angle = odom_rotation_ * init_odom_rotation_.inverse();
  nodes_.push_back(SLAMNode(curr_frame_ID_, odom_timestamp_, RobotPose(loc, angle), features));
  if (curr_frame_ID_ > 0) AddOdometryFactor();
  prev_odom_rotation_ = odom_rotation_;
  prev_odom_translation_ = odom_translation_;
  curr_frame_ID_++;
  if (frame_list_.size() >= config_.frame_life_ && !frame_list_.empty()) frame_list_.erase(frame_list_.begin());
  frame_list_.push_back(curr_frame);
}

// The size of the context a configuration asks for: the resized size where a resize is set, else the camera's.
int ContextWidth(const FrontendConfig& c) { return c.resize_width_ > 0 && c.resize_height_ > 0 ? c.resize_width_ : c.image_width; }
int ContextHeight(const FrontendConfig& c) { return c.resize_width_ > 0 && c.resize_height_ > 0 ? c.resize_height_ : c.image_height; }

// The denominators the library takes are stated in the library: vsf_reduced_size refuses every other one.
static bool ReduceOk(int reduce) {
  int w = 0, h = 0;
  return vsf_reduced_size(1, 1, reduce, &w, &h) == VSF_OK;
}

// slam_frontend_main.cc:98-133 + cc:400-472: the payloads of the two sensor_msgs::CompressedImage messages as they came.
bool Frontend::ObserveCompressedImage(const uint8_t* left, size_t left_bytes, const uint8_t* right, size_t right_bytes,
                                      bool bayer_rggb8, double /*time*/) {
  if (!OdomCheck()) return false;  // (a gated frame is not even parsed)
  if (!fused_ || config_.descriptor_extract_type_ != FrontendConfig::DescriptorExtractorType::ORB ||
      config_.orb_nfeatures + 256 >= 65536 || config_.frame_life_ < 1 || config_.frame_life_ + 1 > 64) {
    last_status_ = VSF_ERR_UNSUPPORTED;  // compressed frames exist in the queue only
    return false;
  }
  const int reduce = config_.imdecode_reduce_;
  if (!ReduceOk(reduce) || (bayer_rggb8 && reduce > 1)) {
    last_status_ = VSF_ERR_INVALID_ARG;  // (a mosaic cannot be reduced in the DCT domain: nothing is booked)
    return false;
  }
  int width = 0, height = 0;
  if (resizing()) {  // every file states its own size; the context's is config.resize_width_ x resize_height_
    last_status_ = reduce > 1 || !left || !right ? VSF_ERR_INVALID_ARG : vsf_compressed_image_size(left, left_bytes, &width, &height);
    if (last_status_ != VSF_OK) return false;  // (a reduced decode and a resize are not combined)
  } else if (ctx_) {
    vsf_params p;
    vsf_get_params(ctx_, &p);
    width = p.width;
    height = p.height;
  } else {  // the first frame sizes the context, as the first ObserveImage does: by what imdecode would return for it
    last_status_ = left && right ? vsf_compressed_image_size(left, left_bytes, &width, &height) : VSF_ERR_INVALID_ARG;
    if (last_status_ == VSF_OK) last_status_ = vsf_reduced_size(width, height, reduce, &width, &height);
    if (last_status_ != VSF_OK) return false;
  }
  FramePayload fp;
  fp.reduce = reduce;
  fp.left = left;
  fp.right = right;
  fp.left_bytes = left_bytes;
  fp.right_bytes = right_bytes;
  fp.compressed = true;
  fp.bayer = bayer_rggb8;
  return ObserveFused(width, height, fp);
}

bool Frontend::ObserveDeviceImage(const void* left, size_t left_pitch, const void* right, size_t right_pitch, void* hip_stream,
                                  double time, bool bayer_rggb8) {
  return ObserveDeviceImage(left, left_pitch, right, right_pitch, hip_stream, time,
                            bayer_rggb8 ? (int)VSF_PIX_BAYER_RGGB8 : (int)VSF_PIX_MONO8);
}

// cc:400-472 for a frame that is in device memory already.
bool Frontend::ObserveDeviceImage(const void* left, size_t left_pitch, const void* right, size_t right_pitch, void* hip_stream,
                                  double /*time*/, int pixfmt) {
  if (!OdomCheck()) return false;
  if (!fused_ || config_.descriptor_extract_type_ != FrontendConfig::DescriptorExtractorType::ORB ||
      config_.orb_nfeatures + 256 >= 65536 || config_.frame_life_ < 1 || config_.frame_life_ + 1 > 64) {
    last_status_ = VSF_ERR_UNSUPPORTED;  // device frames exist in the queue only
    return false;
  }
  int width = config_.image_width, height = config_.image_height;
  if (ctx_ && !resizing()) {  // (with a resize the configuration states the camera's size, the context has the resized one)
    vsf_params p;
    vsf_get_params(ctx_, &p);
    width = p.width;
    height = p.height;
  }
  if (!left || !right || width < 1 || height < 1) {  // (a pointer says nothing about a size: the configuration must)
    last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  FramePayload fp;
  fp.left = static_cast<const uint8_t*>(left);
  fp.right = static_cast<const uint8_t*>(right);
  fp.left_bytes = left_pitch;
  fp.right_bytes = right_pitch;
  fp.device = true;
  fp.pixfmt = pixfmt;
  fp.hip_stream = hip_stream;
  return ObserveFused(width, height, fp);
}

// A raw frame of any pixel format: the queue takes it as it is; per-call mode makes the two gray images first.
bool Frontend::ObserveImage(const Image& left_image, const Image& right_image, double time, int pixfmt) {
  if (pixfmt == VSF_PIX_MONO8) return ObserveImage(left_image, right_image, time);
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (bpp == 0 || left_image.empty() || right_image.empty() || left_image.cols != right_image.cols ||
      left_image.rows != right_image.rows || left_image.step != right_image.step ||
      left_image.step < (size_t)left_image.cols * (size_t)bpp) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  if (fused_ && config_.descriptor_extract_type_ == FrontendConfig::DescriptorExtractorType::ORB &&
      config_.orb_nfeatures + 256 < 65536 && config_.frame_life_ >= 1 && config_.frame_life_ + 1 <= 64) {
    if (!OdomCheck()) return false;
    return ObserveImageFused(left_image, right_image, pixfmt);
  }
  // per-call mode: both images to gray (vsf_to_gray: the queue's kernels, host to host), then the frame as ever -- the
  // odometry gate is asked inside, once
  const int w = left_image.cols, h = left_image.rows;
  if (!EnsureContext(resizing() ? config_.resize_width_ : w, resizing() ? config_.resize_height_ : h)) {
    if (last_status_ == VSF_OK) last_status_ = VSF_ERR_INVALID_ARG;
    return false;
  }
  const Image* in[2] = {&left_image, &right_image};
  for (int k = 0; k < 2; k++) {
    gray_[k].resize((size_t)w * h);
    last_status_ = vsf_to_gray(ctx_, in[k]->data, 1, w, h, pixfmt, 0, in[k]->step, gray_[k].data(), 0, (size_t)w);
    if (last_status_ != VSF_OK) return false;
  }
  return ObserveImage(Image(gray_[0].data(), h, w, (size_t)w), Image(gray_[1].data(), h, w, (size_t)w), time);
}

// cc:400-472
bool Frontend::ObserveImage(const Image& left_image, const Image& right_image, double /*time*/) {
  if (!OdomCheck()) return false;
  if (fused_ && config_.descriptor_extract_type_ == FrontendConfig::DescriptorExtractorType::ORB && !left_image.empty() &&
      !right_image.empty() && left_image.cols == right_image.cols && left_image.rows == right_image.rows &&
      left_image.step == right_image.step && config_.orb_nfeatures + 256 < 65536 && config_.frame_life_ >= 1 &&
      config_.frame_life_ + 1 <= 64)
    return ObserveImageFused(left_image, right_image);
  if (resizing() && !left_image.empty() && !right_image.empty() &&
      (left_image.cols != config_.resize_width_ || left_image.rows != config_.resize_height_)) {
    // per-call mode: cv::resize of both images first (vsf_resize_gray: the queue's kernel, host to host), then the frame as ever
    const int w = config_.resize_width_, h = config_.resize_height_;
    if (left_image.cols != right_image.cols || left_image.rows != right_image.rows || !EnsureContext(w, h)) {
      if (last_status_ == VSF_OK) last_status_ = VSF_ERR_INVALID_ARG;
      return false;
    }
    const Image* in[2] = {&left_image, &right_image};
    for (int k = 0; k < 2; k++) {
      resized_[k].resize((size_t)w * h);
      last_status_ = vsf_resize_gray(ctx_, in[k]->data, 1, in[k]->cols, in[k]->rows, 0, in[k]->step, resized_[k].data(), w, h, 0, (size_t)w);
      if (last_status_ != VSF_OK) return false;
    }
    // (the odometry gate above is asked again inside and answers the same: nothing it reads has changed)
    return ObserveImage(Image(resized_[0].data(), h, w, (size_t)w), Image(resized_[1].data(), h, w, (size_t)w), 0.0);
  }
  Frame curr_frame, right_temp_frame;
  if (!ExtractFeaturesPair(left_image, right_image, &curr_frame, &right_temp_frame)) return false;
  const std::vector<vsf_dmatch> stereo_matches = GetMatches(curr_frame, right_temp_frame, config_.nn_match_ratio_);
  RemoveAmbigStereo(&curr_frame, &right_temp_frame, stereo_matches);
  const size_t first_vision_factor = vision_factors_.size();
  GetFeatureMatchesAll(&frame_list_, &curr_frame, &vision_factors_);
  std::vector<Vector3f> points;
  VisionFactor stereo;
  Calculate3DPoints(&curr_frame, &right_temp_frame, &points, &stereo);
  if (config_.debug_images_) {
    const bool match_image = !frame_list_.empty() && !vision_factors_.empty();  // cc:458-466
    DrawDebugImages(left_image.data, right_image.data, left_image.cols, left_image.rows, left_image.step, curr_frame,
                    right_temp_frame.keypoints_, stereo.feature_matches.empty() ? nullptr : &stereo.feature_matches,
                    match_image ? &frame_list_.back() : nullptr,
                    match_image ? &vision_factors_.back().feature_matches : nullptr);
    if (last_status_ != VSF_OK) return false;
  }
  std::vector<VisionFeature> features;
  for (uint64_t i = 0; i < curr_frame.keypoints_.size(); i++) {
    // The reference indexes points[i] by keypoint although `points` is in sorted-match order and may be shorter
    // (quirk Q5, out-of-range read); the same index is used where it exists, a zero point otherwise.
    const Vector3f p3 = i < points.size() ? points[i] : Vector3f();
    features.push_back(VisionFeature(i, Vector2f(curr_frame.keypoints_[i].x, curr_frame.keypoints_[i].y), p3));
  }
  UndistortFeaturePoints(&features);
  FinishNode(curr_frame, features);
  if (config_.visualization_) {  // the node's points: one vsf_world_points call (the kernel the queue's batches run)
    const SLAMNode& node = nodes_.back();
    std::vector<vsf_vision_feature> records(features.size());
    for (size_t i = 0; i < features.size(); i++) {
      const VisionFeature& f = features[i];
      records[i] = {(uint32_t)f.feature_idx, (uint32_t)(f.feature_idx >> 32), {f.pixel.x(), f.pixel.y()},
                    {f.point3d.x(), f.point3d.y(), f.point3d.z()}};
    }
    const vsf_pose pose = {{node.pose.loc.x(), node.pose.loc.y(), node.pose.loc.z()},
                           {node.pose.angle.x(), node.pose.angle.y(), node.pose.angle.z(), node.pose.angle.w()}};
    float cam_to_robot[12];
    CamToRobot(config_, cam_to_robot);
    std::vector<double> xyz(3 * records.size());
    int n_points = 0;
    last_status_ = vsf_world_points(ctx_, records.data(), (int)records.size(), &pose, cam_to_robot, xyz.data(), (int)records.size(),
                                    &n_points);
    if (last_status_ != VSF_OK) return false;
    BookVisualization(first_vision_factor, xyz.data(), n_points);
  }
  return true;
}

void Frontend::GetSLAMProblem(SLAMProblem* problem) const {
  Sync();  // (pipelined mode: frames still on the GPU are booked first)
  *problem = SLAMProblem(nodes_, vision_factors_, odometry_factors_);
}

int Frontend::GetNumPoses() {
  Flush();
  return (int)nodes_.size();
}

void Frontend::set_debug_images(bool on) {
  // (before the first ObserveImage: the queue's window and frame_list_ must start together)
  if (!nodes_.empty() || pending_count_ > 0) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  config_.debug_images_ = on;
  if (ctx_) last_status_ = vsf_observe_set_debug_images(ctx_, on ? 1 : 0);
}

void Frontend::set_debug_colour_seed(bool seeded, uint32_t seed) {
  if (!nodes_.empty() || pending_count_ > 0 || group_) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  config_.debug_colour_seeded_ = seeded;
  config_.debug_colour_seed_ = seed;
  vsfrand::seed(colour_rng_, seed);
  if (ctx_) last_status_ = ApplyDebugConfig(1);
}

void Frontend::set_debug_jpeg_quality(int quality) {
  if (!nodes_.empty() || pending_count_ > 0 || quality < 0 || quality > 100 || (quality > 0 && (debug_file_form() & kFormPng))) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  config_.debug_jpeg_quality_ = quality;
  if (ctx_ && (config_.debug_images_ || quality == 0)) last_status_ = vsf_observe_set_debug_jpeg(ctx_, quality);
}

void Frontend::set_resize(int width, int height, int camera_width, int camera_height) {
  const bool off = width == 0 && height == 0;
  last_status_ = off || (width >= 1 && height >= 1 && width <= 32767 && height <= 32767) ? VSF_OK : VSF_ERR_INVALID_ARG;
  if (last_status_ != VSF_OK) return;
  config_.resize_width_ = width;
  config_.resize_height_ = height;
  if (camera_width > 0 && camera_height > 0) {
    config_.image_width = camera_width;
    config_.image_height = camera_height;
  }
}

void Frontend::set_bayer_order(int pixfmt) {
  const bool ok = pixfmt == VSF_PIX_BAYER_RGGB8 || pixfmt == VSF_PIX_BAYER_GRBG8 || pixfmt == VSF_PIX_BAYER_GBRG8 ||
                  pixfmt == VSF_PIX_BAYER_BGGR8;
  last_status_ = ok ? VSF_OK : VSF_ERR_INVALID_ARG;
  if (ok) config_.bayer_order_ = pixfmt;
}

void Frontend::set_imdecode_reduce(int reduce) {
  last_status_ = ReduceOk(reduce) ? VSF_OK : VSF_ERR_INVALID_ARG;
  if (last_status_ == VSF_OK) config_.imdecode_reduce_ = reduce;
}

void Frontend::set_compressed_cap(size_t cap_per_image) {
  if (group_) return group_->set_compressed_cap(cap_per_image);
  config_.compressed_cap_ = cap_per_image;
  // (a context that exists takes it now -- the queue must be empty, or not have seen a compressed frame yet; one that does not
  // takes it when it is created)
  last_status_ = ctx_ ? vsf_observe_set_compressed_cap(ctx_, cap_per_image) : VSF_OK;
}

void Frontend::set_debug_png(bool on) {
  if (!nodes_.empty() || pending_count_ > 0 || (on && (debug_file_form() & kFormJpeg))) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  config_.debug_png_ = on;
  if (ctx_ && (config_.debug_images_ || !on)) last_status_ = vsf_observe_set_debug_png(ctx_, on ? 1 : 0);
}

Frontend::CompressedView Frontend::GetLastDebugImageCompressed() {
  Flush();
  CompressedView v;
  if (!debug_files_.empty())
    v.data = debug_files_.back().data(), v.size = debug_files_.back().size(), v.format = debug_file_format();
  return v;
}

Frontend::CompressedView Frontend::GetLastDebugStereoImageCompressed() {
  Flush();
  CompressedView v;
  if (!debug_stereo_files_.empty())
    v.data = debug_stereo_files_.back().data(), v.size = debug_stereo_files_.back().size(),
    v.format = debug_file_format();
  return v;
}

std::vector<Image> Frontend::getDebugImages() {
  Flush();
  std::vector<Image> out;
  for (const OwnedImage& im : debug_images_) out.push_back(im.view());
  return out;
}

std::vector<Image> Frontend::getDebugStereoImages() {
  Flush();
  std::vector<Image> out;
  for (const OwnedImage& im : debug_stereo_images_) out.push_back(im.view());
  return out;
}

Image Frontend::GetLastDebugImage() {
  Flush();
  return debug_images_.empty() ? Image() : debug_images_.back().view();
}

Image Frontend::GetLastDebugStereoImage() {
  Flush();
  return debug_stereo_images_.empty() ? Image() : debug_stereo_images_.back().view();
}

namespace {
int CvRound(float v) { return (int)std::lrint(v); }  // cvRound: round half to even (the default rounding mode)
}  // namespace

// cc:74-115.  Points are cvRound(Point2f) as cv::circle / cv::line take them (cv::Point), the stereo image's right points
// after adding the left image's width to the float x (cc:90).  The line colours are the reference's expression,
// cv::Scalar(rand() % 255, rand() % 255, rand() % 255), one stereo match after the other, frame by frame -- the process's
// own rand() stream, called in the reference's order.  The order in which those three calls run is unspecified in C++; GCC
// evaluates the arguments of that constructor call right to left, so the FIRST draw is channel 2 (the byte the driver
// labels R), the third is channel 0.  This choice follows the reference's usual build and is not pinned by a test against
// it.  With config_.debug_colour_seeded_ the three draws come from the object's own generator instead -- the same statement of
// glibc's rand() the queue's colour kernel runs (csrc/vsf_glibc_random.h).
void Frontend::DrawDebugImages(const uint8_t* left, const uint8_t* right, int w, int h, size_t pitch,
                               const Frame& curr_frame, const std::vector<vsf_keypoint>& right_keypoints,
                               const std::vector<FeatureMatch>* stereo, const Frame* past_frame,
                               const std::vector<FeatureMatch>* temporal) {
  std::vector<vsf_draw_op> ops;
  std::vector<vsf_draw_canvas> canvases;
  auto circle = [&](int x, int y, const uint8_t bgr[3]) {
    vsf_draw_op op = {VSF_DRAW_CIRCLE, x, y, 5, 0, {bgr[0], bgr[1], bgr[2], 0}};
    ops.push_back(op);
  };
  auto line = [&](int x0, int y0, int x1, int y1, const uint8_t bgr[3]) {
    vsf_draw_op op = {VSF_DRAW_LINE, x0, y0, x1, y1, {bgr[0], bgr[1], bgr[2], 0}};
    ops.push_back(op);
  };
  const uint8_t red[3] = {0, 0, 255}, green[3] = {0, 255, 0};  // CV_RGB(255, 0, 0), CV_RGB(0, 255, 0)
  const std::vector<vsf_keypoint>& lk = curr_frame.keypoints_;
  OwnedImage stereo_image, match_image;
  if (stereo) {  // CreateStereoDebugImage
    vsf_draw_canvas c = {left, right, w, h, (int64_t)pitch, nullptr, (int64_t)6 * w, (int32_t)ops.size(), 0};
    for (const FeatureMatch& m : *stereo) {
      uint8_t bgr[3];  // (drawn for every pair, as cc:95 does: the colours keep the reference's sequence)
      if (config_.debug_colour_seeded_) {
        const uint32_t c = vsfrand::next_colour(colour_rng_);
        bgr[0] = (uint8_t)c, bgr[1] = (uint8_t)(c >> 8), bgr[2] = (uint8_t)(c >> 16);
      } else {
        bgr[2] = (uint8_t)(rand() % 255);
        bgr[1] = (uint8_t)(rand() % 255);
        bgr[0] = (uint8_t)(rand() % 255);
      }
      if (m.feature_idx_current >= lk.size() || m.feature_idx_initial >= right_keypoints.size()) continue;
      const vsf_keypoint& l = lk[m.feature_idx_current];
      const vsf_keypoint& r = right_keypoints[m.feature_idx_initial];
      const int lx = CvRound(l.x), ly = CvRound(l.y), rx = CvRound(r.x + (float)w), ry = CvRound(r.y);
      circle(lx, ly, red);
      circle(rx, ry, red);
      line(lx, ly, rx, ry, bgr);
    }
    c.op_count = (int32_t)ops.size() - c.op_begin;
    stereo_image.rows = h;
    stereo_image.cols = 2 * w;
    stereo_image.data.resize((size_t)6 * w * h);
    c.out = stereo_image.data.data();
    canvases.push_back(c);
  }
  if (past_frame && temporal) {  // CreateMatchDebugImage
    vsf_draw_canvas c = {left, nullptr, w, h, (int64_t)pitch, nullptr, (int64_t)3 * w, (int32_t)ops.size(), 0};
    const std::vector<vsf_keypoint>& pk = past_frame->keypoints_;
    for (const FeatureMatch& m : *temporal) {
      if (m.feature_idx_initial >= pk.size() || m.feature_idx_current >= lk.size()) continue;
      const vsf_keypoint& a = pk[m.feature_idx_initial];
      const vsf_keypoint& b = lk[m.feature_idx_current];
      circle(CvRound(a.x), CvRound(a.y), red);
      line(CvRound(a.x), CvRound(a.y), CvRound(b.x), CvRound(b.y), green);
    }
    c.op_count = (int32_t)ops.size() - c.op_begin;
    match_image.rows = h;
    match_image.cols = w;
    match_image.data.resize((size_t)3 * w * h);
    c.out = match_image.data.data();
    canvases.push_back(c);
  }
  if (canvases.empty()) return;
  last_status_ = vsf_draw_canvases(ctx_, canvases.data(), (int)canvases.size(), ops.data(), (int)ops.size());
  if (last_status_ != VSF_OK) return;
  if (stereo) debug_stereo_images_.push_back(std::move(stereo_image));
  if (past_frame && temporal) debug_images_.push_back(std::move(match_image));
}

}  // namespace slam

// ---- FrontendGroup ----
namespace slam {

FrontendGroup::FrontendGroup(const std::vector<FrontendConfig>& configs, int device) {
  if (configs.empty() || configs.size() > (size_t)VSF_OBSERVE_MAX_STREAMS) {
    last_status_ = VSF_ERR_INVALID_ARG;
    return;
  }
  const FrontendConfig& lead = configs[0];
  // debug images of several streams need a colour generator per stream: refused here, not by the context some calls later
  for (const FrontendConfig& c : configs)
    if (configs.size() > 1 && (c.debug_images_ || c.debug_jpeg_quality_ != 0 || c.debug_png_) && !c.debug_colour_seeded_) {
      last_status_ = VSF_ERR_UNSUPPORTED;
      return;
    }
  for (const FrontendConfig& c : configs)  // what the one context is built with
    if (c.orb_nfeatures != lead.orb_nfeatures || c.orb_score_type_ != lead.orb_score_type_ || c.nn_match_ratio_ != lead.nn_match_ratio_ ||
        c.residual_order != lead.residual_order || c.frame_life_ != lead.frame_life_ || ContextWidth(c) != ContextWidth(lead) ||
        ContextHeight(c) != ContextHeight(lead) || c.visualization_ != lead.visualization_ || c.debug_images_ != lead.debug_images_ ||
        c.debug_jpeg_quality_ != lead.debug_jpeg_quality_ || c.debug_png_ != lead.debug_png_ ||
        c.debug_colour_seeded_ != lead.debug_colour_seeded_) {
      last_status_ = VSF_ERR_INVALID_ARG;
      return;
    }
  for (size_t i = 0; i < configs.size(); i++) {
    members_.push_back(new Frontend(configs[i], device, this, (int)i));
    if (last_status_ == VSF_OK) last_status_ = members_.back()->last_status_;
  }
  ready_ = true;
  if (last_status_ == VSF_OK && ContextWidth(lead) > 0 && ContextHeight(lead) > 0) EnsureContext(ContextWidth(lead), ContextHeight(lead));
}

// (frames in flight are dropped, as a Frontend's are; the first member owns the context)
FrontendGroup::~FrontendGroup() {
  for (size_t i = members_.size(); i-- > 0;) delete members_[i];
}

// The queue is the group's: every member holds the same settings (a member's own setters come here).
void FrontendGroup::set_pipelined(bool on) {
  for (Frontend* m : members_) m->pipelined_ = on;
}
void FrontendGroup::set_queue(int depth, int batch_frames, int min_batch) {
  for (Frontend* m : members_) {
    if (depth > 0) m->depth_ = depth > 1024 ? 1024 : depth;
    if (batch_frames > 0) m->batch_frames_ = batch_frames > 256 ? 256 : batch_frames;
    if (min_batch >= 0) m->min_batch_ = min_batch;
  }
}
void FrontendGroup::set_queue_thread(bool on) {
  for (Frontend* m : members_) m->queue_thread_ = on;
}
// (the byte cap is the queue's, and the queue is the group's: one value, whichever member asks for it)
void FrontendGroup::set_compressed_cap(size_t cap_per_image) {
  for (Frontend* m : members_) m->config_.compressed_cap_ = cap_per_image;
  Frontend& lead = *members_[0];
  const vsf_status st = lead.ctx_ ? vsf_observe_set_compressed_cap(lead.ctx_, cap_per_image) : VSF_OK;
  for (Frontend* m : members_) m->last_status_ = st;
}

// (the setters of slam_frontend.h that a group member hands to its group)
void Frontend::set_pipelined(bool on) {
  if (group_) return group_->set_pipelined(on);
  pipelined_ = on;
}
void Frontend::set_queue_depth(int n) {
  if (group_) return group_->set_queue(n < 1 ? 1 : n, 0, -1);
  depth_ = n < 1 ? 1 : (n > 1024 ? 1024 : n);
}
void Frontend::set_batch_frames(int n) {
  if (group_) return group_->set_queue(0, n < 1 ? 1 : n, -1);
  batch_frames_ = n < 1 ? 1 : (n > 256 ? 256 : n);
}
void Frontend::set_min_batch(int n) {
  if (group_) return group_->set_queue(0, 0, n < 0 ? 0 : n);
  min_batch_ = n < 0 ? 0 : n;
}
void Frontend::set_queue_thread(bool on) {
  if (group_) return group_->set_queue_thread(on);
  queue_thread_ = on;
}
void Frontend::set_fused(bool on) {
  if (!group_) fused_ = on;  // (a group's members observe through the queue: fused)
}

// The one context: built (or replaced: another image size, another queue) by the first member with a stream per member,
// then shared.  A replaced context takes every frame in flight with it (booked first, in order, by the member's Flush).
bool FrontendGroup::EnsureContext(int width, int height) {
  if (!ready_) return true;  // (the members are still being constructed: the group's constructor calls again)
  if (members_.empty() || last_status_ != VSF_OK) return false;
  Frontend& lead = *members_[0];
  vsf_ctx* const before = lead.ctx_;
  const int generation = lead.ctx_generation_;
  const bool ok = lead.EnsureOwnContext(width, height, size());
  if (lead.ctx_ != before || lead.ctx_generation_ != generation) {
    order_.clear();
    for (Frontend* m : members_) {
      m->ctx_ = lead.ctx_;
      m->ctx_depth_ = lead.ctx_depth_;
      m->pending_.assign((size_t)(lead.ctx_depth_ > 0 ? lead.ctx_depth_ : 1), Frontend::PendingFrame());
      m->pending_head_ = m->pending_count_ = 0;
      m->declared_w_ = m->declared_h_ = 0;
      m->told_bayer_order_ = 0;
    }
  }
  if (!ok)
    for (Frontend* m : members_) m->last_status_ = lead.last_status_;
  return ok;
}

int64_t FrontendGroup::oldest_ticket() const {
  const Frontend& m = *members_[(size_t)order_.front()];
  return m.pending_[m.pending_head_].ticket;
}

bool FrontendGroup::RetireOldest() {
  if (in_flight() == 0) return true;
  Frontend& m = *members_[(size_t)order_.front()];
  order_.pop_front();
  const bool ok = m.RetireOldest();
  if (!ok) last_status_ = m.last_status_;
  return ok;
}

bool FrontendGroup::Flush() {
  while (in_flight() > 0)
    if (!RetireOldest()) return false;
  return true;
}

}  // namespace slam
