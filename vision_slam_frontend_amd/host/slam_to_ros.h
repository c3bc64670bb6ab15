// slam_to_ros.h -- SURVEY.md section 8(f) row f3: the ROS-1 wire format of the frontend's outputs, as a standalone
// encoder (no ROS here or on the GPU box).  The reference converts slam_types to the generated message structs in
// src/slam_to_ros.h:36-124 and lets roscpp serialise them into the output bag (slam_frontend_main.cc:341-374); the
// bytes below are what that produces for msg/*.msg:
//
//   ROS-1 serialisation: little endian, fields in declaration order, fixed-size primitives raw, a variable-length
//   array T[] as uint32 count + elements, nested messages inline.  geometry_msgs/Point and /Vector3 are three
//   float64 (x, y, z); geometry_msgs/Quaternion is four float64 in the order x, y, z, w.
//
//   FeatureMatch    uint64 id_initial, id_current                                              16 B
//   VisionFeature   uint64 id, Point pixel (z = 0, slam_to_ros.h:49), Point point3d            56 B
//   VisionFactor    uint64 pose_initial, pose_current, FeatureMatch[]                    20 + 16 n B
//   RobotPose       Vector3 loc, Quaternion angle                                              56 B
//   SLAMNode        uint64 id, float64 timestamp, RobotPose, VisionFeature[]             76 + 56 n B
//   OdometryFactor  uint64 pose_i, pose_j, Vector3 translation, Quaternion rotation            72 B
//   SLAMProblem     SLAMNode[], VisionFactor[], OdometryFactor[]
//   CameraIntrinsics  float64 fx, fy, cx, cy (the order of the .msg, not of the struct's assignment)   32 B
//   CameraExtrinsics  float64[3] translation, float64[3] rotation (fixed-size arrays: no count)        48 B
//
// float members widen to float64 exactly as the reference's converters assign them.
//
// The md5sums below are what a bag writer puts into its connection headers beside type=vision_slam_frontend/<Name>:
// computed from the field lists in tools/ros_md5.py by genmsg's rule (the same tool reproduces the known
// md5sums of geometry_msgs/Point, Vector3 and Quaternion); tests/test_ros_md5.py keeps the two in step.
#ifndef VSF_HOST_SLAM_TO_ROS_H_
#define VSF_HOST_SLAM_TO_ROS_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "slam_types.h"
#include "slam_visualization.h"

namespace slam_to_ros {

constexpr const char* kMd5CameraExtrinsics = "c717804541b0303dd7ecf159fee7cb1d";
constexpr const char* kMd5CameraIntrinsics = "5df0bc21162586fd1b49ebbef1d3f4d9";
constexpr const char* kMd5FeatureMatch = "0d28d3a5322605f478774fcde33f4524";
constexpr const char* kMd5OdometryFactor = "970d60bad18953b634b3a66b9842f10f";
constexpr const char* kMd5RobotPose = "8f338562bbd18f0890b5c1878b66b8b5";
constexpr const char* kMd5SLAMNode = "0e51780741a149812c832d6ae619d556";
constexpr const char* kMd5SLAMProblem = "a5ec5d26ada8532dd747269f672dd5f8";
constexpr const char* kMd5VisionFactor = "da3820cf3e135bcd0b601cacc8cf0809";
constexpr const char* kMd5VisionFeature = "9cccef6835ecad8ee3bfb40a17ba67fb";

// sensor_msgs/CompressedImage (another package's message: the debug images as JPEG files, Frontend::GetLastDebugImageCompressed),
// computed by the same tool from ROS-1's field lists (std_msgs/Header header, string format, uint8[] data).
constexpr const char* kCompressedImageMd5 = "8f7a12909da2c9d3332d540a0977563f";

// visualization_msgs/Marker and /MarkerArray (what the driver's PublishVisualization sends to RViz: SerializeMarker /
// SerializeMarkerArray below), by the same tool from ROS-1's field and constant lists (tools/ros_md5.py: EXTERNAL; the Marker
// that has DELETEALL, i.e. Jade and later).  No ROS exists here to confirm them against `rosmsg md5` -- like the ten sums
// above they rest on the tool, which reproduces the sums it knows (geometry_msgs/Point, Vector3, Quaternion, Pose,
// std_msgs/Header, ColorRGBA, sensor_msgs/CompressedImage).
constexpr const char* kMarkerMd5 = "4048c9de2a16f4ae8e0538085ebf1b97";
constexpr const char* kMarkerArrayMd5 = "d155b9ce5188fbaf89745847fd5882d7";

constexpr const char* kCompressedFormatJpeg = "jpeg";
constexpr const char* kCompressedFormatPng = "png";

class Writer {
 public:
  explicit Writer(std::vector<uint8_t>* out) : out_(out) {}
  void u32(uint32_t v) { raw(&v, 4); }
  void u64(uint64_t v) { raw(&v, 8); }
  void f64(double v) { raw(&v, 8); }
  void i32(int32_t v) { raw(&v, 4); }
  void f32(float v) { raw(&v, 4); }
  void u8(uint8_t v) { raw(&v, 1); }
  void str(const std::string& s) {  // string: uint32 length + bytes
    u32((uint32_t)s.size());
    bytes(s.data(), s.size());
  }
  void bytes(const void* p, size_t n) {
    if (n != 0) raw(p, n);
  }

 private:
  void raw(const void* p, size_t n) {  // host is little endian (x86-64), as is the wire
    const uint8_t* b = static_cast<const uint8_t*>(p);
    out_->insert(out_->end(), b, b + n);
  }
  std::vector<uint8_t>* out_;
};

inline void Write(Writer* w, const slam_types::FeatureMatch& m) {  // FeatureMatchToRos, slam_to_ros.h:36-42
  w->u64(m.feature_idx_initial);
  w->u64(m.feature_idx_current);
}

inline void Write(Writer* w, const slam_types::VisionFeature& f) {  // VisionFeatureToRos, :44-58
  w->u64(f.feature_idx);
  w->f64(f.pixel.x());
  w->f64(f.pixel.y());
  w->f64(0.0);
  w->f64(f.point3d.x());
  w->f64(f.point3d.y());
  w->f64(f.point3d.z());
}

inline void Write(Writer* w, const slam_types::RobotPose& p) {  // RobotPoseToRos, :60-71
  w->f64(p.loc.x());
  w->f64(p.loc.y());
  w->f64(p.loc.z());
  w->f64(p.angle.x());
  w->f64(p.angle.y());
  w->f64(p.angle.z());
  w->f64(p.angle.w());
}

inline void Write(Writer* w, const slam_types::SLAMNode& n) {  // SLAMNodeToRos, :73-83
  w->u64(n.node_idx);
  w->f64(n.timestamp);
  Write(w, n.pose);
  w->u32((uint32_t)n.features.size());
  for (const auto& f : n.features) Write(w, f);
}

inline void Write(Writer* w, const slam_types::VisionFactor& c) {  // VisionFactorToRos, :85-94
  w->u64(c.pose_idx_initial);
  w->u64(c.pose_idx_current);
  w->u32((uint32_t)c.feature_matches.size());
  for (const auto& m : c.feature_matches) Write(w, m);
}

inline void Write(Writer* w, const slam_types::OdometryFactor& o) {  // OdometryFactorToRos, :96-109
  w->u64(o.pose_i);
  w->u64(o.pose_j);
  w->f64(o.translation.x());
  w->f64(o.translation.y());
  w->f64(o.translation.z());
  w->f64(o.rotation.x());
  w->f64(o.rotation.y());
  w->f64(o.rotation.z());
  w->f64(o.rotation.w());
}

inline void Write(Writer* w, const slam_types::CameraIntrinsics& k) {  // IntrinsicsToRos, :126-135; CameraIntrinsics.msg
  w->f64(k.fx);
  w->f64(k.fy);
  w->f64(k.cx);
  w->f64(k.cy);
}

inline void Write(Writer* w, const slam_types::CameraExtrinsics& a) {  // ExtrinsicsToRos, :137-146; CameraExtrinsics.msg
  for (int i = 0; i < 3; i++) w->f64(a.translation[i]);
  for (int i = 0; i < 3; i++) w->f64(a.rotation[i]);
}

// slam_frontend_main.cc:341-352: translation + rotation of an affine camera-to-robot transform as scaled angle-axis,
// `AngleAxisf rR(extrinsics.rotation())`: Eigen builds the quaternion of the matrix (Shoemake's branches) and from it
// angle = 2 atan2(|vec|, |w|), axis = vec / (+-|vec|) with the sign of w -- (1, 0, 0) and angle 0 for a zero vector part;
// the message carries axis.normalized() * angle, or zeros when angle <= 1e-8.
// R: row-major 3 x 3 rotation, t: translation.
inline slam_types::CameraExtrinsics ExtrinsicsFromAffine(const float R[9], const float t[3]) {
  auto m = [&](int r, int c) { return R[3 * r + c]; };
  float q[4];  // x y z w
  float tr = m(0, 0) + m(1, 1) + m(2, 2);
  if (tr > 0.f) {
    tr = std::sqrt(tr + 1.0f);
    q[3] = 0.5f * tr;
    tr = 0.5f / tr;
    q[0] = (m(2, 1) - m(1, 2)) * tr;
    q[1] = (m(0, 2) - m(2, 0)) * tr;
    q[2] = (m(1, 0) - m(0, 1)) * tr;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    tr = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0f);
    q[i] = 0.5f * tr;
    tr = 0.5f / tr;
    q[3] = (m(k, j) - m(j, k)) * tr;
    q[j] = (m(j, i) + m(i, j)) * tr;
    q[k] = (m(k, i) + m(i, k)) * tr;
  }
  float n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  float angle = 0.f, axis[3] = {1.f, 0.f, 0.f};
  if (n != 0.f) {
    angle = 2.0f * std::atan2(n, std::fabs(q[3]));
    if (q[3] < 0.f) n = -n;
    for (int i = 0; i < 3; i++) axis[i] = q[i] / n;
  }
  const float an = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  slam_types::CameraExtrinsics a;
  for (int i = 0; i < 3; i++) {
    a.translation[i] = t[i];
    a.rotation[i] = angle > 1e-8 ? (axis[i] / an) * angle : 0.f;
  }
  return a;
}

// The two calibration messages the reference's driver writes beside the problem (topics "extrinsics" and "intrinsics",
// slam_frontend_main.cc:353-365), as payload bytes.
inline void SerializeExtrinsics(const slam_types::CameraExtrinsics& a, std::vector<uint8_t>* out) {
  out->clear();
  Writer w(out);
  Write(&w, a);
}
inline void SerializeIntrinsics(const slam_types::CameraIntrinsics& k, std::vector<uint8_t>* out) {
  out->clear();
  Writer w(out);
  Write(&w, k);
}

// SLAMProblemToRos (:111-124) + roscpp serialisation: the payload of one vision_slam_frontend/SLAMProblem message.
inline void SerializeSLAMProblem(const slam_types::SLAMProblem& p, std::vector<uint8_t>* out) {
  out->clear();
  Writer w(out);
  w.u32((uint32_t)p.nodes.size());
  for (const auto& n : p.nodes) Write(&w, n);
  w.u32((uint32_t)p.vision_factors.size());
  for (const auto& c : p.vision_factors) Write(&w, c);
  w.u32((uint32_t)p.odometry_factors.size());
  for (const auto& o : p.odometry_factors) Write(&w, o);
}

// One sensor_msgs/CompressedImage with format "jpeg" (what image_transport's compressed publisher sends for a JPEG file); pass
// kCompressedFormatPng (Frontend::CompressedView::format says which) for a PNG file, image_transport's lossless setting:
//   Header   uint32 seq, time stamp (uint32 secs, uint32 nsecs), string frame_id (uint32 length + bytes)
//   string format, uint8[] data (uint32 length + bytes)                                  24 + |frame_id| + |format| + n B
inline void SerializeCompressedImage(uint32_t seq, uint32_t stamp_secs, uint32_t stamp_nsecs, const std::string& frame_id,
                                     const uint8_t* file, size_t file_bytes, std::vector<uint8_t>* out,
                                     const std::string& format = "jpeg") {
  out->clear();
  out->reserve(24 + frame_id.size() + format.size() + file_bytes);
  Writer w(out);
  w.u32(seq);
  w.u32(stamp_secs);
  w.u32(stamp_nsecs);
  w.u32((uint32_t)frame_id.size());
  out->insert(out->end(), frame_id.begin(), frame_id.end());
  w.u32((uint32_t)format.size());
  out->insert(out->end(), format.begin(), format.end());
  w.u32((uint32_t)file_bytes);
  out->insert(out->end(), file, file + file_bytes);
}

// The way back (a subscriber's view of the payload): false when the payload is not one whole message.
struct CompressedImageView {
  uint32_t seq = 0, stamp_secs = 0, stamp_nsecs = 0;
  std::string frame_id, format;
  const uint8_t* data = nullptr;
  size_t size = 0;
};
inline bool ParseCompressedImage(const uint8_t* msg, size_t n, CompressedImageView* v) {
  size_t p = 0;
  auto u32 = [&](uint32_t* x) {
    if (n - p < 4) return false;
    std::memcpy(x, msg + p, 4);
    p += 4;
    return true;
  };
  auto str = [&](std::string* s) {
    uint32_t len;
    if (!u32(&len) || n - p < len) return false;
    s->assign(reinterpret_cast<const char*>(msg + p), len);
    p += len;
    return true;
  };
  uint32_t len;
  if (!u32(&v->seq) || !u32(&v->stamp_secs) || !u32(&v->stamp_nsecs) || !str(&v->frame_id) || !str(&v->format) || !u32(&len) ||
      n - p != len)
    return false;
  v->data = msg + p;
  v->size = len;
  return true;
}

// One visualization_msgs/Marker in ROS-1 wire format:
//   Header (uint32 seq, time stamp, string frame_id), string ns, int32 id, type, action, Pose (Point + Quaternion: 7 float64),
//   Vector3 scale, ColorRGBA color (4 float32), duration lifetime (2 int32), bool frame_locked (1 byte), Point[] points,
//   ColorRGBA[] colors, string text, string mesh_resource, bool mesh_use_embedded_materials
//                                   154 + |frame_id| + |ns| + 24 points + 16 colors + |text| + |mesh_resource| B
// The points array -- the cloud: the one part that grows -- is written with ONE memcpy (slam_visualization.h: Point is three
// float64 without padding, the host is little endian as the wire is); the colours likewise.
inline size_t SerializedSize(const slam_visualization::Marker& m) {
  return 154 + m.header.frame_id.size() + m.ns.size() + 24 * m.points.size() + 16 * m.colors.size() + m.text.size() +
         m.mesh_resource.size();
}
inline void Write(Writer* w, const slam_visualization::Marker& m) {
  w->u32(m.header.seq);
  w->u32(m.header.stamp_secs);
  w->u32(m.header.stamp_nsecs);
  w->str(m.header.frame_id);
  w->str(m.ns);
  w->i32(m.id);
  w->i32(m.type);
  w->i32(m.action);
  w->f64(m.pose.position.x);
  w->f64(m.pose.position.y);
  w->f64(m.pose.position.z);
  w->f64(m.pose.orientation.x);
  w->f64(m.pose.orientation.y);
  w->f64(m.pose.orientation.z);
  w->f64(m.pose.orientation.w);
  w->f64(m.scale.x);
  w->f64(m.scale.y);
  w->f64(m.scale.z);
  w->f32(m.color.r);
  w->f32(m.color.g);
  w->f32(m.color.b);
  w->f32(m.color.a);
  w->i32(m.lifetime_secs);
  w->i32(m.lifetime_nsecs);
  w->u8(m.frame_locked ? 1 : 0);
  w->u32((uint32_t)m.points.size());
  w->bytes(m.points.data(), m.points.size() * sizeof(slam_visualization::Point));
  w->u32((uint32_t)m.colors.size());
  w->bytes(m.colors.data(), m.colors.size() * sizeof(slam_visualization::ColorRGBA));
  w->str(m.text);
  w->str(m.mesh_resource);
  w->u8(m.mesh_use_embedded_materials ? 1 : 0);
}
inline void SerializeMarker(const slam_visualization::Marker& m, std::vector<uint8_t>* out) {
  out->clear();
  out->reserve(SerializedSize(m));
  Writer w(out);
  Write(&w, m);
}
// visualization_msgs/MarkerArray: Marker[] markers.
inline void SerializeMarkerArray(const slam_visualization::MarkerArray& a, std::vector<uint8_t>* out) {
  out->clear();
  size_t n = 4;
  for (const auto& m : a.markers) n += SerializedSize(m);
  out->reserve(n);
  Writer w(out);
  w.u32((uint32_t)a.markers.size());
  for (const auto& m : a.markers) Write(&w, m);
}

inline size_t SerializedSize(const slam_types::SLAMProblem& p) {
  size_t n = 12;
  for (const auto& node : p.nodes) n += 76 + 56 * node.features.size();
  for (const auto& c : p.vision_factors) n += 20 + 16 * c.feature_matches.size();
  n += 72 * p.odometry_factors.size();
  return n;
}

}  // namespace slam_to_ros
#endif  // VSF_HOST_SLAM_TO_ROS_H_
