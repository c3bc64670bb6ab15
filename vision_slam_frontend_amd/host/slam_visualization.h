// slam_visualization.h -- what the reference's driver publishes to RViz after every new pose (PublishVisualization,
// slam_frontend_main.cc:194-225): the helpers of src/gui_helpers.{h,cc} and the driver's AddFeaturePoints / AddPoseGraph
// (main.cc:155-192), written from scratch over plain structs (no ROS, no Eigen here).  Header-only and free of the GPU
// library, so tests/cpp/test_visualization.cc builds it for the CPU alone.
//
// visualization_msgs/Marker is restated field for field (Marker below; slam_to_ros.h serialises it).  AddFeaturePoints is
// the CPU restatement of the device's point cloud: it runs the arithmetic of csrc/vsf_world_points.h -- the header the kernel
// itself is compiled from -- so its points equal the device's bit for bit.  Compile without contraction (host/Makefile does).
#ifndef VSF_HOST_SLAM_VISUALIZATION_H_
#define VSF_HOST_SLAM_VISUALIZATION_H_

#include <cstdint>
#include <string>
#include <vector>

#include "../csrc/vsf_world_points.h"
#include "slam_types.h"

namespace slam_visualization {

// RGBA colour with each channel from 0.0 to 1.0 (gui_helpers.h:38-54; the literals of gui_helpers.cc:35-42).
struct Color4f {
  float r, g, b, a;
  Color4f() : r(0), g(0), b(0), a(0) {}
  Color4f(float r, float g, float b, float a) : r(r), g(g), b(b), a(a) {}
  static Color4f kRed() { return Color4f(1, 0, 0, 1); }
  static Color4f kGreen() { return Color4f(0, 1, 0, 1); }
  static Color4f kBlue() { return Color4f(0, 0, 1, 1); }
  static Color4f kWhite() { return Color4f(1, 1, 1, 1); }
  static Color4f kBlack() { return Color4f(0, 0, 0, 1); }
  static Color4f kYellow() { return Color4f(1, 1, 0, 1); }
  static Color4f kCyan() { return Color4f(0, 1, 1, 1); }
  static Color4f kMagenta() { return Color4f(1, 0, 1, 1); }
};

// The parts of a visualization_msgs/Marker, in ROS-1's layouts: Point / Vector3 three float64, Quaternion four float64
// (x, y, z, w), ColorRGBA four float32, time two uint32, duration two int32.  Point and ColorRGBA have no padding, so a
// std::vector of them IS the wire body of a Point[] / ColorRGBA[].
struct Point {
  double x = 0, y = 0, z = 0;
};
struct Quaternion {
  double x = 0, y = 0, z = 0, w = 0;
};
struct Pose {
  Point position;
  Quaternion orientation;
};
struct ColorRGBA {
  float r = 0, g = 0, b = 0, a = 0;
};
struct Header {
  uint32_t seq = 0;
  uint32_t stamp_secs = 0, stamp_nsecs = 0;
  std::string frame_id;
};
static_assert(sizeof(Point) == 24 && sizeof(ColorRGBA) == 16, "Point[] / ColorRGBA[] are written with one memcpy");

struct Marker {
  enum : int32_t {
    ARROW = 0, CUBE = 1, SPHERE = 2, CYLINDER = 3, LINE_STRIP = 4, LINE_LIST = 5, CUBE_LIST = 6, SPHERE_LIST = 7, POINTS = 8,
    TEXT_VIEW_FACING = 9, MESH_RESOURCE = 10, TRIANGLE_LIST = 11
  };
  enum : int32_t { ADD = 0, MODIFY = 0, DELETE = 2, DELETEALL = 3 };
  Header header;
  std::string ns;
  int32_t id = 0;
  int32_t type = 0;
  int32_t action = 0;
  Pose pose;
  Point scale;  // geometry_msgs/Vector3
  ColorRGBA color;
  int32_t lifetime_secs = 0, lifetime_nsecs = 0;  // duration
  uint8_t frame_locked = 0;
  std::vector<Point> points;
  std::vector<ColorRGBA> colors;
  std::string text;
  std::string mesh_resource;
  uint8_t mesh_use_embedded_materials = 0;
};
struct MarkerArray {
  std::vector<Marker> markers;
};

// gui_helpers.cc:44-66: the "map" frame, identity pose, the given type and scale, ids counted up per call.  As in the
// reference, `color` is accepted and NOT stored (msg->color stays zero: the points carry their own colours).
inline int& MarkerIdCounter() {
  static int marker_id = 0;
  return marker_id;
}
inline void InitializeMarker(int marker_type, const Color4f& /*color*/, float scale_x, float scale_y, float scale_z, Marker* msg) {
  msg->id = MarkerIdCounter()++;
  msg->type = marker_type;
  msg->action = Marker::ADD;
  msg->pose.position = Point();
  msg->pose.orientation.x = 0.0;
  msg->pose.orientation.y = 0.0;
  msg->pose.orientation.z = 0.0;
  msg->pose.orientation.w = 1.0;
  msg->scale.x = scale_x;
  msg->scale.y = scale_y;
  msg->scale.z = scale_z;
  msg->header.frame_id = "map";
}

inline Point StdPoint(const slam_types::Vector3f& v) {
  Point p;
  p.x = v.x();
  p.y = v.y();
  p.z = v.z();
  return p;
}
inline ColorRGBA StdColor(const Color4f& c) {
  ColorRGBA o;
  o.r = c.r;
  o.g = c.g;
  o.b = c.b;
  o.a = c.a;
  return o;
}

// gui_helpers.h:84-103.  The reference CHECKs the marker's type; here a marker of another type is left as it is and the call
// says so.
inline bool AddLine(const slam_types::Vector3f& v1, const slam_types::Vector3f& v2, const Color4f& color, Marker* msg) {
  if (msg->type != Marker::LINE_LIST) return false;
  msg->points.push_back(StdPoint(v1));
  msg->points.push_back(StdPoint(v2));
  msg->colors.push_back(StdColor(color));
  msg->colors.push_back(StdColor(color));
  return true;
}
inline bool AddPoint(const slam_types::Vector3f& v, const Color4f& color, Marker* msg) {
  if (msg->type != Marker::POINTS) return false;
  msg->points.push_back(StdPoint(v));
  msg->colors.push_back(StdColor(color));
  return true;
}
inline void ClearMarker(Marker* msg) {
  msg->points.clear();
  msg->colors.clear();
}

// The colour every point of the cloud carries (main.cc:167).
inline Color4f CloudColor() { return Color4f(1, 1, 1, 0.2f); }

// main.cc:155-173 over one node's features: every feature that passes the predicate, in feature order, as
// (RobotToWorldTf() * cam_to_robot) * point3d.  cam_to_robot: config.left_cam_to_robot as 3 x 4 row-major.
inline void AddNodeFeaturePoints(const float cam_to_robot[12], const slam_types::SLAMNode& node, Marker* marker_ptr) {
  if (marker_ptr->type != Marker::POINTS) return;
  const float loc[3] = {node.pose.loc.x(), node.pose.loc.y(), node.pose.loc.z()};
  const float quat[4] = {node.pose.angle.x(), node.pose.angle.y(), node.pose.angle.z(), node.pose.angle.w()};
  const vsfwp::Affine M = vsfwp::camera_to_world(loc, quat, cam_to_robot);
  const ColorRGBA colour = StdColor(CloudColor());
  for (const slam_types::VisionFeature& f : node.features) {
    const float x = f.point3d.x(), y = f.point3d.y(), z = f.point3d.z();
    if (!vsfwp::keep(x, y, z)) continue;
    double w[3];
    vsfwp::transform(M, x, y, z, w);
    Point p;
    p.x = w[0];
    p.y = w[1];
    p.z = w[2];
    marker_ptr->points.push_back(p);
    marker_ptr->colors.push_back(colour);
  }
}
inline void AddFeaturePoints(const float cam_to_robot[12], const slam_types::SLAMProblem& problem, Marker* marker_ptr) {
  for (const slam_types::SLAMNode& node : problem.nodes) AddNodeFeaturePoints(cam_to_robot, node, marker_ptr);
}

// main.cc:175-192.  A factor that names a node the problem does not have is skipped (the reference reads out of range).
inline void AddPoseGraph(const slam_types::SLAMProblem& problem, Marker* nodes_marker, Marker* vision_marker, Marker* odom_marker) {
  const size_t n = problem.nodes.size();
  for (const slam_types::SLAMNode& node : problem.nodes) AddPoint(node.pose.loc, Color4f::kRed(), nodes_marker);
  for (const slam_types::OdometryFactor& factor : problem.odometry_factors) {
    if (factor.pose_i >= n || factor.pose_j >= n) continue;
    AddLine(problem.nodes[factor.pose_i].pose.loc, problem.nodes[factor.pose_j].pose.loc, Color4f::kGreen(), odom_marker);
  }
  for (const slam_types::VisionFactor& factor : problem.vision_factors) {
    if (factor.pose_idx_initial >= n || factor.pose_idx_current >= n) continue;
    AddLine(problem.nodes[factor.pose_idx_initial].pose.loc, problem.nodes[factor.pose_idx_current].pose.loc, Color4f::kBlue(),
            vision_marker);
  }
}

// The four markers of PublishVisualization (main.cc:198-214), empty: ids 0 .. 3, types, scales, the "map" frame.
struct Visualization {
  Marker nodes;          // id 0  POINTS     0.05 / 0.1 / 0      one red point per node
  Marker odometry;       // id 1  LINE_LIST  0.02                a green line per odometry factor
  Marker vision;         // id 2  LINE_LIST  0.01                a blue line per vision factor
  Marker vision_points;  // id 3  POINTS     0.025 x 3           the cloud, colours (1, 1, 1, 0.2)
  // (Frontend::GetVisualization's bookkeeping: whose problem the markers hold, so that the next call only appends)
  const void* source = nullptr;
  // The MarkerArray the driver publishes on slam_frontend/pose_graph (main.cc:219-223); vision_points goes out by itself.
  MarkerArray PoseGraph() const {
    MarkerArray a;
    a.markers.push_back(nodes);
    a.markers.push_back(odometry);
    a.markers.push_back(vision);
    return a;
  }
};
inline void InitializeVisualization(Visualization* v) {
  *v = Visualization();
  InitializeMarker(Marker::POINTS, Color4f::kRed(), 0.05f, 0.1f, 0, &v->nodes);
  InitializeMarker(Marker::LINE_LIST, Color4f::kGreen(), 0.02f, 0, 0, &v->odometry);
  InitializeMarker(Marker::LINE_LIST, Color4f::kBlue(), 0.01f, 0, 0, &v->vision);
  InitializeMarker(Marker::POINTS, Color4f::kWhite(), 0.025f, 0.025f, 0.025f, &v->vision_points);
  v->nodes.id = 0;
  v->odometry.id = 1;
  v->vision.id = 2;
  v->vision_points.id = 3;
}

// PublishVisualization's markers for a whole problem, on the CPU: what the reference's driver computes after every pose.
inline void BuildVisualization(const float cam_to_robot[12], const slam_types::SLAMProblem& problem, Visualization* v) {
  InitializeVisualization(v);
  AddFeaturePoints(cam_to_robot, problem, &v->vision_points);
  AddPoseGraph(problem, &v->nodes, &v->vision, &v->odometry);
}

}  // namespace slam_visualization

#endif  // VSF_HOST_SLAM_VISUALIZATION_H_
