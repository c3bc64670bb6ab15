// test_visualization.cc -- host/slam_visualization.h and the Marker serialisation of host/slam_to_ros.h on the CPU, as a
// stand-alone program (tests/test_visualization_host.py builds it plainly and under AddressSanitizer + UBSan):
//   a Marker with two points and a MarkerArray of two markers against bytes written out by hand below;
//   AddPoseGraph on a three-node problem with a vision factor that skips a node and one that names a node that is not there;
//   the predicate table of AddFeaturePoints (main.cc:162-165) under the identity and under a non-trivial pose, coordinates
//   against a float64 evaluation of the same formula.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../vision_slam_frontend_amd/host/slam_to_ros.h"
#include "../../vision_slam_frontend_amd/host/slam_visualization.h"

namespace sv = slam_visualization;
using slam_types::Quaternionf;
using slam_types::Vector2f;
using slam_types::Vector3f;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                \
    }                                                            \
  } while (0)

// ---- bytes by hand: little endian; a float64 whose low six bytes are zero is given by its two high bytes ----
typedef std::vector<uint8_t> Bytes;
static void u32(Bytes* b, uint32_t v) {
  for (int i = 0; i < 4; i++) b->push_back((uint8_t)(v >> (8 * i)));
}
static void f64_hi(Bytes* b, uint8_t byte6, uint8_t byte7) {
  for (int i = 0; i < 6; i++) b->push_back(0);
  b->push_back(byte6);
  b->push_back(byte7);
}
static void f32_bytes(Bytes* b, uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3) {
  b->push_back(b0), b->push_back(b1), b->push_back(b2), b->push_back(b3);
}
static void text(Bytes* b, const char* s) {
  u32(b, (uint32_t)std::strlen(s));
  for (const char* p = s; *p; p++) b->push_back((uint8_t)*p);
}
static void zero_f64(Bytes* b) { f64_hi(b, 0x00, 0x00); }
static void one_f64(Bytes* b) { f64_hi(b, 0xF0, 0x3F); }  // 1.0 = 0x3FF0000000000000

// Everything of a marker in front of its points: seq, stamp, frame_id, ns, id, type, action, identity pose, scale, colour,
// lifetime 0, frame_locked 0.  scale and colour bytes are appended by the caller.
static void marker_head(Bytes* b, uint32_t seq, uint32_t secs, uint32_t nsecs, const char* frame_id, const char* ns, uint32_t id,
                        uint32_t type) {
  u32(b, seq), u32(b, secs), u32(b, nsecs);
  text(b, frame_id);
  text(b, ns);
  u32(b, id), u32(b, type), u32(b, 0);
  zero_f64(b), zero_f64(b), zero_f64(b);             // position
  zero_f64(b), zero_f64(b), zero_f64(b), one_f64(b);  // orientation x y z w
}

static void test_marker_bytes() {
  sv::Marker m;
  sv::InitializeMarker(sv::Marker::POINTS, sv::Color4f::kRed(), 0.5f, 0.25f, 0, &m);
  CHECK(m.color.r == 0 && m.color.a == 0);  // (the reference's InitializeMarker does not store the colour)
  m.header.seq = 7;
  m.header.stamp_secs = 1;
  m.header.stamp_nsecs = 2;
  m.ns = "n";
  m.id = 3;
  m.color = sv::StdColor(sv::Color4f::kRed());
  CHECK(sv::AddPoint(Vector3f(1, 2, 3), sv::CloudColor(), &m));
  CHECK(sv::AddPoint(Vector3f(-1, 0.5f, 0), sv::Color4f::kBlue(), &m));
  CHECK(!sv::AddLine(Vector3f(), Vector3f(), sv::Color4f::kBlue(), &m) && m.points.size() == 2);  // not a LINE_LIST
  Bytes want;
  marker_head(&want, 7, 1, 2, "map", "n", 3, 8);
  f64_hi(&want, 0xE0, 0x3F), f64_hi(&want, 0xD0, 0x3F), zero_f64(&want);  // scale 0.5, 0.25, 0
  f32_bytes(&want, 0, 0, 0x80, 0x3F), f32_bytes(&want, 0, 0, 0, 0), f32_bytes(&want, 0, 0, 0, 0), f32_bytes(&want, 0, 0, 0x80, 0x3F);
  u32(&want, 0), u32(&want, 0);  // lifetime
  want.push_back(0);             // frame_locked
  u32(&want, 2);                 // points
  one_f64(&want), f64_hi(&want, 0x00, 0x40), f64_hi(&want, 0x08, 0x40);  // 1, 2, 3
  f64_hi(&want, 0xF0, 0xBF), f64_hi(&want, 0xE0, 0x3F), zero_f64(&want);  // -1, 0.5, 0
  u32(&want, 2);                 // colours
  f32_bytes(&want, 0, 0, 0x80, 0x3F), f32_bytes(&want, 0, 0, 0x80, 0x3F), f32_bytes(&want, 0, 0, 0x80, 0x3F);
  f32_bytes(&want, 0xCD, 0xCC, 0x4C, 0x3E);  // 0.2f = 0x3E4CCCCD
  f32_bytes(&want, 0, 0, 0, 0), f32_bytes(&want, 0, 0, 0, 0), f32_bytes(&want, 0, 0, 0x80, 0x3F), f32_bytes(&want, 0, 0, 0x80, 0x3F);
  text(&want, ""), text(&want, "");
  want.push_back(0);  // mesh_use_embedded_materials
  Bytes got;
  slam_to_ros::SerializeMarker(m, &got);
  CHECK(got == want);
  CHECK(got.size() == slam_to_ros::SerializedSize(m) && got.size() == 154 + 3 + 1 + 2 * 24 + 2 * 16);

  // a MarkerArray of two markers: a LINE_LIST with one line and an empty POINTS marker with text, a mesh name and both flags
  sv::MarkerArray a;
  a.markers.resize(2);
  sv::InitializeMarker(sv::Marker::LINE_LIST, sv::Color4f::kGreen(), 0.02f, 0, 0, &a.markers[0]);
  a.markers[0].id = 1;
  CHECK(sv::AddLine(Vector3f(0, 0, 0), Vector3f(2, 0, 0), sv::Color4f::kGreen(), &a.markers[0]));
  CHECK(!sv::AddPoint(Vector3f(), sv::Color4f::kRed(), &a.markers[0]));  // not a POINTS marker
  sv::InitializeMarker(sv::Marker::POINTS, sv::Color4f::kWhite(), 1, 1, 1, &a.markers[1]);
  a.markers[1].id = 2;
  a.markers[1].text = "t";
  a.markers[1].mesh_resource = "ab";
  a.markers[1].frame_locked = 1;
  a.markers[1].mesh_use_embedded_materials = 1;
  a.markers[1].lifetime_secs = -1;
  a.markers[1].lifetime_nsecs = 5;
  Bytes w2;
  u32(&w2, 2);
  marker_head(&w2, 0, 0, 0, "map", "", 1, 5);
  {  // scale.x = (double)0.02f = 0x3F947AE140000000
    const uint8_t s[8] = {0x00, 0x00, 0x00, 0x40, 0xE1, 0x7A, 0x94, 0x3F};
    w2.insert(w2.end(), s, s + 8);
  }
  zero_f64(&w2), zero_f64(&w2);
  for (int i = 0; i < 4; i++) f32_bytes(&w2, 0, 0, 0, 0);  // color: not stored by InitializeMarker
  u32(&w2, 0), u32(&w2, 0);
  w2.push_back(0);
  u32(&w2, 2);
  zero_f64(&w2), zero_f64(&w2), zero_f64(&w2);
  f64_hi(&w2, 0x00, 0x40), zero_f64(&w2), zero_f64(&w2);
  u32(&w2, 2);
  for (int i = 0; i < 2; i++)
    f32_bytes(&w2, 0, 0, 0, 0), f32_bytes(&w2, 0, 0, 0x80, 0x3F), f32_bytes(&w2, 0, 0, 0, 0), f32_bytes(&w2, 0, 0, 0x80, 0x3F);
  text(&w2, ""), text(&w2, "");
  w2.push_back(0);
  marker_head(&w2, 0, 0, 0, "map", "", 2, 8);
  one_f64(&w2), one_f64(&w2), one_f64(&w2);
  for (int i = 0; i < 4; i++) f32_bytes(&w2, 0, 0, 0, 0);
  u32(&w2, 0xFFFFFFFFu), u32(&w2, 5);  // duration: int32 secs -1, nsecs 5
  w2.push_back(1);
  u32(&w2, 0), u32(&w2, 0);
  text(&w2, "t"), text(&w2, "ab");
  w2.push_back(1);
  slam_to_ros::SerializeMarkerArray(a, &got);
  CHECK(got == w2);
}

static slam_types::SLAMNode node_at(uint64_t idx, float x, float y, float z) {
  slam_types::SLAMNode n;
  n.node_idx = idx;
  n.pose = slam_types::RobotPose(Vector3f(x, y, z), Quaternionf());
  return n;
}

static void test_pose_graph() {
  slam_types::SLAMProblem p;
  p.nodes = {node_at(0, 0, 0, 0), node_at(1, 1, 0.5f, 0), node_at(2, 2, -0.25f, 0.125f)};
  p.odometry_factors = {slam_types::OdometryFactor(0, 1, Vector3f(), Quaternionf()),
                        slam_types::OdometryFactor(1, 2, Vector3f(), Quaternionf())};
  p.vision_factors = {slam_types::VisionFactor(0, 1, std::vector<slam_types::FeatureMatch>()),
                      slam_types::VisionFactor(0, 2, std::vector<slam_types::FeatureMatch>()),   // skips node 1
                      slam_types::VisionFactor(1, 7, std::vector<slam_types::FeatureMatch>())};  // node 7 does not exist
  sv::Visualization v;
  const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  sv::BuildVisualization(identity, p, &v);
  CHECK(v.nodes.id == 0 && v.odometry.id == 1 && v.vision.id == 2 && v.vision_points.id == 3);
  CHECK(v.nodes.type == sv::Marker::POINTS && v.odometry.type == sv::Marker::LINE_LIST && v.vision.type == sv::Marker::LINE_LIST &&
        v.vision_points.type == sv::Marker::POINTS);
  CHECK(v.nodes.scale.x == (double)0.05f && v.nodes.scale.y == (double)0.1f && v.nodes.scale.z == 0);
  CHECK(v.odometry.scale.x == (double)0.02f && v.vision.scale.x == (double)0.01f && v.vision_points.scale.z == (double)0.025f);
  CHECK(v.nodes.header.frame_id == "map" && v.vision_points.header.frame_id == "map" && v.nodes.pose.orientation.w == 1.0);
  CHECK(v.nodes.points.size() == 3 && v.nodes.colors.size() == 3);
  CHECK(v.nodes.points[2].x == 2 && v.nodes.points[2].y == -0.25 && v.nodes.points[2].z == 0.125);
  CHECK(v.nodes.colors[1].r == 1 && v.nodes.colors[1].g == 0 && v.nodes.colors[1].b == 0 && v.nodes.colors[1].a == 1);
  CHECK(v.odometry.points.size() == 4 && v.odometry.colors.size() == 4);
  CHECK(v.odometry.points[2].x == 1 && v.odometry.points[2].y == 0.5 && v.odometry.points[3].x == 2);
  CHECK(v.odometry.colors[3].g == 1 && v.odometry.colors[3].r == 0);
  CHECK(v.vision.points.size() == 4 && v.vision.colors.size() == 4);  // two lines: the factor to node 7 is skipped
  CHECK(v.vision.points[2].x == 0 && v.vision.points[3].x == 2 && v.vision.points[3].z == 0.125);
  CHECK(v.vision.colors[0].b == 1 && v.vision.colors[0].a == 1);
  CHECK(v.vision_points.points.empty());
  CHECK(v.PoseGraph().markers.size() == 3 && v.PoseGraph().markers[2].id == 2);
}

struct Row {
  float x, y, z;
  bool keep;
};

static void test_predicate_table() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float z01 = 0.1f, below01 = std::nextafterf(0.1f, 0.f);
  const Row rows[] = {
      {nan, 1, 1, false},  {1, nan, 1, false},  {1, 1, nan, false},  {inf, 1, 1, false},  {1, inf, 1, false},  {1, 1, inf, false},
      {-inf, 1, 1, false}, {1, -inf, 1, false}, {1, 1, -inf, false}, {0, 0, 0, false},
      {0, 0.6f, z01, true},       // (double)0.1f = 0.100000001490116... > 0.1
      {0, 0.6f, below01, false},  // the float below it is below 0.1
      {0, 0, 0.5f, false},        // norm exactly 0.5: not > 0.5
      {0, 0, std::nextafterf(0.5f, 1.f), true},
      {0, 0, std::nextafterf(0.5f, 0.f), false},
      {0, 0, 20.0f, false},       // norm exactly 20: not < 20
      {0, 0, std::nextafterf(20.0f, 0.f), true},
      {0, 0, std::nextafterf(20.0f, 21.f), false},
      {12, 0, 16, false},         // 144 + 256 = 400 exactly, norm 20
      {1.5f, 0, 2, true},         // norm 2.5
      {3, 4, -5, false},          // negative z, large norm
      {5, 5, 0.05f, false},       // z too small
      {-3, 2, 6, true},           // norm 7
  };
  const int n = (int)(sizeof(rows) / sizeof(rows[0]));
  const float cam[12] = {0.009916590468f, -0.2835522866f, 0.9589055021f, -0.01f, -0.9998698619f, -0.01501486552f, 0.005900269087f, 0.06f,
                         0.01272480238f,  -0.9588392225f, -0.2836642819f, 0.53f};
  const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int pass = 0; pass < 2; pass++) {
    const float* c = pass ? cam : identity;
    slam_types::SLAMProblem p;
    p.nodes.resize(1);
    // pass 1: a rotation about a skew axis (a unit quaternion up to float rounding) and a translation
    const Quaternionf q = pass ? Quaternionf(0.5f, 0.5f, -0.5f, 0.5f) : Quaternionf();
    const Vector3f loc = pass ? Vector3f(3.5f, -2.25f, 0.75f) : Vector3f();
    p.nodes[0].pose = slam_types::RobotPose(loc, q);
    for (int i = 0; i < n; i++)
      p.nodes[0].features.push_back(slam_types::VisionFeature((uint64_t)i, Vector2f(), Vector3f(rows[i].x, rows[i].y, rows[i].z)));
    sv::Marker m;
    sv::InitializeMarker(sv::Marker::POINTS, sv::Color4f::kWhite(), 0.025f, 0.025f, 0.025f, &m);
    sv::AddFeaturePoints(c, p, &m);
    size_t k = 0;
    // float64 evaluation of M = (T(loc) * R(q)) * C, then M * p
    const double w = q.w(), x = q.x(), y = q.y(), z = q.z();
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                         2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    const double t[3] = {loc.x(), loc.y(), loc.z()};
    for (int i = 0; i < n; i++) {
      CHECK(vsfwp::keep(rows[i].x, rows[i].y, rows[i].z) == rows[i].keep);
      if (!rows[i].keep) continue;
      CHECK(k < m.points.size());
      if (k >= m.points.size()) break;
      const double pc[3] = {rows[i].x, rows[i].y, rows[i].z};
      double pr[3], pw[3];
      for (int r = 0; r < 3; r++) pr[r] = c[4 * r] * pc[0] + c[4 * r + 1] * pc[1] + c[4 * r + 2] * pc[2] + c[4 * r + 3];
      for (int r = 0; r < 3; r++) pw[r] = R[3 * r] * pr[0] + R[3 * r + 1] * pr[1] + R[3 * r + 2] * pr[2] + t[r];
      const double got[3] = {m.points[k].x, m.points[k].y, m.points[k].z};
      const double bound = 1e-5 * (std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) +
                                   std::sqrt((double)c[3] * c[3] + (double)c[7] * c[7] + (double)c[11] * c[11]) +
                                   std::sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]));
      for (int r = 0; r < 3; r++) {
        CHECK(std::fabs(got[r] - pw[r]) <= bound);
        CHECK((double)(float)got[r] == got[r]);  // a float, widened
        if (!pass) CHECK(got[r] == pc[r]);       // the identity is exact
      }
      CHECK(m.colors[k].r == 1 && m.colors[k].g == 1 && m.colors[k].b == 1 && m.colors[k].a == 0.2f);
      k++;
    }
    CHECK(k == m.points.size() && m.colors.size() == m.points.size());
  }
}

int main() {
  test_marker_bytes();
  test_pose_graph();
  test_predicate_table();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok visualization\n");
  return 0;
}
