// Known-answer and round-trip test of slam_to_ros::SerializeCompressedImage / ParseCompressedImage (host/slam_to_ros.h): one
// sensor_msgs/CompressedImage against bytes assembled field by field from the ROS-1 serialisation rules, then parsed back; cut
// and over-long payloads are refused.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../vision_slam_frontend_amd/host/slam_to_ros.h"

static std::vector<uint8_t> expect;
static void U32(uint32_t v) { for (int i = 0; i < 4; i++) expect.push_back((uint8_t)(v >> (8 * i))); }
static void Str(const char* s) { U32((uint32_t)std::strlen(s)); for (; *s; s++) expect.push_back((uint8_t)*s); }

int main() {
  std::vector<uint8_t> file = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0xFF, 0x00, 0xFF, 0xD9};
  std::vector<uint8_t> got;
  slam_to_ros::SerializeCompressedImage(7, 1500000000u, 999999999u, "stereo_left", file.data(), file.size(), &got);
  U32(7); U32(1500000000u); U32(999999999u); Str("stereo_left"); Str("jpeg");
  U32((uint32_t)file.size());
  expect.insert(expect.end(), file.begin(), file.end());
  if (got != expect || got.size() != 24 + 11 + 4 + file.size()) { std::printf("FAIL bytes (%zu vs %zu)\n", got.size(), expect.size()); return 1; }
  slam_to_ros::CompressedImageView v;
  if (!slam_to_ros::ParseCompressedImage(got.data(), got.size(), &v) || v.seq != 7 || v.stamp_secs != 1500000000u ||
      v.stamp_nsecs != 999999999u || v.frame_id != "stereo_left" || v.format != "jpeg" || v.size != file.size() ||
      std::memcmp(v.data, file.data(), file.size()) != 0) { std::printf("FAIL round trip\n"); return 1; }
  for (size_t n = 0; n < got.size(); n++) {  // every cut payload is refused (heap copies: a read past the end is an error)
    std::vector<uint8_t> cut(got.begin(), got.begin() + n);
    if (slam_to_ros::ParseCompressedImage(cut.data(), cut.size(), &v)) { std::printf("FAIL cut at %zu accepted\n", n); return 1; }
  }
  got.push_back(0);
  if (slam_to_ros::ParseCompressedImage(got.data(), got.size(), &v)) { std::printf("FAIL trailing byte accepted\n"); return 1; }
  // an empty frame_id and an empty file are messages too
  slam_to_ros::SerializeCompressedImage(0, 0, 0, "", nullptr, 0, &got);
  if (got.size() != 24 + 4 || !slam_to_ros::ParseCompressedImage(got.data(), got.size(), &v) || v.size != 0 || !v.frame_id.empty()) {
    std::printf("FAIL empty\n");
    return 1;
  }
  if (std::strlen(slam_to_ros::kCompressedImageMd5) != 32) return 1;
  std::printf("ok %s\n", slam_to_ros::kCompressedImageMd5);
  return 0;
}
