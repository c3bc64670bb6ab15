// The host half of slam::BagExtract (vision_slam_frontend_amd/host/bag_extract.h), stand-alone on the CPU: the reference's file
// name (src/test/bag_extract.cc:81-87: the index zero-filled to the truncated NATURAL log of the message count) at the counts
// where the width changes, and the grouping of a message list that changes size and flag into calls.  No device, no library:
// the size of a "file" comes from a stand-in for vsf_compressed_image_size that reads a PNG's IHDR.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../vision_slam_frontend_amd/host/bag_extract.h"

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
      fails++;                                              \
    }                                                       \
  } while (0)

static vsf_status ihdr_size(const uint8_t* f, size_t n, int* w, int* h) {
  *w = *h = 0;
  if (n < 24 || std::memcmp(f, "\x89PNG\r\n\x1a\n", 8) != 0) return VSF_ERR_UNSUPPORTED;
  *w = (f[16] << 24) | (f[17] << 16) | (f[18] << 8) | f[19];
  *h = (f[20] << 24) | (f[21] << 16) | (f[22] << 8) | f[23];
  return VSF_OK;
}

static std::vector<uint8_t> file_of(int w, int h) {
  std::vector<uint8_t> f = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
  for (int v : {w, h})
    for (int s = 24; s >= 0; s -= 8) f.push_back((uint8_t)(v >> s));
  return f;
}

static std::vector<uint8_t> message_of(const std::vector<uint8_t>& file, const std::string& format) {
  std::vector<uint8_t> m;
  slam_to_ros::SerializeCompressedImage(1, 2, 3, "cam", file.data(), file.size(), &m, format);
  return m;
}

int main() {
  using slam::BagExtractPath;
  // ln 1 = 0, ln 2 = 0.69, ln 3 = 1.10, ln 7 = 1.95, ln 8 = 2.08, ln 20 = 2.996, ln 21 = 3.04, ln 1000 = 6.9
  const struct { unsigned long long count; int width; } widths[] = {{1, 0}, {2, 0}, {3, 1}, {7, 1}, {8, 2}, {20, 2}, {21, 3}, {1000, 6}};
  for (const auto& c : widths) CHECK(slam::BagExtractIndexWidth(c.count) == c.width);
  CHECK(slam::BagExtractIndexWidth(0) == 0);
  CHECK(BagExtractPath("out", 1, 0) == "out/image0.jpg");
  CHECK(BagExtractPath("out", 2, 1) == "out/image1.jpg");
  CHECK(BagExtractPath("out", 3, 2) == "out/image2.jpg");
  CHECK(BagExtractPath("/a/b", 7, 6) == "/a/b/image6.jpg");
  CHECK(BagExtractPath("out", 8, 7) == "out/image07.jpg");
  CHECK(BagExtractPath("out", 20, 19) == "out/image19.jpg");
  CHECK(BagExtractPath("out", 20, 3) == "out/image03.jpg");
  CHECK(BagExtractPath("out", 21, 3) == "out/image003.jpg");
  CHECK(BagExtractPath("out", 21, 20) == "out/image020.jpg");
  CHECK(BagExtractPath("", 1000, 999) == "/image000999.jpg");
  CHECK(BagExtractPath("out", 1000, 0) == "out/image000000.jpg");
  // an index longer than the width is printed whole (setw never cuts)
  CHECK(BagExtractPath("out", 3, 12) == "out/image12.jpg");
  CHECK(BagExtractPath("out", 8, 123) == "out/image123.jpg");
  CHECK(BagExtractPath("out", 2, 10) == "out/image10.jpg");

  // a topic that changes size and flag: (w, h, format)
  const struct { int w, h; const char* format; } topic[] = {
      {640, 480, "jpeg"},                    // 0  call 0
      {640, 480, "jpeg"},                    // 1
      {640, 480, "bayer_rggb8; jpeg compressed"},  // 2  call 1: the flag changes
      {640, 480, "bayer_rggb8; jpeg compressed"},  // 3
      {320, 240, "bayer_rggb8; jpeg compressed"},  // 4  call 2: the size changes
      {0, 0, "jpeg"},                        // 5  call 3: a file without a size, alone
      {320, 240, "bayer_rggb8; jpeg compressed"},  // 6  call 4 (consecutive only: not joined to 4)
      {320, 240, "bayer_rggb8; jpeg compressed"},  // 7
      {320, 240, "bayer_rggb8; jpeg compressed"},  // 8
      {320, 240, "bayer_rggb8; jpeg compressed"},  // 9  call 5: max_per_call = 3
      {320, 241, "bayer_rggb8; jpeg compressed"},  // 10 call 6: one row more
      {320, 241, "rgb8; bayer_rggb8 png"},   // 11         find(), not equality
      {320, 241, "bayer_grbg8; jpeg"},       // 12 call 7: another order is no flag (the reference knows one)
  };
  std::vector<std::vector<uint8_t>> wire;
  std::vector<slam::BagExtractMessage> msgs;
  for (const auto& t : topic) wire.push_back(message_of(t.w ? file_of(t.w, t.h) : std::vector<uint8_t>{1, 2, 3}, t.format));
  for (size_t i = 0; i < wire.size(); i++) {
    slam::BagExtractMessage m;
    CHECK(slam::ViewBagExtractMessage(wire[i].data(), wire[i].size(), ihdr_size, &m));
    CHECK(m.width == topic[i].w && m.height == topic[i].h);
    CHECK(m.bayer == (std::strstr(topic[i].format, "bayer_rggb8") != nullptr));
    CHECK(m.bytes == (topic[i].w ? 24u : 3u) && m.file >= wire[i].data() && m.file + m.bytes == wire[i].data() + wire[i].size());
    msgs.push_back(m);
  }
  const std::vector<slam::BagExtractCall> calls = slam::PlanBagExtract(msgs, 3);
  const struct { size_t first, count; int w, h; bool bayer; } want[] = {
      {0, 2, 640, 480, false}, {2, 2, 640, 480, true}, {4, 1, 320, 240, true}, {5, 1, 0, 0, false},
      {6, 3, 320, 240, true},  {9, 1, 320, 240, true}, {10, 2, 320, 241, true}, {12, 1, 320, 241, false}};
  CHECK(calls.size() == sizeof(want) / sizeof(want[0]));
  size_t covered = 0;
  for (size_t i = 0; i < calls.size() && i < sizeof(want) / sizeof(want[0]); i++) {
    CHECK(calls[i].first == want[i].first && calls[i].count == want[i].count);
    CHECK(calls[i].width == want[i].w && calls[i].height == want[i].h && calls[i].bayer == want[i].bayer);
    CHECK(calls[i].first == covered);  // every message in exactly one call, in order
    covered += calls[i].count;
  }
  CHECK(covered == msgs.size());
  // one call takes them all when nothing changes; none for an empty topic; max_per_call is held inside 1 .. 65535
  std::vector<slam::BagExtractMessage> same(1000, msgs[0]);
  CHECK(slam::PlanBagExtract(same, 512).size() == 2 && slam::PlanBagExtract(same, 512)[1].count == 488);
  CHECK(slam::PlanBagExtract(same, 0).size() == 1000);
  CHECK(slam::PlanBagExtract(same, 1u << 20).size() == 1);
  CHECK(slam::PlanBagExtract({}, 512).empty());
  // bytes that are no message: every cut of one, and a null pointer
  slam::BagExtractMessage m;
  for (size_t n = 0; n < wire[0].size(); n++) {
    std::vector<uint8_t> cut(wire[0].begin(), wire[0].begin() + n);  // (a heap copy: a read past the end is an error)
    CHECK(!slam::ViewBagExtractMessage(cut.data(), cut.size(), ihdr_size, &m));
  }
  CHECK(!slam::ViewBagExtractMessage(nullptr, 0, ihdr_size, &m));
  // an empty payload is a message without a size
  const std::vector<uint8_t> empty = message_of({}, "jpeg");
  CHECK(slam::ViewBagExtractMessage(empty.data(), empty.size(), ihdr_size, &m) && m.width == 0 && m.bytes == 0);
  if (fails) return 1;
  std::printf("ok %zu calls\n", calls.size());
  return 0;
}
