// bag_extract.h -- the reference's second program, src/test/bag_extract.cc, without the bag: serialized
// sensor_msgs/CompressedImage messages of one topic in, colour JPEG files on disk out (reading a bag stays the caller's).
//   for every message (bag_extract.cc:67-92):
//     image = cv::imdecode(data, 1);  if format contains "bayer_rggb8": channel 0 -> cvtColor(COLOR_BayerBG2BGR)
//     cv::imwrite(output + "/image" + zero-filled index + ".jpg", image)
// The three steps run on the device as vsf_bag_extract_batch (include/vsf.h); this file holds what stays on the host: the file
// name, and which consecutive messages share a call.  Everything above `class BagExtract` is plain C++ with no device call in
// it (tests/cpp/test_bag_extract_plan.cc compiles it alone, under ASan + UBSan too).
#ifndef SLAM_BAG_EXTRACT_H_
#define SLAM_BAG_EXTRACT_H_

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vsf.h"
#include "slam_to_ros.h"

namespace slam {

// bag_extract.cc:81-87:  ss << output << "/image" << setfill('0') << setw(log(distance(view.begin(), view.end()))) << image_num++
// << ".jpg".  std::log is the NATURAL logarithm and setw takes an int, so the width is the truncated ln of the message count
// (1, 2 -> 0; 3 .. 7 -> 1; 8 .. 20 -> 2; 21 .. 54 -> 3; 1000 -> 6): an index with more digits than that is printed whole, as
// setw never cuts.  count < 1 (the reference would pass -inf): width 0.
inline int BagExtractIndexWidth(uint64_t count) { return count < 1 ? 0 : (int)std::log((double)count); }
inline std::string BagExtractPath(const std::string& output, uint64_t count, uint64_t index) {
  std::string digits = std::to_string(index);
  const size_t width = (size_t)BagExtractIndexWidth(count);
  if (digits.size() < width) digits.insert(0, width - digits.size(), '0');
  return output + "/image" + digits + ".jpg";
}

// One message as the plan sees it: the file inside the message, its size as the file's header states it, the topic's flag.
struct BagExtractMessage {
  const uint8_t* file = nullptr;
  size_t bytes = 0;
  int width = 0, height = 0;  // 0 x 0: the header states none (the message takes no part in a call and yields no file)
  bool bayer = false;         // format.find("bayer_rggb8") != npos (bag_extract.cc:74)
};
// vsf_compressed_image_size's signature (the plan takes the function, so that it links against nothing)
using BagExtractSizeFn = vsf_status (*)(const uint8_t* file, size_t nbytes, int* width, int* height);

// A serialized sensor_msgs/CompressedImage -> its BagExtractMessage; false when the bytes are not one whole message (the
// reference's instantiate<> returns NULL: the message is skipped and takes no index).
inline bool ViewBagExtractMessage(const uint8_t* msg, size_t n, BagExtractSizeFn size_of, BagExtractMessage* out) {
  slam_to_ros::CompressedImageView v;
  if (!msg || !slam_to_ros::ParseCompressedImage(msg, n, &v)) return false;
  *out = BagExtractMessage();
  out->file = v.data;
  out->bytes = v.size;
  out->bayer = v.format.find("bayer_rggb8") != std::string::npos;
  int w = 0, h = 0;
  if (v.size > 0 && size_of(v.data, v.size, &w, &h) == VSF_OK && w > 0 && h > 0) {
    out->width = w;
    out->height = h;
  }
  return true;
}

// Messages [first, first + count) go into ONE vsf_bag_extract_batch: consecutive, of one size and one flag, at most
// max_per_call of them.  width = 0: the one message has no size; no call is made for it.
struct BagExtractCall {
  size_t first = 0, count = 0;
  int width = 0, height = 0;
  bool bayer = false;
};
inline std::vector<BagExtractCall> PlanBagExtract(const std::vector<BagExtractMessage>& m, size_t max_per_call) {
  std::vector<BagExtractCall> calls;
  if (max_per_call < 1) max_per_call = 1;
  if (max_per_call > 65535) max_per_call = 65535;  // vsf_bag_extract_batch's n_images
  for (size_t i = 0; i < m.size(); i++) {
    const bool sized = m[i].width > 0 && m[i].height > 0;
    if (sized && !calls.empty()) {
      BagExtractCall& c = calls.back();
      if (c.width == m[i].width && c.height == m[i].height && c.bayer == m[i].bayer && c.count < max_per_call &&
          c.first + c.count == i) {
        c.count++;
        continue;
      }
    }
    BagExtractCall c;
    c.first = i;
    c.count = 1;
    c.width = sized ? m[i].width : 0;
    c.height = sized ? m[i].height : 0;
    c.bayer = m[i].bayer;
    calls.push_back(c);
  }
  return calls;
}

// The program's loop on a context of its own (created by the first Run; any image size: the context's own size plays no part
// in vsf_bag_extract_batch).
class BagExtract {
 public:
  // quality: as vsf_bag_extract_batch (0 = 95, cv::imwrite's); max_per_call: the most messages one call takes
  explicit BagExtract(int device = 0, int quality = 0, size_t max_per_call = 512);
  ~BagExtract();
  BagExtract(const BagExtract&) = delete;
  BagExtract& operator=(const BagExtract&) = delete;

  // messages: (pointer, bytes) of serialized sensor_msgs/CompressedImage, in topic order.  Writes output + "/imageNNN.jpg" for
  // every message that is one (the index counts those; the zero-fill follows messages.size(), as distance(view) does) and
  // returns the paths in message order.  A message whose file could not be written -- no size in its header, refused by a
  // decoder, the file system -- has an EMPTY path in its place, and last_status() is the first such call's status
  // (VSF_ERR_INVALID_ARG for a file without a size or a path that cannot be written).
  std::vector<std::string> Run(const std::vector<std::pair<const uint8_t*, size_t>>& messages, const std::string& output);
  vsf_status last_status() const { return last_status_; }
  size_t calls() const { return calls_; }  // vsf_bag_extract_batch calls of the last Run

 private:
  int device_, quality_;
  size_t max_per_call_;
  vsf_ctx* ctx_ = nullptr;
  vsf_status last_status_ = VSF_OK;
  size_t calls_ = 0;
  std::vector<uint8_t> out_;
  std::vector<int32_t> out_bytes_;
};

}  // namespace slam

#endif  // SLAM_BAG_EXTRACT_H_
