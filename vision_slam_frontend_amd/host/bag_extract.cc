// bag_extract.cc -- slam::BagExtract: the loop of src/test/bag_extract.cc:67-92 over serialized messages, one
// vsf_bag_extract_batch per run of messages PlanBagExtract (bag_extract.h) puts together.
#include "bag_extract.h"

#include <cstdio>

namespace slam {

BagExtract::BagExtract(int device, int quality, size_t max_per_call)
    : device_(device), quality_(quality), max_per_call_(max_per_call) {}

BagExtract::~BagExtract() {
  if (ctx_) vsf_destroy(ctx_);
}

static bool WriteFile(const std::string& path, const uint8_t* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(data, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

std::vector<std::string> BagExtract::Run(const std::vector<std::pair<const uint8_t*, size_t>>& messages,
                                         const std::string& output) {
  last_status_ = VSF_OK;
  calls_ = 0;
  auto fail = [&](vsf_status st) {
    if (last_status_ == VSF_OK) last_status_ = st;
  };
  // the messages that are messages, and where each stands in the caller's list
  std::vector<BagExtractMessage> msgs;
  std::vector<size_t> at;
  for (size_t i = 0; i < messages.size(); i++) {
    BagExtractMessage m;
    if (ViewBagExtractMessage(messages[i].first, messages[i].second, vsf_compressed_image_size, &m)) {
      msgs.push_back(m);
      at.push_back(i);
    }
  }
  std::vector<std::string> paths(messages.size());
  if (msgs.empty()) return paths;
  if (!ctx_) {
    vsf_params p;
    vsf_status st = vsf_params_default(&p, 64, 64, 2);
    if (st == VSF_OK) st = vsf_create(&p, device_, &ctx_);
    if (st != VSF_OK) {
      ctx_ = nullptr;
      fail(st);
      return paths;
    }
  }
  const uint64_t count = messages.size();  // distance(view.begin(), view.end())
  for (const BagExtractCall& c : PlanBagExtract(msgs, max_per_call_)) {
    if (c.width == 0) {  // (cv::imdecode returns an empty Mat and the reference dies in imwrite)
      fail(VSF_ERR_INVALID_ARG);
      continue;
    }
    const size_t stride = vsf_jpeg_encode_capacity(c.width, c.height, 3);
    std::vector<const uint8_t*> files(c.count);
    std::vector<size_t> sizes(c.count);
    for (size_t k = 0; k < c.count; k++) {
      files[k] = msgs[c.first + k].file;
      sizes[k] = msgs[c.first + k].bytes;
    }
    if (out_.size() < stride * c.count) out_.resize(stride * c.count);
    out_bytes_.assign(c.count, -1);
    const vsf_status st = vsf_bag_extract_batch(ctx_, files.data(), sizes.data(), (int)c.count, c.width, c.height,
                                                c.bayer ? VSF_PIX_BAYER_RGGB8 : 0, quality_, out_.data(), stride, out_bytes_.data());
    calls_++;
    if (st != VSF_OK) fail(st);
    for (size_t k = 0; k < c.count; k++) {
      if (out_bytes_[k] <= 0) continue;
      const std::string path = BagExtractPath(output, count, c.first + k);
      if (WriteFile(path, out_.data() + k * stride, (size_t)out_bytes_[k]))
        paths[at[c.first + k]] = path;
      else
        fail(VSF_ERR_INVALID_ARG);
    }
  }
  return paths;
}

}  // namespace slam
