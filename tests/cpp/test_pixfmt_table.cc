// The pixel-format table of include/vsf.h (vsf_pixfmt_bytes_per_pixel, vsf_pixfmt_from_encoding; csrc/vsf_observe_plan.cc)
// as a stand-alone program on the CPU, built plainly and under AddressSanitizer + UBSan (tests/test_pixfmt_ref.py).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/vsf.h"
#include "../../vision_slam_frontend_amd/csrc/vsf_observe_plan.h"

static int failures = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                            \
    }                                                        \
  } while (0)

int main() {
  static const struct {
    const char* name;
    int code, bpp;
  } kWant[] = {{"mono8", 0, 1},        {"bayer_rggb8", 1, 1}, {"bayer_grbg8", 16, 1}, {"bayer_gbrg8", 17, 1}, {"bayer_bggr8", 18, 1},
               {"bgr8", 19, 3},        {"rgb8", 20, 3},       {"bgra8", 21, 4},       {"rgba8", 22, 4}};
  CHECK(VSF_PIX_MONO8 == 0 && VSF_PIX_BAYER_RGGB8 == 1 && VSF_PIX_BAYER_GRBG8 == 16 && VSF_PIX_BAYER_GBRG8 == 17 &&
        VSF_PIX_BAYER_BGGR8 == 18 && VSF_PIX_BGR8 == 19 && VSF_PIX_RGB8 == 20 && VSF_PIX_BGRA8 == 21 && VSF_PIX_RGBA8 == 22);
  int n = 0;
  for (const auto& w : kWant) {
    int code = -7;
    CHECK(vsf_pixfmt_from_encoding(w.name, &code) == VSF_OK && code == w.code);
    CHECK(vsf_pixfmt_bytes_per_pixel(w.code) == w.bpp);
    // a name is matched whole: a prefix, a longer name and another case are other encodings
    std::string s(w.name);
    code = -7;
    CHECK(vsf_pixfmt_from_encoding((s + "x").c_str(), &code) == VSF_ERR_UNSUPPORTED && code == -7);
    CHECK(vsf_pixfmt_from_encoding(s.substr(0, s.size() - 1).c_str(), &code) == VSF_ERR_UNSUPPORTED && code == -7);
    s[0] = (char)(s[0] - 'a' + 'A');
    CHECK(vsf_pixfmt_from_encoding(s.c_str(), &code) == VSF_ERR_UNSUPPORTED && code == -7);
    n++;
  }
  // every other code is unknown: 2 .. 15 for good, negatives, everything above 22
  for (int c = -40; c <= 300; c++) {
    bool known = false;
    for (const auto& w : kWant) known = known || w.code == c;
    if (!known) CHECK(vsf_pixfmt_bytes_per_pixel(c) == 0);
  }
  CHECK(vsf_pixfmt_bytes_per_pixel(INT_MIN) == 0 && vsf_pixfmt_bytes_per_pixel(INT_MAX) == 0);
  int code = -7;
  CHECK(vsf_pixfmt_from_encoding("", &code) == VSF_ERR_UNSUPPORTED && code == -7);
  CHECK(vsf_pixfmt_from_encoding("mono16", &code) == VSF_ERR_UNSUPPORTED && code == -7);
  CHECK(vsf_pixfmt_from_encoding("yuv422", &code) == VSF_ERR_UNSUPPORTED && code == -7);
  CHECK(vsf_pixfmt_from_encoding(nullptr, &code) == VSF_ERR_INVALID_ARG && code == -7);
  CHECK(vsf_pixfmt_from_encoding("mono8", nullptr) == VSF_ERR_INVALID_ARG);
  // the big slots' arithmetic in bytes per row (vsf_observe_plan.h): bpp = 1 is the declared sizes' own
  using namespace vsfi;
  for (int w : {1, 63, 64, 65, 320, 326, 640, 16384, 32767})
    for (int h : {1, 2, 240, 480, 32767}) {
      CHECK(observe_pix_pitch(w, 1) == observe_input_pitch(w));
      CHECK(observe_pix_image_bytes(w, h, 1) == observe_input_image_bytes(w, h) || (size_t)observe_input_pitch(w) * h > 0x7FFFFFFFu);
      for (int bpp : {3, 4}) {
        const size_t pitch = observe_pix_pitch(w, bpp), bytes = observe_pix_image_bytes(w, h, bpp);
        CHECK(pitch % 64 == 0 && pitch >= (size_t)w * bpp && pitch < (size_t)w * bpp + 64);
        if (pitch * (size_t)h <= 0x7FFFFFFFu)
          CHECK(bytes % 256 == 0 && bytes >= pitch * h && bytes < pitch * h + 256);
        else
          CHECK(bytes == 0);  // (the conversion kernel addresses an image with 32-bit offsets)
      }
    }
  CHECK(observe_pix_pitch(0, 3) == 0 && observe_pix_pitch(32768, 3) == 0 && observe_pix_pitch(640, 2) == 0 &&
        observe_pix_pitch(640, 0) == 0 && observe_pix_pitch(640, 5) == 0 && observe_pix_pitch(-1, 4) == 0);
  CHECK(observe_pix_image_bytes(640, 0, 3) == 0 && observe_pix_image_bytes(640, 32768, 3) == 0 &&
        observe_pix_image_bytes(640, 480, 3) == 1920 * 480 && observe_pix_image_bytes(640, 480, 4) == 2560 * 480 &&
        observe_pix_image_bytes(326, 246, 3) == ((1024 * 246 + 255) & ~255));
  if (failures) return 1;
  std::printf("ok %d formats\n", n);
  return 0;
}
