// vsf_ingest_host.cc -- what vsf_observe_submit_compressed does with a payload before anything is booked: the staging
// ring's sizes, the format by the file's first bytes (as cv::imdecode's findDecoder does), the per-file byte cap and the
// decoder's own host checks (vsf_jpeg_plan / vsf_png_plan of the ONE file: every marker, table and chunk length).  The
// bytes are UNTRUSTED (slam_frontend_main.cc:98-100 hands cv::imdecode whatever the topic carried).  Plain C++, no HIP call:
// the same translation unit is part of the sanitizer build (make asan) and needs no device.
#include <cstring>

#include "vsf_internal.h"

extern "C" {

size_t vsf_observe_default_compressed_cap(int width, int height) {
  if (width < 1 || height < 1) return 0;
  // (a lossless file of a noisy image is a little larger than the image; a camera's JPEG a tenth of it)
  return (size_t)width * (size_t)height + 65536;
}

size_t vsf_observe_compressed_slot_bytes(size_t cap_per_image) {
  if (cap_per_image == 0 || cap_per_image > 0x40000000u) return 0;
  return (cap_per_image + 63) & ~(size_t)63;
}

size_t vsf_observe_compressed_ring_bytes(int depth, size_t cap_per_image) {
  const size_t slot = vsf_observe_compressed_slot_bytes(cap_per_image);
  if (depth < 1 || depth > 1024 || slot == 0) return 0;
  return (size_t)depth * 2 * slot;
}

// Width and height as the file's header states them (PNG: IHDR; JPEG: the first SOF0 / SOF1 / SOF2 segment); nothing else
// of the file is looked at or promised -- the submit's checks follow.
vsf_status vsf_compressed_image_size(const uint8_t* file, size_t nbytes, int* width, int* height) {
  static const uint8_t kPng[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (!file || !width || !height) return VSF_ERR_INVALID_ARG;
  *width = *height = 0;
  uint32_t w = 0, h = 0;
  if (nbytes >= 8 && std::memcmp(file, kPng, 8) == 0) {
    if (nbytes < 24 || std::memcmp(file + 12, "IHDR", 4) != 0) return VSF_ERR_INVALID_ARG;
    w = ((uint32_t)file[16] << 24) | ((uint32_t)file[17] << 16) | ((uint32_t)file[18] << 8) | file[19];
    h = ((uint32_t)file[20] << 24) | ((uint32_t)file[21] << 16) | ((uint32_t)file[22] << 8) | file[23];
  } else if (nbytes >= 3 && file[0] == 0xFF && file[1] == 0xD8 && file[2] == 0xFF) {
    size_t pos = 2;
    while (pos + 4 <= nbytes) {
      if (file[pos] != 0xFF) return VSF_ERR_INVALID_ARG;
      while (pos < nbytes && file[pos] == 0xFF) pos++;
      if (pos >= nbytes) return VSF_ERR_INVALID_ARG;
      const int m = file[pos++];
      if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
      if (m == 0xD9 || m == 0xDA || pos + 2 > nbytes) return VSF_ERR_INVALID_ARG;  // (no frame header in front of the data)
      const size_t len = ((size_t)file[pos] << 8) | file[pos + 1];
      if (len < 2 || len > nbytes - pos) return VSF_ERR_INVALID_ARG;
      if (m >= 0xC0 && m <= 0xC2) {
        if (len < 7) return VSF_ERR_INVALID_ARG;
        h = ((uint32_t)file[pos + 3] << 8) | file[pos + 4];
        w = ((uint32_t)file[pos + 5] << 8) | file[pos + 6];
        break;
      }
      pos += len;
    }
  } else {
    return VSF_ERR_UNSUPPORTED;
  }
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return VSF_ERR_INVALID_ARG;
  *width = (int)w;
  *height = (int)h;
  return VSF_OK;
}

vsf_status vsf_observe_probe_compressed(const uint8_t* file, size_t nbytes, int width, int height, size_t cap_per_image,
                                        int force_serial, int* kind) {
  static const uint8_t kPng[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (kind) *kind = 0;
  if (!file || width < 1 || height < 1 || width > 65535 || height > 65535) return VSF_ERR_INVALID_ARG;
  int k = 0;
  if (nbytes >= 8 && std::memcmp(file, kPng, 8) == 0)
    k = 2;
  else if (nbytes >= 3 && file[0] == 0xFF && file[1] == 0xD8 && file[2] == 0xFF)
    k = 1;
  if (k == 0) return VSF_ERR_UNSUPPORTED;  // (imdecode's other formats -- BMP, TIFF, WebP ... -- are not built)
  if (nbytes > cap_per_image || nbytes > 0x40000000u) return VSF_ERR_CAPACITY;
  const uint8_t* files[1] = {file};
  const size_t sizes[1] = {nbytes};
  vsf_status st;
  if (k == 1) {
    if (nbytes < 4) return VSF_ERR_INVALID_ARG;
    VsfJpegPlan plan;
    st = vsf_jpeg_plan(files, sizes, 1, width, height, force_serial != 0, &plan);
  } else {
    VsfPngPlan plan;
    st = vsf_png_plan(files, sizes, 1, width, height, &plan);
  }
  if (st == VSF_OK && kind) *kind = k;
  return st;
}

}  // extern "C"
