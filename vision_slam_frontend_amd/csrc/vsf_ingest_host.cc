// vsf_ingest_host.cc -- the host half of "decode these files on the device", shared by the C ABI's decoders and the
// ObserveImage queue: the format by the file's first bytes (as cv::imdecode's findDecoder does), the runs of one format in a
// list of files, the plan of ONE upload for all of them (vsf_jpeg_plan / vsf_png_plan per run: every marker, table and chunk
// length) and its fill.  And what vsf_observe_submit_compressed does with a payload before anything is booked: the staging
// ring's sizes, the per-file byte cap and the same plan for the ONE file.  The bytes are UNTRUSTED (slam_frontend_main.cc:98-100
// hands cv::imdecode whatever the topic carried).  Plain C++, no HIP call: the same translation unit is part of the sanitizer
// build (make asan) and needs no device.
#include <cstring>

#include "vsf_internal.h"
#include "vsf_png_host.h"

int vsf_file_kind(const uint8_t* file, size_t nbytes) {
  if (!file) return VSF_FILE_NONE;
  if (nbytes >= 8 && std::memcmp(file, vsf_png::kSignature, 8) == 0) return VSF_FILE_PNG;
  if (nbytes >= 3 && file[0] == 0xFF && file[1] == 0xD8 && file[2] == 0xFF) return VSF_FILE_JPEG;  // (SOI + a marker)
  return VSF_FILE_NONE;  // (imdecode's other formats -- BMP, TIFF, WebP ... -- are not built)
}

int vsf_run_end(const uint8_t* kinds, int n, int i0) {
  int i1 = i0 + 1;
  while (i1 < n && kinds[i1] == kinds[i0]) ++i1;
  return i1;
}

// Every run of JPEG or PNG files among files [0, n) planned as one upload of its own, the uploads one after the other at
// 256-byte-aligned offsets of ONE blob of out->total bytes.  The first refusal of a decoder's host half is returned as it is.
// reduces[i] > 1: file i decodes at 1 / reduces[i] into width x height (JPEG only: imdecode would resize a PNG); a run is
// files of one format AND one denominator.
vsf_status vsf_plan_runs(const uint8_t* const* files, const size_t* nbytes, const uint8_t* kinds, int n, int width, int height,
                         bool force_serial, VsfDecodeRuns* out, const uint8_t* reduces, int out_format) {
  out->runs.clear();
  out->total = 0;
  if (out_format != VSF_OUT_GRAY && out_format != VSF_OUT_BGR) return VSF_ERR_INVALID_ARG;
  const bool bgr = out_format == VSF_OUT_BGR;
  for (int i0 = 0, i1; i0 < n; i0 = i1) {
    i1 = vsf_run_end(kinds, n, i0);
    if (kinds[i0] == VSF_FILE_NONE) continue;
    const int reduce = reduces ? reduces[i0] : 1;
    if (!vsf_reduce_ok(reduce)) return VSF_ERR_INVALID_ARG;
    if (reduces)
      for (int i = i0 + 1; i < i1; i++)
        if (reduces[i] != reduces[i0]) i1 = i;
    out->runs.emplace_back();
    VsfDecodeRun& r = out->runs.back();
    r.i0 = i0;
    r.n = i1 - i0;
    r.kind = kinds[i0];
    r.off = (out->total + 255) & ~(size_t)255;
    if (r.kind == VSF_FILE_PNG && reduce > 1) return VSF_ERR_UNSUPPORTED;
    if (bgr && reduce > 1) return VSF_ERR_UNSUPPORTED;  // (no reduced colour decode)
    const vsf_status st = r.kind == VSF_FILE_JPEG ? vsf_jpeg_plan(files + i0, nbytes + i0, r.n, width, height, force_serial, &r.jp, reduce, bgr)
                                                  : vsf_png_plan(files + i0, nbytes + i0, r.n, width, height, &r.pp, bgr);
    if (st != VSF_OK) return st;
    out->total = r.off + (r.kind == VSF_FILE_JPEG ? r.jp.total : r.pp.total);
  }
  return VSF_OK;
}

void vsf_fill_runs(const VsfDecodeRuns& plan, const uint8_t* const* files, uint8_t* dst) {
  for (const VsfDecodeRun& r : plan.runs) {
    if (r.kind == VSF_FILE_JPEG)
      vsf_jpeg_fill(r.jp, files + r.i0, r.n, dst + r.off);
    else
      vsf_png_fill(r.pp, files + r.i0, r.n, dst + r.off);
  }
}

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
  if (!file || !width || !height) return VSF_ERR_INVALID_ARG;
  *width = *height = 0;
  uint32_t w = 0, h = 0;
  const int kind = vsf_file_kind(file, nbytes);
  if (kind == VSF_FILE_PNG) {
    if (nbytes < 24 || std::memcmp(file + 12, "IHDR", 4) != 0) return VSF_ERR_INVALID_ARG;
    w = ((uint32_t)file[16] << 24) | ((uint32_t)file[17] << 16) | ((uint32_t)file[18] << 8) | file[19];
    h = ((uint32_t)file[20] << 24) | ((uint32_t)file[21] << 16) | ((uint32_t)file[22] << 8) | file[23];
  } else if (kind == VSF_FILE_JPEG) {
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

}  // extern "C"

// The component count of a JPEG file's frame header -- the first SOF0 / SOF1 / SOF2 segment, reached by the walk of
// vsf_compressed_image_size above; vsf_jpeg_plan takes its ncomp from the same segment and refuses a second one.  0: no such
// segment in front of the data.
int vsf_jpeg_frame_components(const uint8_t* file, size_t nbytes) {
  if (vsf_file_kind(file, nbytes) != VSF_FILE_JPEG) return 0;
  size_t pos = 2;
  while (pos + 4 <= nbytes) {
    if (file[pos] != 0xFF) return 0;
    while (pos < nbytes && file[pos] == 0xFF) pos++;
    if (pos >= nbytes) return 0;
    const int m = file[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9 || m == 0xDA || pos + 2 > nbytes) return 0;
    const size_t len = ((size_t)file[pos] << 8) | file[pos + 1];
    if (len < 2 || len > nbytes - pos) return 0;
    if (m >= 0xC0 && m <= 0xC2) return len >= 8 ? file[pos + 7] : 0;
    pos += len;
  }
  return 0;
}

extern "C" {

// What libjpeg's jpeg_calc_output_dimensions makes of w x h at scale 1 / reduce -- the size cv::imdecode returns for
// IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8 (reduce = 1: the size itself).
vsf_status vsf_reduced_size(int w, int h, int reduce, int* rw, int* rh) {
  if (rw) *rw = 0;
  if (rh) *rh = 0;
  if (!rw || !rh || w < 1 || h < 1 || !vsf_reduce_ok(reduce)) return VSF_ERR_INVALID_ARG;
  *rw = (int)(((long long)w + reduce - 1) / reduce);
  *rh = (int)(((long long)h + reduce - 1) / reduce);
  return VSF_OK;
}

vsf_status vsf_observe_probe_compressed(const uint8_t* file, size_t nbytes, int width, int height, size_t cap_per_image,
                                        int force_serial, int* kind) {
  return vsf_observe_probe_compressed_reduced(file, nbytes, 1, width, height, cap_per_image, force_serial, kind);
}

vsf_status vsf_observe_probe_compressed_reduced(const uint8_t* file, size_t nbytes, int reduce, int width, int height,
                                                size_t cap_per_image, int force_serial, int* kind) {
  if (kind) *kind = VSF_FILE_NONE;
  if (!vsf_reduce_ok(reduce)) return VSF_ERR_INVALID_ARG;
  if (!file || width < 1 || height < 1 || width > 65535 || height > 65535) return VSF_ERR_INVALID_ARG;
  const uint8_t k = (uint8_t)vsf_file_kind(file, nbytes);
  if (k == VSF_FILE_NONE) return VSF_ERR_UNSUPPORTED;
  if (nbytes > cap_per_image || nbytes > 0x40000000u) return VSF_ERR_CAPACITY;
  if (k == VSF_FILE_JPEG && nbytes < 4) return VSF_ERR_INVALID_ARG;
  VsfDecodeRuns plan;
  const uint8_t d = (uint8_t)reduce;
  const vsf_status st = vsf_plan_runs(&file, &nbytes, &k, 1, width, height, force_serial != 0, &plan, &d);
  if (st == VSF_OK && kind) *kind = k;
  return st;
}

}  // extern "C"
