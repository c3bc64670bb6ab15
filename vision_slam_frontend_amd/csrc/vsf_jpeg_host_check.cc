// vsf_jpeg_host_check.cc -- entry points of the sanitizer build of the decoders' host half (make asan): a batch of files of
// one format goes through vsf_plan_runs + vsf_fill_runs -- the routines every device decode plans and fills its upload with --
// into a heap buffer of exactly the planned bytes (so that AddressSanitizer sees any write past the planned layout).
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vsf_internal.h"

namespace {

int host_check(const uint8_t* const* files, const size_t* nbytes, int n, uint8_t kind, int width, int height, bool force_serial,
               uint64_t* total_out, uint32_t* checksum_out) {
  if (total_out) *total_out = 0;
  if (checksum_out) *checksum_out = 0;
  const std::vector<uint8_t> kinds((size_t)(n > 0 ? n : 0), kind);
  VsfDecodeRuns plan;
  const vsf_status st = vsf_plan_runs(files, nbytes, kinds.data(), n, width, height, force_serial, &plan);
  if (st != VSF_OK) return (int)st;
  std::vector<uint8_t> blob(plan.total);
  vsf_fill_runs(plan, files, blob.data());
  // (self-test of the harness: with this variable set the function writes one byte past its buffer, which the sanitizer
  // must catch -- tests/test_jpeg_host_asan.py checks that it does, i.e. that the instrumentation is live)
  if (kind == VSF_FILE_JPEG && std::getenv("VSF_ASAN_SELFTEST")) {
    volatile uint8_t* past = blob.data() + blob.size();
    *past = 1;
  }
  uint32_t sum = 0;
  for (uint8_t b : blob) sum = sum * 16777619u ^ b;  // (every byte of the upload is read once)
  if (total_out) *total_out = plan.total;
  if (checksum_out) *checksum_out = sum;
  return (int)VSF_OK;
}

}  // namespace

extern "C" int vsf_jpeg_host_check(const uint8_t* const* jpeg, const size_t* nbytes, int n, int width, int height,
                                   int force_serial, uint64_t* total_out, uint32_t* checksum_out) {
  return host_check(jpeg, nbytes, n, VSF_FILE_JPEG, width, height, force_serial != 0, total_out, checksum_out);
}

extern "C" int vsf_png_host_check(const uint8_t* const* png, const size_t* nbytes, int n, int width, int height,
                                  uint64_t* total_out, uint32_t* checksum_out) {
  return host_check(png, nbytes, n, VSF_FILE_PNG, width, height, false, total_out, checksum_out);
}
