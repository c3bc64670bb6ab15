// The host half of the JPEG decode (csrc/vsf_jpeg_host.cc) on files of every sampling layout the parser accepts and of the ones
// it refuses, as a stand-alone program on the CPU: compiled together with the host sources, plainly and under AddressSanitizer +
// UBSan (tests/test_jpeg_sampling_plan.py writes the files and a manifest, and judges what this program prints).
//   per file    vsf_jpeg_plan alone at reduce 1, 2, 4, 8, with and without force_serial; the upload is filled into a heap buffer
//               of exactly the planned bytes (vsf_jpeg_fill) and read once
//               -> "file <index> <reduce> <serial> <status> <n_par> <n_prog> <max_luma_blocks> <mcus_x> <mcus_y>"
//   per batch   the accepted files of one size through vsf_jpeg_host_check (vsf_plan_runs + vsf_fill_runs into an exactly
//               sized buffer) -> "batch <w> <h> <n> <serial> <status> <total>"
// manifest: one line per file, "<path> <width> <height> <batch: 0 / 1>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_internal.h"
#include "../../vision_slam_frontend_amd/csrc/vsf_jpeg_host.h"

extern "C" int vsf_jpeg_host_check(const uint8_t* const* jpeg, const size_t* nbytes, int n, int width, int height, int force_serial,
                                   uint64_t* total_out, uint32_t* checksum_out);

struct File {
  std::vector<uint8_t> bytes;  // (exactly the file: a read past its end is a heap overflow the sanitizer sees)
  int w = 0, h = 0, batch = 0;
};

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out->resize((size_t)(n > 0 ? n : 0));
  const bool ok = n > 0 && std::fread(out->data(), 1, (size_t)n, f) == (size_t)n;
  std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s manifest\n", argv[0]);
    return 2;
  }
  std::FILE* m = std::fopen(argv[1], "r");
  if (!m) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<File> files;
  char path[4096];
  int w, h, batch;
  while (std::fscanf(m, "%4095s %d %d %d", path, &w, &h, &batch) == 4) {
    files.emplace_back();
    files.back().w = w;
    files.back().h = h;
    files.back().batch = batch;
    if (!read_file(path, &files.back().bytes)) {
      std::printf("cannot read %s\n", path);
      return 2;
    }
  }
  std::fclose(m);
  uint32_t sum = 0;
  for (size_t i = 0; i < files.size(); i++) {
    const File& f = files[i];
    const uint8_t* p = f.bytes.data();
    const size_t n = f.bytes.size();
    for (int reduce : {1, 2, 4, 8})
      for (int serial = 0; serial < 2; serial++) {
        VsfJpegPlan plan;
        const vsf_status st = vsf_jpeg_plan(&p, &n, 1, (f.w + reduce - 1) / reduce, (f.h + reduce - 1) / reduce, serial != 0, &plan, reduce);
        if (st != VSF_OK) {
          std::printf("file %zu %d %d %d 0 0 0 0 0\n", i, reduce, serial, (int)st);
          continue;
        }
        std::vector<uint8_t> blob(plan.total);
        vsf_jpeg_fill(plan, &p, 1, blob.data());
        for (uint8_t b : blob) sum = sum * 16777619u ^ b;
        vsf_jpeg::DevImage im;
        std::memcpy(&im, blob.data() + plan.off_images, sizeof(im));
        std::printf("file %zu %d %d %d %d %d %d %d %d\n", i, reduce, serial, (int)st, plan.n_par, plan.n_prog, plan.max_luma_blocks,
                    (int)im.mcus_x, (int)im.mcus_y);
      }
  }
  std::map<std::pair<int, int>, std::vector<size_t>> by_size;
  for (size_t i = 0; i < files.size(); i++)
    if (files[i].batch) by_size[{files[i].w, files[i].h}].push_back(i);
  for (const auto& kv : by_size) {
    std::vector<const uint8_t*> ptrs;
    std::vector<size_t> sizes;
    for (size_t i : kv.second) {
      ptrs.push_back(files[i].bytes.data());
      sizes.push_back(files[i].bytes.size());
    }
    for (int serial = 0; serial < 2; serial++) {
      uint64_t total = 0;
      uint32_t check = 0;
      const int st = vsf_jpeg_host_check(ptrs.data(), sizes.data(), (int)ptrs.size(), kv.first.first, kv.first.second, serial, &total, &check);
      sum ^= check;
      std::printf("batch %d %d %zu %d %d %llu\n", kv.first.first, kv.first.second, ptrs.size(), serial, st, (unsigned long long)total);
    }
  }
  std::printf("ok jpeg sampling plan: %zu files, checksum %08x\n", files.size(), sum);
  return 0;
}
