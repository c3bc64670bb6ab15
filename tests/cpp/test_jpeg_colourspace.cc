// The host half of the colour JPEG read (csrc/vsf_jpeg_host.cc: libjpeg's colour-space decision from the JFIF and Adobe markers
// and the component ids, the chroma quantisation tables, the refusals) as a stand-alone program on the CPU: compiled together
// with the host sources, plainly and under AddressSanitizer + UBSan (tests/test_jpeg_colourspace.py writes the files and a
// manifest, and judges what this program prints).
//   per file   vsf_plan_runs for a colour read (VSF_OUT_BGR) and for a gray one; an accepted plan is filled into a heap buffer of
//              exactly the planned bytes and read once
//              -> "file <index> <status colour> <status gray> <bytes colour> <bytes gray> <n_par colour> <n_prog colour>"
//   then       every file `rounds` times with a few bytes of its header (everything in front of the first scan's data) replaced
//              at random, through the colour plan: whatever the status, nothing may be read or written out of bounds
// manifest: one line per file, "<path> <width> <height>"; argv[2]: rounds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_internal.h"

struct File {
  std::vector<uint8_t> bytes;  // (exactly the file: a read past its end is a heap overflow the sanitizer sees)
  int w = 0, h = 0;
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

// -> status; *total: bytes of the upload, *sum: a checksum over every byte of it
static int plan_and_fill(const std::vector<uint8_t>& bytes, int w, int h, int out_format, size_t* total, uint32_t* sum,
                         int* n_par = nullptr, int* n_prog = nullptr) {
  const std::vector<uint8_t> copy(bytes);  // (a heap block of its own)
  const uint8_t* p = copy.data();
  const size_t n = copy.size();
  const uint8_t kind = VSF_FILE_JPEG;
  VsfDecodeRuns plan;
  *total = 0;
  const vsf_status st = vsf_plan_runs(&p, &n, &kind, 1, w, h, false, &plan, nullptr, out_format);
  if (st != VSF_OK) return (int)st;
  std::vector<uint8_t> blob(plan.total);
  vsf_fill_runs(plan, &p, blob.data());
  for (uint8_t b : blob) *sum = *sum * 16777619u ^ b;
  *total = plan.total;
  if (n_par) *n_par = plan.runs[0].jp.n_par;
  if (n_prog) *n_prog = plan.runs[0].jp.n_prog;
  return (int)VSF_OK;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: %s manifest rounds\n", argv[0]);
    return 2;
  }
  std::FILE* m = std::fopen(argv[1], "r");
  if (!m) return 2;
  const int rounds = std::atoi(argv[2]);
  std::vector<File> files;
  char path[4096];
  int w, h;
  while (std::fscanf(m, "%4095s %d %d", path, &w, &h) == 3) {
    files.emplace_back();
    files.back().w = w;
    files.back().h = h;
    if (!read_file(path, &files.back().bytes)) {
      std::printf("cannot read %s\n", path);
      return 2;
    }
  }
  std::fclose(m);
  uint32_t sum = 0;
  for (size_t i = 0; i < files.size(); i++) {
    size_t tc = 0, tg = 0;
    int n_par = -1, n_prog = -1;  // which decoder a colour read sends the file to
    const int sc = plan_and_fill(files[i].bytes, files[i].w, files[i].h, VSF_OUT_BGR, &tc, &sum, &n_par, &n_prog);
    const int sg = plan_and_fill(files[i].bytes, files[i].w, files[i].h, VSF_OUT_GRAY, &tg, &sum);
    std::printf("file %zu %d %d %zu %zu %d %d\n", i, sc, sg, tc, tg, n_par, n_prog);
  }
  uint32_t rng = 12345u;
  auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
  long accepted = 0, tried = 0;
  for (size_t i = 0; i < files.size(); i++) {
    size_t head = files[i].bytes.size();  // the header ends behind the first SOS segment
    for (size_t k = 2; k + 4 <= files[i].bytes.size(); k++)
      if (files[i].bytes[k] == 0xFF && files[i].bytes[k + 1] == 0xDA) {
        head = k + 2 + (((size_t)files[i].bytes[k + 2] << 8) | files[i].bytes[k + 3]);
        break;
      }
    if (head > files[i].bytes.size()) head = files[i].bytes.size();
    for (int r = 0; r < rounds; r++) {
      std::vector<uint8_t> b(files[i].bytes);
      const int edits = 1 + (int)(next() % 3);
      for (int e = 0; e < edits; e++) b[2 + next() % (head - 2)] = (uint8_t)next();
      if (next() % 8 == 0) b.resize(2 + next() % (b.size() - 2));  // ... or cut anywhere
      size_t t = 0;
      accepted += plan_and_fill(b, files[i].w, files[i].h, VSF_OUT_BGR, &t, &sum) == VSF_OK;
      tried++;
    }
  }
  std::printf("ok jpeg colourspace: %zu files, %ld of %ld mutated headers accepted, checksum %08x\n", files.size(), accepted, tried, sum);
  return 0;
}
