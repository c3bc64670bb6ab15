// test_idct_reduced.cc -- stand-alone CPU program (tests/test_jpeg_idct_reduced.py): applies the reduced inverse DCTs of
// vision_slam_frontend_amd/csrc/vsf_jpeg_idct_reduced.h -- the header k_jpeg.hip's kernels include -- to quantised coefficient
// blocks and writes the cropped ceil(W / d) x ceil(H / d) image, so the test can hold it against what the system's libjpeg
// decodes from a file made of the same coefficients.  No GPU, no library of this project.
//     g++ -O2 -std=c++17 [-fsanitize=address,undefined] -I vision_slam_frontend_amd/csrc tests/cpp/test_idct_reduced.cc -o <out>
//     <out> cases.bin pixels.bin
// cases.bin:  int32 n_cases, then per case  int32 d, width, height;  uint16 qt[64];  int16 coef[blocks_y][blocks_x][64]
//             (natural order, blocks_* = ceil(size / 8));   pixels.bin: the images one after the other, rows packed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vsf_jpeg_idct_reduced.h"

template <int D>
static void decode(const std::vector<int16_t>& coef, const uint16_t* qt, int width, int height, std::vector<uint8_t>* out) {
  constexpr int S = 8 / D;
  const int bx = (width + 7) / 8, by = (height + 7) / 8, ow = (width + D - 1) / D, oh = (height + D - 1) / D;
  out->assign((size_t)ow * oh, 0);
  for (int y = 0; y < by; y++)
    for (int x = 0; x < bx; x++) {
      uint8_t px[S * S];
      vsf_idct::block_reduced<D>(&coef[((size_t)y * bx + x) * 64], qt, px);
      for (int r = 0; r < S && y * S + r < oh; r++)
        for (int c = 0; c < S && x * S + c < ow; c++) (*out)[(size_t)(y * S + r) * ow + x * S + c] = px[r * S + c];
    }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t n = 0;
  if (std::fread(&n, 4, 1, in) != 1 || n < 0 || n > 100000) return 3;
  for (int32_t i = 0; i < n; i++) {
    int32_t head[3];
    uint16_t qt[64];
    if (std::fread(head, 4, 3, in) != 3 || std::fread(qt, 2, 64, in) != 64) return 3;
    const int d = head[0], w = head[1], h = head[2];
    if (w < 1 || h < 1 || w > 4096 || h > 4096) return 3;
    std::vector<int16_t> coef((size_t)((w + 7) / 8) * ((h + 7) / 8) * 64);
    if (std::fread(coef.data(), 2, coef.size(), in) != coef.size()) return 3;
    std::vector<uint8_t> px;
    if (d == 2)
      decode<2>(coef, qt, w, h, &px);
    else if (d == 4)
      decode<4>(coef, qt, w, h, &px);
    else if (d == 8)
      decode<8>(coef, qt, w, h, &px);
    else
      return 3;
    if (std::fwrite(px.data(), 1, px.size(), out) != px.size()) return 4;
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 4;
}
