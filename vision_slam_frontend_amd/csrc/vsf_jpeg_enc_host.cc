// vsf_jpeg_enc_host.cc -- host half of the baseline JPEG encoder: quality -> quantisation tables (jcparam.c
// jpeg_set_quality / jpeg_add_quant_table), the marker segments libjpeg writes in front of the scan (jcmarker.c write_file_header /
// write_frame_header / write_scan_header as cv::imencode(".jpg") of OpenCV 3.2 sets the encoder up: JFIF 1.01, baseline, the
// standard Huffman tables, no restart interval) and the size bound.  No device code: the CPU tests and the sanitizer build use
// this file as it is.
#include "vsf_jpeg_enc_host.h"

#include <string.h>

#include "../../include/vsf.h"

namespace {

// Annex K.1, natural order
const uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: code counts per length 1..16, then the symbols
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct Writer {
  uint8_t* p;
  int n = 0;
  void u8(int v) { p[n++] = (uint8_t)v; }
  void u16(int v) {
    u8(v >> 8);
    u8(v & 255);
  }
  void marker(int m) {
    u8(0xFF);
    u8(m);
  }
};

void emit_dht(Writer& w, int index, const uint8_t bits[16], const uint8_t* vals) {
  int count = 0;
  for (int i = 0; i < 16; i++) count += bits[i];
  w.marker(0xC4);
  w.u16(2 + 1 + 16 + count);
  w.u8(index);
  for (int i = 0; i < 16; i++) w.u8(bits[i]);
  for (int i = 0; i < count; i++) w.u8(vals[i]);
}

// jchuff.c jpeg_make_c_derived_tbl: codes in order of length, counting up
template <class T>
void derive(const uint8_t bits[16], const uint8_t* vals, T* out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; len++) {
    for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = (T)(code++ << 5 | (uint32_t)len);
    code <<= 1;
  }
}

}  // namespace

void vsf_jpeg_enc_quant(int quality, uint16_t quant[2][64]) {
  if (quality <= 0) quality = 1;  // jpeg_quality_scaling
  if (quality > 100) quality = 100;
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 64; i++) {
      long v = ((long)kStdQuant[t][i] * scale + 50L) / 100L;
      if (v <= 0) v = 1;
      if (v > 255) v = 255;  // force_baseline
      quant[t][i] = (uint16_t)v;
    }
}

void vsf_jpeg_enc_codes(VsfJpegEncTables* t) {
  memset(t->dc_code, 0, sizeof(t->dc_code));
  memset(t->ac_code, 0, sizeof(t->ac_code));
  for (int i = 0; i < 2; i++) {
    derive(kDcBits[i], kDcVals, t->dc_code[i]);
    derive(kAcBits[i], kAcVals[i], t->ac_code[i]);
  }
}

int vsf_jpeg_enc_header(int width, int height, int channels, int quality, uint8_t out[VSF_JPEG_ENC_HEADER_MAX]) {
  uint16_t quant[2][64];
  vsf_jpeg_enc_quant(quality, quant);
  const int ncomp = channels == 3 ? 3 : 1, ntab = ncomp == 3 ? 2 : 1;
  Writer w{out};
  w.marker(0xD8);
  w.marker(0xE0);  // JFIF 1.01, no units, 1:1, no thumbnail
  w.u16(16);
  for (const char* c = "JFIF"; *c; c++) w.u8(*c);
  w.u8(0);
  w.u8(1);
  w.u8(1);
  w.u8(0);
  w.u16(1);
  w.u16(1);
  w.u8(0);
  w.u8(0);
  for (int t = 0; t < ntab; t++) {
    w.marker(0xDB);
    w.u16(64 + 1 + 2);
    w.u8(t);
    for (int i = 0; i < 64; i++) w.u8(quant[t][kZigzag[i]]);
  }
  w.marker(0xC0);
  w.u16(3 * ncomp + 2 + 5 + 1);
  w.u8(8);
  w.u16(height);
  w.u16(width);
  w.u8(ncomp);
  for (int c = 0; c < ncomp; c++) {
    w.u8(c + 1);
    w.u8(ncomp == 3 && c == 0 ? 0x22 : 0x11);
    w.u8(c ? 1 : 0);
  }
  for (int t = 0; t < ntab; t++) {
    emit_dht(w, t, kDcBits[t], kDcVals);
    emit_dht(w, t | 0x10, kAcBits[t], kAcVals[t]);
  }
  w.marker(0xDA);
  w.u16(2 * ncomp + 2 + 1 + 3);
  w.u8(ncomp);
  for (int c = 0; c < ncomp; c++) {
    w.u8(c + 1);
    w.u8(c ? 0x11 : 0x00);
  }
  w.u8(0);
  w.u8(63);
  w.u8(0);
  return w.n;
}

size_t vsf_jpeg_enc_blocks(int width, int height, int channels) {
  if (channels == 3) return (size_t)((width + 15) / 16) * (size_t)((height + 15) / 16) * 6;
  return (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
}

extern "C" {

// Header + every block at its longest, every scan byte an FF that takes a stuffed 00, the final padding byte, EOI.
size_t vsf_jpeg_encode_capacity(int width, int height, int channels) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || (channels != 1 && channels != 3)) return 0;
  return VSF_JPEG_ENC_HEADER_MAX + vsf_jpeg_enc_blocks(width, height, channels) * (2 * VSF_JPEG_ENC_BLOCK_BYTES) + 16;
}

vsf_status vsf_debug_jpeg_encode_header(int width, int height, int channels, int quality, uint8_t* out, size_t cap,
                                        size_t* n_bytes) {
  if (!out || !n_bytes || width < 1 || height < 1 || width > 65535 || height > 65535 || (channels != 1 && channels != 3) ||
      quality < 0 || quality > 100)
    return VSF_ERR_INVALID_ARG;
  uint8_t buf[VSF_JPEG_ENC_HEADER_MAX];
  const int n = vsf_jpeg_enc_header(width, height, channels, quality ? quality : 95, buf);
  *n_bytes = (size_t)n;
  if ((size_t)n > cap) return VSF_ERR_CAPACITY;
  memcpy(out, buf, (size_t)n);
  return VSF_OK;
}

}  // extern "C"
