// vsf_jpeg_enc_host.h -- host half of the baseline JPEG encoder (k_jpeg_enc.hip): what cv::imencode(".jpg") of OpenCV 3.2
// makes libjpeg write around the entropy-coded segment, and the tables the device needs to write that segment.  Plain C++.
#ifndef VSF_JPEG_ENC_HOST_H_
#define VSF_JPEG_ENC_HOST_H_

#include <stddef.h>
#include <stdint.h>

#define VSF_JPEG_ENC_HEADER_MAX 640  // SOI .. SOS header: 328 bytes with one component, 623 with three
// Scan bytes one 8x8 block can take before stuffing: a DC code (<= 11 bits) + 11 magnitude bits and 63 AC codes of <= 16 bits
// + 10 magnitude bits = 1660 bits.
#define VSF_JPEG_ENC_BLOCK_BYTES 208

// What travels to the kernels by value.
struct VsfJpegEncTables {
  uint16_t quant[2][64];   // luminance / chrominance quantisers, natural (row-major) order
  uint32_t recip[2][64];   // ceil(2^32 / (quantiser << 3)): the device divides by multiplying (filled by the launcher)
  uint16_t dc_code[2][12]; // Huffman code of DC size category s: code << 5 | length
  uint32_t ac_code[2][256];  // ... of AC symbol run << 4 | size: code << 5 | length (0: not in the table)
};
struct VsfJpegEncHeader {
  uint8_t bytes[VSF_JPEG_ENC_HEADER_MAX];
  int32_t len;
};

// jpeg_set_quality(quality, TRUE): the two standard tables (Annex K.1) scaled and clamped to 1..255.  quality 1..100.
void vsf_jpeg_enc_quant(int quality, uint16_t quant[2][64]);
// The standard Huffman tables (Annex K.3) as code words.
void vsf_jpeg_enc_codes(VsfJpegEncTables* t);
// SOI, JFIF APP0, DQT(s), SOF0, DHT(s), SOS: every byte in front of the entropy-coded segment.  -> its length.
int vsf_jpeg_enc_header(int width, int height, int channels, int quality, uint8_t out[VSF_JPEG_ENC_HEADER_MAX]);
// Blocks of one image's scan: ceil(w/8) ceil(h/8) with one component, 6 per 16x16 MCU with three (4:2:0).
size_t vsf_jpeg_enc_blocks(int width, int height, int channels);

#endif  // VSF_JPEG_ENC_HOST_H_
