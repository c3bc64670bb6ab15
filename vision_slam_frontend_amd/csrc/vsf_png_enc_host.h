// vsf_png_enc_host.h -- host half of the PNG encoder (k_png_enc.hip): what cv::imencode(".png") of OpenCV 3.2 makes libpng 1.6 write
// around the deflate stream (signature, IHDR, IEND, the two zlib header bytes with libpng's window rule, the filter type), the size
// bound, and the CRC-32 constants the device needs.  Plain C++.
#ifndef VSF_PNG_ENC_HOST_H_
#define VSF_PNG_ENC_HOST_H_

#include <stddef.h>
#include <stdint.h>

#define VSF_PNG_ENC_HEADER_BYTES 33   // signature + IHDR chunk
#define VSF_PNG_ENC_IDAT 8192         // libpng's zbuffer_size: bytes of every IDAT chunk but the last
#define VSF_PNG_ENC_BLOCK_SYMS 16383  // zlib's lit_bufsize - 1 at memLevel 8: a deflate block ends when that many symbols are tallied
// CRC of a chunk in one pass: the chunk's type + data, right-aligned in VSF_PNG_ENC_CRC_LANES segments of VSF_PNG_ENC_CRC_SEG bytes
#define VSF_PNG_ENC_CRC_LANES 256
#define VSF_PNG_ENC_CRC_SEG 36        // 256 * 36 = 9216 >= 4 + 8192

// What travels to the kernels by value.
struct VsfPngEncConsts {
  uint32_t crc_table[256];                      // the reflected CRC-32 table (polynomial EDB88320)
  uint32_t seg_mul[VSF_PNG_ENC_CRC_LANES];      // x^(8 * SEG * k) mod P: advances a CRC register over k segments
  uint32_t pow_mul[16];                         // x^(8 * 2^k) mod P: advances it over 2^k bytes
  uint8_t header[VSF_PNG_ENC_HEADER_BYTES + 3]; // signature + IHDR
  uint8_t zhdr[2];                              // CMF, FLG of the zlib stream
  uint8_t filter;                               // the filter byte in front of every row: 1 (Sub), 0 where libpng falls back
};

// a * b mod P in the reflected representation (bit 31 is x^0)
uint32_t vsf_png_enc_mulmod(uint32_t a, uint32_t b);
void vsf_png_enc_consts(int width, int height, int channels, VsfPngEncConsts* c);
// Bytes of the filtered image: (width * channels + 1) * height.
uint64_t vsf_png_enc_filtered_bytes(int width, int height, int channels);
// An upper bound of the zlib stream for n filtered bytes: every block stored (see the .cc).
uint64_t vsf_png_enc_stream_bound(uint64_t n_filtered);
// signature + IHDR -> 33 bytes
void vsf_png_enc_header(int width, int height, int channels, uint8_t out[VSF_PNG_ENC_HEADER_BYTES]);
// the zlib header for an image of n filtered bytes (libpng's png_deflate_claim + optimize_cmf)
void vsf_png_enc_zlib_header(uint64_t n_filtered, uint8_t out[2]);
// The filter type libpng writes when asked for PNG_FILTER_SUB alone.
int vsf_png_enc_filter_type(int width, int height);
// The whole encoder on the CPU, built from the same per-block code the kernels run (vsf_png_enc_trees.h): -> the file's size, 0
// when it does not fit cap.  For tests without a GPU.
size_t vsf_png_enc_cpu(const uint8_t* src, int width, int height, int channels, size_t row_stride, uint8_t* out, size_t cap);

#endif  // VSF_PNG_ENC_HOST_H_
