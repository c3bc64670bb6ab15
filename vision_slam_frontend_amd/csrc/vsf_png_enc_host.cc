// vsf_png_enc_host.cc -- host half of the PNG encoder: the bytes cv::imencode(".png", img) of OpenCV 3.2 makes libpng 1.6 write around
// the deflate stream, libpng's window rule for the zlib header, the filter type it falls back to, the size bound, the CRC-32
// constants of the device, and the whole encoder on the CPU (vsf_png_enc_cpu: the per-block code of vsf_png_enc_trees.h driven
// serially), which the tests without a GPU compare with the real library.  Plain C++: part of the sanitizer build.
#include "vsf_png_enc_host.h"

#include <string.h>

#include <vector>

#include "../../include/vsf.h"
#include "vsf_png_enc_trees.h"

namespace {

constexpr uint32_t kPoly = 0xEDB88320u;

void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

uint32_t crc_update(const uint32_t* table, uint32_t reg, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) reg = table[(reg ^ p[i]) & 255u] ^ (reg >> 8);
  return reg;
}

void crc_table(uint32_t table[256]) {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
    table[i] = c;
  }
}

bool good(int width, int height, int channels) {
  return width >= 1 && height >= 1 && width <= 65535 && height <= 65535 && (channels == 1 || channels == 3);
}

}  // namespace

uint32_t vsf_png_enc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m != 0; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}

int vsf_png_enc_filter_type(int width, int height) {
  // png_write_start_row: an image one pixel wide has nothing to the left of any byte, and libpng drops Sub from the filters it
  // may use; with nothing left it writes type 0
  (void)height;
  return width == 1 ? 0 : 1;
}

uint64_t vsf_png_enc_filtered_bytes(int width, int height, int channels) {
  return ((uint64_t)width * (uint64_t)channels + 1u) * (uint64_t)height;
}

uint64_t vsf_png_enc_stream_bound(uint64_t n) {
  // A block of `len` bytes takes at most 3 + 7 + 32 + 8 len bits stored (header, padding, LEN / NLEN); zlib writes another form
  // only when (bits + 3 + 7) / 8 < len + 4, so at most 8 len + 42 bits: under len + 6 bytes.  A block ends after 16383 symbols
  // and a symbol covers at least a byte: at most n / 16383 + 1 blocks.  Around them 2 header bytes, the last byte's padding
  // (counted in the blocks) and the Adler-32.
  return 2 + n + 6 * (n / VSF_PNG_ENC_BLOCK_SYMS + 1) + 4;
}

void vsf_png_enc_header(int width, int height, int channels, uint8_t out[VSF_PNG_ENC_HEADER_BYTES]) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  uint32_t table[256];
  crc_table(table);
  memcpy(out, sig, 8);
  put_be32(out + 8, 13);
  memcpy(out + 12, "IHDR", 4);
  put_be32(out + 16, (uint32_t)width);
  put_be32(out + 20, (uint32_t)height);
  out[24] = 8;                          // bit depth
  out[25] = channels == 1 ? 0 : 2;      // colour type: gray / RGB
  out[26] = out[27] = out[28] = 0;      // compression, filter method, no interlace
  put_be32(out + 29, ~crc_update(table, 0xFFFFFFFFu, out + 12, 17));
}

void vsf_png_enc_zlib_header(uint64_t n, uint8_t out[2]) {
  // png_deflate_claim: for at most 16384 bytes the window asked of zlib is halved while the data plus 262 bytes fits half of it;
  // optimize_cmf (when the first IDAT leaves): CINFO goes down further while the data fits half of that window
  unsigned cinfo = 7;
  if (n <= 16384) {
    unsigned half = 1u << 14;
    while (n + 262 <= half) {
      half >>= 1;
      cinfo--;
    }
    half = 1u << (cinfo + 7);
    if (n <= half) {
      do {
        half >>= 1;
        cinfo--;
      } while (cinfo > 0 && n <= half);
    }
  }
  const unsigned cmf = (cinfo << 4) | 8u;
  out[0] = (uint8_t)cmf;
  out[1] = (uint8_t)(31u - (cmf << 8) % 31u);  // FLEVEL 0 (level 1), no dictionary
}

void vsf_png_enc_consts(int width, int height, int channels, VsfPngEncConsts* c) {
  memset(c, 0, sizeof(*c));
  crc_table(c->crc_table);
  // x^8 = the register after one zero byte from x^0 (0x80000000)
  const uint32_t x8 = crc_update(c->crc_table, 0x80000000u, (const uint8_t*)"\0", 1);
  uint32_t p = x8;
  for (int k = 0; k < 16; k++) {
    c->pow_mul[k] = p;
    p = vsf_png_enc_mulmod(p, p);
  }
  uint32_t seg = 0x80000000u;  // x^(8 * SEG)
  for (int k = 0, n = VSF_PNG_ENC_CRC_SEG; n; k++, n >>= 1)
    if (n & 1) seg = vsf_png_enc_mulmod(seg, c->pow_mul[k]);
  uint32_t m = 0x80000000u;
  for (int k = 0; k < VSF_PNG_ENC_CRC_LANES; k++) {
    c->seg_mul[k] = m;
    m = vsf_png_enc_mulmod(m, seg);
  }
  vsf_png_enc_header(width, height, channels, c->header);
  vsf_png_enc_zlib_header(vsf_png_enc_filtered_bytes(width, height, channels), c->zhdr);
  c->filter = (uint8_t)vsf_png_enc_filter_type(width, height);
}

size_t vsf_png_enc_cpu(const uint8_t* src, int width, int height, int channels, size_t row_stride, uint8_t* out, size_t cap) {
  VsfPngEncConsts k;
  vsf_png_enc_consts(width, height, channels, &k);
  const size_t rowbytes = (size_t)width * (size_t)channels, n = (rowbytes + 1) * (size_t)height;
  std::vector<uint8_t> f(n);
  for (int y = 0; y < height; y++) {
    const uint8_t* row = src + (size_t)y * row_stride;
    uint8_t* d = f.data() + (size_t)y * (rowbytes + 1);
    d[0] = k.filter;
    for (size_t x = 0; x < rowbytes; x++) {
      const size_t px = x / (size_t)channels, comp = x % (size_t)channels;
      const size_t at = px * (size_t)channels + ((size_t)channels - 1 - comp);  // B G R in memory, R G B in the file
      d[1 + x] = (uint8_t)(row[at] - (k.filter == 1 && px > 0 ? row[at - (size_t)channels] : 0));
    }
  }
  // the symbols: run by run
  std::vector<uint16_t> sym;
  std::vector<size_t> pos;  // where each symbol starts
  for (size_t s = 0; s < n;) {
    size_t e = s + 1;
    while (e < n && f[e] == f[s]) e++;
    for (size_t p = s; p < e; p++) {
      const uint32_t v = vsf_pe_symbol((uint32_t)(p - s), (uint32_t)(e - s));
      if (v == 0) continue;
      sym.push_back(v == 1 ? (uint16_t)f[p] : (uint16_t)(256 + v - 3));
      pos.push_back(p);
    }
    s = e;
  }
  std::vector<uint8_t> z((size_t)vsf_png_enc_stream_bound(n) + 16, 0);
  uint64_t bit = 16;
  z[0] = k.zhdr[0];
  z[1] = k.zhdr[1];
  auto put = [&](uint64_t v, int len) {
    for (int i = 0; i < len; i++, bit++) z[bit >> 3] |= (uint8_t)(((v >> i) & 1u) << (bit & 7u));
  };
  const size_t blocks = sym.size() / VSF_PNG_ENC_BLOCK_SYMS + 1;
  std::vector<VsfPeWork> work(1);
  std::vector<VsfPePlan> plan(1);
  for (size_t b = 0; b < blocks; b++) {
    const size_t s0 = b * VSF_PNG_ENC_BLOCK_SYMS, s1 = b + 1 == blocks ? sym.size() : s0 + VSF_PNG_ENC_BLOCK_SYMS;
    const size_t p0 = s0 < sym.size() ? pos[s0] : n, p1 = s1 < sym.size() ? pos[s1] : n;
    VsfPeWork& w = work[0];
    for (int i = 0; i < VSF_PE_L_CODES; i++) w.freq[i] = 0;
    uint32_t matches = 0;
    for (size_t i = s0; i < s1; i++) {
      if (sym[i] < 256) {
        w.freq[sym[i]]++;
      } else {
        int extra;
        uint32_t value;
        w.freq[257 + vsf_pe_length_code(sym[i] - 256u, &extra, &value)]++;
        matches++;
      }
    }
    w.freq[256] = 1;
    vsf_pe_plan_block(w, matches, (uint32_t)(p1 - p0), b + 1 == blocks, &plan[0]);
    const VsfPePlan& pl = plan[0];
    for (uint32_t i = 0; i < pl.hdr_bits; i += 32) put(pl.hdr[i >> 5], pl.hdr_bits - i < 32 ? (int)(pl.hdr_bits - i) : 32);
    if (pl.type == 0) {
      bit = (bit + 7) & ~(uint64_t)7;
      const uint32_t len = (uint32_t)(p1 - p0);
      put(len & 0xFFFFu, 16);
      put(~len & 0xFFFFu, 16);
      for (size_t p = p0; p < p1; p++) put(f[p], 8);
    } else {
      for (size_t i = s0; i <= s1; i++) {
        uint64_t bits;
        const int nb = vsf_pe_symbol_bits(pl.lcode, pl.dcode0, i == s1 ? 512u : sym[i], &bits);
        put(bits, nb);
      }
    }
  }
  bit = (bit + 7) & ~(uint64_t)7;
  uint32_t a = 1, bsum = 0;
  for (size_t i = 0; i < n; i++) {
    a = (a + f[i]) % 65521u;
    bsum = (bsum + a) % 65521u;
  }
  size_t zn = (size_t)(bit >> 3);
  put_be32(z.data() + zn, bsum << 16 | a);
  zn += 4;
  const size_t chunks = (zn + VSF_PNG_ENC_IDAT - 1) / VSF_PNG_ENC_IDAT;
  const size_t total = VSF_PNG_ENC_HEADER_BYTES + zn + 12 * chunks + 12;
  if (total > cap) return 0;
  memcpy(out, k.header, VSF_PNG_ENC_HEADER_BYTES);
  uint8_t* o = out + VSF_PNG_ENC_HEADER_BYTES;
  for (size_t c = 0; c <= chunks; c++) {  // the last round writes IEND
    const size_t len = c == chunks ? 0 : (zn - c * VSF_PNG_ENC_IDAT < VSF_PNG_ENC_IDAT ? zn - c * VSF_PNG_ENC_IDAT : VSF_PNG_ENC_IDAT);
    put_be32(o, (uint32_t)len);
    memcpy(o + 4, c == chunks ? "IEND" : "IDAT", 4);
    if (len) memcpy(o + 8, z.data() + c * VSF_PNG_ENC_IDAT, len);
    put_be32(o + 8 + len, ~crc_update(k.crc_table, 0xFFFFFFFFu, o + 4, 4 + len));
    o += 12 + len;
  }
  return total;
}

extern "C" {

size_t vsf_png_encode_capacity(int width, int height, int channels) {
  if (!good(width, height, channels)) return 0;
  const uint64_t z = vsf_png_enc_stream_bound(vsf_png_enc_filtered_bytes(width, height, channels));
  return (size_t)(VSF_PNG_ENC_HEADER_BYTES + z + 12 * ((z + VSF_PNG_ENC_IDAT - 1) / VSF_PNG_ENC_IDAT) + 12);
}

vsf_status vsf_debug_png_encode_header(int width, int height, int channels, uint8_t* out, size_t cap, size_t* n_bytes) {
  if (!good(width, height, channels) || !out || !n_bytes) return VSF_ERR_INVALID_ARG;
  *n_bytes = VSF_PNG_ENC_HEADER_BYTES + 2;
  if (cap < *n_bytes) return VSF_ERR_CAPACITY;
  uint8_t h[VSF_PNG_ENC_HEADER_BYTES];
  vsf_png_enc_header(width, height, channels, h);
  memcpy(out, h, VSF_PNG_ENC_HEADER_BYTES);
  vsf_png_enc_zlib_header(vsf_png_enc_filtered_bytes(width, height, channels), out + VSF_PNG_ENC_HEADER_BYTES);
  return VSF_OK;
}

vsf_status vsf_debug_png_encode_cpu(const uint8_t* src, int width, int height, int channels, size_t src_row_stride, uint8_t* out,
                                    size_t cap, size_t* n_bytes) {
  if (!good(width, height, channels) || !src || !out || !n_bytes || src_row_stride < (size_t)width * (size_t)channels)
    return VSF_ERR_INVALID_ARG;
  if (vsf_png_encode_capacity(width, height, channels) > 0x7FFFFFFFu) return VSF_ERR_UNSUPPORTED;
  *n_bytes = vsf_png_enc_cpu(src, width, height, channels, src_row_stride, out, cap);
  return *n_bytes ? VSF_OK : VSF_ERR_CAPACITY;
}

}  // extern "C"
