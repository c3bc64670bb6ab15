// k_jpeg_enc.hip -- baseline JPEG encoder for gfx950: the files cv::imencode(".jpg") of OpenCV 3.2 makes libjpeg write, byte for
// byte (1 channel: one component; 3 channels: BGR -> YCbCr 4:2:0).  Four launches per batch, all integer VALU work:
//   1  dct     one thread per 8x8 block of the scan: samples (jccolor.c rgb_ycc_convert's fixed-point sums, jcsample.c
//              h2v2_downsample's alternating 1 / 2 bias, edges replicated as jcprepct.c / jcsample.c do), jfdctint.c's forward
//              DCT, jcdctmgr.c's symmetric quantisation; writes the coefficients in zig-zag order and the bits its AC
//              symbols take.  The blocks libjpeg invents to fill the last MCU column / row (jccoefct.c: all zero, DC copied
//              from the block before) are written as such.
//   2  scan    one workgroup per image: every block's length (DC difference against the block before of its component: no
//              restart interval, so the chain is a shifted subtraction) and a prefix sum that places its bits; zeroes the words
//              the image's scan will take
//   3  pack    one thread per block: (run, size) symbols with ZRL / EOB, Huffman codes + magnitude bits into the placed
//              position (whole words stored, the two shared words at a block's ends OR-ed in atomically)
//   4  stuff   one workgroup per image: header, the scan with a 00 behind every FF (a second placed pass: prefix sum of the FF
//              counts), the last byte padded with 1-bits, EOI, the byte count.
// A file that does not fit its slot sets its count to -1 and bit 0 of the status word; nothing is written past a slot.
#include "vsf_internal.h"
#include "vsf_jpeg_enc_host.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ int clampi(int v, int hi) { return v < hi ? v : hi; }

// jfdctint.c (CONST_BITS 13, PASS1_BITS 2): one 1-D pass over eight values
template <bool kFirst>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int kShift = kFirst ? 13 - 2 : 13 + 2;
  constexpr int kHalf = 1 << (kShift - 1);
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kFirst) {
    d0 = (t10 + t11) << 2;
    d4 = (t10 - t11) << 2;
  } else {
    d0 = (t10 + t11 + 2) >> 2;
    d4 = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d2 = (z1 + t13 * 6270 + kHalf) >> kShift;
  d6 = (z1 - t12 * 15137 + kHalf) >> kShift;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = (a4 + z1 + z3 + kHalf) >> kShift;
  d5 = (a5 + z2 + z4 + kHalf) >> kShift;
  d3 = (a6 + z2 + z3 + kHalf) >> kShift;
  d1 = (a7 + z1 + z4 + kHalf) >> kShift;
}

// natural index of zig-zag position k
__device__ constexpr int zz(int k) {
  constexpr int t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}

__device__ __forceinline__ int size_category(int v) {  // bits of |v|
  const int a = v < 0 ? -v : v;
  return 32 - __clz(a);
}

struct EncGeom {
  int n, w, h, channels;
  int bw, bh;           // 1 channel: blocks; 3 channels: MCUs (16x16) across / down
  uint32_t blocks;      // per image, in scan order
  size_t src_image_stride, src_row_stride;
};

// The component block b of the scan belongs to: 0 luminance, 1 Cb, 2 Cr -- and the block before it in that component's DC
// chain (-1: none).
__device__ __forceinline__ int block_component(const EncGeom& g, uint32_t b, int64_t* prev) {
  if (g.channels == 1) {
    *prev = (int64_t)b - 1;
    return 0;
  }
  const uint32_t k = b % 6u;
  if (k == 0) {
    *prev = b == 0 ? -1 : (int64_t)b - 3;  // the MCU before: its fourth luminance block
    return 0;
  }
  if (k < 4) {
    *prev = (int64_t)b - 1;
    return 0;
  }
  *prev = b < 6 ? -1 : (int64_t)b - 6;
  return (int)k - 3;
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_dct_kernel(const uint8_t* __restrict__ src, EncGeom g, VsfJpegEncTables tab,
                                                                 int16_t* __restrict__ coef, uint32_t* __restrict__ ac_bits) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  const int img = blockIdx.y;
  if (b >= g.blocks) return;
  const uint8_t* im = src + (size_t)img * g.src_image_stride;
  const int xmax = g.w - 1, ymax = g.h - 1;
  int d[64];
  int comp = 0;
  bool dummy = false;
  if (g.channels == 1) {
    const int x0 = (int)(b % (uint32_t)g.bw) * 8, y0 = (int)(b / (uint32_t)g.bw) * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
      const uint8_t* row = im + (size_t)clampi(y0 + y, ymax) * g.src_row_stride;
#pragma unroll
      for (int x = 0; x < 8; x++) d[y * 8 + x] = (int)row[clampi(x0 + x, xmax)] - 128;
    }
  } else {
    const uint32_t m = b / 6u, k = b % 6u;
    const int mx = (int)(m % (uint32_t)g.bw), my = (int)(m / (uint32_t)g.bw);
    if (k < 4) {
      // luminance: the component is ceil(w / 8) x ceil(h / 8) blocks; what the MCU holds beyond that is a dummy block, all zero
      // but for the DC it copies from the block before it in the MCU -- which resolves to the MCU's first or second block
      const int ybw = (g.w + 7) >> 3, ybh = (g.h + 7) >> 3;
      int bx = 2 * mx + (int)(k & 1), by = 2 * my + (int)(k >> 1);
      if (by >= ybh) {
        dummy = true;
        by = 2 * my;
        bx = 2 * mx + 1 < ybw ? 2 * mx + 1 : 2 * mx;
      } else if (bx >= ybw) {
        dummy = true;
        bx = 2 * mx;
      }
#pragma unroll
      for (int y = 0; y < 8; y++) {
        const uint8_t* row = im + (size_t)clampi(by * 8 + y, ymax) * g.src_row_stride;
#pragma unroll
        for (int x = 0; x < 8; x++) {
          const uint8_t* p = row + 3 * clampi(bx * 8 + x, xmax);
          const int B = p[0], G = p[1], R = p[2];
          d[y * 8 + x] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
        }
      }
    } else {
      comp = (int)k - 3;
      // chrominance: 2x2 means of the converted samples, bias 1 in even and 2 in odd output columns
#pragma unroll
      for (int y = 0; y < 8; y++) {
        // (rows: the image is padded to an even height before the downsampling, the DOWNSAMPLED rows to the MCU's height after it;
        // columns: the full-size rows are padded to the MCU's width before it)
        const int cy = clampi(my * 8 + y, (g.h - 1) >> 1);
        const uint8_t* row0 = im + (size_t)clampi(2 * cy, ymax) * g.src_row_stride;
        const uint8_t* row1 = im + (size_t)clampi(2 * cy + 1, ymax) * g.src_row_stride;
#pragma unroll
        for (int x = 0; x < 8; x++) {
          int sum = (x & 1) ? 2 : 1;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint8_t* p = ((q & 2) ? row1 : row0) + 3 * clampi(mx * 16 + 2 * x + (q & 1), xmax);
            const int B = p[0], G = p[1], R = p[2];
            const int v = comp == 1 ? -11059 * R - 21709 * G + 32768 * B : 32768 * R - 27439 * G - 5329 * B;
            sum += (v + (128 << 16) + 32767) >> 16;
          }
          d[y * 8 + x] = (sum >> 2) - 128;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; r++)
    fdct8<true>(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7]);
#pragma unroll
  for (int c = 0; c < 8; c++) fdct8<false>(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c]);
  // jcdctmgr.c: divisor = quantiser << 3, rounded half away from zero.  floor(n / q) as a multiplication by ceil(2^32 / q): exact
  // for n e < 2^32, e = q ceil(2^32 / q) - 2^32 < q <= 2040 and n < 2^15
  const int t = comp ? 1 : 0;
  int q[64];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    const uint32_t qv = (uint32_t)tab.quant[t][i] << 3;
    const int v = d[i];
    const uint32_t a = (uint32_t)(v < 0 ? -v : v) + (qv >> 1);
    const int r = (int)__umulhi(a, tab.recip[t][i]);
    q[i] = v < 0 ? -r : r;
  }
  // zig-zag order out; the bits of the AC symbols (jchuff.c encode_one_block)
  uint32_t bits = 0;
  int run = 0;
  uint32_t packed[32];
#pragma unroll
  for (int k = 0; k < 64; k++) {
    const int v = (dummy && k > 0) ? 0 : q[zz(k)];
    if (k & 1)
      packed[k >> 1] |= (uint32_t)(uint16_t)v << 16;
    else
      packed[k >> 1] = (uint32_t)(uint16_t)v;
    if (k > 0) {
      if (v == 0) {
        run++;
      } else {
        const int s = size_category(v);
        bits += (uint32_t)(run >> 4) * (tab.ac_code[t][0xF0] & 31u) + (tab.ac_code[t][((run & 15) << 4) | s] & 31u) + (uint32_t)s;
        run = 0;
      }
    }
  }
  if (run > 0) bits += tab.ac_code[t][0] & 31u;
  const size_t gb = (size_t)img * g.blocks + b;
  uint4* out = reinterpret_cast<uint4*>(coef + gb * 64);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = make_uint4(packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]);
  ac_bits[gb] = bits;
}

// exclusive prefix sum over the workgroup's kThreads values; *total: their sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();  // (lds may still be read by the round before)
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < kThreads / 64; i++) {
    if (i < wave) base += lds[i];
    sum += lds[i];
  }
  *total = sum;
  return base + incl - v;
}

__device__ __forceinline__ int dc_difference(const int16_t* coef_img, uint32_t b, int64_t prev) {
  const int dc = coef_img[(size_t)b * 64];
  return prev < 0 ? dc : dc - (int)coef_img[(size_t)prev * 64];
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_scan_kernel(EncGeom g, VsfJpegEncTables tab, const int16_t* __restrict__ coef,
                                                                  const uint32_t* __restrict__ ac_bits, uint64_t* __restrict__ bit_off,
                                                                  uint64_t* __restrict__ tot_bits, uint32_t* __restrict__ stream,
                                                                  size_t stream_stride, int header_len, size_t out_cap,
                                                                  int32_t* __restrict__ out_bytes, int32_t* __restrict__ status) {
  __shared__ uint32_t lds[kThreads / 64];
  const int img = blockIdx.x;
  const int16_t* coef_img = coef + (size_t)img * g.blocks * 64;
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < g.blocks; b0 += kThreads) {
    const uint32_t b = b0 + threadIdx.x;
    uint32_t len = 0;
    if (b < g.blocks) {
      int64_t prev;
      const int comp = block_component(g, b, &prev);
      const int s = size_category(dc_difference(coef_img, b, prev));
      len = ac_bits[(size_t)img * g.blocks + b] + (tab.dc_code[comp ? 1 : 0][s] & 31u) + (uint32_t)s;
    }
    uint32_t total;
    const uint32_t excl = block_exclusive_scan(len, lds, &total);
    if (b < g.blocks) bit_off[(size_t)img * g.blocks + b] = carry + excl;
    carry += total;
  }
  const uint64_t nbytes = (carry + 7) >> 3;
  // (the packer may touch the word behind the last byte: stream_stride leaves room for it)
  const bool fits = (uint64_t)header_len + nbytes + 2 <= (uint64_t)out_cap && nbytes + 8 <= (uint64_t)stream_stride;
  if (threadIdx.x == 0) {
    tot_bits[img] = carry;
    out_bytes[img] = fits ? 0 : -1;
    if (!fits) atomicOr(status, 1);
  }
  if (!fits) return;
  uint32_t* words = stream + (size_t)img * (stream_stride / 4);
  const uint64_t nwords = (nbytes + 3) / 4 + 1;
  for (uint64_t i = threadIdx.x; i < nwords; i += kThreads) words[i] = 0;
}

struct BitWriter {
  uint32_t* words;  // the image's scan as big-endian 32-bit words
  uint64_t wi;      // word being filled
  uint64_t acc;     // its bits from the top; the first `fill` are taken (those in front of this block by its predecessors)
  int fill;
  bool shared;      // the word being filled holds bits of the block before
  __device__ __forceinline__ void put(uint32_t value, int len) {  // len <= 26
    acc |= (uint64_t)value << (64 - fill - len);
    fill += len;
    if (fill >= 32) {
      const uint32_t w = __builtin_bswap32((uint32_t)(acc >> 32));
      if (shared)
        atomicOr(words + wi, w);
      else
        words[wi] = w;
      shared = false;
      wi++;
      acc <<= 32;
      fill -= 32;
    }
  }
  __device__ __forceinline__ void finish() {  // (the block behind shares this word)
    if (fill > 0) atomicOr(words + wi, __builtin_bswap32((uint32_t)(acc >> 32)));
  }
};

__global__ __launch_bounds__(kThreads) void jpeg_enc_pack_kernel(EncGeom g, VsfJpegEncTables tab, const int16_t* __restrict__ coef,
                                                                  const uint64_t* __restrict__ bit_off, uint32_t* __restrict__ stream,
                                                                  size_t stream_stride, const int32_t* __restrict__ out_bytes) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  const int img = blockIdx.y;
  if (b >= g.blocks || out_bytes[img] < 0) return;
  const int16_t* coef_img = coef + (size_t)img * g.blocks * 64;
  int64_t prev;
  const int comp = block_component(g, b, &prev);
  const int t = comp ? 1 : 0;
  const uint64_t pos = bit_off[(size_t)img * g.blocks + b];
  BitWriter bw{stream + (size_t)img * (stream_stride / 4), pos >> 5, 0, (int)(pos & 31), (pos & 31) != 0};
  const uint4* in = reinterpret_cast<const uint4*>(coef_img + (size_t)b * 64);
  {
    const int diff = dc_difference(coef_img, b, prev);
    const int s = size_category(diff);
    const uint32_t c = tab.dc_code[t][s];
    const uint32_t mag = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u);
    bw.put((c >> 5) << s | mag, (int)(c & 31u) + s);
  }
  int run = 0;
  const uint32_t zrl = tab.ac_code[t][0xF0];
  for (int i = 0; i < 8; i++) {
    const uint4 v4 = in[i];
    const uint32_t w4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (i == 0 && j == 0) continue;
      const int v = (int)(int16_t)(w4[j >> 1] >> ((j & 1) * 16));
      if (v == 0) {
        run++;
        continue;
      }
      while (run > 15) {
        bw.put(zrl >> 5, (int)(zrl & 31u));
        run -= 16;
      }
      const int s = size_category(v);
      const uint32_t c = tab.ac_code[t][(run << 4) | s];
      const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
      bw.put((c >> 5) << s | mag, (int)(c & 31u) + s);
      run = 0;
    }
  }
  if (run > 0) {
    const uint32_t c = tab.ac_code[t][0];
    bw.put(c >> 5, (int)(c & 31u));
  }
  bw.finish();
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_stuff_kernel(VsfJpegEncHeader hdr, const uint64_t* __restrict__ tot_bits,
                                                                   const uint8_t* __restrict__ stream, size_t stream_stride,
                                                                   uint8_t* __restrict__ out, size_t out_stride, size_t out_cap,
                                                                   int32_t* __restrict__ out_bytes, int32_t* __restrict__ status) {
  __shared__ uint32_t lds[kThreads / 64];
  const int img = blockIdx.x;
  const bool skip = out_bytes[img] < 0;  // (the scan kernel's verdict; thread 0 overwrites the word at the end)
  __syncthreads();
  if (skip) return;
  uint8_t* dst = out + (size_t)img * out_stride;
  for (int i = threadIdx.x; i < hdr.len; i += kThreads) dst[i] = hdr.bytes[i];  // (the scan kernel checked that it fits)
  const uint64_t bits = tot_bits[img], nbytes = (bits + 7) >> 3;
  const uint8_t last_pad = (bits & 7) ? (uint8_t)(0xFFu >> (bits & 7)) : 0;  // the last byte is filled up with 1-bits
  const uint8_t* in = stream + (size_t)img * stream_stride;
  uint64_t at = (uint64_t)hdr.len;  // where the chunk's first byte goes
  for (uint64_t c0 = 0; c0 < nbytes; c0 += (uint64_t)kThreads * 16) {
    const uint64_t i0 = c0 + (uint64_t)threadIdx.x * 16;
    uint8_t by[16];
    uint32_t ff = 0;
    if (i0 < nbytes) {
      const uint4 v = *reinterpret_cast<const uint4*>(in + i0);
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; j++) {
        uint8_t x = (uint8_t)(w4[j >> 2] >> ((j & 3) * 8));
        if (i0 + j == nbytes - 1) x |= last_pad;
        by[j] = x;
        ff += (i0 + j < nbytes && x == 0xFF) ? 1u : 0u;
      }
    }
    uint32_t total;
    const uint32_t before = block_exclusive_scan(ff, lds, &total);
    if (i0 < nbytes) {
      uint64_t o = at + (i0 - c0) + before;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if (i0 + j < nbytes) {
          if (o < out_cap) dst[o] = by[j];
          o++;
          if (by[j] == 0xFF) {
            if (o < out_cap) dst[o] = 0;
            o++;
          }
        }
      }
    }
    const uint64_t left = nbytes - c0;
    at += (left < (uint64_t)kThreads * 16 ? left : (uint64_t)kThreads * 16) + total;
  }
  if (threadIdx.x == 0) {
    if (at + 2 <= out_cap && at + 2 <= 0x7FFFFFFFull) {
      dst[at] = 0xFF;
      dst[at + 1] = 0xD9;
      out_bytes[img] = (int32_t)(at + 2);
    } else {
      out_bytes[img] = -1;
      atomicOr(status, 1);
    }
  }
}

// Where everything sits in the scratch of a job: coefficients | bit offsets | totals | AC bits | streams, each part a multiple of
// 16 bytes.  The ONE statement of it: the need and the launcher both read it.
struct JeLayout {
  size_t blocks;         // of the whole batch
  size_t stream_stride;  // bytes between the images' scans before stuffing: the worst case or what a file may take, whichever is less
  size_t off_bit_off, off_tot_bits, off_ac_bits, off_stream, total;  // (the coefficients start at 0)
};

JeLayout layout(const VsfEncodeJob& job) {
  JeLayout L;
  const size_t per_image = vsf_jpeg_enc_blocks(job.width, job.height, job.channels), worst = per_image * VSF_JPEG_ENC_BLOCK_BYTES;
  L.blocks = per_image * (size_t)job.n;
  L.stream_stride = ((worst < job.cap() ? worst : job.cap()) + 16 + 15) & ~(size_t)15;
  L.off_bit_off = L.blocks * 128;
  L.off_tot_bits = L.off_bit_off + ((L.blocks * 8 + 15) & ~(size_t)15);
  L.off_ac_bits = L.off_tot_bits + (((size_t)job.n * 8 + 15) & ~(size_t)15);
  L.off_stream = L.off_ac_bits + ((L.blocks * 4 + 15) & ~(size_t)15);
  L.total = L.off_stream + (size_t)job.n * L.stream_stride;
  return L;
}

}  // namespace

size_t vsf_jpeg_enc_scratch_need(const VsfEncodeJob& job) { return layout(job).total; }

int vsf_jpeg_enc_launches() { return 4; }  // (dct, scan, pack, stuff: the launches below)

void vsf_jpeg_enc_launch(const VsfEncodeJob& job, const uint8_t* d_src, void* d_scratch, uint8_t* d_out, int32_t* d_out_bytes,
                         int32_t* d_status, hipStream_t s) {
  const size_t out_cap = job.cap();
  VsfJpegEncTables tab;
  vsf_jpeg_enc_quant(job.quality, tab.quant);
  vsf_jpeg_enc_codes(&tab);
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 64; i++) {
      const uint64_t q = (uint64_t)tab.quant[t][i] << 3;
      tab.recip[t][i] = (uint32_t)(((1ull << 32) + q - 1) / q);
    }
  VsfJpegEncHeader hdr;
  hdr.len = vsf_jpeg_enc_header(job.width, job.height, job.channels, job.quality, hdr.bytes);
  const bool mcu16 = job.channels == 3;  // (EncGeom: blocks across / down, or 16x16 MCUs)
  const EncGeom g{job.n, job.width, job.height, job.channels, mcu16 ? (job.width + 15) / 16 : (job.width + 7) / 8,
                  mcu16 ? (job.height + 15) / 16 : (job.height + 7) / 8, (uint32_t)vsf_jpeg_enc_blocks(job.width, job.height, job.channels),
                  job.src_image_stride, job.src_row_stride};
  const JeLayout L = layout(job);
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  int16_t* coef = reinterpret_cast<int16_t*>(p);
  uint64_t* bit_off = reinterpret_cast<uint64_t*>(p + L.off_bit_off);
  uint64_t* tot_bits = reinterpret_cast<uint64_t*>(p + L.off_tot_bits);
  uint32_t* ac_bits = reinterpret_cast<uint32_t*>(p + L.off_ac_bits);
  uint32_t* stream = reinterpret_cast<uint32_t*>(p + L.off_stream);
  const dim3 per_block((g.blocks + kThreads - 1) / kThreads, (unsigned)job.n), per_image((unsigned)job.n);
  hipLaunchKernelGGL(jpeg_enc_dct_kernel, per_block, dim3(kThreads), 0, s, d_src, g, tab, coef, ac_bits);
  hipLaunchKernelGGL(jpeg_enc_scan_kernel, per_image, dim3(kThreads), 0, s, g, tab, coef, ac_bits, bit_off, tot_bits, stream,
                     L.stream_stride, hdr.len, out_cap, d_out_bytes, d_status);
  hipLaunchKernelGGL(jpeg_enc_pack_kernel, per_block, dim3(kThreads), 0, s, g, tab, coef, bit_off, stream, L.stream_stride, d_out_bytes);
  hipLaunchKernelGGL(jpeg_enc_stuff_kernel, per_image, dim3(kThreads), 0, s, hdr, tot_bits, reinterpret_cast<const uint8_t*>(stream),
                     L.stream_stride, d_out, job.out_stride, out_cap, d_out_bytes, d_status);
}

