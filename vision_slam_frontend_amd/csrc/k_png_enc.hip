// k_png_enc.hip -- PNG encoder for gfx950: the files cv::imencode(".png") of OpenCV 3.2 makes libpng 1.6 / zlib 1.2.11 write, byte
// for byte (Sub filter, deflate level 1 with Z_RLE, memLevel 8, IDAT chunks of 8192 bytes; 1 channel: gray, 3 channels: B G R in,
// R G B out).  With Z_RLE zlib's matches all have distance 1, so its symbols follow from the runs of equal bytes of the filtered
// stream in closed form (vsf_pe_symbol).  All integer work; nine launches per batch:
//   1  filter  one thread per tile of 64 filtered bytes: Sub per row behind a filter byte; the first and last run start in the tile
//   2  runs    one workgroup per image: max / min scans over the tiles -> the run every tile is entered in and left in
//   3  count   one thread per tile: the symbols that start in it
//   4  index   one workgroup per image: prefix sum of the counts; the image's symbol and block counts
//   5  emit    one thread per tile: its symbols (u16 each) at their index; where every block of 16383 symbols starts
//   6  plan    one wave per deflate block: the histograms, then one lane restates trees.c (vsf_png_enc_trees.h): the block's form,
//              header bits and code tables
//   7  place   one workgroup per image: the blocks' bit positions (a stored block is byte-aligned), the fit check, the Adler-32
//              of the filtered bytes; zeroes the words the stream will take
//   8  write   one workgroup per block: header bits, then 64 symbols per lane at the placed position (whole words stored, the
//              shared words at a lane's ends OR-ed in atomically), or the stored bytes
//   9  file    one workgroup per image: header, the stream cut into IDAT chunks with their CRC-32 (36 bytes per lane, combined
//              with the host's multipliers), IEND, the byte count.
// A file that does not fit its slot sets its count to -1 and bit 0 of the status word; nothing is written past a slot.
#include "vsf_internal.h"
#include "vsf_png_enc_host.h"
#include "vsf_png_enc_trees.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 64;
constexpr uint32_t kBlockSyms = VSF_PNG_ENC_BLOCK_SYMS;

struct PeGeom {
  int n, w, h, channels;
  uint32_t rowbytes1;   // bytes of a filtered row: w * channels + 1
  uint32_t nf;          // filtered bytes of an image
  uint32_t tiles;       // ceil(nf / 64)
  uint32_t max_blocks;  // nf / 16383 + 1
  size_t src_image_stride, src_row_stride;
  size_t f_stride;      // bytes between the filtered images (a multiple of 64, with 64 to spare)
  size_t stream_stride; // ... between the zlib streams (a multiple of 16)
};

struct PeBufs {
  uint8_t* filt;        // [n][f_stride]
  uint32_t* last_brk;   // [n][tiles]   last run start in the tile + 1 (0: none)
  uint32_t* first_brk;  // [n][tiles]   first run start in the tile (0xffffffff: none)
  uint32_t* run_in;     // [n][tiles]   start of the run the tile's first byte continues
  uint32_t* run_out;    // [n][tiles]   end of the run the tile's last byte belongs to, if it leaves the tile
  uint32_t* sym_base;   // [n][tiles]   count, then index of the tile's first symbol
  uint16_t* sym;        // [n][nf]
  uint32_t* n_sym;      // [n]
  uint32_t* block_pos;  // [n][max_blocks + 1]  filtered byte every block starts at
  VsfPePlan* plan;      // [n][max_blocks]
  uint64_t* block_bit;  // [n][max_blocks]  bit of the zlib stream the block starts at
  uint32_t* z_bytes;    // [n]  bytes of the zlib stream
  uint32_t* stream;     // [n][stream_stride / 4]
};

__device__ __forceinline__ uint8_t filtered_byte(const uint8_t* im, const PeGeom& g, uint32_t row, uint32_t c, uint8_t filter) {
  if (c == 0) return filter;
  const uint32_t x = c - 1;
  const uint8_t* r = im + (size_t)row * g.src_row_stride;
  if (g.channels == 1) return (uint8_t)(r[x] - (filter && x > 0 ? r[x - 1] : 0));
  const uint32_t px = x / 3u, at = px * 3u + (2u - (x - px * 3u));  // B G R in memory, R G B in the file
  return (uint8_t)(r[at] - (filter && px > 0 ? r[at - 3] : 0));
}

__global__ __launch_bounds__(kThreads) void png_enc_filter_kernel(const uint8_t* __restrict__ src, PeGeom g, uint8_t filter, PeBufs b) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  const int img = blockIdx.y;
  if (t >= g.tiles) return;
  const uint8_t* im = src + (size_t)img * g.src_image_stride;
  const uint32_t p0 = t * kTile;
  uint32_t row = p0 / g.rowbytes1, c = p0 - row * g.rowbytes1;
  uint32_t prev = 256;  // (no byte in front of the stream: its first byte starts a run)
  if (p0 > 0) prev = c > 0 ? filtered_byte(im, g, row, c - 1, filter) : filtered_byte(im, g, row - 1, g.rowbytes1 - 1, filter);
  uint32_t words[16];
  uint32_t first = 0xFFFFFFFFu, last = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) words[i] = 0;
  for (uint32_t i = 0; i < kTile; i++) {
    const uint32_t p = p0 + i;
    if (p >= g.nf) break;
    const uint32_t v = filtered_byte(im, g, row, c, filter);
    words[i >> 2] |= v << ((i & 3u) * 8u);
    if (v != prev) {
      if (first == 0xFFFFFFFFu) first = p;
      last = p + 1;
    }
    prev = v;
    if (++c == g.rowbytes1) {
      c = 0;
      row++;
    }
  }
  uint4* out = reinterpret_cast<uint4*>(b.filt + (size_t)img * g.f_stride + p0);  // (f_stride covers whole tiles)
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = make_uint4(words[4 * i], words[4 * i + 1], words[4 * i + 2], words[4 * i + 3]);
  b.last_brk[(size_t)img * g.tiles + t] = last;
  b.first_brk[(size_t)img * g.tiles + t] = first;
}

// inclusive scans over the workgroup's kThreads values; *total: the reduction of all of them
template <int kOp>  // 0 sum, 1 max, 2 min
__device__ __forceinline__ uint32_t op(uint32_t a, uint32_t x) {
  return kOp == 0 ? a + x : kOp == 1 ? (a > x ? a : x) : (a < x ? a : x);
}
template <int kOp>
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  constexpr uint32_t kNeutral = kOp == 2 ? 0xFFFFFFFFu : 0u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl = op<kOp>(incl, up);
  }
  __syncthreads();  // (lds may still be read by the round before)
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  uint32_t base = kNeutral, all = kNeutral;
#pragma unroll
  for (int i = 0; i < kThreads / 64; i++) {
    if (i < wave) base = op<kOp>(base, lds[i]);
    all = op<kOp>(all, lds[i]);
  }
  *total = all;
  return op<kOp>(base, incl);
}

__global__ __launch_bounds__(kThreads) void png_enc_runs_kernel(PeGeom g, PeBufs b) {
  __shared__ uint32_t lds[kThreads / 64];
  const int img = blockIdx.x;
  const uint32_t* last_brk = b.last_brk + (size_t)img * g.tiles;
  const uint32_t* first_brk = b.first_brk + (size_t)img * g.tiles;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < g.tiles; t0 += kThreads) {  // the last run start in front of every tile
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < g.tiles ? last_brk[t] : 0;
    uint32_t total;
    uint32_t incl = block_inclusive_scan<1>(v, lds, &total);
    incl = incl > carry ? incl : carry;
    // exclusive: what the tiles in front hold
    const uint32_t up = __shfl_up(incl, 1, 64);
    __syncthreads();
    __shared__ uint32_t edge[kThreads / 64];
    if ((threadIdx.x & 63) == 63) edge[threadIdx.x >> 6] = incl;
    __syncthreads();
    const uint32_t excl = (threadIdx.x & 63) ? up : (threadIdx.x >> 6) ? edge[(threadIdx.x >> 6) - 1] : carry;
    if (t < g.tiles) b.run_in[(size_t)img * g.tiles + t] = excl ? excl - 1 : 0;
    carry = total > carry ? total : carry;
    __syncthreads();
  }
  carry = g.nf;
  for (uint32_t t0 = 0; t0 < g.tiles; t0 += kThreads) {  // the first run start behind every tile: the same from the end
    const uint32_t r = t0 + threadIdx.x;
    const uint32_t v = r < g.tiles ? first_brk[g.tiles - 1 - r] : 0xFFFFFFFFu;
    uint32_t total;
    uint32_t incl = block_inclusive_scan<2>(v, lds, &total);
    incl = incl < carry ? incl : carry;
    const uint32_t up = __shfl_up(incl, 1, 64);
    __syncthreads();
    __shared__ uint32_t edge2[kThreads / 64];
    if ((threadIdx.x & 63) == 63) edge2[threadIdx.x >> 6] = incl;
    __syncthreads();
    const uint32_t excl = (threadIdx.x & 63) ? up : (threadIdx.x >> 6) ? edge2[(threadIdx.x >> 6) - 1] : carry;
    if (r < g.tiles) b.run_out[(size_t)img * g.tiles + (g.tiles - 1 - r)] = excl;
    carry = total < carry ? total : carry;
    __syncthreads();
  }
}

// Walks the runs of tile t and calls f(position, symbol) for every symbol that starts in it.
template <typename F>
__device__ __forceinline__ void for_each_symbol(const PeGeom& g, const PeBufs& b, int img, uint32_t t, F f) {
  const uint8_t* fb = b.filt + (size_t)img * g.f_stride;
  const uint32_t p0 = t * kTile, p1 = p0 + kTile < g.nf ? p0 + kTile : g.nf;
  const uint32_t run_out = b.run_out[(size_t)img * g.tiles + t];
  uint32_t s = b.run_in[(size_t)img * g.tiles + t];  // start of the run the byte at p belongs to
  const uint4* in = reinterpret_cast<const uint4*>(fb + p0);
  uint32_t words[16];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint4 v = in[i];
    words[4 * i] = v.x;
    words[4 * i + 1] = v.y;
    words[4 * i + 2] = v.z;
    words[4 * i + 3] = v.w;
  }
  uint32_t p = p0;
  uint32_t prev = p0 > 0 ? fb[p0 - 1] : 256u;
  while (p < p1) {
    const uint32_t v = (words[(p - p0) >> 2] >> (((p - p0) & 3u) * 8u)) & 255u;
    if (v != prev) s = p;
    // the end of this run: inside the tile, or where the scan says
    uint32_t e = p + 1;
    while (e < p1 && ((words[(e - p0) >> 2] >> (((e - p0) & 3u) * 8u)) & 255u) == v) e++;
    const uint32_t run_end = e < p1 ? e : run_out;
    const uint32_t L = run_end - s;
    for (uint32_t q = p; q < e; q++) {
      const uint32_t sym = vsf_pe_symbol(q - s, L);
      if (sym) f(q, sym == 1 ? v : 256u + sym - 3u);
    }
    prev = v;
    p = e;
  }
}

__global__ __launch_bounds__(kThreads) void png_enc_count_kernel(PeGeom g, PeBufs b) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  const int img = blockIdx.y;
  if (t >= g.tiles) return;
  uint32_t n = 0;
  for_each_symbol(g, b, img, t, [&](uint32_t, uint32_t) { n++; });
  b.sym_base[(size_t)img * g.tiles + t] = n;
}

__global__ __launch_bounds__(kThreads) void png_enc_index_kernel(PeGeom g, PeBufs b) {
  __shared__ uint32_t lds[kThreads / 64];
  const int img = blockIdx.x;
  uint32_t* base = b.sym_base + (size_t)img * g.tiles;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < g.tiles; t0 += kThreads) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < g.tiles ? base[t] : 0;
    uint32_t total;
    const uint32_t incl = block_inclusive_scan<0>(v, lds, &total);
    if (t < g.tiles) base[t] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    b.n_sym[img] = carry;
    // floor(symbols / 16383) + 1 blocks; a last block without symbols starts at the stream's end, as does the block behind the last
    const uint32_t blocks = carry / kBlockSyms + 1;
    uint32_t* pos = b.block_pos + (size_t)img * (g.max_blocks + 1);
    pos[blocks] = g.nf;
    if (carry % kBlockSyms == 0) pos[blocks - 1] = g.nf;
  }
}

__global__ __launch_bounds__(kThreads) void png_enc_emit_kernel(PeGeom g, PeBufs b) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  const int img = blockIdx.y;
  if (t >= g.tiles) return;
  uint32_t i = b.sym_base[(size_t)img * g.tiles + t];
  uint16_t* sym = b.sym + (size_t)img * g.nf;
  uint32_t* pos = b.block_pos + (size_t)img * (g.max_blocks + 1);
  for_each_symbol(g, b, img, t, [&](uint32_t p, uint32_t s) {
    sym[i] = (uint16_t)s;  // (i < symbols <= nf)
    if (i % kBlockSyms == 0) pos[i / kBlockSyms] = p;
    i++;
  });
}

__device__ __forceinline__ uint32_t block_count(uint32_t n_sym) { return n_sym / kBlockSyms + 1; }

__global__ __launch_bounds__(64) void png_enc_plan_kernel(PeGeom g, PeBufs b) {
  __shared__ VsfPeWork work;
  __shared__ uint32_t hist[VSF_PE_L_CODES + 1];  // [286]: matches
  const int img = blockIdx.y;
  const uint32_t blk = blockIdx.x, n_sym = b.n_sym[img], blocks = block_count(n_sym);
  if (blk >= blocks) return;
  for (int i = threadIdx.x; i <= VSF_PE_L_CODES; i += 64) hist[i] = 0;
  __syncthreads();
  const uint32_t s0 = blk * kBlockSyms, s1 = blk + 1 == blocks ? n_sym : s0 + kBlockSyms;
  const uint16_t* sym = b.sym + (size_t)img * g.nf;
  for (uint32_t i = s0 + threadIdx.x; i < s1; i += 64) {
    const uint32_t s = sym[i];
    if (s < 256u) {
      atomicAdd(&hist[s], 1u);
    } else {
      int extra;
      uint32_t value;
      atomicAdd(&hist[257 + vsf_pe_length_code(s - 256u, &extra, &value)], 1u);
      atomicAdd(&hist[VSF_PE_L_CODES], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < VSF_PE_L_CODES; i += 64) work.freq[i] = (uint16_t)(i == 256 ? 1u : hist[i]);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t* pos = b.block_pos + (size_t)img * (g.max_blocks + 1);
    vsf_pe_plan_block(work, hist[VSF_PE_L_CODES], pos[blk + 1] - pos[blk], blk + 1 == blocks,
                      b.plan + (size_t)img * g.max_blocks + blk);
  }
}

__global__ __launch_bounds__(kThreads) void png_enc_place_kernel(PeGeom g, PeBufs b, VsfPngEncConsts k, size_t out_cap,
                                                                  int32_t* __restrict__ out_bytes, int32_t* __restrict__ status) {
  __shared__ uint64_t red[2][kThreads / 64];
  __shared__ uint32_t z_total;
  const int img = blockIdx.x;
  const uint32_t blocks = block_count(b.n_sym[img]);
  if (threadIdx.x == 0) {
    const VsfPePlan* plan = b.plan + (size_t)img * g.max_blocks;
    uint64_t bit = 16;
    for (uint32_t i = 0; i < blocks; i++) {
      b.block_bit[(size_t)img * g.max_blocks + i] = bit;
      bit += plan[i].hdr_bits;
      if (plan[i].type == 0) bit = (bit + 7) & ~(uint64_t)7;
      bit += plan[i].body_bits;
    }
    z_total = (uint32_t)((bit + 7) >> 3) + 4;  // (bi_windup after the last block, then the Adler-32)
  }
  __syncthreads();
  const uint64_t z = z_total;
  const uint64_t file = VSF_PNG_ENC_HEADER_BYTES + z + 12 * ((z + VSF_PNG_ENC_IDAT - 1) / VSF_PNG_ENC_IDAT) + 12;
  // (the writer may touch the word behind the last byte: stream_stride leaves room for it)
  const bool fits = file <= (uint64_t)out_cap && file <= 0x7FFFFFFFull && z + 8 <= (uint64_t)g.stream_stride;
  if (threadIdx.x == 0) {
    b.z_bytes[img] = (uint32_t)z;
    out_bytes[img] = fits ? 0 : -1;
    if (!fits) atomicOr(status, 1);
  }
  if (!fits) return;
  uint32_t* words = b.stream + (size_t)img * (g.stream_stride / 4);
  const uint64_t nwords = (z + 3) / 4 + 1;
  for (uint64_t i = threadIdx.x; i < nwords; i += kThreads) words[i] = 0;
  // Adler-32 of the filtered bytes as two dot products: A = 1 + sum d_i, B = n + sum (n - i) d_i  (mod 65521)
  const uint8_t* fb = b.filt + (size_t)img * g.f_stride;
  uint64_t sa = 0, sb = 0;
  for (uint32_t i = threadIdx.x * 16u; i < g.nf; i += kThreads * 16u) {
    const uint4 v = *reinterpret_cast<const uint4*>(fb + i);  // (bytes behind nf up to the tile's end are zero)
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    uint32_t s = 0, ws = 0;  // sum d, sum j d over the 16 bytes
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t d = (w4[j >> 2] >> ((j & 3) * 8)) & 255u;
      s += d;
      ws += (uint32_t)j * d;
    }
    sa += s;
    sb += (uint64_t)((g.nf - i) % 65521u) * s + 65521ull * 16 * 255 - ws;  // (n - i - j) d, kept non-negative
  }
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_down(sa, o, 64);
    sb += __shfl_down(sb, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sa;
    red[1][threadIdx.x >> 6] = sb % 65521u;
  }
  __syncthreads();  // (also: the zeroes above are in place for this workgroup's own atomics)
  if (threadIdx.x == 0) {
    uint64_t a = 1, bb = g.nf % 65521u;
    for (int i = 0; i < kThreads / 64; i++) {
      a += red[0][i];
      bb += red[1][i];
    }
    const uint32_t adler = (uint32_t)(bb % 65521u) << 16 | (uint32_t)(a % 65521u);
    atomicOr(words, (uint32_t)k.zhdr[0] | (uint32_t)k.zhdr[1] << 8);
    const uint64_t at = z - 4;
    for (int i = 0; i < 4; i++) {
      const uint32_t byte = (adler >> (24 - 8 * i)) & 255u;
      atomicOr(words + ((at + i) >> 2), byte << (((at + i) & 3u) * 8u));
    }
  }
}

struct PeBitWriter {
  uint32_t* words;  // the image's stream as little-endian words: deflate fills bytes from bit 0
  uint64_t wi;      // word being filled
  uint64_t acc;     // its bits from the bottom; the first `fill` are taken (those of the lanes in front)
  int fill;
  bool shared;      // the word being filled holds bits of somebody else
  __device__ __forceinline__ void put(uint64_t value, int len) {  // len <= 32
    acc |= value << fill;
    fill += len;
    if (fill >= 32) {
      const uint32_t w = (uint32_t)acc;
      if (shared)
        atomicOr(words + wi, w);
      else
        words[wi] = w;
      shared = false;
      wi++;
      acc >>= 32;
      fill -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (fill > 0) atomicOr(words + wi, (uint32_t)acc);
  }
};

__device__ __forceinline__ void or_bits(uint32_t* words, uint64_t bit, uint32_t value) {  // 32 bits at any position
  const uint32_t sh = (uint32_t)(bit & 31u);
  if (value << sh) atomicOr(words + (bit >> 5), value << sh);
  if (sh && (value >> (32u - sh))) atomicOr(words + (bit >> 5) + 1, value >> (32u - sh));
}

__global__ __launch_bounds__(kThreads) void png_enc_write_kernel(PeGeom g, PeBufs b, const int32_t* __restrict__ out_bytes) {
  __shared__ uint32_t lcode[VSF_PE_L_CODES];
  __shared__ uint32_t lds[kThreads / 64];
  const int img = blockIdx.y;
  const uint32_t blk = blockIdx.x, n_sym = b.n_sym[img], blocks = block_count(n_sym);
  if (blk >= blocks || out_bytes[img] < 0) return;
  const VsfPePlan* plan = b.plan + (size_t)img * g.max_blocks + blk;
  uint32_t* words = b.stream + (size_t)img * (g.stream_stride / 4);
  const uint64_t bit0 = b.block_bit[(size_t)img * g.max_blocks + blk];
  const uint32_t hdr_bits = plan->hdr_bits, type = plan->type;
  for (uint32_t i = threadIdx.x; i * 32u < hdr_bits; i += kThreads) or_bits(words, bit0 + i * 32u, plan->hdr[i]);
  if (type == 0) {
    const uint32_t* pos = b.block_pos + (size_t)img * (g.max_blocks + 1);
    const uint32_t p0 = pos[blk], len = pos[blk + 1] - p0;
    const uint64_t at = (bit0 + hdr_bits + 7) & ~(uint64_t)7;
    if (threadIdx.x == 0) or_bits(words, at, (len & 0xFFFFu) | (~len & 0xFFFFu) << 16);
    const uint8_t* fb = b.filt + (size_t)img * g.f_stride + p0;
    for (uint32_t i = threadIdx.x * 4u; i < len; i += kThreads * 4u) {
      uint32_t v = 0;
      for (uint32_t j = 0; j < 4 && i + j < len; j++) v |= (uint32_t)fb[i + j] << (8u * j);
      or_bits(words, at + 32 + 8ull * i, v);
    }
    return;
  }
  for (int i = threadIdx.x; i < VSF_PE_L_CODES; i += kThreads) lcode[i] = plan->lcode[i];
  const uint32_t dcode0 = plan->dcode0;
  __syncthreads();
  const uint32_t s0 = blk * kBlockSyms, s1 = blk + 1 == blocks ? n_sym : s0 + kBlockSyms;
  const uint32_t count = s1 - s0 + 1;  // with END_BLOCK
  const uint16_t* sym = b.sym + (size_t)img * g.nf;
  const uint32_t mine = threadIdx.x * 64u;  // 256 lanes x 64 symbols >= 16384
  uint32_t my_bits = 0;
  for (uint32_t j = mine; j < mine + 64u && j < count; j++) {
    uint64_t bits;
    my_bits += (uint32_t)vsf_pe_symbol_bits(lcode, dcode0, j + 1 == count ? 512u : sym[s0 + j], &bits);
  }
  uint32_t total;
  const uint32_t before = block_inclusive_scan<0>(my_bits, lds, &total) - my_bits;
  if (mine >= count) return;
  const uint64_t at = bit0 + hdr_bits + before;
  PeBitWriter bw{words, at >> 5, 0, (int)(at & 31u), true};  // (the first word may hold the header's bits even at bit 0 of it)
  for (uint32_t j = mine; j < mine + 64u && j < count; j++) {
    uint64_t bits;
    const int n = vsf_pe_symbol_bits(lcode, dcode0, j + 1 == count ? 512u : sym[s0 + j], &bits);
    if (n > 32) {
      bw.put(bits & 0xFFFFFFFFull, 32);
      bw.put(bits >> 32, n - 32);
    } else {
      bw.put(bits, n);
    }
  }
  bw.finish();
}

__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m != 0; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}

__device__ __forceinline__ void store_be32(uint8_t* dst, uint64_t at, uint32_t v, uint64_t cap) {
  for (int i = 0; i < 4; i++)
    if (at + i < cap) dst[at + i] = (uint8_t)(v >> (24 - 8 * i));
}

__global__ __launch_bounds__(kThreads) void png_enc_file_kernel(PeGeom g, PeBufs b, VsfPngEncConsts k, uint8_t* __restrict__ out,
                                                                 size_t out_stride, size_t out_cap, int32_t* __restrict__ out_bytes) {
  __shared__ uint32_t lds[kThreads / 64];
  const int img = blockIdx.x;
  const bool skip = out_bytes[img] < 0;  // (the place kernel's verdict; thread 0 overwrites the word at the end)
  __syncthreads();
  if (skip) return;
  uint8_t* dst = out + (size_t)img * out_stride;
  const uint64_t cap = out_cap;
  for (int i = threadIdx.x; i < VSF_PNG_ENC_HEADER_BYTES; i += kThreads)
    if ((uint64_t)i < cap) dst[i] = k.header[i];
  const uint8_t* z = reinterpret_cast<const uint8_t*>(b.stream + (size_t)img * (g.stream_stride / 4));
  const uint32_t zn = b.z_bytes[img], chunks = (zn + VSF_PNG_ENC_IDAT - 1) / VSF_PNG_ENC_IDAT;
  constexpr uint32_t kPadded = VSF_PNG_ENC_CRC_LANES * VSF_PNG_ENC_CRC_SEG;
  for (uint32_t c = 0; c <= chunks; c++) {  // the last round writes IEND
    const uint32_t len = c == chunks ? 0u : (zn - c * VSF_PNG_ENC_IDAT < VSF_PNG_ENC_IDAT ? zn - c * VSF_PNG_ENC_IDAT : VSF_PNG_ENC_IDAT);
    const uint64_t at = VSF_PNG_ENC_HEADER_BYTES + (c == chunks ? (uint64_t)zn + 12ull * chunks : (uint64_t)c * (VSF_PNG_ENC_IDAT + 12));
    const uint32_t type = c == chunks ? 0x49454E44u : 0x49444154u;  // "IEND" / "IDAT"
    // the chunk's type + data, right-aligned in kPadded bytes: lane i takes bytes [36 i, 36 i + 36) of that and the zeroes in
    // front change no CRC register that starts at zero
    const uint32_t m = 4 + len, lead = kPadded - m;
    uint32_t reg = 0;
    for (uint32_t j = 0; j < VSF_PNG_ENC_CRC_SEG; j++) {
      const uint32_t q = threadIdx.x * VSF_PNG_ENC_CRC_SEG + j;
      if (q < lead) continue;
      const uint32_t i = q - lead;  // byte of the message
      const uint8_t v = i < 4 ? (uint8_t)(type >> (24 - 8 * i)) : z[(size_t)c * VSF_PNG_ENC_IDAT + (i - 4)];
      if (at + 4 + i < cap) dst[at + 4 + i] = v;
      reg = k.crc_table[(reg ^ v) & 255u] ^ (reg >> 8);
    }
    uint32_t part = reg ? mulmod(reg, k.seg_mul[VSF_PNG_ENC_CRC_LANES - 1 - threadIdx.x]) : 0u;
    if (threadIdx.x == 0) {  // the register's start value, advanced over the m bytes
      uint32_t adv = 0xFFFFFFFFu;
      for (int bit = 0; bit < 16; bit++)
        if ((m >> bit) & 1u) adv = mulmod(adv, k.pow_mul[bit]);
      part ^= adv;
    }
    for (int o = 32; o > 0; o >>= 1) part ^= __shfl_down(part, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t crc = 0;
      for (int i = 0; i < kThreads / 64; i++) crc ^= lds[i];
      store_be32(dst, at, len, cap);
      store_be32(dst, at + 8 + len, ~crc, cap);
    }
  }
  if (threadIdx.x == 0)
    out_bytes[img] = (int32_t)(VSF_PNG_ENC_HEADER_BYTES + (uint64_t)zn + 12ull * chunks + 12);  // (the place kernel checked that it fits)
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct PeLayout {
  PeGeom g;
  size_t off[13];
  size_t total;
};

PeLayout layout(const VsfEncodeJob& job) {
  PeLayout L;
  PeGeom& g = L.g;
  g.n = job.n;
  g.w = job.width;
  g.h = job.height;
  g.channels = job.channels;
  g.rowbytes1 = (uint32_t)job.width * (uint32_t)job.channels + 1u;
  g.nf = (uint32_t)vsf_png_enc_filtered_bytes(job.width, job.height, job.channels);
  g.tiles = (g.nf + kTile - 1) / kTile;
  g.max_blocks = g.nf / kBlockSyms + 1;
  g.src_image_stride = job.src_image_stride;
  g.src_row_stride = job.src_row_stride;
  g.f_stride = (size_t)g.tiles * kTile + kTile;
  const size_t worst = (size_t)vsf_png_enc_stream_bound(g.nf);
  g.stream_stride = align_up((worst < job.cap() ? worst : job.cap()) + 16, 16);
  const size_t N = (size_t)job.n;
  const size_t sizes[13] = {N * g.f_stride,
                            N * g.tiles * 4,
                            N * g.tiles * 4,
                            N * g.tiles * 4,
                            N * g.tiles * 4,
                            N * g.tiles * 4,
                            N * g.nf * 2,
                            N * 4,
                            N * (g.max_blocks + 1) * 4,
                            N * g.max_blocks * sizeof(VsfPePlan),
                            N * g.max_blocks * 8,
                            N * 4,
                            N * g.stream_stride};
  size_t at = 0;
  for (int i = 0; i < 13; i++) {
    L.off[i] = at;
    at += align_up(sizes[i], 64);
  }
  L.total = at;
  return L;
}

}  // namespace

size_t vsf_png_enc_scratch_need(const VsfEncodeJob& job) { return layout(job).total; }

int vsf_png_enc_launches() { return 9; }  // (filter .. file: the launches below)

void vsf_png_enc_launch(const VsfEncodeJob& job, const uint8_t* d_src, void* d_scratch, uint8_t* d_out, int32_t* d_out_bytes,
                        int32_t* d_status, hipStream_t s) {
  const size_t out_cap = job.cap();
  const int n = job.n;
  const PeLayout L = layout(job);
  const PeGeom& g = L.g;
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  PeBufs b;
  b.filt = p + L.off[0];
  b.last_brk = reinterpret_cast<uint32_t*>(p + L.off[1]);
  b.first_brk = reinterpret_cast<uint32_t*>(p + L.off[2]);
  b.run_in = reinterpret_cast<uint32_t*>(p + L.off[3]);
  b.run_out = reinterpret_cast<uint32_t*>(p + L.off[4]);
  b.sym_base = reinterpret_cast<uint32_t*>(p + L.off[5]);
  b.sym = reinterpret_cast<uint16_t*>(p + L.off[6]);
  b.n_sym = reinterpret_cast<uint32_t*>(p + L.off[7]);
  b.block_pos = reinterpret_cast<uint32_t*>(p + L.off[8]);
  b.plan = reinterpret_cast<VsfPePlan*>(p + L.off[9]);
  b.block_bit = reinterpret_cast<uint64_t*>(p + L.off[10]);
  b.z_bytes = reinterpret_cast<uint32_t*>(p + L.off[11]);
  b.stream = reinterpret_cast<uint32_t*>(p + L.off[12]);
  VsfPngEncConsts k;
  vsf_png_enc_consts(job.width, job.height, job.channels, &k);
  const dim3 per_tile((g.tiles + kThreads - 1) / kThreads, (unsigned)n), per_image((unsigned)n), per_block(g.max_blocks, (unsigned)n);
  hipLaunchKernelGGL(png_enc_filter_kernel, per_tile, dim3(kThreads), 0, s, d_src, g, k.filter, b);
  hipLaunchKernelGGL(png_enc_runs_kernel, per_image, dim3(kThreads), 0, s, g, b);
  hipLaunchKernelGGL(png_enc_count_kernel, per_tile, dim3(kThreads), 0, s, g, b);
  hipLaunchKernelGGL(png_enc_index_kernel, per_image, dim3(kThreads), 0, s, g, b);
  hipLaunchKernelGGL(png_enc_emit_kernel, per_tile, dim3(kThreads), 0, s, g, b);
  hipLaunchKernelGGL(png_enc_plan_kernel, per_block, dim3(64), 0, s, g, b);
  hipLaunchKernelGGL(png_enc_place_kernel, per_image, dim3(kThreads), 0, s, g, b, k, out_cap, d_out_bytes, d_status);
  hipLaunchKernelGGL(png_enc_write_kernel, per_block, dim3(kThreads), 0, s, g, b, d_out_bytes);
  hipLaunchKernelGGL(png_enc_file_kernel, per_image, dim3(kThreads), 0, s, g, b, k, d_out, job.out_stride, out_cap, d_out_bytes);
}

