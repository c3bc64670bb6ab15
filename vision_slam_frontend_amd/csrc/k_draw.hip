// k_draw.hip -- the reference's debug images (slam_frontend.cc:74-115): cv::circle and cv::line at thickness 1, LINE_8,
// shift 0 onto GRAY2BGR canvases of one image or of two side by side (cv::hconcat), in batches of canvases.
//
// OpenCV 3.2 drawing.cpp draws primitive after primitive and a later one overwrites an earlier one.  Here every primitive
// runs at once, one wave each, and the draw order is made explicit instead: a pixel a primitive covers gets a 64-bit
// atomicMax of (ordinal + 1) << 32 | bgr in the canvas's winner buffer, so the highest ordinal -- the last writer -- wins.
// The resolve pass then writes every canvas pixel: the winner's colour, or the grey value where nothing landed; it also
// puts the winners it read back to zero, so the buffer is clean for the next call without a clearing pass.
// (Chosen because the resolve reads every pixel anyway; not measured against clearing only the touched pixels or the
// whole canvas in a pass of its own.)
//   Circle():  the integer midpoint routine; lane l takes iteration l / 8 (+ 8 per pass) and its point l % 8, writing only
//              pixels inside the canvas (its `inside` and clipped branches write exactly those).
//   Line():    LineIterator(8-connected, left_to_right) after clipLine; lane l takes major-axis steps l, l + 64, ...  The
//              minor offset after k steps follows from the Bresenham error term in closed form: the iterator steps the
//              minor axis at step j when dx - 2 dy (j + 1) + 2 dx m_j < 0, whose solution is
//              m_k = ceil((2 dy k - dx) / (2 dx)) = floor((2 dy k + dx - 1) / (2 dx))  (dx = major >= dy = minor >= 0);
//              tests/test_draw_ref.py checks it against the iteration for every |dx|, |dy| <= 300.
// Plain HIP; integer work, except clipLine's one double product / quotient per clipped end, as OpenCV computes it.
#include <algorithm>
#include <cstring>

#include "vsf_ctx.h"
#include "vsf_glibc_random.h"

using namespace vsfi;

namespace {

struct DrawCanvasDev {
  const uint8_t* src0;
  const uint8_t* src1;
  int32_t width, height, cw;  // of one source; cw: canvas width
  int32_t op_begin, op_count, skip;  // skip: the canvas is not drawn at all (an image the reference does not make)
  int64_t src_pitch, out_pitch;
  uint8_t* out;
  uint64_t* win;  // [height][cw]
};

__device__ __forceinline__ void put(uint64_t* win, int cw, int h, int64_t x, int64_t y, uint64_t key) {
  if (x >= 0 && x < cw && y >= 0 && y < h) atomicMax(reinterpret_cast<unsigned long long*>(win + y * cw + x), (unsigned long long)key);
}

// drawing.cpp clipLine(Size2l, Point2l&, Point2l&), statement for statement
__device__ bool clip_line(int64_t w, int64_t h, int64_t& x1, int64_t& y1, int64_t& x2, int64_t& y2) {
  const int64_t right = w - 1, bottom = h - 1;
  if (w <= 0 || h <= 0) return false;
  int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
  int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
  if ((c1 & c2) == 0 && (c1 | c2) != 0) {
    int64_t a;
    if (c1 & 12) {
      a = c1 < 8 ? 0 : bottom;
      x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
      y1 = a;
      c1 = (x1 < 0) + (x1 > right) * 2;
    }
    if (c2 & 12) {
      a = c2 < 8 ? 0 : bottom;
      x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
      y2 = a;
      c2 = (x2 < 0) + (x2 > right) * 2;
    }
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
      if (c1) {
        a = c1 == 1 ? 0 : right;
        y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
        x1 = a;
        c1 = 0;
      }
      if (c2) {
        a = c2 == 1 ? 0 : right;
        y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
        x2 = a;
        c2 = 0;
      }
    }
  }
  return (c1 | c2) == 0;
}

// one operation per wave (ordinal j) onto canvas c
__device__ void draw_op(const DrawCanvasDev& c, const vsf_draw_op* __restrict__ ops, int j, int lane) {
  const int oi = c.op_begin + j;
  const vsf_draw_op op = ops[oi];
  const uint64_t key = ((uint64_t)(uint32_t)(oi + 1) << 32) |
                       (uint64_t)(op.bgr[0] | ((uint32_t)op.bgr[1] << 8) | ((uint32_t)op.bgr[2] << 16));
  const int cw = c.cw, h = c.height;
  if (op.kind == VSF_DRAW_CIRCLE) {
    const int cx = op.x0, cy = op.y0, r = op.x1;
    if (r < 0 || r > 65535 || cx - r >= cw || cx + r < 0 || cy - r >= h || cy + r < 0) return;  // (nothing to draw)
    int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
    auto step = [&]() {
      dy++;
      err += plus;
      plus += 2;
      const int mask = (err <= 0) - 1;
      err -= minus & mask;
      dx += mask;
      minus -= mask & 2;
    };
    for (int i = 0; i < (lane >> 3); i++) step();
    const int pt = lane & 7;
    while (dx >= dy) {  // (once false it stays false: dy grows by one per iteration, dx never grows)
      const int a = pt < 4 ? dx : dy, b = pt < 4 ? dy : dx;  // points 0-3: (+-dx, +-dy); 4-7: (+-dy, +-dx)
      const int x = (pt & 2) ? cx + a : cx - a, y = (pt & 1) ? cy + b : cy - b;
      put(c.win, cw, h, x, y, key);
      for (int i = 0; i < 8; i++) step();
    }
    return;
  }
  if (op.kind != VSF_DRAW_LINE) return;
  int64_t x1 = op.x0, y1 = op.y0, x2 = op.x1, y2 = op.y1;
  if ((uint64_t)x1 >= (uint64_t)cw || (uint64_t)x2 >= (uint64_t)cw || (uint64_t)y1 >= (uint64_t)h ||
      (uint64_t)y2 >= (uint64_t)h) {
    if (!clip_line(cw, h, x1, y1, x2, y2)) return;
  }
  int64_t dx = x2 - x1, dy = y2 - y1;
  if (dx < 0) {  // left_to_right: start at the left end
    x1 = x2;
    y1 = y2;
    dx = -dx;
    dy = -dy;
  }
  const int64_t sy = dy < 0 ? -1 : 1, ady = dy < 0 ? -dy : dy;
  const bool ymajor = ady > dx;
  const int64_t major = ymajor ? ady : dx, minor = ymajor ? dx : ady;
  for (int64_t k = lane; k <= major; k += 64) {
    const int64_t m = major > 0 ? (2 * minor * k + major - 1) / (2 * major) : 0;
    const int64_t x = ymajor ? x1 + m : x1 + k, y = ymajor ? y1 + sy * k : y1 + sy * m;
    put(c.win, cw, h, x, y, key);
  }
}

// blockIdx.y: canvas; waves blockIdx.x * 4 + wave, + 4 gridDim.x, ...: its operations
__global__ __launch_bounds__(256) void draw_raster_kernel(const DrawCanvasDev* __restrict__ canvases,
                                                          const vsf_draw_op* __restrict__ ops) {
  const DrawCanvasDev& c = canvases[blockIdx.y];
  const int lane = (int)(threadIdx.x & 63), n = c.op_count;
  for (int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6); j < n; j += gridDim.x * 4) draw_op(c, ops, j, lane);
}

// blockIdx.y: canvas; one thread per canvas pixel: GRAY2BGR of its source, or the winning primitive's colour
__global__ __launch_bounds__(256) void draw_resolve_kernel(const DrawCanvasDev* __restrict__ canvases) {
  const DrawCanvasDev c = canvases[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c.skip || i >= (int64_t)c.cw * c.height) return;
  const int y = (int)(i / c.cw), x = (int)(i - (int64_t)y * c.cw);
  uint8_t* o = c.out + y * c.out_pitch + 3 * (int64_t)x;
  const uint64_t w = c.win[i];
  if (w != 0) {
    c.win[i] = 0;
    o[0] = (uint8_t)w;
    o[1] = (uint8_t)(w >> 8);
    o[2] = (uint8_t)(w >> 16);
  } else {
    const uint8_t g = x < c.width ? c.src0[y * c.src_pitch + x] : c.src1[y * c.src_pitch + (x - c.width)];
    o[0] = o[1] = o[2] = g;
  }
}

vsf_status check_canvas(const vsf_draw_canvas& c, int n_ops) {
  if (c.width <= 0 || c.height <= 0 || c.width > (1 << 28) / (c.src1 ? 2 : 1) || c.height > (1 << 28) || !c.src0 || !c.out ||
      c.src_pitch < c.width || c.out_pitch < 3 * (int64_t)c.width * (c.src1 ? 2 : 1) || c.op_begin < 0 || c.op_count < 0 ||
      (int64_t)c.op_begin + c.op_count > n_ops)
    return VSF_ERR_INVALID_ARG;
  return VSF_OK;
}

vsf_status draw_dev(vsf_ctx* ctx, const vsf_draw_canvas* canvases, int n, const vsf_draw_op* d_ops) {
  // winners: one u64 per canvas pixel, canvases back to back
  size_t win = 0;
  int max_ops = 0;
  int64_t max_pixels = 0;
  for (int i = 0; i < n; i++) {
    const int64_t px = (int64_t)canvases[i].width * (canvases[i].src1 ? 2 : 1) * canvases[i].height;
    win += (size_t)px;
    max_pixels = std::max(max_pixels, px);
    max_ops = std::max(max_ops, canvases[i].op_count);
  }
  if (win > ctx->dr_win_cap) {
    vsf_status st = grow_scratch(ctx, ctx->dr_win, win * sizeof(uint64_t));
    if (st != VSF_OK) return st;
    VSF_HIP(hipMemsetAsync(ctx->dr_win, 0, win * sizeof(uint64_t), ctx->stream));
    ctx->dr_win_cap = win;
  }
  if (n > ctx->dr_canv_cap) {
    vsf_status st = grow_scratch(ctx, ctx->dr_canv, (size_t)n * sizeof(DrawCanvasDev));
    if (st != VSF_OK) return st;
    ctx->dr_canv_cap = n;
  }
  // the table's host image is rewritten only after the previous call's upload has left it
  if (!ctx->dr_uploaded) VSF_HIP(ctx->dr_uploaded.alloc(hipEventDisableTiming));
  VSF_HIP(hipEventSynchronize(ctx->dr_uploaded));
  ctx->dr_canv_host.resize((size_t)n * sizeof(DrawCanvasDev));
  DrawCanvasDev* t = reinterpret_cast<DrawCanvasDev*>(ctx->dr_canv_host.data());
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    const vsf_draw_canvas& s = canvases[i];
    DrawCanvasDev d;
    d.src0 = s.src0;
    d.src1 = s.src1;
    d.width = s.width;
    d.height = s.height;
    d.cw = s.width * (s.src1 ? 2 : 1);
    d.op_begin = s.op_begin;
    d.op_count = s.op_count;
    d.skip = 0;
    d.src_pitch = s.src_pitch;
    d.out_pitch = s.out_pitch;
    d.out = s.out;
    d.win = ctx->dr_win + off;
    off += (size_t)d.cw * d.height;
    t[i] = d;
  }
  VSF_HIP(hipMemcpyAsync(ctx->dr_canv, t, (size_t)n * sizeof(DrawCanvasDev), hipMemcpyHostToDevice, ctx->stream));
  VSF_HIP(hipEventRecord(ctx->dr_uploaded, ctx->stream));
  const DrawCanvasDev* dc = static_cast<const DrawCanvasDev*>(ctx->dr_canv.get());
  if (max_ops > 0)
    hipLaunchKernelGGL(draw_raster_kernel, dim3((unsigned)((max_ops + 3) / 4), (unsigned)n), dim3(256), 0, ctx->stream, dc, d_ops);
  hipLaunchKernelGGL(draw_resolve_kernel, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)n), dim3(256), 0, ctx->stream, dc);
  VSF_STICKY();
  return VSF_OK;
}

// ---- the stereo lines' colours with a generator per stream (vsf_observe_set_debug_seeds) ----
// One wave per frame of the batch; the wave of a stream's FIRST frame in the batch (params[f].prev < 0) walks that stream's
// frames in submission order, every other wave leaves at once.  The chain is serial -- a draw needs the draw three before it
// --, so every lane computes the same values and lane j keeps colour j of a block of 31 for one store.  The window of 31
// words stays in registers: colours31 (vsf_glibc_random.h) names every word by a constant as long as the rear pointer is 0
// when a block starts, so after each frame the window goes through LDS once, written at the rotated index and read back
// in order.  A frame takes clamp(npairs, 0, K) colours whether or not its rows are valid (cc:95), as debug_ops_kernel reads them.
__global__ __launch_bounds__(64) void debug_colours_kernel(VsfObserveDebugArgs a) {
  __shared__ uint32_t s_win[32];
  const int f0 = blockIdx.x, n = a.n_frames, K = a.max_rows, lane = (int)threadIdx.x;
  const VsfObserveParam p0 = a.params[f0];
  if (p0.prev >= 0) return;
  uint32_t* st = a.rand_state + (size_t)p0.stream * 32;
  {
    const int rear = min(max((int)st[31], 0), vsfrand::kWords - 1);
    if (lane < vsfrand::kWords) s_win[vsfrand::normalised_index(lane, rear)] = st[lane];
  }
  __syncthreads();
  uint32_t r[vsfrand::kWords];
#pragma unroll
  for (int i = 0; i < vsfrand::kWords; i++) r[i] = s_win[i];
  __syncthreads();
  for (int g0 = f0 & ~63; g0 < n; g0 += 64) {
    // the stream's frames among frames [g0, g0 + 64), as bits; walked lowest first: submission order
    const int g = g0 + lane;
    unsigned long long mine = __ballot(g >= f0 && g < n && a.params[min(g, n - 1)].stream == p0.stream);
    while (mine) {
      const int f = g0 + __ffsll((long long)mine) - 1;
      mine &= mine - 1;
      const int ns = min(max(a.npairs[f], 0), K);
      uint32_t* out = a.stream_colours + (size_t)f * K;
      for (int base = 0; base < ns; base += vsfrand::kWords) {
        const int m = min(ns - base, vsfrand::kWords);
        uint32_t keep = 0;
        vsfrand::colours31(r, m, [&](int j, uint32_t c) { keep = lane == j ? c : keep; });
        if (lane < m) out[base + lane] = keep;
      }
      const int rear = (int)((3 * (int64_t)ns) % vsfrand::kWords);
      if (rear != 0) {  // (uniform) the window back to rear pointer 0
        if (lane == 0) {
#pragma unroll
          for (int i = 0; i < vsfrand::kWords; i++) s_win[vsfrand::normalised_index(i, rear)] = r[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < vsfrand::kWords; i++) r[i] = s_win[i];
        __syncthreads();
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < vsfrand::kWords; i++) st[i] = r[i];
    st[31] = 0;
  }
}

// ---- the ObserveImage queue's debug images (vsf_observe_set_debug_images): one block per frame of a batch ----
// Stereo canvas 2f: cc:84-96 for every right -> left pair (pair f: initial = right row, current = left row), colours from
// the host's ring at the frame's offset (the colour cursor + the stereo pairs of the frames before it in the batch); absent
// when the frame has no such pair (cc:131-133).  Match canvas 2f + 1: cc:105-113 for the pairs of the factor against the
// newest kept frame (the frame before, in this batch or kept from the last); absent for a frame without kept frames.
__global__ __launch_bounds__(256) void debug_ops_kernel(VsfObserveDebugArgs a) {
  __shared__ int64_t s_col;
  const int f = blockIdx.x, K = a.max_rows, w = a.width, h = a.height, tid = (int)threadIdx.x;
  const VsfObserveFrame fm = a.frames[f];
  const int ns = min(max(a.npairs[f], 0), K);
  const bool per_stream = a.rand_state != nullptr;  // (vsf_observe_set_debug_seeds: the frame's colours are in stream_colours)
  if (tid == 0 && !per_stream) {
    int64_t c = *a.colour_cursor;
    for (int g = 0; g < f; g++) c += min(max(a.npairs[g], 0), K);
    s_col = c;
  }
  __syncthreads();
  const vsf_keypoint* kl = a.kp_f + (size_t)(2 * f) * K;
  const vsf_keypoint* kr = a.kp_f + (size_t)(2 * f + 1) * K;
  const int nl = min(max(a.counts_f[2 * f], 0), K), nr = min(max(a.counts_f[2 * f + 1], 0), K);
  vsf_draw_op* ops = a.ops + (size_t)f * 5 * K;
  const uint64_t* sp = a.pairs + (size_t)f * K * 2;
  for (int i = tid; i < ns; i += 256) {
    const uint64_t ri = sp[2 * i], li = sp[2 * i + 1];
    // (taken whether or not the rows are valid: cc:95)
    const uint32_t col = per_stream ? a.stream_colours[(size_t)f * K + i] : a.colours[(s_col + i) % a.colour_ring];
    vsf_draw_op* o = ops + 3 * i;
    if (ri >= (uint64_t)nr || li >= (uint64_t)nl) {
      o[0].kind = o[1].kind = o[2].kind = -1;  // (draws nothing)
      continue;
    }
    const int lx = __float2int_rn(kl[li].x), ly = __float2int_rn(kl[li].y);
    const int rx = __float2int_rn(kr[ri].x + (float)w), ry = __float2int_rn(kr[ri].y);  // cvRound, half to even
    o[0] = vsf_draw_op{VSF_DRAW_CIRCLE, lx, ly, 5, 0, {0, 0, 255, 0}};
    o[1] = vsf_draw_op{VSF_DRAW_CIRCLE, rx, ry, 5, 0, {0, 0, 255, 0}};
    o[2] = vsf_draw_op{VSF_DRAW_LINE, lx, ly, rx, ry, {(uint8_t)col, (uint8_t)(col >> 8), (uint8_t)(col >> 16), 0}};
  }
  int nm = 0;
  if (fm.n_past > 0) {
    const int p = fm.tp0 + fm.n_past - 1;
    nm = min(max(a.npairs[p], 0), K);
    // the newest kept frame: the frame of ITS stream in front of it in this batch, else what the stream kept from the last
    const int pf = a.params ? a.params[f].prev : f - 1, ps = a.params ? a.params[f].stream : 0;
    const vsf_keypoint* kp = pf >= 0 ? a.kp_f + (size_t)(2 * pf) * K : a.prev_kp + (size_t)ps * K;
    const int np = min(max(pf >= 0 ? a.counts_f[2 * pf] : a.prev_n[ps], 0), K);
    const uint64_t* tp = a.pairs + (size_t)p * K * 2;
    for (int i = tid; i < nm; i += 256) {
      const uint64_t pi = tp[2 * i], ci = tp[2 * i + 1];
      vsf_draw_op* o = ops + 3 * ns + 2 * i;
      if (pi >= (uint64_t)np || ci >= (uint64_t)nl) {
        o[0].kind = o[1].kind = -1;
        continue;
      }
      const int px = __float2int_rn(kp[pi].x), py = __float2int_rn(kp[pi].y);
      o[0] = vsf_draw_op{VSF_DRAW_CIRCLE, px, py, 5, 0, {0, 0, 255, 0}};
      o[1] = vsf_draw_op{VSF_DRAW_LINE, px, py, __float2int_rn(kl[ci].x), __float2int_rn(kl[ci].y), {0, 255, 0, 0}};
    }
  }
  if (tid < 2) {
    DrawCanvasDev d;
    const uint8_t* left = a.images + (size_t)(2 * f) * a.image_stride;
    d.src0 = left;
    d.src1 = tid == 0 ? left + a.image_stride : nullptr;
    d.width = w;
    d.height = h;
    d.cw = tid == 0 ? 2 * w : w;
    d.op_begin = f * 5 * K + (tid == 0 ? 0 : 3 * ns);
    d.op_count = tid == 0 ? 3 * ns : 2 * nm;
    d.skip = tid == 0 ? ns == 0 : fm.n_past == 0;
    d.src_pitch = (int64_t)a.image_pitch;
    d.out_pitch = (int64_t)3 * d.cw;
    d.out = a.canvas + (size_t)f * a.canvas_stride + (tid == 0 ? 0 : (size_t)6 * w * h);
    d.win = a.winners + (size_t)f * 3 * w * h + (tid == 0 ? 0 : (size_t)2 * w * h);
    static_cast<DrawCanvasDev*>(a.canvases)[2 * f + tid] = d;
  }
  if (tid == 0) {
    uint32_t* hdr = reinterpret_cast<uint32_t*>(a.out + (size_t)fm.out_slot * a.out_stride);
    hdr[14] = (ns > 0 ? 1u : 0u) | (fm.n_past > 0 ? 2u : 0u);
    hdr[15] = (uint32_t)ns;
  }
}

// after the batch: its newest frame's keypoints for the next batch's first match image; the colour cursor moves on
// (with a generator per stream: block f, where frame f is the first of its stream in the batch, keeps the stream's LAST frame
// of the batch -- params[f].tail -- in the stream's entry; a stream that is not in the batch keeps what it has)
__global__ __launch_bounds__(256) void debug_finish_kernel(VsfObserveDebugArgs a) {
  const int K = a.max_rows, tid = (int)threadIdx.x;
  int last = a.n_frames - 1, stream = 0;
  if (a.params) {
    const VsfObserveParam p = a.params[blockIdx.x];
    if (p.prev >= 0) return;
    last = p.tail;
    stream = p.stream;
  }
  const int n = min(max(a.counts_f[2 * last], 0), K);
  const vsf_keypoint* src = a.kp_f + (size_t)(2 * last) * K;
  vsf_keypoint* dst = a.prev_kp + (size_t)stream * K;
  for (int i = tid; i < n; i += 256) dst[i] = src[i];
  if (tid == 0) a.prev_n[stream] = n;
  if (tid == 0 && !a.rand_state) {
    int64_t c = *a.colour_cursor;
    for (int g = 0; g < a.n_frames; g++) c += min(max(a.npairs[g], 0), K);
    *a.colour_cursor = c;
  }
}

}  // namespace

void vsf_launch_observe_debug(const VsfObserveDebugArgs& a, hipStream_t s) {
  if (a.rand_state) hipLaunchKernelGGL(debug_colours_kernel, dim3((unsigned)a.n_frames), dim3(64), 0, s, a);
  hipLaunchKernelGGL(debug_ops_kernel, dim3((unsigned)a.n_frames), dim3(256), 0, s, a);
  const DrawCanvasDev* dc = static_cast<const DrawCanvasDev*>(a.canvases);
  hipLaunchKernelGGL(draw_raster_kernel, dim3(32, (unsigned)(2 * a.n_frames)), dim3(256), 0, s, dc, a.ops);
  hipLaunchKernelGGL(draw_resolve_kernel, dim3((unsigned)((2 * a.width * a.height + 255) / 256), (unsigned)(2 * a.n_frames)),
                     dim3(256), 0, s, dc);
  hipLaunchKernelGGL(debug_finish_kernel, dim3(a.params ? (unsigned)a.n_frames : 1u), dim3(256), 0, s, a);
}

extern "C" {

vsf_status vsf_draw_canvases_dev(vsf_ctx* ctx, const vsf_draw_canvas* canvases, int n, const vsf_draw_op* d_ops, int n_ops) {
  VsfErrorScope scope_(ctx);
  if (!ctx || n < 0 || n_ops < 0 || (n > 0 && !canvases) || (n_ops > 0 && !d_ops) || n > 65535) return VSF_ERR_INVALID_ARG;
  for (int i = 0; i < n; i++)
    if (check_canvas(canvases[i], n_ops) != VSF_OK) return VSF_ERR_INVALID_ARG;
  if (n == 0) return VSF_OK;
  VSF_HIP(hipSetDevice(ctx->device));
  return draw_dev(ctx, canvases, n, d_ops);
}

vsf_status vsf_draw_canvases(vsf_ctx* ctx, const vsf_draw_canvas* canvases, int n, const vsf_draw_op* ops, int n_ops) {
  VsfErrorScope scope_(ctx);
  if (!ctx || n < 0 || n_ops < 0 || (n > 0 && !canvases) || (n_ops > 0 && !ops) || n > 65535) return VSF_ERR_INVALID_ARG;
  for (int i = 0; i < n; i++)
    if (check_canvas(canvases[i], n_ops) != VSF_OK) return VSF_ERR_INVALID_ARG;
  if (n == 0) return VSF_OK;
  VSF_HIP(hipSetDevice(ctx->device));
  // one staging buffer: operations | per canvas its source(s) and its canvas, rows packed
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t total = up((size_t)n_ops * sizeof(vsf_draw_op));
  std::vector<vsf_draw_canvas> dev(canvases, canvases + n);
  std::vector<size_t> src_off((size_t)n), out_off((size_t)n);
  for (int i = 0; i < n; i++) {
    const vsf_draw_canvas& c = canvases[i];
    src_off[i] = total;
    total += up((size_t)c.width * c.height * (c.src1 ? 2 : 1));
    out_off[i] = total;
    total += up((size_t)3 * c.width * (c.src1 ? 2 : 1) * c.height);
  }
  VSF_HIP(hipStreamSynchronize(ctx->stream));  // (the previous call's kernels may still read the staging buffer)
  if (total > ctx->dr_buf_cap) {
    ctx->dr_buf_cap = 0;
    VSF_HIP(ctx->dr_buf.alloc(total));
    ctx->dr_buf_cap = total;
  }
  uint8_t* b = ctx->dr_buf;
  if (n_ops > 0) VSF_HIP(hipMemcpyAsync(b, ops, (size_t)n_ops * sizeof(vsf_draw_op), hipMemcpyHostToDevice, ctx->stream));
  for (int i = 0; i < n; i++) {
    const vsf_draw_canvas& c = canvases[i];
    vsf_draw_canvas& d = dev[(size_t)i];
    d.src0 = b + src_off[i];
    d.src1 = c.src1 ? b + src_off[i] + (size_t)c.width * c.height : nullptr;
    d.src_pitch = c.width;
    d.out = b + out_off[i];
    d.out_pitch = (int64_t)3 * c.width * (c.src1 ? 2 : 1);
    VSF_HIP(hipMemcpy2DAsync(b + src_off[i], (size_t)c.width, c.src0, (size_t)c.src_pitch, (size_t)c.width, (size_t)c.height,
                             hipMemcpyHostToDevice, ctx->stream));
    if (c.src1)
      VSF_HIP(hipMemcpy2DAsync(b + src_off[i] + (size_t)c.width * c.height, (size_t)c.width, c.src1, (size_t)c.src_pitch,
                               (size_t)c.width, (size_t)c.height, hipMemcpyHostToDevice, ctx->stream));
  }
  vsf_status st = draw_dev(ctx, dev.data(), n, reinterpret_cast<const vsf_draw_op*>(b));
  if (st != VSF_OK) return st;
  for (int i = 0; i < n; i++) {
    const vsf_draw_canvas& c = canvases[i];
    VSF_HIP(hipMemcpy2DAsync(c.out, (size_t)c.out_pitch, dev[(size_t)i].out, (size_t)dev[(size_t)i].out_pitch,
                             (size_t)dev[(size_t)i].out_pitch, (size_t)c.height, hipMemcpyDeviceToHost, ctx->stream));
  }
  VSF_HIP(hipStreamSynchronize(ctx->stream));
  VSF_STICKY();
  return VSF_OK;
}

}  // extern "C"
