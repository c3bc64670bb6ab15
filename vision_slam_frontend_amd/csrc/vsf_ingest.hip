// vsf_ingest.hip -- SURVEY section 8(f) row f4: the entry points of the image ingest (slam_frontend_main.cc:98-109):
// cv::imdecode(IMREAD_GRAYSCALE) for JPEG and PNG payloads, COLOR_BayerBG2BGR + COLOR_BGR2GRAY.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "vsf_ctx.h"

using namespace vsfi;

namespace {

// One policy for everything a decode or an encode outgrows: a quarter of headroom, and no wait for the GPU -- the outgrown buffer is
// retired (an upload or a decode already queued may still be using it) and released by the next vsf_sync, like every other
// scratch a *_dev call outgrows.
template <class T>
vsf_status grow_decode_scratch(vsf_ctx* ctx, DevBuf<T>& ptr, size_t& cap, size_t need) {
  if (need <= cap) return VSF_OK;
  const size_t want = need + need / 4;
  const vsf_status st = grow_scratch(ctx, ptr, want);
  if (st == VSF_OK) cap = want;
  return st;
}

vsf_status grow_staging(vsf_ctx* ctx, VsfStaging& stage, size_t need) {
  const size_t cap = need + need / 4 + 4096;
  PinnedBuf<uint8_t> host;
  DevBuf<uint8_t> dev;
  VSF_HIP(host.alloc(cap, hipHostMallocDefault));
  if (dev.alloc(cap) != hipSuccess) {
    (void)hipGetLastError();
    return VSF_ERR_HIP;
  }
  if (stage.h) ctx->retired_host.emplace_back(stage.h.release());
  if (stage.d) ctx->retired.emplace_back(stage.d.release());
  stage.h = std::move(host);
  stage.d = std::move(dev);
  stage.cap = cap;
  return VSF_OK;
}

// a pipelined extract that follows (vsf_set_pipeline) builds its pyramid off this stream: give it something to wait for
vsf_status record_ingest_done(vsf_ctx* ctx) {
  if (!ctx->ev_ingest_done) VSF_HIP(ctx->ev_ingest_done.alloc(hipEventDisableTiming));
  VSF_HIP(hipEventRecord(ctx->ev_ingest_done, ctx->stream));
  ctx->ingest_done_valid = true;
  return VSF_OK;
}

// vsf_jpeg_decode_gray_batch / vsf_png_decode_gray_batch and their _bgr_ siblings: n_images files of ONE format, asynchronous
// on the context's stream.  out_format = VSF_OUT_BGR: three bytes a pixel, and a row must hold them rounded up to a dword.
vsf_status decode_batch(vsf_ctx* ctx, uint8_t kind, const uint8_t* const* files, const size_t* nbytes, int n_images,
                        int width, int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride,
                        int reduce = 1, int out_format = VSF_OUT_GRAY) {
  VsfErrorScope scope_(ctx);
  if (!vsf_reduce_ok(reduce)) return VSF_ERR_INVALID_ARG;
  if (!ctx || !files || !nbytes || n_images < 1 || n_images > 65535 || width < 1 || height < 1 || width > 65535 ||
      height > 65535 || !d_dst)
    return VSF_ERR_INVALID_ARG;
  const size_t min_row = out_format == VSF_OUT_BGR ? (3 * (size_t)width + 3) & ~(size_t)3 : (size_t)width;
  if (((uintptr_t)d_dst & 3) || (dst_image_stride & 3) || (dst_row_stride & 3) || dst_row_stride < min_row ||
      dst_row_stride > 0x7FFFFFFF || dst_image_stride < dst_row_stride * (size_t)height)
    return VSF_ERR_INVALID_ARG;
  const size_t min_bytes = kind == VSF_FILE_JPEG ? 4 : 8;
  for (int i = 0; i < n_images; i++)
    if (!files[i] || nbytes[i] < min_bytes || nbytes[i] > 0x40000000u) return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  // the staging pair the call before the previous one used: its upload has left it long ago (the previous call's upload and
  // decode are what may still be running, out of the OTHER pair)
  VsfStaging& stage = ctx->ingest_stage[ctx->ingest_flip];
  if (!stage.uploaded) VSF_HIP(stage.uploaded.alloc(hipEventDisableTiming));
  const std::vector<uint8_t> kinds((size_t)n_images, kind), reduces((size_t)n_images, (uint8_t)reduce);
  const vsf_status st = decode_runs(ctx, files, nbytes, kinds.data(), n_images, width, height, stage, ctx->ingest_scratch, d_dst,
                                    dst_image_stride, (int)dst_row_stride, ctx->d_status, 0, ctx->stream, nullptr,
                                    reduce > 1 ? reduces.data() : nullptr, out_format);
  if (st != VSF_OK) return st;  // (refused by the host half: nothing was uploaded or launched)
  ctx->ingest_flip ^= 1;
  VSF_STICKY();
  return record_ingest_done(ctx);  // (a pipelined extract waits for its images, as after the Bayer step)
}

// ---- the ONE way pixels leave the device as files: vsf_jpeg_encode* and vsf_png_encode* are argument adapters of these two ----
bool encode_job_ok(const VsfEncodeJob& j) {  // what both forms of the call refuse as VSF_ERR_INVALID_ARG
  return j.n >= 1 && j.n <= 65535 && j.width >= 1 && j.height >= 1 && j.width <= 65535 && j.height <= 65535 &&
         (j.channels == 1 || j.channels == 3) && j.quality >= 0 && j.quality <= 100 && j.out_stride >= 1 &&
         j.src_row_stride >= (size_t)j.width * (size_t)j.channels && j.src_image_stride >= j.src_row_stride * (size_t)j.height;
}

vsf_status encode_batch_dev(vsf_ctx* ctx, VsfEncodeJob job, const uint8_t* d_src, uint8_t* d_out, int32_t* d_out_bytes) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !d_src || !d_out || !d_out_bytes || !encode_job_ok(job) || ((uintptr_t)d_out_bytes & 3)) return VSF_ERR_INVALID_ARG;
  // the byte count of a file is an int32, the block / byte index of the kernels a u32
  if (vsf_encode_capacity(job.kind, job.width, job.height, job.channels) > 0x7FFFFFFFu) return VSF_ERR_UNSUPPORTED;
  VSF_HIP(hipSetDevice(ctx->device));
  if (job.quality == 0) job.quality = 95;
  VsfEncodeScratch& e = ctx->encode;
  const vsf_status gs = grow_decode_scratch(ctx, e.scratch, e.scratch_cap, vsf_encode_scratch_need(job));  // (no wait)
  if (gs != VSF_OK) return gs;
  vsf_launch_encode(job, d_src, e.scratch, d_out, d_out_bytes, ctx->d_status, ctx->stream);
  VSF_STICKY();
  return VSF_OK;
}

vsf_status encode_host(vsf_ctx* ctx, VsfEncodeJob job, const uint8_t* src, uint8_t* out, int32_t* out_bytes) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !src || !out || !out_bytes || !encode_job_ok(job)) return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  // device staging: images (packed rows) | files | byte counts
  const size_t row = (size_t)job.width * (size_t)job.channels, n = (size_t)job.n;
  const size_t img_bytes = (row * (size_t)job.height + 15) & ~(size_t)15, files_bytes = (n * job.out_stride + 15) & ~(size_t)15;
  const size_t need = n * (img_bytes + sizeof(int32_t)) + files_bytes;
  VsfEncodeScratch& e = ctx->encode;
  if (need > e.staging_cap) {
    const vsf_status gs = grow_scratch(ctx, e.staging, need);
    if (gs != VSF_OK) return gs;
    e.staging_cap = need;
  }
  uint8_t* d_img = e.staging;
  uint8_t* d_files = d_img + n * img_bytes;
  int32_t* d_bytes = reinterpret_cast<int32_t*>(d_files + files_bytes);
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(d_img + i * img_bytes, row, src + i * job.src_image_stride, job.src_row_stride, row, (size_t)job.height,
                             hipMemcpyHostToDevice, ctx->stream));
  job.src_image_stride = img_bytes;
  job.src_row_stride = row;
  vsf_status st = encode_batch_dev(ctx, job, d_img, d_files, d_bytes);
  if (st != VSF_OK) return st;
  VSF_HIP(hipMemcpyAsync(out_bytes, d_bytes, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  st = check_status_word(ctx);  // synchronises
  if (st != VSF_OK && st != VSF_ERR_CAPACITY) return st;
  for (size_t i = 0; i < n; i++)
    if (out_bytes[i] > 0)
      VSF_HIP(hipMemcpy(out + i * job.out_stride, d_files + i * job.out_stride, (size_t)out_bytes[i], hipMemcpyDeviceToHost));
  return st;
}

}  // namespace

namespace vsfi {

vsf_status decode_runs(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, const uint8_t* kinds, int n, int width,
                       int height, VsfStaging& stage, VsfDecodeScratch& scratch, uint8_t* d_dst, size_t dst_image_stride,
                       int dst_pitch, int32_t* d_status, int status_stride, hipStream_t s, int* n_runs, const uint8_t* reduces,
                       int out_format) {
  if (n_runs) *n_runs = 0;
  const bool serial = ctx->tuning.jpeg_serial != 0;
  VsfDecodeRuns plan;
  vsf_status st = vsf_plan_runs(files, nbytes, kinds, n, width, height, serial, &plan, reduces, out_format);
  if (st != VSF_OK || plan.runs.empty()) return st;
  VsfDecodeNeed need;  // the runs decode one after the other on `s`: they share one scratch of the largest need
  for (const VsfDecodeRun& r : plan.runs) {
    const VsfDecodeNeed q = r.kind == VSF_FILE_JPEG ? vsf_jpeg_scratch_need(r.jp) : vsf_png_scratch_need(r.pp, r.n);
    need.clean = std::max(need.clean, q.clean);
    need.coef = std::max(need.coef, q.coef);
    need.flags = std::max(need.flags, q.flags);
    need.filtered = std::max(need.filtered, q.filtered);
    need.file_status = std::max(need.file_status, q.file_status);
    need.planes = std::max(need.planes, q.planes);
  }
  if (plan.total > stage.cap)
    st = grow_staging(ctx, stage, plan.total);
  else if (stage.uploaded)
    VSF_HIP(hipEventSynchronize(stage.uploaded));
  if (st == VSF_OK) st = grow_decode_scratch(ctx, scratch.clean, scratch.clean_cap, need.clean);
  if (st == VSF_OK) st = grow_decode_scratch(ctx, scratch.coef, scratch.coef_cap, need.coef);
  if (st == VSF_OK) st = grow_decode_scratch(ctx, scratch.flags, scratch.flags_cap, need.flags);
  if (st == VSF_OK) st = grow_decode_scratch(ctx, scratch.filtered, scratch.filtered_cap, need.filtered);
  if (st == VSF_OK) st = grow_decode_scratch(ctx, scratch.file_status, scratch.file_status_cap, need.file_status);
  if (st == VSF_OK) st = grow_decode_scratch(ctx, scratch.planes, scratch.planes_cap, need.planes);
  if (st != VSF_OK) return st;
  vsf_fill_runs(plan, files, stage.h);  // the one pass over the compressed bytes on the host
  VSF_HIP(hipMemcpyAsync(stage.d, stage.h, plan.total, hipMemcpyHostToDevice, s));
  if (stage.uploaded) VSF_HIP(hipEventRecord(stage.uploaded, s));
  for (const VsfDecodeRun& r : plan.runs) {
    const uint8_t* blob = stage.d + r.off;
    uint8_t* dst = d_dst + (size_t)r.i0 * dst_image_stride;
    int32_t* status = d_status + (size_t)r.i0 * status_stride;
    if (r.kind == VSF_FILE_JPEG)
      vsf_launch_jpeg_decode(blob, r.jp, r.n, width, height, scratch, dst, dst_image_stride, dst_pitch, status, status_stride,
                             serial, s);
    else
      vsf_launch_png_decode(blob, r.pp, r.n, width, height, scratch, dst, dst_image_stride, dst_pitch, status, status_stride, s);
  }
  if (n_runs) *n_runs = (int)plan.runs.size();
  return VSF_OK;
}

}  // namespace vsfi

extern "C" {

vsf_status vsf_bayer_bg_to_gray_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height,
                                          size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst,
                                          size_t dst_image_stride, size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !d_src || !d_dst || n_images < 1 || width < 1 || height < 1 || width > 16384 || height > 65535 ||
      n_images > 65535)
    return VSF_ERR_INVALID_ARG;
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3) || (src_image_stride & 3) || (src_row_stride & 3) ||
      (dst_image_stride & 3) || (dst_row_stride & 3) || src_row_stride < (size_t)width ||
      dst_row_stride < (size_t)((width + 3) & ~3) || src_row_stride > 0x7FFFFFFF || dst_row_stride > 0x7FFFFFFF ||
      src_image_stride < src_row_stride * (size_t)height || dst_image_stride < dst_row_stride * (size_t)height)
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  vsf_launch_bayer_bg_gray(d_src, n_images, width, height, src_image_stride, (int)src_row_stride, d_dst,
                           dst_image_stride, (int)dst_row_stride, ctx->stream);
  VSF_STICKY();
  return record_ingest_done(ctx);
}

// Every raw pixel format -> gray (k_ingest.hip): the four Bayer orders, packed colour, and the copy MONO8 is.
vsf_status vsf_to_gray_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int pixfmt,
                                 size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst, size_t dst_image_stride,
                                 size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (!ctx || !d_src || !d_dst || bpp == 0 || n_images < 1 || width < 1 || height < 1 || width > 16384 || height > 65535 ||
      n_images > 65535)
    return VSF_ERR_INVALID_ARG;
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3) || (src_image_stride & 3) || (src_row_stride & 3) ||
      (dst_image_stride & 3) || (dst_row_stride & 3) || src_row_stride < (size_t)width * (size_t)bpp ||
      dst_row_stride < (size_t)((width + 3) & ~3) || src_row_stride * (size_t)height > 0x7FFFFFFF ||
      dst_row_stride * (size_t)height > 0x7FFFFFFF || src_image_stride < src_row_stride * (size_t)height ||
      dst_image_stride < dst_row_stride * (size_t)height)
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  vsf_launch_to_gray(pixfmt, d_src, n_images, width, height, src_image_stride, (int)src_row_stride, d_dst, dst_image_stride,
                     (int)dst_row_stride, ctx->stream);
  VSF_STICKY();
  return record_ingest_done(ctx);
}

// cv::resize(src, dst, Size(dst_width, dst_height)), INTER_LINEAR on CV_8UC1 (k_resize.hip): what cv::imdecode's reduced
// modes do to a PNG, and how a camera of another size than the context's gets in.
vsf_status vsf_resize_gray_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int src_width, int src_height,
                                     size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst, int dst_width,
                                     int dst_height, size_t dst_image_stride, size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !d_src || !d_dst || n_images < 1 || !vsf_resize_size_ok(src_width, src_height) ||
      !vsf_resize_size_ok(dst_width, dst_height) || src_row_stride < (size_t)src_width || dst_row_stride < (size_t)dst_width)
    return VSF_ERR_INVALID_ARG;
  // (images may overlap their neighbours' padding, not their pixels; one image: the stride is not looked at)
  if (n_images > 1 && (src_image_stride < (size_t)(src_height - 1) * src_row_stride + (size_t)src_width ||
                       dst_image_stride < (size_t)(dst_height - 1) * dst_row_stride + (size_t)dst_width))
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  vsf_launch_resize_gray(d_src, n_images, src_width, src_height, src_image_stride, src_row_stride, d_dst, dst_width, dst_height,
                         dst_image_stride, dst_row_stride, ctx->stream);
  VSF_STICKY();
  return record_ingest_done(ctx);
}

// ... for host pointers, synchronous: up, the kernel, down (device staging shared with the host-pointer encoders: both wait).
vsf_status vsf_resize_gray(vsf_ctx* ctx, const uint8_t* src, int n_images, int src_width, int src_height, size_t src_image_stride,
                           size_t src_row_stride, uint8_t* dst, int dst_width, int dst_height, size_t dst_image_stride,
                           size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !src || !dst || n_images < 1 || n_images > 65535 || !vsf_resize_size_ok(src_width, src_height) ||
      !vsf_resize_size_ok(dst_width, dst_height) || src_row_stride < (size_t)src_width || dst_row_stride < (size_t)dst_width)
    return VSF_ERR_INVALID_ARG;
  if (n_images > 1 && (src_image_stride < (size_t)(src_height - 1) * src_row_stride + (size_t)src_width ||
                       dst_image_stride < (size_t)(dst_height - 1) * dst_row_stride + (size_t)dst_width))
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  // device staging: sources (packed rows) | destinations (rows at a multiple of 4: dword stores)
  const size_t n = (size_t)n_images, sp = (size_t)src_width, dp = ((size_t)dst_width + 3) & ~(size_t)3;
  const size_t s_img = (sp * (size_t)src_height + 15) & ~(size_t)15, d_img = (dp * (size_t)dst_height + 15) & ~(size_t)15;
  const size_t need = n * (s_img + d_img);
  VsfEncodeScratch& e = ctx->encode;
  if (need > e.staging_cap) {
    const vsf_status gs = grow_scratch(ctx, e.staging, need);
    if (gs != VSF_OK) return gs;
    e.staging_cap = need;
  }
  uint8_t* d_src = e.staging;
  uint8_t* d_dst = d_src + n * s_img;
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(d_src + i * s_img, sp, src + i * src_image_stride, src_row_stride, sp, (size_t)src_height,
                             hipMemcpyHostToDevice, ctx->stream));
  vsf_launch_resize_gray(d_src, n_images, src_width, src_height, s_img, sp, d_dst, dst_width, dst_height, d_img, dp, ctx->stream);
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(dst + i * dst_image_stride, dst_row_stride, d_dst + i * d_img, dp, (size_t)dst_width,
                             (size_t)dst_height, hipMemcpyDeviceToHost, ctx->stream));
  VSF_HIP(hipStreamSynchronize(ctx->stream));
  VSF_STICKY();
  return VSF_OK;
}

// vsf_to_gray_batch_dev host to host (the per-call mode's way in for frames that are not gray): upload, the one launch, download.
vsf_status vsf_to_gray(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int pixfmt, size_t src_image_stride,
                       size_t src_row_stride, uint8_t* dst, size_t dst_image_stride, size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (!ctx || !src || !dst || bpp == 0 || n_images < 1 || n_images > 65535 || width < 1 || height < 1 || width > 16384 ||
      height > 32767 || src_row_stride < (size_t)width * (size_t)bpp || dst_row_stride < (size_t)width)
    return VSF_ERR_INVALID_ARG;
  const size_t n = (size_t)n_images, row = (size_t)width * (size_t)bpp;
  if (n > 1 && (src_image_stride < (size_t)(height - 1) * src_row_stride + row ||
                dst_image_stride < (size_t)(height - 1) * dst_row_stride + (size_t)width))
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  // device staging: sources | destinations, rows at a multiple of 4 on both sides (the kernels' rule)
  const size_t sp = (row + 3) & ~(size_t)3, dp = ((size_t)width + 3) & ~(size_t)3;
  const size_t s_img = (sp * (size_t)height + 15) & ~(size_t)15, d_img = (dp * (size_t)height + 15) & ~(size_t)15;
  if (s_img > 0x7FFFFFFFu) return VSF_ERR_INVALID_ARG;
  const size_t need = n * (s_img + d_img);
  VsfEncodeScratch& e = ctx->encode;
  if (need > e.staging_cap) {
    const vsf_status gs = grow_scratch(ctx, e.staging, need);
    if (gs != VSF_OK) return gs;
    e.staging_cap = need;
  }
  uint8_t* d_src = e.staging;
  uint8_t* d_dst = d_src + n * s_img;
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(d_src + i * s_img, sp, src + i * src_image_stride, src_row_stride, row, (size_t)height,
                             hipMemcpyHostToDevice, ctx->stream));
  vsf_launch_to_gray(pixfmt, d_src, n_images, width, height, s_img, (int)sp, d_dst, d_img, (int)dp, ctx->stream);
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(dst + i * dst_image_stride, dst_row_stride, d_dst + i * d_img, dp, (size_t)width, (size_t)height,
                             hipMemcpyDeviceToHost, ctx->stream));
  VSF_HIP(hipStreamSynchronize(ctx->stream));
  VSF_STICKY();
  return VSF_OK;
}

// Every raw pixel format -> B G R (k_to_bgr.hip): the four Bayer orders (cvtColor(COLOR_Bayer??2BGR), bag_extract.cc:78-82), and the
// packed formats as cv_bridge converts them for "bgr8".  The sibling of vsf_to_gray_batch_dev; the destination is
// vsf_imdecode_bgr_batch's layout.
vsf_status vsf_to_bgr_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int pixfmt,
                                size_t src_image_stride, size_t src_row_stride, uint8_t* d_dst, size_t dst_image_stride,
                                size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (!ctx || !d_src || !d_dst || bpp == 0 || n_images < 1 || width < 1 || height < 1 || width > 16384 || height > 65535 ||
      n_images > 65535)
    return VSF_ERR_INVALID_ARG;
  if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3) || (src_image_stride & 3) || (src_row_stride & 3) ||
      (dst_image_stride & 3) || (dst_row_stride & 3) || src_row_stride < (size_t)width * (size_t)bpp ||
      dst_row_stride < ((3 * (size_t)width + 3) & ~(size_t)3) || src_row_stride * (size_t)height > 0x7FFFFFFF ||
      dst_row_stride * (size_t)height > 0x7FFFFFFF || src_image_stride < src_row_stride * (size_t)height ||
      dst_image_stride < dst_row_stride * (size_t)height)
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  vsf_launch_to_bgr(pixfmt, d_src, n_images, width, height, src_image_stride, (int)src_row_stride, d_dst, dst_image_stride,
                    (int)dst_row_stride, ctx->stream);
  VSF_STICKY();
  return record_ingest_done(ctx);
}

// vsf_to_bgr_batch_dev host to host: upload, the one launch, download (device staging shared with vsf_to_gray and the encoders).
vsf_status vsf_to_bgr(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int pixfmt, size_t src_image_stride,
                      size_t src_row_stride, uint8_t* dst, size_t dst_image_stride, size_t dst_row_stride) {
  VsfErrorScope scope_(ctx);
  const int bpp = vsf_pixfmt_bytes_per_pixel(pixfmt);
  if (!ctx || !src || !dst || bpp == 0 || n_images < 1 || n_images > 65535 || width < 1 || height < 1 || width > 16384 ||
      height > 32767 || src_row_stride < (size_t)width * (size_t)bpp || dst_row_stride < 3 * (size_t)width)
    return VSF_ERR_INVALID_ARG;
  const size_t n = (size_t)n_images, row = (size_t)width * (size_t)bpp, out_row = 3 * (size_t)width;
  if (n > 1 && (src_image_stride < (size_t)(height - 1) * src_row_stride + row ||
                dst_image_stride < (size_t)(height - 1) * dst_row_stride + out_row))
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  // device staging: sources | destinations, rows at a multiple of 4 on both sides (the kernels' rule)
  const size_t sp = (row + 3) & ~(size_t)3, dp = (out_row + 3) & ~(size_t)3;
  const size_t s_img = (sp * (size_t)height + 15) & ~(size_t)15, d_img = (dp * (size_t)height + 15) & ~(size_t)15;
  if (s_img > 0x7FFFFFFFu || d_img > 0x7FFFFFFFu) return VSF_ERR_INVALID_ARG;
  const size_t need = n * (s_img + d_img);
  VsfEncodeScratch& e = ctx->encode;
  if (need > e.staging_cap) {
    const vsf_status gs = grow_scratch(ctx, e.staging, need);
    if (gs != VSF_OK) return gs;
    e.staging_cap = need;
  }
  uint8_t* d_src = e.staging;
  uint8_t* d_dst = d_src + n * s_img;
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(d_src + i * s_img, sp, src + i * src_image_stride, src_row_stride, row, (size_t)height,
                             hipMemcpyHostToDevice, ctx->stream));
  vsf_launch_to_bgr(pixfmt, d_src, n_images, width, height, s_img, (int)sp, d_dst, d_img, (int)dp, ctx->stream);
  for (size_t i = 0; i < n; i++)
    VSF_HIP(hipMemcpy2DAsync(dst + i * dst_image_stride, dst_row_stride, d_dst + i * d_img, dp, out_row, (size_t)height,
                             hipMemcpyDeviceToHost, ctx->stream));
  VSF_HIP(hipStreamSynchronize(ctx->stream));
  VSF_STICKY();
  return VSF_OK;
}

// src/test/bag_extract.cc:73-90 for n payloads of one size: cv::imdecode(data, 1); on a "bayer_rggb8" topic cv::split -> channel 0
// -> cvtColor(COLOR_BayerBG2BGR); cv::imwrite(".jpg") (quality 95).  Host to host, synchronous; between the stages nothing leaves
// the device.  The mosaic is channel 0 of the COLOUR read of every file.  Per file, from the frame header the host parser reads:
//   a JPEG file of ONE component -- B = G = R = Y, and with one component vsf_jpeg_plan does the same in both output formats (its
//     colour argument acts on three components only), so the refusals are the same too -- is decoded by the gray decoders straight
//     into its mosaic;
//   every other file (three components: the mosaic is the BLUE channel, not the gray read; every PNG: the gray read of a PNG
//     refuses gamma chunks the colour read ignores) takes the colour decode, and k_to_bgr.hip keeps the first byte of every pixel.
vsf_status vsf_bag_extract_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images, int width,
                                 int height, int bayer_pixfmt, int quality, uint8_t* out, size_t out_stride, int32_t* out_bytes) {
  VsfErrorScope scope_(ctx);
  if (out_bytes && n_images >= 1 && n_images <= 65535)
    for (int i = 0; i < n_images; i++) out_bytes[i] = -1;  // (whatever follows: no partial delivery)
  const bool bayer = bayer_pixfmt != 0;
  if (bayer && bayer_pixfmt != VSF_PIX_BAYER_RGGB8 && bayer_pixfmt != VSF_PIX_BAYER_GRBG8 && bayer_pixfmt != VSF_PIX_BAYER_GBRG8 &&
      bayer_pixfmt != VSF_PIX_BAYER_BGGR8)
    return VSF_ERR_INVALID_ARG;
  if (!ctx || !files || !nbytes || !out || !out_bytes || n_images < 1 || n_images > 65535 || width < 1 || height < 1 ||
      width > 65535 || height > 65535 || quality < 0 || quality > 100 || out_stride < 1)
    return VSF_ERR_INVALID_ARG;
  const size_t n = (size_t)n_images;
  const size_t bp = (3 * (size_t)width + 3) & ~(size_t)3, mp = ((size_t)width + 3) & ~(size_t)3;  // rows of B G R / of a mosaic
  if (bp * (size_t)height > 0x7FFFFFFF || (bayer && width > 16384)) return VSF_ERR_INVALID_ARG;  // (vsf_to_bgr_batch_dev's limits)
  // which decode each file takes: kinds_bgr / kinds_gray name the file in ONE of the two lists and VSF_FILE_NONE in the other
  std::vector<uint8_t> kinds_bgr(n), kinds_gray(n, (uint8_t)VSF_FILE_NONE);
  size_t n_gray = 0;
  for (size_t i = 0; i < n; i++) {
    if (!files[i] || nbytes[i] > 0x40000000u) return VSF_ERR_INVALID_ARG;
    kinds_bgr[i] = (uint8_t)vsf_file_kind(files[i], nbytes[i]);
    if (kinds_bgr[i] == VSF_FILE_NONE) return VSF_ERR_UNSUPPORTED;
    if (nbytes[i] < (kinds_bgr[i] == VSF_FILE_JPEG ? 4u : 8u)) return VSF_ERR_INVALID_ARG;
    if (bayer && kinds_bgr[i] == VSF_FILE_JPEG && vsf_jpeg_frame_components(files[i], nbytes[i]) == 1) {
      kinds_gray[i] = VSF_FILE_JPEG;
      kinds_bgr[i] = VSF_FILE_NONE;
      n_gray++;
    }
  }
  VSF_HIP(hipSetDevice(ctx->device));
  // scratch: [the mosaics | what cv::imwrite gets | the colour reads in front of cv::split] on a Bayer topic, else the colour reads alone
  const size_t bgr_img = (bp * (size_t)height + 15) & ~(size_t)15, mono_img = (mp * (size_t)height + 15) & ~(size_t)15;
  const size_t files_bytes = (n * out_stride + 15) & ~(size_t)15;
  VsfBagScratch& b = ctx->bag;
  const size_t images_need = !bayer ? n * bgr_img : n * (mono_img + bgr_img) + (n_gray < n ? n * bgr_img : 0);
  vsf_status st = grow_decode_scratch(ctx, b.images, b.images_cap, images_need);
  if (st == VSF_OK) st = grow_decode_scratch(ctx, b.files, b.files_cap, files_bytes + n * sizeof(int32_t));
  if (st != VSF_OK) return st;
  uint8_t* d_mosaic = b.images;
  uint8_t* d_colour = bayer ? d_mosaic + n * mono_img : b.images.get();  // what cv::imwrite gets
  uint8_t* d_read = bayer ? d_colour + n * bgr_img : d_colour;             // cv::imdecode(data, 1)
  uint8_t* d_files = b.files;
  int32_t* d_bytes = reinterpret_cast<int32_t*>(d_files + files_bytes);
  bool launched = false;
  for (int pass = 0; pass < 2 && st == VSF_OK; pass++) {  // the colour reads, then the gray ones: a staging pair each
    if (pass == 0 ? n_gray == n : n_gray == 0) continue;
    VsfStaging& stage = ctx->ingest_stage[ctx->ingest_flip];
    if (!stage.uploaded) VSF_HIP(stage.uploaded.alloc(hipEventDisableTiming));
    st = pass == 0 ? decode_runs(ctx, files, nbytes, kinds_bgr.data(), n_images, width, height, stage, ctx->ingest_scratch, d_read,
                                 bgr_img, (int)bp, ctx->d_status, 0, ctx->stream, nullptr, nullptr, VSF_OUT_BGR)
                   : decode_runs(ctx, files, nbytes, kinds_gray.data(), n_images, width, height, stage, ctx->ingest_scratch,
                                 d_mosaic, mono_img, (int)mp, ctx->d_status, 0, ctx->stream, nullptr, nullptr, VSF_OUT_GRAY);
    if (st != VSF_OK) break;  // (refused by the host half -- another size among them --: this pass uploaded and launched nothing)
    ctx->ingest_flip ^= 1;
    launched = true;
  }
  if (st != VSF_OK) {
    if (launched) (void)check_status_word(ctx);  // the other pass is under way: wait for it and drop what it reports
    return st;
  }
  if (bayer) {
    for (int i0 = 0, i1; i0 < n_images; i0 = i1) {  // cv::split -> channel 0 of every run of colour reads
      i1 = vsf_run_end(kinds_gray.data(), n_images, i0);
      if (kinds_gray[i0] != VSF_FILE_NONE) continue;
      vsf_launch_bgr_channel0(d_read + (size_t)i0 * bgr_img, i1 - i0, width, height, bgr_img, (int)bp, d_mosaic + (size_t)i0 * mono_img,
                              mono_img, (int)mp, ctx->stream);
    }
    vsf_launch_to_bgr(bayer_pixfmt, d_mosaic, n_images, width, height, mono_img, (int)mp, d_colour, bgr_img, (int)bp, ctx->stream);
  }
  VSF_STICKY();
  st = encode_batch_dev(ctx, {VSF_FILE_JPEG, n_images, width, height, 3, bgr_img, bp, quality, out_stride, 0}, d_colour, d_files,
                        d_bytes);
  std::vector<int32_t> sizes(n, -1);
  if (st == VSF_OK) VSF_HIP(hipMemcpyAsync(sizes.data(), d_bytes, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  const vsf_status word = check_status_word(ctx);  // synchronises (and clears what the decoders reported, whatever the encoder said)
  if (st == VSF_OK) st = word;
  if (st != VSF_OK && st != VSF_ERR_CAPACITY) return st;
  // The files home: packed one behind the other into pinned memory by asynchronous copies, ONE wait, then the host's own copies
  // into the caller's slots (a hipMemcpy into pageable memory waits for itself, file after file).
  size_t total = 0;
  for (size_t i = 0; i < n; i++)
    if (sizes[i] > 0) total += ((size_t)sizes[i] + 15) & ~(size_t)15;
  if (total > b.home_cap) {  // (the stream is idle: nothing reads the outgrown buffer)
    b.home_cap = 0;
    VSF_HIP(b.home.alloc(total + total / 4, hipHostMallocDefault));
    b.home_cap = total + total / 4;
  }
  size_t off = 0;
  for (size_t i = 0; i < n; i++)
    if (sizes[i] > 0) {
      VSF_HIP(hipMemcpyAsync(b.home + off, d_files + i * out_stride, (size_t)sizes[i], hipMemcpyDeviceToHost, ctx->stream));
      off += ((size_t)sizes[i] + 15) & ~(size_t)15;
    }
  VSF_HIP(hipStreamSynchronize(ctx->stream));
  off = 0;
  for (size_t i = 0; i < n; i++) {
    if (sizes[i] > 0) {
      std::memcpy(out + i * out_stride, b.home + off, (size_t)sizes[i]);
      off += ((size_t)sizes[i] + 15) & ~(size_t)15;
    }
    out_bytes[i] = sizes[i] > 0 ? sizes[i] : -1;
  }
  return st;
}

// cv::imdecode(IMREAD_GRAYSCALE) for JPEG files (slam_frontend_main.cc:99-100): markers and tables on the host, the entropy
// decode and the IDCT on the device (k_jpeg.hip).
vsf_status vsf_jpeg_decode_gray_batch(vsf_ctx* ctx, const uint8_t* const* jpeg, const size_t* nbytes, int n_images,
                                      int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                      size_t dst_row_stride) {
  return decode_batch(ctx, VSF_FILE_JPEG, jpeg, nbytes, n_images, width, height, d_dst, dst_image_stride, dst_row_stride);
}

// ... and for PNG files: chunks and CRCs on the host, inflate + filters on the device (k_png.hip).  Same staging and the same
// asynchronous contract.
vsf_status vsf_png_decode_gray_batch(vsf_ctx* ctx, const uint8_t* const* png, const size_t* nbytes, int n_images,
                                     int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                     size_t dst_row_stride) {
  return decode_batch(ctx, VSF_FILE_PNG, png, nbytes, n_images, width, height, d_dst, dst_image_stride, dst_row_stride);
}

// cv::imdecode(msg.data, IMREAD_GRAYSCALE) as the reference calls it (slam_frontend_main.cc:99-100): whatever the payload
// is.  Files are told apart by their first bytes and handed, run by run of one format and in order, to the JPEG or the PNG
// decode above (an upload per run: a run a decoder refuses undoes nothing of the runs before it); image i lands at
// d_dst + i * dst_image_stride either way.
vsf_status vsf_imdecode_gray_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images,
                                   int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                   size_t dst_row_stride) {
  if (!ctx || !files || !nbytes || n_images < 1 || !d_dst) return VSF_ERR_INVALID_ARG;
  std::vector<uint8_t> kinds((size_t)n_images);
  for (int i = 0; i < n_images; i++) {
    kinds[i] = (uint8_t)vsf_file_kind(files[i], nbytes[i]);
    if (kinds[i] == VSF_FILE_NONE) return VSF_ERR_UNSUPPORTED;
  }
  for (int i0 = 0, i1; i0 < n_images; i0 = i1) {
    i1 = vsf_run_end(kinds.data(), n_images, i0);
    const vsf_status st = decode_batch(ctx, kinds[i0], files + i0, nbytes + i0, i1 - i0, width, height,
                                            d_dst + (size_t)i0 * dst_image_stride, dst_image_stride, dst_row_stride);
    if (st != VSF_OK) return st;
  }
  return VSF_OK;
}

// cv::imdecode(data, cv::IMREAD_COLOR) for PNG files (bag_extract.cc:73 reads a CompressedImage that way): the same chunks,
// inflate and filters; the last step per pixel is png_set_bgr / png_set_gray_to_rgb in place of png_set_rgb_to_gray.
vsf_status vsf_png_decode_bgr_batch(vsf_ctx* ctx, const uint8_t* const* png, const size_t* nbytes, int n_images, int width,
                                    int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride) {
  return decode_batch(ctx, VSF_FILE_PNG, png, nbytes, n_images, width, height, d_dst, dst_image_stride, dst_row_stride, 1, VSF_OUT_BGR);
}

vsf_status vsf_jpeg_decode_bgr_batch(vsf_ctx* ctx, const uint8_t* const* jpeg, const size_t* nbytes, int n_images, int width,
                                     int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride) {
  return decode_batch(ctx, VSF_FILE_JPEG, jpeg, nbytes, n_images, width, height, d_dst, dst_image_stride, dst_row_stride, 1, VSF_OUT_BGR);
}

// ... and whatever the payload is, run by run as vsf_imdecode_gray_batch: the runs in front of one that is refused have been
// launched and are not undone.
vsf_status vsf_imdecode_bgr_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images, int width,
                                  int height, uint8_t* d_dst, size_t dst_image_stride, size_t dst_row_stride) {
  if (!ctx || !files || !nbytes || n_images < 1 || !d_dst) return VSF_ERR_INVALID_ARG;
  std::vector<uint8_t> kinds((size_t)n_images);
  for (int i = 0; i < n_images; i++) {
    kinds[i] = (uint8_t)vsf_file_kind(files[i], nbytes[i]);
    if (kinds[i] == VSF_FILE_NONE) return VSF_ERR_UNSUPPORTED;
  }
  for (int i0 = 0, i1; i0 < n_images; i0 = i1) {
    i1 = vsf_run_end(kinds.data(), n_images, i0);
    const vsf_status st = decode_batch(ctx, kinds[i0], files + i0, nbytes + i0, i1 - i0, width, height,
                                       d_dst + (size_t)i0 * dst_image_stride, dst_image_stride, dst_row_stride, 1, VSF_OUT_BGR);
    if (st != VSF_OK) return st;
  }
  return VSF_OK;
}

// cv::imdecode(data, IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) for reduce = 2, 4, 8 (reduce = 1: vsf_imdecode_gray_batch): a JPEG
// file of W x H is decoded by libjpeg's reduced inverse DCTs straight to ceil(W / reduce) x ceil(H / reduce) pixels -- width
// x height here -- through the same upload-and-decode path.  A PNG file with reduce > 1 is VSF_ERR_UNSUPPORTED: cv::imdecode
// decodes it at full size and calls cv::resize: vsf_png_decode_gray_batch + vsf_resize_gray_batch_dev, not this call.
vsf_status vsf_imdecode_reduced_gray_batch(vsf_ctx* ctx, const uint8_t* const* files, const size_t* nbytes, int n_images,
                                           int reduce, int width, int height, uint8_t* d_dst, size_t dst_image_stride,
                                           size_t dst_row_stride) {
  if (!vsf_reduce_ok(reduce)) return VSF_ERR_INVALID_ARG;  // (nothing is looked at, nothing launched)
  if (reduce == 1) return vsf_imdecode_gray_batch(ctx, files, nbytes, n_images, width, height, d_dst, dst_image_stride, dst_row_stride);
  if (!ctx || !files || !nbytes || n_images < 1 || !d_dst) return VSF_ERR_INVALID_ARG;
  for (int i = 0; i < n_images; i++) {  // (before anything is launched: a list with a PNG or an unknown file launches nothing)
    const int kind = vsf_file_kind(files[i], nbytes[i]);
    if (kind != VSF_FILE_JPEG) return VSF_ERR_UNSUPPORTED;
  }
  return decode_batch(ctx, VSF_FILE_JPEG, files, nbytes, n_images, width, height, d_dst, dst_image_stride, dst_row_stride,
                           reduce);
}

// cv::imencode(".jpg", img, {IMWRITE_JPEG_QUALITY, quality}) / cv::imencode(".png", img) for a batch of equally sized images
// (k_jpeg_enc.hip, k_png_enc.hip): the way out of the device for pixels, as the decoders above are the way in.  Asynchronous on the
// context's stream.
// (a job as the caller gave it: quality 0 = 95, and a PNG job carries 0; out_cap 0: a file may take all of its slot)
vsf_status vsf_jpeg_encode_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int channels,
                                     size_t src_image_stride, size_t src_row_stride, int quality, uint8_t* d_out,
                                     size_t out_stride, int32_t* d_out_bytes) {
  return encode_batch_dev(ctx, {VSF_FILE_JPEG, n_images, width, height, channels, src_image_stride, src_row_stride, quality, out_stride, 0},
                          d_src, d_out, d_out_bytes);
}

vsf_status vsf_png_encode_batch_dev(vsf_ctx* ctx, const uint8_t* d_src, int n_images, int width, int height, int channels,
                                    size_t src_image_stride, size_t src_row_stride, uint8_t* d_out, size_t out_stride,
                                    int32_t* d_out_bytes) {
  return encode_batch_dev(ctx, {VSF_FILE_PNG, n_images, width, height, channels, src_image_stride, src_row_stride, 0, out_stride, 0},
                          d_src, d_out, d_out_bytes);
}

// The same for host pointers, synchronous: images up, files and byte counts back.  out_bytes[i] = -1 and VSF_ERR_CAPACITY for a
// file that does not fit out_stride.
vsf_status vsf_jpeg_encode(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int channels,
                           size_t src_image_stride, size_t src_row_stride, int quality, uint8_t* out, size_t out_stride,
                           int32_t* out_bytes) {
  return encode_host(ctx, {VSF_FILE_JPEG, n_images, width, height, channels, src_image_stride, src_row_stride, quality, out_stride, 0},
                     src, out, out_bytes);
}

vsf_status vsf_png_encode(vsf_ctx* ctx, const uint8_t* src, int n_images, int width, int height, int channels,
                          size_t src_image_stride, size_t src_row_stride, uint8_t* out, size_t out_stride, int32_t* out_bytes) {
  return encode_host(ctx, {VSF_FILE_PNG, n_images, width, height, channels, src_image_stride, src_row_stride, 0, out_stride, 0}, src,
                     out, out_bytes);
}

}  // extern "C"
