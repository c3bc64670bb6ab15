// vsf_mask.hip -- detection masks: the slots of a context (include/vsf.h "Detection masks"; the pyramid's rule and its
// kernels: k_mask.hip; the predicate: k_fast.hip).
#include <vector>

#include "vsf_ctx.h"

using namespace vsfi;

namespace vsfi {

VsfFastMask image_masks(const vsf_ctx* ctx, int i0) {
  VsfFastMask m;
  auto block = [&](int slot) -> const uint8_t* {
    return slot >= 0 && slot < VSF_MAX_MASKS && ctx->masks[slot].set ? ctx->masks[slot].block.get() : nullptr;
  };
  m.even = block(ctx->mask_even);
  m.odd = block(ctx->mask_odd);
  m.parity = i0 & 1;
  m.bytes = ctx->orb.g.pyr_bytes;
  return m;
}

}  // namespace vsfi

namespace {

bool slot_ok(int slot) { return slot >= 0 && slot < VSF_MAX_MASKS; }

// d_mask: device memory, or null with `h_mask` set (uploaded into a buffer of this call)
vsf_status mask_set(vsf_ctx* ctx, int slot, const uint8_t* h_mask, const uint8_t* d_mask, int w, int h, size_t stride) {
  if (!ctx || !slot_ok(slot) || (!h_mask && !d_mask) || w != ctx->p.width || h != ctx->p.height || stride < (size_t)w)
    return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  flush_observe(ctx);
  sync_all_streams(ctx);  // every frame submitted so far has read the slot as it was
  vsf_ctx::MaskSlot& m = ctx->masks[slot];
  const uint32_t bytes = ctx->orb.g.pyr_bytes;
  if (!m.block) VSF_HIP(m.block.alloc(bytes));
  DevBuf<uint8_t> up;
  size_t pitch = stride;
  if (!d_mask) {
    pitch = (size_t)align_up(w, 64);
    VSF_HIP(up.alloc(pitch * (size_t)h));
    VSF_HIP(hipMemcpy2DAsync(up, pitch, h_mask, stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    d_mask = up;
  }
  m.set = false;  // (a build that fails leaves no half-built mask behind)
  vsf_launch_mask_pyramid(d_mask, pitch, ctx->orb.levels.data(), ctx->orb.g.nlevels, bytes, m.block, ctx->stream);
  VSF_HIP(hipStreamSynchronize(ctx->stream));  // the pyramid is built: any stream may read it, the caller's mask is free
  VSF_STICKY();
  m.set = true;
  return VSF_OK;
}

}  // namespace

extern "C" {

vsf_status vsf_mask_set(vsf_ctx* ctx, int slot, const uint8_t* mask, int w, int h, size_t stride) {
  VsfErrorScope scope_(ctx);
  return mask_set(ctx, slot, mask, nullptr, w, h, stride);
}

vsf_status vsf_mask_set_dev(vsf_ctx* ctx, int slot, const uint8_t* d_mask, int w, int h, size_t stride) {
  VsfErrorScope scope_(ctx);
  return mask_set(ctx, slot, nullptr, d_mask, w, h, stride);
}

vsf_status vsf_mask_clear(vsf_ctx* ctx, int slot) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !slot_ok(slot)) return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  flush_observe(ctx);
  sync_all_streams(ctx);
  ctx->masks[slot].set = false;
  VSF_STICKY();
  return VSF_OK;
}

vsf_status vsf_mask_is_set(const vsf_ctx* ctx, int slot, int* is_set) {
  if (!ctx || !slot_ok(slot) || !is_set) return VSF_ERR_INVALID_ARG;
  *is_set = ctx->masks[slot].set ? 1 : 0;
  return VSF_OK;
}

vsf_status vsf_mask_slot_bytes(const vsf_ctx* ctx, size_t* bytes) {
  if (!ctx || !bytes) return VSF_ERR_INVALID_ARG;
  *bytes = ctx->orb.g.pyr_bytes;
  return VSF_OK;
}

vsf_status vsf_set_image_masks(vsf_ctx* ctx, int even_slot, int odd_slot) {
  VsfErrorScope scope_(ctx);
  if (!ctx || even_slot < -1 || even_slot >= VSF_MAX_MASKS || odd_slot < -1 || odd_slot >= VSF_MAX_MASKS)
    return VSF_ERR_INVALID_ARG;
  ctx->mask_even = even_slot;
  ctx->mask_odd = odd_slot;
  return VSF_OK;
}

vsf_status vsf_get_image_masks(const vsf_ctx* ctx, int* even_slot, int* odd_slot) {
  if (!ctx || !even_slot || !odd_slot) return VSF_ERR_INVALID_ARG;
  *even_slot = ctx->mask_even;
  *odd_slot = ctx->mask_odd;
  return VSF_OK;
}

vsf_status vsf_debug_mask_level(vsf_ctx* ctx, int slot, int level, uint8_t* out, size_t ostride) {
  VsfErrorScope scope_(ctx);
  if (!ctx || !slot_ok(slot) || !out || level < 0 || level >= ctx->orb.g.nlevels || !ctx->masks[slot].set) return VSF_ERR_INVALID_ARG;
  const VsfLevel& L = ctx->orb.levels[level];
  if (ostride < (size_t)L.w) return VSF_ERR_INVALID_ARG;
  VSF_HIP(hipSetDevice(ctx->device));
  VSF_HIP(hipMemcpy2D(out, ostride, ctx->masks[slot].block.get() + L.offset, (size_t)L.pitch, (size_t)L.w, (size_t)L.h,
                      hipMemcpyDeviceToHost));
  return VSF_OK;
}

}  // extern "C"
