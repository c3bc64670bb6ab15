// A flat C view for tests/test_resize_plan.py (built with g++ into a small library, no device): vsf_resize.h's taps and span
// rule as the kernel and its launch evaluate them, and the slot / run arithmetic of the queue's declared input sizes
// (vsf_observe_plan.cc).
#include <cstdint>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_observe_plan.h"
#include "../../vision_slam_frontend_amd/csrc/vsf_resize.h"

extern "C" {

// xofs[dw], ialpha[2 dw], x1[dw] (the second tap's index), yofs0[dh], yofs1[dh], ibeta[2 dh]
void t_resize_taps(int sw, int sh, int dw, int dh, int32_t* xofs, int32_t* x1, int16_t* ialpha, int32_t* yofs0, int32_t* yofs1,
                   int16_t* ibeta) {
  const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
  for (int dx = 0; dx < dw; dx++) {
    const VsfTap t = resize_xtap(dx, scale_x, sw);
    xofs[dx] = t.i0;
    x1[dx] = t.i1;
    ialpha[2 * dx] = t.c0;
    ialpha[2 * dx + 1] = t.c1;
  }
  for (int dy = 0; dy < dh; dy++) {
    const VsfTap32 t = resize_ytap32(dy, scale_y, sh);
    yofs0[dy] = t.i0;
    yofs1[dy] = t.i1;
    ibeta[2 * dy] = (int16_t)t.c0;
    ibeta[2 * dy + 1] = (int16_t)t.c1;
  }
}

int t_resize_span_dwords(int sw, int dw) { return resize_span_dwords(sw, dw); }

uint64_t t_input_pitch(int w) { return vsfi::observe_input_pitch(w); }
uint64_t t_input_image_bytes(int w, int h) { return vsfi::observe_input_image_bytes(w, h); }
uint64_t t_input_half_bytes(const int* w, const int* h, int n) { return vsfi::observe_input_half_bytes(w, h, n); }
uint64_t t_input_ring_bytes(int depth, uint64_t half) { return vsfi::observe_input_ring_bytes(depth, (size_t)half); }

int t_upload_max_gap(uint64_t slot_bytes) { return vsfi::observe_upload_max_gap((size_t)slot_bytes); }

// in: n x {w, h, kind}; runs: up to cap x {where, f0, n, src0, w, h}; uploads: up to cap x {f0, n, slot0};
// counts: {uploads, n_resized}.  Returns the number of runs, -1: refused.
int t_resize_plan(const int32_t* in, int n, int64_t t0, int depth, int max_gap, int32_t* runs, int cap, int32_t* uploads,
                  int32_t* counts) {
  std::vector<vsfi::ObserveResizeIn> v;
  for (int i = 0; i < n; i++) v.push_back({in[3 * i], in[3 * i + 1], (uint8_t)in[3 * i + 2]});
  vsfi::ObserveResizePlan p;
  if (!vsfi::observe_resize_plan(v.data(), n, t0, depth, max_gap, &p)) return -1;
  for (int i = 0; i < (int)p.runs.size() && i < cap; i++) {
    const vsfi::ObserveResizeRun& r = p.runs[(size_t)i];
    const int32_t e[6] = {r.where, r.f0, r.n, r.src0, r.w, r.h};
    for (int k = 0; k < 6; k++) runs[6 * i + k] = e[k];
  }
  for (int i = 0; i < (int)p.uploads.size() && i < cap; i++)
    uploads[3 * i] = p.uploads[(size_t)i].f0, uploads[3 * i + 1] = p.uploads[(size_t)i].n, uploads[3 * i + 2] = p.uploads[(size_t)i].slot0;
  counts[0] = (int32_t)p.uploads.size(), counts[1] = p.n_resized;
  return (int)p.runs.size();
}

}  // extern "C"
