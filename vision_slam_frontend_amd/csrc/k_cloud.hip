// k_cloud.hip -- the RViz point cloud of the reference's driver (AddFeaturePoints, slam_frontend_main.cc:155-173) for a batch of
// frames whose vsf_vision_feature records sit in HBM: per frame, every feature that passes the predicate, in feature order,
// as M_f * point3d widened to three doubles -- the body of a geometry_msgs/Point[].  The arithmetic is vsf_world_points.h's,
// which the host's AddFeaturePoints includes too.
//
// One wave64 per frame walks 64 records per step.  A lane's place in the output is the running base of the steps before plus
// the number of kept lanes below it (ballot + prefix count): no atomics, so the order is the feature order and the output is
// the same bytes every time.  Nothing is written behind the frame's count.
#include "vsf_internal.h"
#include "vsf_world_points.h"

#pragma clang fp contract(off)

namespace {

// The walk of one frame by one wave: its records `in`, its transform, where its points and its count go.
__device__ __forceinline__ void world_points_frame(const vsf_vision_feature* __restrict__ in, int n, const vsfwp::Affine M,
                                                   double* __restrict__ out, int32_t* __restrict__ count) {
  const int lane = (int)threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    float x = 0.f, y = 0.f, z = 0.f;
    if (i < n) {
      x = in[i].point3d[0];
      y = in[i].point3d[1];
      z = in[i].point3d[2];
    }
    const bool kept = i < n && vsfwp::keep(x, y, z);
    const unsigned long long mask = __ballot(kept);
    if (kept) {
      const int k = base + __popcll(mask & ((1ull << lane) - 1ull));  // k <= i < n <= max_rows: inside the frame's slot
      double w[3];
      vsfwp::transform(M, x, y, z, w);
      out[3 * (size_t)k] = w[0];
      out[3 * (size_t)k + 1] = w[1];
      out[3 * (size_t)k + 2] = w[2];
    }
    base += __popcll(mask);
  }
  if (lane == 0) *count = base;
}

// vsf_world_points_batch_dev: frames [f0, f0 + gridDim.x), their transforms in the kernel arguments, frame f's points in slot f.
__global__ __launch_bounds__(64) void world_points_kernel(const vsf_vision_feature* __restrict__ features,  // [frames][max_rows]
                                                           const int32_t* __restrict__ nfeatures,            // [frames]
                                                           int max_rows, int f0, VsfWorldTransforms tf,
                                                           double* __restrict__ points,      // [frames][max_rows][3]
                                                           int32_t* __restrict__ npoints) {  // [frames]
  const int f = f0 + (int)blockIdx.x;  // (the workgroup's: what depends on it alone is wave-uniform)
  const int n = min(max(nfeatures[f], 0), max_rows);
  world_points_frame(features + (size_t)f * max_rows, n, tf.m[blockIdx.x], points + (size_t)f * max_rows * 3, npoints + f);
}

// The ObserveImage queue: frame f's transform is tf[f] in the batch's pinned block; its points go to slot frames[f].out_slot of
// the pinned ring of points, its count to counts[out_slot].
__global__ __launch_bounds__(64) void world_points_table_kernel(const vsf_vision_feature* __restrict__ features,
                                                                 const int32_t* __restrict__ nfeatures, int max_rows,
                                                                 const vsfwp::Affine* __restrict__ tf,        // [frames]
                                                                 const VsfObserveFrame* __restrict__ frames,  // [frames]
                                                                 double* __restrict__ points,      // [slots][max_rows][3]
                                                                 int32_t* __restrict__ npoints) {  // [slots]
  const int f = (int)blockIdx.x;
  const int n = min(max(nfeatures[f], 0), max_rows);
  const int slot = frames[f].out_slot;
  world_points_frame(features + (size_t)f * max_rows, n, tf[f], points + (size_t)slot * max_rows * 3, npoints + slot);
}

}  // namespace

void vsf_launch_world_points(const vsf_vision_feature* d_features, const int32_t* d_nfeatures, int f0, int n_frames, int max_rows,
                             const VsfWorldTransforms& tf, double* d_points, int32_t* d_npoints, hipStream_t s) {
  hipLaunchKernelGGL(world_points_kernel, dim3(n_frames), dim3(64), 0, s, d_features, d_nfeatures, max_rows, f0, tf, d_points,
                     d_npoints);
}

void vsf_launch_world_points_table(const vsf_vision_feature* d_features, const int32_t* d_nfeatures, int n_frames, int max_rows,
                                   const vsfwp::Affine* tf, const VsfObserveFrame* frames, double* points, int32_t* npoints,
                                   hipStream_t s) {
  hipLaunchKernelGGL(world_points_table_kernel, dim3(n_frames), dim3(64), 0, s, d_features, d_nfeatures, max_rows, tf, frames,
                     points, npoints);
}
