// vsf_world_points.h -- the arithmetic of the RViz point cloud (the reference's AddFeaturePoints, slam_frontend_main.cc:155-173),
// stated ONCE: k_cloud.hip's kernel and the host's AddFeaturePoints (host/slam_visualization.h) both include this file, so the
// device's points and the CPU restatement's are the same float operations in the same order.
//
//   keep(p)  :  x, y, z finite  &&  (double)z > 0.1  &&  (double)norm > 0.5  &&  (double)norm < 20.0,
//               norm = sqrtf(float sum of squares)                (Vector3f::norm() is a float; the literals are doubles)
//   point    :  M * p, widened to double,   M = (Translation3f(loc) * quat) * cam_to_robot   (RobotPose::RobotToWorldTf,
//               slam_types.h:122-124; `robot_to_world * cam_to_robot * p` associates to the left), every step in float.
//
// ROUNDING.  Every product and every sum is rounded by itself: __fmul_rn / __fadd_rn on the device, plain operators on the
// host, where the translation unit must be compiled without contraction (-ffp-contract=off; x86-64 without -mfma has no FMA
// to contract into).  The square root is the correctly rounded one on both sides.
//
// SUMMATION ORDER -- chosen here, not inherited: Eigen's order in a fixed-size product depends on its unroller and its
// vectorisation (vsf_params::residual_order documents the same for RemoveAmbigStereo), and nothing in this project can pin it.
//   three-term dot product     (a0 b0 + a1 b1) + a2 b2                    left to right
//   affine x affine            linear = the dot products above;  translation = ((a0 b0 + a1 b1) + a2 b2) + t
//   affine x vector            ((m0 x + m1 y) + m2 z) + t                 left to right, translation last
//   sum of squares             (x x + y y) + z z
//   quaternion -> rotation     Eigen's QuaternionBase::toRotationMatrix, statement for statement (tx = 2 x ... twx = tx w ...)
// Against a float64 evaluation the chain is ~20 roundings of 2^-24 of the magnitudes involved.
#ifndef VSF_WORLD_POINTS_H_
#define VSF_WORLD_POINTS_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VSF_WP_FN __host__ __device__ __forceinline__
#else
#define VSF_WP_FN inline
#endif

namespace vsfwp {

VSF_WP_FN float mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
VSF_WP_FN float add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}
VSF_WP_FN float sub(float a, float b) { return add(a, -b); }  // (a - b == a + (-b) exactly in IEEE arithmetic)
// (sqrtf, not __fsqrt_rn: HIP's header maps the latter to the 1-ulp native square root; sqrtf is the correctly rounded one in a
// device build with -fhip-fp32-correctly-rounded-divide-sqrt, which csrc/Makefile does not let anybody take away)
VSF_WP_FN float root(float a) { return sqrtf(a); }
VSF_WP_FN bool finite(float a) {
  uint32_t u;
  __builtin_memcpy(&u, &a, 4);
  return (u & 0x7F800000u) != 0x7F800000u;
}

VSF_WP_FN float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return add(add(mul(a0, b0), mul(a1, b1)), mul(a2, b2));
}

// A 3 x 4 row-major affine transform: m[4 r + c], c = 3 the translation.
struct Affine {
  float m[12];
};

// Translation3f(loc) * Quaternionf(w, x, y, z): the rotation matrix as Eigen writes it, the translation beside it.
VSF_WP_FN Affine robot_to_world(const float loc[3], const float quat_xyzw[4]) {
  const float x = quat_xyzw[0], y = quat_xyzw[1], z = quat_xyzw[2], w = quat_xyzw[3];
  const float tx = mul(2.0f, x), ty = mul(2.0f, y), tz = mul(2.0f, z);
  const float twx = mul(tx, w), twy = mul(ty, w), twz = mul(tz, w);
  const float txx = mul(tx, x), txy = mul(ty, x), txz = mul(tz, x);
  const float tyy = mul(ty, y), tyz = mul(tz, y), tzz = mul(tz, z);
  Affine a;
  a.m[0] = sub(1.0f, add(tyy, tzz));
  a.m[1] = sub(txy, twz);
  a.m[2] = add(txz, twy);
  a.m[3] = loc[0];
  a.m[4] = add(txy, twz);
  a.m[5] = sub(1.0f, add(txx, tzz));
  a.m[6] = sub(tyz, twx);
  a.m[7] = loc[1];
  a.m[8] = sub(txz, twy);
  a.m[9] = add(tyz, twx);
  a.m[10] = sub(1.0f, add(txx, tyy));
  a.m[11] = loc[2];
  return a;
}

VSF_WP_FN Affine compose(const Affine& a, const Affine& b) {  // a * b
  Affine o;
  for (int r = 0; r < 3; r++) {
    const float a0 = a.m[4 * r], a1 = a.m[4 * r + 1], a2 = a.m[4 * r + 2];
    for (int c = 0; c < 3; c++) o.m[4 * r + c] = dot3(a0, a1, a2, b.m[c], b.m[4 + c], b.m[8 + c]);
    o.m[4 * r + 3] = add(dot3(a0, a1, a2, b.m[3], b.m[7], b.m[11]), a.m[4 * r + 3]);
  }
  return o;
}

// M_f of one node: (Translation(loc) * quat) * cam_to_robot (3 x 4 row-major).
VSF_WP_FN Affine camera_to_world(const float loc[3], const float quat_xyzw[4], const float cam_to_robot[12]) {
  Affine c;
  for (int i = 0; i < 12; i++) c.m[i] = cam_to_robot[i];
  return compose(robot_to_world(loc, quat_xyzw), c);
}

VSF_WP_FN float squared_norm(float x, float y, float z) { return add(add(mul(x, x), mul(y, y)), mul(z, z)); }

// The predicate of AddFeaturePoints (main.cc:162-165).
VSF_WP_FN bool keep(float x, float y, float z) {
  if (!(finite(x) && finite(y) && finite(z))) return false;
  const float norm = root(squared_norm(x, y, z));
  return (double)z > 0.1 && (double)norm > 0.5 && (double)norm < 20.0;
}

// out = M * p, widened: three consecutive doubles, the body of one geometry_msgs/Point.
VSF_WP_FN void transform(const Affine& M, float x, float y, float z, double out[3]) {
  for (int r = 0; r < 3; r++)
    out[r] = (double)add(dot3(M.m[4 * r], M.m[4 * r + 1], M.m[4 * r + 2], x, y, z), M.m[4 * r + 3]);
}

}  // namespace vsfwp

#endif  // VSF_WORLD_POINTS_H_
