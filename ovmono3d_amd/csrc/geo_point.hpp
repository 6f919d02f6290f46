// Step 1 of OVMono3D-GEO, shared by the lift (geo.hip) and the ground plane (ground.hip): a pixel and its depth -> the point
// p = (z (x - cx) / fx, -(z (y - cy) / fy), -z) in fp64, and with a frame U (9 doubles, row-major) U p instead.
#pragma once
#include <hip/hip_runtime.h>

// The restatements are numpy: no fused multiply-adds.
#pragma clang fp contract(off)

// records the message ovm_geo_last_error returns on this thread and passes the code through (geo.hip)
int geo_fail(int code, const char* msg);

__device__ __forceinline__ void geo_unproject(float zf, int x, int y, double fx, double fy, double cx, double cy, const double* __restrict__ frame,
                                              double* p) {
  const double z = (double)zf;
  const double p0 = z * ((double)x - cx) / fx, p1 = -(z * ((double)y - cy) / fy), p2 = -z;
  if (!frame) {
    p[0] = p0; p[1] = p1; p[2] = p2;
  } else {
    for (int r = 0; r < 3; ++r) p[r] = (frame[3 * r] * p0 + frame[3 * r + 1] * p1) + frame[3 * r + 2] * p2;
  }
}
