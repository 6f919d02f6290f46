// Drawing rules shared by the scene view (render.hip) and the evaluation panels (panels.hip): the thick-line coverage test, the
// segment clip that feeds it, and the host helpers that restate the reference's int() / np.round / K @ v. All fp64, contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace ovm_draw {

// Squared distance of (px, py) to the segment (x0, y0)-(x1, y1). A thick line covers a pixel when this is <= (thickness / 2)^2.
__host__ __device__ inline double seg_dist2(double px, double py, double x0, double y0, double x1, double y1) {
#pragma clang fp contract(off)
  const double dx = x1 - x0, dy = y1 - y0;
  const double ex = px - x0, ey = py - y0;
  const double ll = dx * dx + dy * dy;
  double t = ll > 0.0 ? (ex * dx + ey * dy) / ll : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double fx = ex - t * dx, fy = ey - t * dy;
  return fx * fx + fy * fy;
}

inline double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline int64_t to_i64(double v) { return (int64_t)clampd(v, -1e15, 1e15); }   // int() of a finite projection
inline int iround(double v) { return (int)std::nearbyint(v); }                  // np.round: half to even

// K @ v / div, summed left to right as the numpy restatements do
__host__ __device__ inline void project(const double* K, const double* v, double div, double* u) {
#pragma clang fp contract(off)
  u[0] = (K[0] * v[0] + K[1] * v[1] + K[2] * v[2]) / div;
  u[1] = (K[3] * v[0] + K[4] * v[1] + K[5] * v[2]) / div;
}

// Segment clipped (Liang-Barsky, fp64) to [-r, W - 1 + r] x [-r, H - 1 + r]: no pixel of the canvas within r of the segment
// is lost. seg: the clipped x0, y0, x1, y1; bbox: inclusive pixel box x0, y0, x1, y1 on the canvas. False when nothing is left.
inline bool clip_segment(double x0, double y0, double x1, double y1, double r, int W, int H, double* seg, int32_t* bbox) {
#pragma clang fp contract(off)
  const double dx = x1 - x0, dy = y1 - y0;
  const double pk[4] = {-dx, dx, -dy, dy};
  const double qk[4] = {x0 - (-r), (W - 1 + r) - x0, y0 - (-r), (H - 1 + r) - y0};
  double t0 = 0.0, t1 = 1.0;
  for (int k = 0; k < 4; ++k) {
    if (pk[k] == 0.0) {
      if (qk[k] < 0.0) return false;
    } else {
      const double t = qk[k] / pk[k];
      if (pk[k] < 0.0) t0 = t > t0 ? t : t0;
      else t1 = t < t1 ? t : t1;
    }
  }
  if (t0 > t1) return false;
  seg[0] = x0 + t0 * dx; seg[1] = y0 + t0 * dy; seg[2] = x0 + t1 * dx; seg[3] = y0 + t1 * dy;
  const double bx0 = std::floor(std::fmin(seg[0], seg[2]) - r), bx1 = std::ceil(std::fmax(seg[0], seg[2]) + r);
  const double by0 = std::floor(std::fmin(seg[1], seg[3]) - r), by1 = std::ceil(std::fmax(seg[1], seg[3]) + r);
  bbox[0] = (int32_t)clampd(bx0, 0, W - 1); bbox[1] = (int32_t)clampd(by0, 0, H - 1);
  bbox[2] = (int32_t)clampd(bx1, 0, W - 1); bbox[3] = (int32_t)clampd(by1, 0, H - 1);
  return true;
}

}  // namespace ovm_draw
