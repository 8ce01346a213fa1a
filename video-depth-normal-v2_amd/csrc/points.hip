// Point cloud of a metric depth map (metric_depth/depth_to_pointcloud.py:99-104):
//   for the pixel at (row, col) of an h x w map, in float64:  x = (col - w / 2) / fx,  y = (row - h / 2) / fy,
//   point = (x z, y z, z) with z the float32 depth widened,  colour = rgb / 255
// in one launch. Every value is one subtraction, one division and one product of float64 numbers, each correctly rounded
// on this hardware as on the host, and nothing here can contract into an fma (contraction is switched off all the same):
// the result is numpy's, bit for bit (tests/test_gpu_metric_model.py).
// A lane owns TWO neighbouring pixels = 48 contiguous bytes of each output, written as three 16-byte stores per output (a
// wave covers 3 KiB of contiguous rows per store group); an odd last pixel goes out as single doubles. Memory-bound: 7 bytes
// read and 48 written per pixel.
#include "common.hpp"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct PointPx {
  double px, py, pz, r, g, b;
};

__device__ __forceinline__ PointPx point_px(const float* __restrict__ depth, const uint8_t* __restrict__ rgb, size_t i, int w,
                                            double cx, double cy, double fx, double fy) {
#pragma clang fp contract(off)
  const int row = (int)(i / (size_t)w), col = (int)(i - (size_t)row * w);
  const double x = ((double)col - cx) / fx, y = ((double)row - cy) / fy, z = (double)depth[i];
  const uint8_t* c = rgb + 3 * i;
  return PointPx{x * z, y * z, z, (double)c[0] / 255.0, (double)c[1] / 255.0, (double)c[2] / 255.0};
}

__global__ __launch_bounds__(256) void depth_to_points_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                                              int h, int w, double fx, double fy, double* __restrict__ points,
                                                              double* __restrict__ colors) {
  const size_t n = (size_t)h * w, pairs = (n + 1) / 2;
  const double cx = (double)w / 2.0, cy = (double)h / 2.0;   // width / 2, height / 2: Python's true division
  for (size_t p = blockIdx.x * (size_t)256 + threadIdx.x; p < pairs; p += (size_t)gridDim.x * 256) {
    const size_t i = 2 * p;
    const PointPx a = point_px(depth, rgb, i, w, cx, cy, fx, fy);
    if (i + 1 < n) {
      const PointPx b = point_px(depth, rgb, i + 1, w, cx, cy, fx, fy);
      f64x2* po = (f64x2*)(points + 3 * i);   // 24 i bytes with i even: 16-byte aligned
      f64x2* co = (f64x2*)(colors + 3 * i);
      po[0] = f64x2{a.px, a.py}; po[1] = f64x2{a.pz, b.px}; po[2] = f64x2{b.py, b.pz};
      co[0] = f64x2{a.r, a.g};   co[1] = f64x2{a.b, b.r};   co[2] = f64x2{b.g, b.b};
    } else {   // h * w odd: the last pixel alone
      points[3 * i] = a.px; points[3 * i + 1] = a.py; points[3 * i + 2] = a.pz;
      colors[3 * i] = a.r;  colors[3 * i + 1] = a.g;  colors[3 * i + 2] = a.b;
    }
  }
}

}  // namespace

extern "C" int vdn_depth_to_points(const float* depth, const uint8_t* rgb, int h, int w, double fx, double fy, double* points,
                                   double* colors, vdn_stream stream) {
  if (!depth || !rgb || !points || !colors || h <= 0 || w <= 0) return VDN_EINVAL;
  if (!(fx > 0.0 || fx < 0.0) || !(fy > 0.0 || fy < 0.0)) return VDN_EINVAL;   // zero or NaN
  if (((uintptr_t)points | (uintptr_t)colors) & 15) return VDN_EALIGN;
  const size_t pairs = ((size_t)h * w + 1) / 2;
  hipLaunchKernelGGL(depth_to_points_kernel, dim3(grid_for(pairs, 4096)), dim3(256), 0, (hipStream_t)stream, depth, rgb, h, w, fx,
                     fy, points, colors);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
