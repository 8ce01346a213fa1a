// What the passes of the normal criterion share (normals.hip forward, normals_grad.hip backward): the blocks per frame
// (swept and summed as frame_sums.hpp states), the Sobel stencil and the unit normal made from it, the 3 x 3 erosion, the clamped norm of F.cosine_similarity, and
// the neighbourhood of a lane's pixels. Include it AFTER the unit's `#pragma clang fp contract(off)`: every product here feeds
// a sum, and both units must round them apart.
#pragma once
#include "common.hpp"
#include "frame_sums.hpp"
#include <math.h>

namespace {

constexpr int NE_BPF = 64;  // blocks per frame, fixed so that the forward's workspace depends on the frame count alone

// cross-correlation with kx = [[1,0,-1],[2,0,-2],[1,0,-1]], ky = [[1,2,1],[0,0,0],[-1,-2,-1]] (times 1/8 = k), in fp64.
// a[r][c] is the 3 x 3 window; its centre is not used.
__device__ __forceinline__ void sobel(const float (&a)[3][3], double k, double& ix, double& iy) {
  const double a00 = a[0][0], a01 = a[0][1], a02 = a[0][2], a10 = a[1][0], a12 = a[1][2], a20 = a[2][0], a21 = a[2][1],
               a22 = a[2][2];
  ix = ((a00 - a02) + 2.0 * (a10 - a12) + (a20 - a22)) * k;
  iy = ((a00 - a20) + 2.0 * (a01 - a21) + (a02 - a22)) * k;
}

// n = (-sxy Ix, -sxy Iy, sz) / sqrt(nx^2 + ny^2 + nz^2 + eps)
__device__ __forceinline__ void unit_normal(double ix, double iy, double sxy, double sz, double eps, double (&n)[3]) {
  const double nx = -sxy * ix, ny = -sxy * iy;
  const double norm = sqrt(((nx * nx + ny * ny) + sz * sz) + eps);
  n[0] = nx / norm;
  n[1] = ny / norm;
  n[2] = sz / norm;
}

__device__ __forceinline__ void window_at(const float* __restrict__ df, int y, int x, int H, int W, float (&a)[3][3]) {
  const int ys[3] = {refl_lo(y), y, refl_hi(y, H)}, xs[3] = {refl_lo(x), x, refl_hi(x, W)};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[r][c] = (r == 1 && c == 1) ? 0.f : df[(size_t)ys[r] * W + xs[c]];
}

// erosion at (y, x): the pixel and its neighbours inside the image are all non-zero
__device__ __forceinline__ bool kept_at(const uint8_t* __restrict__ mf, int y, int x, int H, int W) {
  bool k = true;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) k = k && mf[(size_t)yy * W + xx] != 0;
    }
  return k;
}

// |a| as F.cosine_similarity(eps = 1e-8) of torch 2.x takes it, before the clamp
__device__ __forceinline__ double norm3(const double (&a)[3]) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
// max(|a|, 1e-8); the comparison (not fmax) keeps a NaN norm
__device__ __forceinline__ double clamp_norm(double n) { return n < 1e-8 ? 1e-8 : n; }

// The neighbourhood of a lane's PPL consecutive pixels, the first at (y, x). A quad that lies in one row with a column to spare
// on either side shares its neighbours: per row six columns serve the four erosion tests and the four stencils (18 + 18 loads
// in place of 36 + 32). Other quads, and single pixels, go pixel by pixel. DEPTH: tf is a depth map and the target normal is
// made here, with normal_vector's default arguments.
template <int PPL, bool DEPTH>
struct Hood {
  bool fast;
  bool keepq[PPL];
  float dq[3][PPL + 2];
  __device__ __forceinline__ Hood(const float* __restrict__ tf, const uint8_t* __restrict__ mf, int y, int x, int H, int W) {
    fast = PPL == 4 && x >= 1 && x + PPL < W;
    if (fast) {
#pragma unroll
      for (int j = 0; j < PPL; ++j) keepq[j] = true;
      if (mf) {
        bool v[PPL + 2];  // the column's pixels in rows y - 1 .. y + 1 inside the image are all non-zero
#pragma unroll
        for (int c = 0; c < PPL + 2; ++c) {
          const size_t o = (size_t)y * W + (x - 1 + c);
          bool k = mf[o] != 0;
          if (y > 0) k &= mf[o - W] != 0;
          if (y < H - 1) k &= mf[o + W] != 0;
          v[c] = k;
        }
#pragma unroll
        for (int j = 0; j < PPL; ++j) keepq[j] = v[j] & v[j + 1] & v[j + 2];
      }
      bool any = false;
#pragma unroll
      for (int j = 0; j < PPL; ++j) any |= keepq[j];
      if (DEPTH && any) {
        const int ys[3] = {refl_lo(y), y, refl_hi(y, H)};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < PPL + 2; ++c) dq[r][c] = tf[(size_t)ys[r] * W + (x - 1 + c)];
      }
    }
  }
  // does the erosion keep pixel j, which lies at (y, x)
  __device__ __forceinline__ bool keep(const uint8_t* __restrict__ mf, int j, int y, int x, int H, int W) const {
    return fast ? keepq[j] : (!mf || kept_at(mf, y, x, H, W));
  }
  // the target normal of the kept pixel j at (y, x), from the depth stencil (DEPTH only)
  __device__ __forceinline__ void normal(const float* __restrict__ tf, int j, int y, int x, int H, int W, double (&t)[3]) const {
    const double eps = (double)1e-8f;  // normal_vector's default, as vdn_normal_vector receives it
    float win[3][3];
    if (fast) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) win[r][c] = dq[r][j + c];
    } else {
      window_at(tf, y, x, H, W, win);
    }
    double ix, iy;
    sobel(win, 0.125, ix, iy);
    unit_normal(ix, iy, 1.0, 1.0, eps, t);
  }
};

// A lane's PPL consecutive pixels of the three planes of a frame, loaded and stored as frame_sums.hpp does.
template <int PPL>
__device__ __forceinline__ void load3(const float* __restrict__ f, int hw, int p0, float (&v)[3][PPL]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) load_px<PPL>(f + (size_t)c * hw + p0, v[c]);
}
template <int PPL>
__device__ __forceinline__ void store3(float* __restrict__ f, int hw, int p0, const float (&v)[3][PPL]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) store_px<PPL>(f + (size_t)c * hw + p0, v[c]);
}

}  // namespace
