// Hiera trunk (hiera_{tiny,small,base}_224 as the depth + normal model builds it, models/hiera_image_encoder.py:35,60):
// the three kernels of its path that the shared GEMM / LayerNorm / attention kernels do not cover (its mask-unit / global
// attention, vdn_hiera_attn, is lane_attn_kernel: lane_attn.hip).
//   hiera_embed_kernel   7x7 stride-4 pad-3 patch gather -> GEMM rows, written in UNROLLED token order
//   hiera_pool_kernel    max over the 4 token groups of a width-changing block's residual
//   hiera_reroll_kernel  unrolled tokens of a stage -> f32 NHWC map
// Token order ("unroll"): the three nested stride-2 levels of the 56 x 56 grid are the leading digits of the token index,
//   u = ((d1*4 + d2)*4 + d3)*49 + Y*7 + X,  d_k = 2*sy_k + sx_k,  y = 8 Y + 4 sy3 + 2 sy2 + sy1 (x alike),
// so a 2 x 2 max-pool is a max over 4 contiguous quarters of the token axis. A stage that has consumed s levels keeps the
// last n = 3 - s digits: y = Y 2^n + sum_k sy_k 2^(k-1) with d_1 the most significant digit.
#include "common.hpp"

namespace {

constexpr int HI_SIDE = 56;    // tokens per side after the patch embedding of a 224 x 224 frame
constexpr int HI_IMG = 224;
constexpr int HI_K = 147;      // 3 * 7 * 7

// token index u of a stage with n unroll levels left and side (7 << n) -> (y, x)
__device__ __forceinline__ void unrolled_to_yx(int u, int n, int& y, int& x) {
  const int cell = u % 49;
  int d = u / 49;
  y = (cell / 7) << n;
  x = (cell % 7) << n;
  for (int k = n; k >= 1; --k) {   // the last digit is level n (weight 2^(n-1)), the first is level 1 (weight 1)
    const int dk = d & 3;
    d >>= 2;
    y += (dk >> 1) << (k - 1);
    x += (dk & 1) << (k - 1);
  }
}

__device__ __forceinline__ int yx_to_unrolled(int y, int x, int n) {
  int d = 0;
  for (int k = 1; k <= n; ++k) d = d * 4 + (((y >> (k - 1)) & 1) * 2 + ((x >> (k - 1)) & 1));
  return d * 49 + (y >> n) * 7 + (x >> n);
}

// ------------------------------------------------------------------------------------------------------------------
// hiera_embed_kernel — rows[(f*3136 + u), k] = img[f, c, 4y - 3 + ky, 4x - 3 + kx] (0 outside), k = (c*7 + ky)*7 + kx,
// (y, x) the position of unrolled token u; zero tail up to ldk. One thread per 8 consecutive k (16-byte stores).
template <int DT>
__global__ __launch_bounds__(256) void hiera_embed_kernel(const float* __restrict__ img, typename Half<DT>::T* __restrict__ rows,
                                                          typename Half<DT>::T* __restrict__ rows_lo, int frames, int ldk) {
  using T = typename Half<DT>::T;
  using V8 = typename Half<DT>::V8;
  const int kv = ldk >> 3;
  const size_t total = (size_t)frames * HI_SIDE * HI_SIDE * kv;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k8 = (int)(i % kv);
    const size_t row = i / kv;
    const int u = (int)(row % (HI_SIDE * HI_SIDE));
    const size_t f = row / (HI_SIDE * HI_SIDE);
    int y, x;
    unrolled_to_yx(u, 3, y, x);
    V8 o, ol;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k8 * 8 + e;
      float v = 0.f;
      if (k < HI_K) {
        const int c = k / 49, rem = k - c * 49;
        const int ky = rem / 7, kx = rem - ky * 7;
        const int sy = 4 * y - 3 + ky, sx = 4 * x - 3 + kx;
        if (sy >= 0 && sy < HI_IMG && sx >= 0 && sx < HI_IMG) v = img[((f * 3 + c) * HI_IMG + sy) * HI_IMG + sx];
      }
      const T h = (T)v;
      o[e] = h;
      ol[e] = (T)(v - (float)h);
    }
    *(V8*)(rows + row * ldk + k8 * 8) = o;
    if (rows_lo) *(V8*)(rows_lo + row * ldk + k8 * 8) = ol;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// hiera_pool_kernel — y[f, j, :] = max over g < 4 of x[f, g*n + j, :], 4 channels per thread.
__global__ __launch_bounds__(256) void hiera_pool_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total4, int n,
                                                         int c4) {
  const size_t per = (size_t)n * c4;   // float4 elements of one group of one frame
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const size_t f = i / per, r = i - f * per;
    const f32x4* src = (const f32x4*)x + f * 4 * per + r;
    f32x4 a = src[0];
    const f32x4 b = src[per], c = src[2 * per], d = src[3 * per];
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
    ((f32x4*)y)[i] = a;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// hiera_reroll_kernel — map[f, y, x, :] = tokens[f, u(y, x), :] for a stage with n unroll levels left, 4 channels per thread.
__global__ __launch_bounds__(256) void hiera_reroll_kernel(const float* __restrict__ tok, float* __restrict__ map, size_t total4,
                                                           int n, int c4) {
  const int side = 7 << n;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % c4);
    size_t t = i / c4;
    const int x = (int)(t % side);
    t /= side;
    const int y = (int)(t % side);
    const size_t f = t / side;
    const int u = yx_to_unrolled(y, x, n);
    ((f32x4*)map)[i] = ((const f32x4*)tok)[(f * side * side + u) * c4 + c];
  }
}

}  // namespace

extern "C" int vdn_hiera_embed(int dt, const float* img, void* rows, void* rows_lo, int frames, int ldk, vdn_stream stream) {
  if (!img || !rows || frames <= 0) return VDN_EINVAL;
  if (ldk < HI_K || (ldk & 63) || ((uintptr_t)rows & 15) || ((uintptr_t)rows_lo & 15)) return VDN_EALIGN;
  if ((int64_t)frames * HI_SIDE * HI_SIDE > 0x7fffffff) return VDN_EUNSUPPORTED;   // rows are int32 in vdn_gemm
  const unsigned g = grid_for((size_t)frames * HI_SIDE * HI_SIDE * (ldk >> 3), 16384);
  return with_half(dt, [&](auto t) -> int {
    using T = typename Half<decltype(t)::value>::T;
    hipLaunchKernelGGL(hiera_embed_kernel<decltype(t)::value>, dim3(g), dim3(256), 0, (hipStream_t)stream, img, (T*)rows, (T*)rows_lo,
                       frames, ldk);
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
}

extern "C" int vdn_hiera_pool(const float* x, float* y, int frames, int n, int C, vdn_stream stream) {
  if (!x || !y || frames <= 0 || n <= 0 || C <= 0) return VDN_EINVAL;
  if ((C & 3) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return VDN_EALIGN;
  const size_t total4 = (size_t)frames * n * (C >> 2);
  hipLaunchKernelGGL(hiera_pool_kernel, dim3(grid_for(total4, 16384)), dim3(256), 0, (hipStream_t)stream, x, y, total4, n,
                     C >> 2);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_hiera_reroll(const float* tokens, float* map, int frames, int stage, int C, vdn_stream stream) {
  if (!tokens || !map || frames <= 0 || stage < 0 || stage > 3 || C <= 0) return VDN_EINVAL;
  if ((C & 3) || ((uintptr_t)tokens & 15) || ((uintptr_t)map & 15)) return VDN_EALIGN;
  const int n = 3 - stage, side = 7 << n;
  const size_t total4 = (size_t)frames * side * side * (C >> 2);
  hipLaunchKernelGGL(hiera_reroll_kernel, dim3(grid_for(total4, 16384)), dim3(256), 0, (hipStream_t)stream, tokens, map,
                     total4, n, C >> 2);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
