// Hiera trunk (hiera_{tiny,small,base}_224 as the depth + normal model builds it, models/hiera_image_encoder.py:35,60):
// the four kernels of its path that the shared GEMM / LayerNorm kernels do not cover.
//   hiera_embed_kernel   7x7 stride-4 pad-3 patch gather -> GEMM rows, written in UNROLLED token order
//   hiera_attn_kernel    mask-unit / global attention with the query max-pool fused on load, head dim 96
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
constexpr int HI_DH = 96;      // head dim at every stage
constexpr int HI_KT = 64;      // key rows per LDS tile

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
// hiera_attn_kernel — softmax(scale q k^T) v for every (frame, window, head). Token t of window w of frame f is row
// f*W*Lkv + t*W + w of qkv [rows, 3C] (columns q | k | v, each [heads][96]). With query stride qs, t = g*Lq + j and query j
// is the element-wise max over its qs groups, taken while q is loaded; output row f*W*Lq + j*W + w of out [rows/qs, C].
// One wave per (64 queries, head, frame x window); a lane owns one query row: q, the output accumulator and the running
// (max, sum) of the softmax stay in fp32 registers. Key / value tiles of 64 rows are staged in LDS as fp32 (hi + lo summed)
// and every lane reads the same key row (an LDS broadcast).
template <int DT>
__global__ __launch_bounds__(64) void hiera_attn_kernel(const typename Half<DT>::T* __restrict__ qkv,
                                                        const typename Half<DT>::T* __restrict__ qkv_lo,
                                                        typename Half<DT>::T* __restrict__ out, typename Half<DT>::T* __restrict__ out_lo,
                                                        int C, int W, int Lkv, int qs, float sl2) {
  __shared__ float ks[HI_KT][HI_DH];
  __shared__ float vs[HI_KT][HI_DH];
  const int lane = threadIdx.x;
  const int head = blockIdx.y;
  const int f = blockIdx.x / W, w = blockIdx.x - f * W;
  const int Lq = Lkv / qs;
  const size_t ld = 3 * (size_t)C;
  const size_t in0 = (size_t)f * W * Lkv + w;    // row of token 0 of this window; token t is W rows further per step
  const int qi = blockIdx.z * 64 + lane;
  const bool active = qi < Lq;
  float q[HI_DH], o[HI_DH];
  {
    const int j = active ? qi : 0;
#pragma unroll
    for (int e = 0; e < HI_DH; ++e) q[e] = -INFINITY;
    for (int g = 0; g < qs; ++g) {
      const size_t r = (in0 + (size_t)(g * Lq + j) * W) * ld + head * HI_DH;
#pragma unroll
      for (int e = 0; e < HI_DH; ++e) q[e] = fmaxf(q[e], load_half(qkv, qkv_lo, r + e));
    }
#pragma unroll
    for (int e = 0; e < HI_DH; ++e) {
      q[e] *= sl2;   // scale and log2(e) folded into q: exp2 below
      o[e] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < Lkv; k0 += HI_KT) {
    const int nk = min(HI_KT, Lkv - k0);
    __syncthreads();
    for (int i = lane; i < nk * HI_DH; i += 64) {
      const int j = i / HI_DH, e = i - j * HI_DH;
      const size_t r = (in0 + (size_t)(k0 + j) * W) * ld + head * HI_DH + e;
      ks[j][e] = load_half(qkv, qkv_lo, r + C);
      vs[j][e] = load_half(qkv, qkv_lo, r + 2 * C);
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < HI_DH; ++e) s = fmaf(q[e], ks[j][e], s);
      if (s > m) {   // rescale the accumulator only when the running max moves
        const float c = exp2f(m - s);
        l *= c;
#pragma unroll
        for (int e = 0; e < HI_DH; ++e) o[e] *= c;
        m = s;
      }
      const float p = exp2f(s - m);
      l += p;
#pragma unroll
      for (int e = 0; e < HI_DH; ++e) o[e] = fmaf(p, vs[j][e], o[e]);
    }
  }
  if (!active) return;
  const float inv = 1.f / l;
  const size_t r = ((size_t)f * W * Lq + (size_t)qi * W + w) * C + head * HI_DH;
#pragma unroll
  for (int e = 0; e < HI_DH; ++e) store_half_nearest(out, out_lo, r + e, o[e] * inv);
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

inline int grid_for(size_t n, size_t cap = 16384) {
  const size_t b = (n + 255) / 256;
  return (int)(b < cap ? (b ? b : 1) : cap);
}

}  // namespace

extern "C" int vdn_hiera_embed(int dt, const float* img, void* rows, void* rows_lo, int frames, int ldk, vdn_stream stream) {
  if (!img || !rows || frames <= 0) return VDN_EINVAL;
  if (ldk < HI_K || (ldk & 63) || ((uintptr_t)rows & 15) || ((uintptr_t)rows_lo & 15)) return VDN_EALIGN;
  if ((int64_t)frames * HI_SIDE * HI_SIDE > 0x7fffffff) return VDN_EUNSUPPORTED;   // rows are int32 in vdn_gemm
  const int g = grid_for((size_t)frames * HI_SIDE * HI_SIDE * (ldk >> 3));
  hipStream_t s = (hipStream_t)stream;
  if (dt == VDN_F16)
    hipLaunchKernelGGL(hiera_embed_kernel<VDN_F16>, dim3(g), dim3(256), 0, s, img, (_Float16*)rows, (_Float16*)rows_lo, frames, ldk);
  else if (dt == VDN_BF16)
    hipLaunchKernelGGL(hiera_embed_kernel<VDN_BF16>, dim3(g), dim3(256), 0, s, img, (__bf16*)rows, (__bf16*)rows_lo, frames, ldk);
  else
    return VDN_EUNSUPPORTED;
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_hiera_attn(int dt, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int frames, int heads, int W,
                              int Lkv, int q_stride, float scale, vdn_stream stream) {
  if (!qkv || !out || frames <= 0 || heads <= 0 || W <= 0 || Lkv <= 0 || q_stride <= 0 || Lkv % q_stride) return VDN_EINVAL;
  if ((qkv_lo == nullptr) != (out_lo == nullptr)) return VDN_EINVAL;
  if (dt != VDN_F16 && dt != VDN_BF16) return VDN_EUNSUPPORTED;
  const int64_t rows = (int64_t)frames * W * Lkv;
  if (rows * 3 * heads * HI_DH > ((int64_t)1 << 40) || (int64_t)frames * W > 0x7fffffff || heads > 65535) return VDN_EUNSUPPORTED;
  const int Lq = Lkv / q_stride;
  const dim3 grid((unsigned)(frames * W), heads, (Lq + 63) / 64);
  if (grid.z > 65535) return VDN_EUNSUPPORTED;
  const float sl2 = scale * 1.44269504088896340736f;
  const int C = heads * HI_DH;
  hipStream_t s = (hipStream_t)stream;
  if (dt == VDN_F16)
    hipLaunchKernelGGL(hiera_attn_kernel<VDN_F16>, grid, dim3(64), 0, s, (const _Float16*)qkv, (const _Float16*)qkv_lo, (_Float16*)out,
                       (_Float16*)out_lo, C, W, Lkv, q_stride, sl2);
  else
    hipLaunchKernelGGL(hiera_attn_kernel<VDN_BF16>, grid, dim3(64), 0, s, (const __bf16*)qkv, (const __bf16*)qkv_lo, (__bf16*)out,
                       (__bf16*)out_lo, C, W, Lkv, q_stride, sl2);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_hiera_pool(const float* x, float* y, int frames, int n, int C, vdn_stream stream) {
  if (!x || !y || frames <= 0 || n <= 0 || C <= 0) return VDN_EINVAL;
  if ((C & 3) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return VDN_EALIGN;
  const size_t total4 = (size_t)frames * n * (C >> 2);
  hipLaunchKernelGGL(hiera_pool_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, x, y, total4, n, C >> 2);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_hiera_reroll(const float* tokens, float* map, int frames, int stage, int C, vdn_stream stream) {
  if (!tokens || !map || frames <= 0 || stage < 0 || stage > 3 || C <= 0) return VDN_EINVAL;
  if ((C & 3) || ((uintptr_t)tokens & 15) || ((uintptr_t)map & 15)) return VDN_EALIGN;
  const int n = 3 - stage, side = 7 << n;
  const size_t total4 = (size_t)frames * side * side * (C >> 2);
  hipLaunchKernelGGL(hiera_reroll_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, tokens, map, total4, n, C >> 2);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
