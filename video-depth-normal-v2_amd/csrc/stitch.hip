// Device-side window stitcher for VideoDepthAnything.infer_video_depth (video_depth.py:118-156,
// utils/util.py:40-73): the closed-form scale/shift fit of a new 32-frame window to the running result
// on the 2 alignment frames, the clamp, the 8-frame linear cross-fade and the reference-frame update,
// so that a clip needs ONE device-to-host copy instead of 32 per window.
// vdn_dn_stitch_apply is the same step of VideoDepthEstimationModel.infer_video: depth and the normal's three planes of one
// window, mapped, cross-faded over the overlap and stored into the clip in one launch (the fit is vdn_stitch_fit).
// All HBM-bound, one pass each; the sums are deterministic (fixed partial order, fp64).
#include "common.hpp"
#include "reduce.hpp"

namespace {

constexpr int SUM_BLOCKS = 256;

// partial[b] = {sum p*p, sum p, count, sum p*t, sum t} over this block's grid-stride share
__global__ __launch_bounds__(256) void align_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                            size_t n, double* __restrict__ partial) {
  Tuple<double, 5> s = {{0, 0, 0, 0, 0}};
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 p = *(const f32x4*)(pred + 4 * i), t = *(const f32x4*)(target + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s.v[0] += (double)p[e] * p[e];
      s.v[1] += p[e];
      s.v[3] += (double)p[e] * t[e];
      s.v[4] += t[e];
    }
    s.v[2] += 4.0;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail elements
    const size_t i = (n4 << 2) + threadIdx.x;
    s.v[0] += (double)pred[i] * pred[i];
    s.v[1] += pred[i];
    s.v[2] += 1.0;
    s.v[3] += (double)pred[i] * target[i];
    s.v[4] += target[i];
  }
  __shared__ WaveSlots<Tuple<double, 5>> red;
  red.put(s, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    s = red.get(SumOp{});
#pragma unroll
    for (int k = 0; k < 5; ++k) partial[blockIdx.x * 5 + k] = s.v[k];
  }
}

// coef = {scale, shift}: x = A^-1 b of compute_scale_and_shift_full (utils/util.py:49-60), (1, 0) when det == 0
__global__ void align_solve_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s[5] = {0, 0, 0, 0, 0};
  for (int b = 0; b < nblocks; ++b)
    for (int k = 0; k < 5; ++k) s[k] += partial[b * 5 + k];
  const double det = s[0] * s[2] - s[1] * s[1];
  if (det == 0.0) {
    coef[0] = 1.f;
    coef[1] = 0.f;
  } else {
    coef[0] = (float)((s[2] * s[3] - s[1] * s[4]) / det);
    coef[1] = (float)((-s[1] * s[3] + s[0] * s[4]) / det);
  }
}

// The pixel arithmetic of both stitchers (align_apply_kernel, dn_apply_kernel), written once. Every operation has a rounding
// of its own, as numpy evaluates the float32 expression: plain products and sums with contraction switched off in each
// function. (__fmul_rn and __fadd_rn are a plain product and sum compiled under their header's mode, not this one: nested,
// they came out as one fma.)
__device__ __forceinline__ float affine_px(float d, float scale, float shift) {  // d * scale + shift
#pragma clang fp contract(off)
  return d * scale + shift;
}
// weight of the new window on blend frame k of n: 0, 1/(n-1), .., 1 (get_interpolate_frames, utils/util.py:65-73)
__device__ __forceinline__ float fade_weight(int k, int n, float step) {
#pragma clang fp contract(off)
  return k == 0 ? 0.f : (k == n - 1 ? 1.f : (float)k * step);
}
__device__ __forceinline__ float fade_px(float pre, float post, float w) {  // pre * (1 - w) + post * w
#pragma clang fp contract(off)
  return pre * (1.f - w) + post * w;
}

// One pass over frames `first_fit` .. T-1 of the window (frame-major [T, hw]):
//   frames align_len .. overlap-1      : out_tail[i] = out_tail[i] * (1 - w_i) + fit(frame) * w_i   (i = 0 .. interp-1)
//   frames overlap .. T-1              : out_new[j]  = fit(frame)
//   frame ref_frame (the 2nd keyframe) : ref1        = fit(frame)                                    (extra write)
// fit(d) = max(d * scale + shift, 0) with separate multiply and add roundings (affine_px).
__global__ __launch_bounds__(256) void align_apply_kernel(const float* __restrict__ win, const float* __restrict__ coef,
                                                          float* __restrict__ out_tail, float* __restrict__ out_new,
                                                          float* __restrict__ ref1, size_t hw, int T, int align_len,
                                                          int overlap, int ref_frame) {
  const float scale = coef[0], shift = coef[1];
  const int interp = overlap - align_len;
  const float step = 1.0f / (float)(interp - 1);
  const size_t total = (size_t)(T - align_len) * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int f = align_len + (int)(i / hw);
    const size_t px = i - (size_t)(f - align_len) * hw;
    const float d = fmaxf(affine_px(win[(size_t)f * hw + px], scale, shift), 0.f);
    if (f < overlap) {
      const int k = f - align_len;
      float* o = out_tail + (size_t)k * hw + px;
      *o = fade_px(*o, d, fade_weight(k, interp, step));
    } else {
      out_new[(size_t)(f - overlap) * hw + px] = d;
    }
    if (f == ref_frame) ref1[px] = d;
  }
}

// vdn_dn_stitch_apply: one (frame, plane) of the window per blockIdx.y, plane 0 the depth and 1..3 the normal's nx, ny, nz;
// blockIdx.x strides over the plane's hw / V groups of V pixels (V = 4: 16-byte loads and stores; V = 1 where hw or a pointer
// does not allow them). No index is divided. Streaming: every byte is touched once, DN_BLOCKS blocks and a grid-stride loop.
constexpr unsigned DN_BLOCKS = 2048;

template <int V>
__global__ __launch_bounds__(256) void dn_apply_kernel(const float* __restrict__ depth, const float* __restrict__ normal,
                                                       const float* __restrict__ coef, float* __restrict__ out_depth,
                                                       float* __restrict__ out_normal, size_t hw, int overlap, int clamp0) {
  typedef float Vec __attribute__((ext_vector_type(V)));
  const int t = blockIdx.y >> 2, plane = blockIdx.y & 3;
  const float scale = coef[0], shift = coef[1];
  const bool blend = t < overlap;
  const float w = blend ? fade_weight(t, overlap, 1.0f / (float)(overlap - 1)) : 1.f;
  const size_t at = plane == 0 ? (size_t)t * hw : ((size_t)t * 3 + (plane - 1)) * hw;
  const float* __restrict__ src = (plane == 0 ? depth : normal) + at;
  float* __restrict__ dst = (plane == 0 ? out_depth : out_normal) + at;
  const size_t groups = hw / V;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    Vec v;
    if (plane == 3) {   // nz of (-dx, -dy, 1): 1 before and after the map, and 1 blended with 1
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = 1.f;
    } else {
      v = *(const Vec*)(src + g * V);
      if (plane == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float d = affine_px(v[e], scale, shift);
          v[e] = (clamp0 && d < 0.f) ? 0.f : d;   // np.maximum(d, 0): a NaN stays a NaN
        }
      } else {
        v *= scale;   // gradient of scale * d + shift
      }
      if (blend) {
        const Vec pre = *(const Vec*)(dst + g * V);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = fade_px(pre[e], v[e], w);
      }
    }
    *(Vec*)(dst + g * V) = v;
  }
}

}  // namespace

extern "C" size_t vdn_stitch_workspace_bytes(void) { return (size_t)SUM_BLOCKS * 5 * sizeof(double); }

extern "C" int vdn_stitch_fit(const float* pred, const float* target, size_t n, void* workspace, float* coef,
                              vdn_stream stream) {
  if (!pred || !target || !workspace || !coef || n == 0) return VDN_EINVAL;
  if (((uintptr_t)pred & 15) || ((uintptr_t)target & 15) || ((uintptr_t)workspace & 7)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(align_partial_kernel, dim3(SUM_BLOCKS), dim3(256), 0, s, pred, target, n, (double*)workspace);
  hipLaunchKernelGGL(align_solve_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, SUM_BLOCKS, coef);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_stitch_apply(const float* window, const float* coef, float* out_tail, float* out_new, float* ref1,
                                size_t hw, int T, int align_len, int overlap, int ref_frame, vdn_stream stream) {
  if (!window || !coef || !out_tail || !out_new || !ref1 || hw == 0) return VDN_EINVAL;
  if (T <= overlap || align_len < 0 || overlap - align_len < 2 || ref_frame < align_len || ref_frame >= T) return VDN_EINVAL;
  const size_t total = (size_t)(T - align_len) * hw;
  hipLaunchKernelGGL(align_apply_kernel, dim3(grid_for(total, 16384)), dim3(256), 0, (hipStream_t)stream, window, coef,
                     out_tail, out_new, ref1, hw, T, align_len, overlap, ref_frame);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_dn_stitch_apply(const float* depth, const float* normal, const float* coef, float* out_depth,
                                   float* out_normal, size_t hw, int T, int overlap, int keep, int clamp0, vdn_stream stream) {
  if (!depth || !normal || !coef || !out_depth || !out_normal || hw == 0) return VDN_EINVAL;
  if (T < 1 || T > 8192 || overlap < 0 || overlap == 1 || overlap > T / 2 || keep < 1 || keep > T || (overlap > 0 && keep <= overlap))
    return VDN_EINVAL;
  const unsigned planes = 4u * (unsigned)keep, cap = DN_BLOCKS / planes ? DN_BLOCKS / planes : 1;
  const bool vec = hw % 4 == 0 && !(((uintptr_t)depth | (uintptr_t)normal | (uintptr_t)out_depth | (uintptr_t)out_normal) & 15);
  const dim3 grid(grid_for(vec ? hw / 4 : hw, cap), planes);
  if (vec)
    hipLaunchKernelGGL(dn_apply_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, depth, normal, coef, out_depth, out_normal,
                       hw, overlap, clamp0);
  else
    hipLaunchKernelGGL(dn_apply_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, depth, normal, coef, out_depth, out_normal,
                       hw, overlap, clamp0);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
