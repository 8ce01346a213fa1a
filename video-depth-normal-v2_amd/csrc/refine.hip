// Pre/post-processing kernels of the depth-refiner wrappers v2 .. v5 (models/video_depth_model_v5.py:63-87,160-192,
// models/video_depth_model_v4.py:117-148, models/video_depth_model_v3.py:167-206, models/video_depth_model_v2.py:75-100,
// utils/normal_utils.py:4-51):
//   vdn_frame_median  — torch.quantile(x, 0.5) per frame (linear interpolation between the two middle order
//                       statistics) as the exact 3-pass radix select of select.hpp (integer atomics: deterministic),
//                       both ranks in the same passes. A frame that holds a NaN of either sign gets a NaN, as
//                       torch.quantile gives it: the select orders keys by bit pattern, where a NaN sits beyond the
//                       infinity of its sign and would be passed over, so the key functor raises a per-frame flag (a
//                       plain store of 1: every writer stores the same word) that the last kernel reads;
//   vdn_refine_scale  — x / max_depth * exp(tanh(w * median / max_depth + b) * max_log_scale)  (GlobalScaleHead);
//   vdn_refine_pack   — network input [F,3,H,W] = (d, nx, ny) with n = (-Ix, -Iy, 1)/|.|, Sobel/8 on a reflect pad;
//   vdn_refine_finish — (scaled + (w * depth + b)) * max_depth  (scalar 1x1 'ZeroConv' shift + residual; v3: max_depth 1);
//   vdn_refine_normalize — x / max_depth, a true fp32 division (v2 has no scale head, so no median is computed for it);
//   vdn_refine_mix    — relu(a2 * relu(a0 * depth + a1 * x + c0) + c1): v2's final_res (Conv2d(2,1,1) - BatchNorm - ReLU -
//                       Conv2d(1,1,1) - BatchNorm - ReLU) with the eval-mode BatchNorms folded on the host, NaN in -> NaN out.
//   vdn_refine_window_tail — the end of one window of the clip driver (refiner.refine_video_depth): for window slot t, which
//                       shows clip frame f = slots[t], the head's rectified map of slot t sampled at the output pixel
//                       (ac_sample_f32 of resample.hpp, rectified again; or read in place at equal sizes), then the finish
//                       (finish_px) or the mix (MixOp) against scaled[f], the frame of the clip-level scaled input. The
//                       pixel functions are those of vdn_upsample_bilinear_f32, vdn_refine_finish and vdn_refine_mix, so the
//                       result has the bits of gather -> upsample -> finish without the gathered and the resized window.
// All one pass over HBM.
#include "common.hpp"
#include "resample.hpp"
#include "select.hpp"

namespace {

// the plain sample: both slots select among the same keys; nan[f] = 1 when frame f holds a NaN (zeroed before the select)
struct MedianKey {
  static constexpr int SLOTS = 2, PER = 1;
  const float* x;
  size_t n;
  uint32_t* nan;
  __device__ __forceinline__ uint32_t operator()(int f, size_t i, uint32_t (&key)[1][2]) const {
    const float v = x[(size_t)f * n + i];
    if (v != v) nan[f] = 1u;
    key[0][0] = key[0][1] = ordered_key(v);
    return 3u;
  }
};

// the flags sit behind the select's state
inline uint32_t* median_nan_flags(void* workspace, int frames) {
  return (uint32_t*)(select_state(workspace, frames, 2) + (size_t)frames * 2);
}

__global__ void median_final_kernel(const SelState* st, const uint32_t* nan, int F, size_t n, float* median) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  if (nan[f]) {
    median[f] = __builtin_nanf("");
    return;
  }
  const float a = key_value(st[f * 2].prefix), b = key_value(st[f * 2 + 1].prefix);
  const float w = (n & 1) ? 0.f : 0.5f;  // fractional part of 0.5 (n - 1)
  median[f] = w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w);  // at::lerp's two-sided form
}

__global__ __launch_bounds__(256) void refine_scale_kernel(const float* __restrict__ x, const float* __restrict__ median, float w,
                                                           float b, float max_log_scale, float max_depth, float* __restrict__ out,
                                                           float* __restrict__ scale_out, size_t n) {
  const int f = blockIdx.y;
  const float s = __expf(tanhf(__fadd_rn(__fmul_rn(__fdiv_rn(median[f], max_depth), w), b)) * max_log_scale);
  if (blockIdx.x == 0 && threadIdx.x == 0 && scale_out) scale_out[f] = s;
  const float* xf = x + (size_t)f * n;
  float* of = out + (size_t)f * n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    of[i] = __fmul_rn(__fdiv_rn(xf[i], max_depth), s);
}

__global__ __launch_bounds__(256) void refine_pack_kernel(const float* __restrict__ d, float* __restrict__ out, int F, int H, int W,
                                                          int normals) {
  const size_t hw = (size_t)H * W, total = (size_t)F * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int f = (int)(i / hw);
    const int p = (int)(i - (size_t)f * hw);
    const int y = p / W, x = p - y * W;
    const float* df = d + (size_t)f * hw;
    float* of = out + (size_t)f * 3 * hw;
    const float c = df[p];
    of[p] = c;
    if (!normals) {
      of[hw + p] = c;
      of[2 * hw + p] = c;
      continue;
    }
    const int ym = refl_lo(y), yp = refl_hi(y, H), xm = refl_lo(x), xp = refl_hi(x, W);
    const float a00 = df[ym * W + xm], a01 = df[ym * W + x], a02 = df[ym * W + xp];
    const float a10 = df[y * W + xm], a12 = df[y * W + xp];
    const float a20 = df[yp * W + xm], a21 = df[yp * W + x], a22 = df[yp * W + xp];
    // cross-correlation with kx = [[1,0,-1],[2,0,-2],[1,0,-1]]/8, ky = [[1,2,1],[0,0,0],[-1,-2,-1]]/8
    const float ix = ((a00 - a02) + 2.f * (a10 - a12) + (a20 - a22)) * 0.125f;
    const float iy = ((a00 - a20) + 2.f * (a01 - a21) + (a02 - a22)) * 0.125f;
    const float inv = 1.0f / sqrtf(ix * ix + iy * iy + 1.0f + 1e-8f);
    of[hw + p] = -ix * inv;
    of[2 * hw + p] = -iy * inv;
  }
}

// the shift finish on one pixel: (scaled + (w * depth + b)) * max_depth. w * depth + b is ONE fused operation, the sum and the
// product are rounded on their own: what hipcc has always made of refine_finish_kernel's __fadd_rn(__fmul_rn(d, w), b) (the _rn
// intrinsics are plain operators to it, and it contracts them), written out under contract(off) so that every caller, the window
// tail included, gets these roundings whatever the compiler would choose there.
__device__ __forceinline__ float finish_px(float s, float d, float w, float b, float max_depth) {
#pragma clang fp contract(off)
  return (s + fmaf(d, w, b)) * max_depth;
}
// without the residual: depth * max_depth
__device__ __forceinline__ float finish_px(float d, float max_depth) { return d * max_depth; }

__global__ __launch_bounds__(256) void refine_finish_kernel(const float* __restrict__ scaled, const float* __restrict__ depth, float w,
                                                            float b, float max_depth, int residual, float* __restrict__ out,
                                                            size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float d = depth[i];
    out[i] = residual ? finish_px(scaled[i], d, w, b, max_depth) : finish_px(d, max_depth);
  }
}

template <int PPL>
__device__ __forceinline__ void load_px(const float* p, int i, float (&v)[PPL]) {
  if constexpr (PPL == 4) {
    const f32x4 q = *(const f32x4*)(p + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  } else {
    v[0] = p[i];
  }
}
template <int PPL>
__device__ __forceinline__ void store_px(float* p, int i, const float (&v)[PPL]) {
  if constexpr (PPL == 4) *(f32x4*)(p + i) = f32x4{v[0], v[1 % PPL], v[2 % PPL], v[3 % PPL]};
  else p[i] = v[0];
}

// v2's folded final_res on one pixel; the comparison (not fmaxf) keeps torch.relu's NaN: NaN < 0 is false
struct MixOp {
  static constexpr int kInputs = 2;
  float a0, a1, c0, a2, c1;
  __device__ __forceinline__ float relu(float v) const { return v < 0.f ? 0.f : v; }
  __device__ __forceinline__ float operator()(float d, float x) const {
    return relu(fmaf(a2, relu(fmaf(a0, d, fmaf(a1, x, c0))), c1));
  }
};

struct NormalizeOp {
  static constexpr int kInputs = 1;
  float max_depth;
  __device__ __forceinline__ float operator()(float x, float) const { return __fdiv_rn(x, max_depth); }
};

// out[i] = op(a[i], b[i]) over n floats. Elements [head, head + 4 nvec) are 16-byte aligned in every array and go as
// float4 per lane; the < 4 in front and the < 4 behind go one float per lane. Arrays whose offsets inside a 16-byte line
// differ get nvec = 0 from the host: everything is the scalar part then.
template <class Op>
__global__ __launch_bounds__(256) void elementwise_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ out, size_t n, size_t head, size_t nvec, Op op) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const float4* a4 = reinterpret_cast<const float4*>(a + head);
  const float4* b4 = reinterpret_cast<const float4*>(b + head);
  float4* o4 = reinterpret_cast<float4*>(out + head);
  for (size_t i = tid; i < nvec; i += stride) {
    const float4 va = a4[i];
    float4 vb = va;
    if constexpr (Op::kInputs == 2) vb = b4[i];
    o4[i] = make_float4(op(va.x, vb.x), op(va.y, vb.y), op(va.z, vb.z), op(va.w, vb.w));
  }
  const size_t rest = n - 4 * nvec;
  for (size_t i = tid; i < rest; i += stride) {
    const size_t j = i < head ? i : i + 4 * nvec;
    float vb = 0.f;
    if constexpr (Op::kInputs == 2) vb = b[j];
    out[j] = op(a[j], vb);
  }
}

// The window tail's finish kinds as (depth, scaled) -> out functors; kInputs == 1 never reads `scaled`.
struct ShiftOp {
  static constexpr int kInputs = 2;
  float w, b, max_depth;
  __device__ __forceinline__ float operator()(float d, float s) const { return finish_px(s, d, w, b, max_depth); }
};
struct UnitOp {
  static constexpr int kInputs = 1;
  float max_depth;
  __device__ __forceinline__ float operator()(float d, float) const { return finish_px(d, max_depth); }
};

// One window: block (b, t) owns the pixels (b * 256 + lane) * PPL + k * trip of slot t, trip = WT_BPS * 256 * PPL; PPL = 4 where
// a row is a multiple of 4 pixels and the bases are 16-byte aligned (the host decides), so a lane's four pixels lie in one row
// and go as one 16-byte load per input and one 16-byte store. RESAMPLE: net is [T, IH, IW] and is sampled; otherwise it has
// the output's size and is read in place. A slot outside [0, frames) (the host range-checks the table, so: a corrupted one)
// reads nothing of `scaled` and writes NaN, which the driver's range check reports.
constexpr int WT_BPS = 64;  // blocks per window slot
template <class Op, bool RESAMPLE, int PPL>
__global__ __launch_bounds__(256) void refine_window_tail_kernel(const float* __restrict__ net, int IH, int IW,
                                                                 const float* __restrict__ scaled, int frames,
                                                                 const int32_t* __restrict__ slots, int OH, int OW,
                                                                 float* __restrict__ out, Op op) {
  const int t = blockIdx.y, f = slots[t];
  const bool bad = (unsigned)f >= (unsigned)frames;
  const int n = OH * OW;
  const float* nb = net + (size_t)t * (RESAMPLE ? (size_t)IH * IW : (size_t)n);
  const float* sb = scaled + (size_t)(bad ? 0 : f) * n;   // not dereferenced when Op::kInputs == 1 (scaled may be null) or bad
  float* ob = out + (size_t)t * n;
  const float sy = ac_scale(IH, OH), sx = ac_scale(IW, OW);
  const int trip = WT_BPS * 256 * PPL;
  for (int64_t q64 = (int64_t)(blockIdx.x * 256 + (int)threadIdx.x) * PPL; q64 < n; q64 += trip) {
    const int q = (int)q64;
    float d[PPL], s[PPL] = {}, o[PPL];
    if constexpr (RESAMPLE) {
      const int oy = q / OW, ox = q - oy * OW;
#pragma unroll
      for (int j = 0; j < PPL; ++j) d[j] = ac_sample_f32(nb, IH, IW, oy, ox + j, sy, sx, 1);
    } else {
      load_px<PPL>(nb, q, d);
    }
    if constexpr (Op::kInputs == 2) {
      if (!bad) load_px<PPL>(sb, q, s);
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) o[j] = bad ? __builtin_nanf("") : op(d[j], s[j]);
    store_px<PPL>(ob, q, o);
  }
}

template <class Op>
int launch_window_tail(const float* net, int IH, int IW, const float* scaled, int frames, const int32_t* slots, int T, int OH, int OW,
                       float* out, Op op, vdn_stream stream) {
  const bool resample = IH != OH || IW != OW;
  const uintptr_t bases = (uintptr_t)out | (Op::kInputs == 2 ? (uintptr_t)scaled : 0) | (resample ? 0 : (uintptr_t)net);
  const bool wide = OW % 4 == 0 && (bases & 15) == 0;
  const dim3 grid(WT_BPS, T), block(256);
  hipStream_t s = (hipStream_t)stream;
#define VDN_WT(R, P) \
  hipLaunchKernelGGL((refine_window_tail_kernel<Op, R, P>), grid, block, 0, s, net, IH, IW, scaled, frames, slots, OH, OW, out, op)
  if (resample) {
    if (wide) VDN_WT(true, 4); else VDN_WT(true, 1);
  } else {
    if (wide) VDN_WT(false, 4); else VDN_WT(false, 1);
  }
#undef VDN_WT
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

template <class Op>
int launch_elementwise(const float* a, const float* b, float* out, size_t n, Op op, vdn_stream stream) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)(b ? b : a), po = (uintptr_t)out;
  if ((pa | pb | po) & 3) return VDN_EINVAL;
  size_t head = 0, nvec = 0;
  if ((pa & 15) == (pb & 15) && (pa & 15) == (po & 15)) {
    head = ((16 - (pa & 15)) & 15) / 4;
    if (head > n) head = n;
    nvec = (n - head) / 4;
  }
  const size_t lanes = nvec > n - 4 * nvec ? nvec : n - 4 * nvec;
  hipLaunchKernelGGL(elementwise_kernel<Op>, dim3(grid_for(lanes, 16384)), dim3(256), 0, (hipStream_t)stream, a, b ? b : a, out, n,
                     head, nvec, op);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

}  // namespace

extern "C" size_t vdn_frame_median_workspace_bytes(int frames) {
  return frames <= 0 ? 0 : select_workspace_bytes(frames, 2) + (size_t)frames * sizeof(uint32_t);   // + the NaN flags
}

extern "C" int vdn_frame_median(const float* x, int frames, size_t n, float* median, void* workspace, vdn_stream stream) {
  if (!x || !median || !workspace || frames <= 0 || n == 0) return VDN_EINVAL;
  if (n >= ((size_t)1 << 32)) return VDN_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* nan = median_nan_flags(workspace, frames);
  const hipError_t e = hipMemsetAsync(nan, 0, (size_t)frames * sizeof(uint32_t), s);
  if (e != hipSuccess) return -(1000 + (int)e);
  select_launch(MedianKey{x, n, nan}, frames, 1, n, SelRanks<2>{{(uint32_t)((n - 1) / 2), (uint32_t)(n / 2)}, nullptr}, workspace, s);  // floor / ceil of 0.5 (n - 1)
  hipLaunchKernelGGL(median_final_kernel, dim3((frames + 63) / 64), dim3(64), 0, s, select_state(workspace, frames, 2), nan, frames, n,
                     median);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_refine_scale(const float* x, const float* median, int frames, size_t n, float w, float b, float max_log_scale,
                                float max_depth, float* out, float* scale_out, vdn_stream stream) {
  if (!x || !median || !out || frames <= 0 || n == 0 || !(max_depth > 0.f)) return VDN_EINVAL;
  hipLaunchKernelGGL(refine_scale_kernel, dim3(grid_for(n, 256), frames), dim3(256), 0, (hipStream_t)stream, x, median, w, b,
                     max_log_scale, max_depth, out, scale_out, n);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_refine_pack(const float* d, float* out, int frames, int H, int W, int normals, vdn_stream stream) {
  if (!d || !out || frames <= 0 || H < 2 || W < 2) return VDN_EINVAL;
  hipLaunchKernelGGL(refine_pack_kernel, dim3(grid_for((size_t)frames * H * W, 16384)), dim3(256), 0, (hipStream_t)stream, d, out,
                     frames, H, W, normals);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_refine_finish(const float* scaled, const float* depth, float w, float b, float max_depth, int residual,
                                 float* out, size_t n, vdn_stream stream) {
  if (!depth || !out || n == 0 || (residual && !scaled)) return VDN_EINVAL;
  hipLaunchKernelGGL(refine_finish_kernel, dim3(grid_for(n, 16384)), dim3(256), 0, (hipStream_t)stream, scaled, depth, w, b,
                     max_depth, residual, out, n);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_refine_normalize(const float* x, float max_depth, float* out, size_t n, vdn_stream stream) {
  if (!x || !out || n == 0 || !(max_depth > 0.f)) return VDN_EINVAL;
  return launch_elementwise(x, nullptr, out, n, NormalizeOp{max_depth}, stream);
}

extern "C" int vdn_refine_mix(const float* depth, const float* x, float a0, float a1, float c0, float a2, float c1, float* out,
                              size_t n, vdn_stream stream) {
  if (!depth || !x || !out || n == 0) return VDN_EINVAL;
  return launch_elementwise(depth, x, out, n, MixOp{a0, a1, c0, a2, c1}, stream);
}

extern "C" int vdn_refine_window_tail_trip(int wide) { return WT_BPS * 256 * (wide ? 4 : 1); }

extern "C" int vdn_refine_window_tail(const float* net, int IH, int IW, const float* scaled, int frames, const int32_t* slots, int T,
                                      int OH, int OW, int kind, int residual, float c0, float c1, float c2, float c3, float c4,
                                      float* out, vdn_stream stream) {
  if (!net || !slots || !out || T <= 0 || T > 65535 || frames <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return VDN_EINVAL;
  if (kind != VDN_TAIL_SHIFT && kind != VDN_TAIL_MIX) return VDN_EINVAL;
  if ((kind == VDN_TAIL_MIX || residual) && !scaled) return VDN_EINVAL;
  if ((size_t)OH * OW > (size_t)INT32_MAX || (size_t)IH * IW > (size_t)INT32_MAX) return VDN_EUNSUPPORTED;
  if (((uintptr_t)net | (uintptr_t)scaled | (uintptr_t)out | (uintptr_t)slots) & 3) return VDN_EALIGN;
  if (kind == VDN_TAIL_MIX)
    return launch_window_tail(net, IH, IW, scaled, frames, slots, T, OH, OW, out, MixOp{c0, c1, c2, c3, c4}, stream);
  if (residual) return launch_window_tail(net, IH, IW, scaled, frames, slots, T, OH, OW, out, ShiftOp{c0, c1, c2}, stream);
  return launch_window_tail(net, IH, IW, nullptr, frames, slots, T, OH, OW, out, UnitOp{c2}, stream);
}
