// Depth + normal model (models/video_depth_model.py:64-119, models/video_depth_head_v2_sangyu.py:17-317):
// the two kernels of its path that the shared GEMM / LayerNorm / resize / attention kernels do not cover (the grouped
// 8-head self-attention of the head's TransformerBlocks, vdn_dn_attn, is lane_attn_kernel: lane_attn.hip).
//   dn_prologue_kernel  trunk-feature sum + the .view reinterpretation + APE -> frame-major token rows
//   dn_tail_kernel      conv3x3 48->3 + bias, bilinear resize, residual / ReLU, normal assembly
#include "common.hpp"
#include "resample.hpp"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// dn_prologue_kernel — token[(f hw + p), c] = a[f][c hw + p] (+ b[f][c hw + p]) (+ ape[f % S][c]). Each frame's input
// is read as a flat [C, hw] array: for the trunk's NHWC buffers that IS the `.view(B, S, D, H, W)` of
// video_depth_model.py:101-103, for the head's own [B, S, C, h, w] input it is the layout itself. One thread per input
// element (coalesced reads), scattered 2- / 4-byte stores.
template <int DT>
__global__ __launch_bounds__(256) void dn_prologue_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ ape, int S, int C, int hw, size_t n,
                                                          float* __restrict__ out_f, typename Half<DT>::T* __restrict__ out_h,
                                                          typename Half<DT>::T* __restrict__ out_lo) {
  const size_t per = (size_t)C * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t f = i / per;
    const int r = (int)(i - f * per);
    const int c = r / hw, p = r - c * hw;
    float v = a[i];
    if (b) v += b[i];
    if (ape) v += ape[(size_t)(f % S) * C + c];
    const size_t o = (f * hw + p) * C + c;
    if (out_f) out_f[o] = v;
    if (out_h) store_half_nearest(out_h, out_lo, o, v);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// dn_tail_kernel — one thread per output pixel (f, y, x) of the (OH, OW) grid. The 3-channel conv3x3 (pad 1) of the f32
// NHWC map x [F, IH, IW, Cin] is evaluated at the 1 (no resize) or 4 (bilinear, align_corners) source pixels the output
// needs; weights and bias sit in LDS. Outputs: raw [F, 3, OH, OW] (the head's own result) and / or depth [F, OH, OW] =
// relu?(ch0 + depth_in?) with normal [F, 3, OH, OW] = (-ch1, -ch2, 1).
constexpr int TAIL_MAXC = 128;

__device__ __forceinline__ void conv3_at(const float* __restrict__ x, const float* w, int IH, int IW, int Cin, int y, int xx,
                                         float acc[3]) {
  for (int ky = 0; ky < 3; ++ky) {
    const int sy = y + ky - 1;
    if (sy < 0 || sy >= IH) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int sx = xx + kx - 1;
      if (sx < 0 || sx >= IW) continue;
      const float* px = x + ((size_t)sy * IW + sx) * Cin;
      const float* wt = w + (ky * 3 + kx) * 3 * Cin;   // LDS layout [tap][co][ci]
      for (int ci = 0; ci < Cin; ++ci) {
        const float v = px[ci];
        acc[0] = fmaf(wt[ci], v, acc[0]);
        acc[1] = fmaf(wt[Cin + ci], v, acc[1]);
        acc[2] = fmaf(wt[2 * Cin + ci], v, acc[2]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void dn_tail_kernel(const float* __restrict__ x, int F, int IH, int IW, int Cin,
                                                      const float* __restrict__ w, const float* __restrict__ bias, int OH, int OW,
                                                      const float* __restrict__ depth_in, int relu, float* __restrict__ raw,
                                                      float* __restrict__ depth, float* __restrict__ normal) {
  __shared__ float ws[9 * 3 * TAIL_MAXC];
  for (int i = threadIdx.x; i < 27 * Cin; i += 256) {   // w is [3, Cin, 3, 3] (nn.Conv2d) -> [tap][co][ci]
    const int tap = i / (3 * Cin), r = i - tap * 3 * Cin, co = r / Cin, ci = r - co * Cin;
    ws[i] = w[(co * Cin + ci) * 9 + tap];
  }
  __syncthreads();
  const size_t hw = (size_t)OH * OW, n = (size_t)F * hw;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i / hw);
  const int pix = (int)(i - (size_t)f * hw);
  const int oy = pix / OW, ox = pix - oy * OW;
  const float* xf = x + (size_t)f * IH * IW * Cin;
  float v[3] = {bias[0], bias[1], bias[2]};
  if (IH == OH && IW == OW) {
    float acc[3] = {0.f, 0.f, 0.f};
    conv3_at(xf, ws, IH, IW, Cin, oy, ox, acc);
    for (int c = 0; c < 3; ++c) v[c] += acc[c];
  } else {   // F.interpolate(bilinear, align_corners=True) of the conv's output, rounded weights (resample.hpp)
#pragma clang fp contract(off)
    const auto [y0, y1, wy] = ac_coord<AcWeight::rounded>(oy, ac_scale(IH, OH), IH);
    const auto [x0, x1, wx] = ac_coord<AcWeight::rounded>(ox, ac_scale(IW, OW), IW);
    float a00[3] = {0.f, 0.f, 0.f}, a01[3] = {0.f, 0.f, 0.f}, a10[3] = {0.f, 0.f, 0.f}, a11[3] = {0.f, 0.f, 0.f};
    conv3_at(xf, ws, IH, IW, Cin, y0, x0, a00);
    conv3_at(xf, ws, IH, IW, Cin, y0, x1, a01);
    conv3_at(xf, ws, IH, IW, Cin, y1, x0, a10);
    conv3_at(xf, ws, IH, IW, Cin, y1, x1, a11);
    // The blend, with the roundings this kernel has always had written out (the compiler chose them; a call of bilerp, or
    // any change to the lines above, made it choose others): (1 - wx) a0 fused into the rounded wx a1, the two rows' products
    // rounded apart. The bias is constant over the source pixels and the weights sum to 1.
    for (int c = 0; c < 3; ++c) {
      const float top = fmaf(1.f - wx, a00[c], wx * a01[c]), bot = fmaf(1.f - wx, a10[c], wx * a11[c]);
      v[c] += (1.f - wy) * top + wy * bot;
    }
  }
  if (raw) {
    for (int c = 0; c < 3; ++c) raw[((size_t)f * 3 + c) * hw + pix] = v[c];
  }
  if (depth) {
    float d = v[0];
    if (depth_in) d += depth_in[i];
    if (relu) d = fmaxf(d, 0.f);
    depth[i] = d;
    normal[((size_t)f * 3 + 0) * hw + pix] = -v[1];
    normal[((size_t)f * 3 + 1) * hw + pix] = -v[2];
    normal[((size_t)f * 3 + 2) * hw + pix] = 1.f;
  }
}

}  // namespace

extern "C" int vdn_dn_prologue(int dt, const float* a, const float* b, int frames, int C, int hw, const float* ape, int S,
                               float* out_f, void* out_h, void* out_lo, vdn_stream stream) {
  if (!a || frames <= 0 || C <= 0 || hw <= 0 || (!out_f && !out_h) || (out_lo && !out_h)) return VDN_EINVAL;
  if (ape && S <= 0) return VDN_EINVAL;
  if (out_h && dt != VDN_F16 && dt != VDN_BF16) return VDN_EUNSUPPORTED;
  if (!ape) S = 1;
  const size_t n = (size_t)frames * C * hw;
  const int blocks = (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
  hipStream_t s = (hipStream_t)stream;
  return with_half(out_h ? dt : VDN_F16, [&](auto t) -> int {   // without 16-bit planes dt selects nothing
    using T = typename Half<decltype(t)::value>::T;
    hipLaunchKernelGGL(dn_prologue_kernel<decltype(t)::value>, dim3(blocks), dim3(256), 0, s, a, b, ape, S, C, hw, n, out_f, (T*)out_h,
                       (T*)out_lo);
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
}

extern "C" int vdn_dn_tail(const float* x, int F, int IH, int IW, int Cin, const float* w, const float* bias, int OH, int OW,
                           const float* depth_in, int relu, float* raw, float* depth, float* normal, vdn_stream stream) {
  if (!x || !w || !bias || F <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return VDN_EINVAL;
  if (Cin <= 0 || Cin > TAIL_MAXC) return VDN_EUNSUPPORTED;
  if ((!depth) != (!normal) || (!raw && !depth) || (depth_in && !depth)) return VDN_EINVAL;
  const size_t n = (size_t)F * OH * OW;
  if ((n + 255) / 256 > 0x7fffffff) return VDN_EUNSUPPORTED;
  hipLaunchKernelGGL(dn_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, F, IH, IW, Cin, w,
                     bias, OH, OW, depth_in, relu, raw, depth, normal);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
