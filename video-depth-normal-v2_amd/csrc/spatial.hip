// Spatial / gather kernels (HBM-bound): bilinear resize, patchify, pos-embed bicubic, cubic preprocess, head output,
// MaskDownSampler stages, depthwise 7x7, oc1 combine. (The fused depth tail is tail.hip.)
#include "common.hpp"
#include "resample.hpp"
#include <stddef.h>

namespace {

template <int DT>
__global__ __launch_bounds__(256) void upsample_kernel(const typename Half<DT>::T* __restrict__ x,
                                                       const typename Half<DT>::T* __restrict__ xl,
                                                       typename Half<DT>::T* __restrict__ y,
                                                       typename Half<DT>::T* __restrict__ yl, int B, int IH, int IW,
                                                       int OH, int OW, int C) {
  using T = typename Half<DT>::T;
  using V8 = typename Half<DT>::V8;
  const int cv = C >> 3;
  const size_t total = (size_t)B * OH * OW * cv;
  const float sy = ac_scale(IH, OH), sx = ac_scale(IW, OW);
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c8 = (int)(i % cv);
    size_t pix = i / cv;
    const int ox = (int)(pix % OW);
    pix /= OW;
    const int oy = (int)(pix % OH);
    const int b = (int)(pix / OH);
    const auto [y0, y1, ly] = ac_coord<AcWeight::rounded>(oy, sy, IH);
    const auto [x0, x1, lx] = ac_coord<AcWeight::rounded>(ox, sx, IW);
    const size_t xo = (size_t)b * IH * IW * C + c8 * 8;
    const size_t o00 = xo + ((size_t)y0 * IW + x0) * C, o01 = xo + ((size_t)y0 * IW + x1) * C;
    const size_t o10 = xo + ((size_t)y1 * IW + x0) * C, o11 = xo + ((size_t)y1 * IW + x1) * C;
    const V8 v00 = *(const V8*)(x + o00), v01 = *(const V8*)(x + o01);
    const V8 v10 = *(const V8*)(x + o10), v11 = *(const V8*)(x + o11);
    V8 l00, l01, l10, l11, o, ol;
    if (xl) {
      l00 = *(const V8*)(xl + o00); l01 = *(const V8*)(xl + o01);
      l10 = *(const V8*)(xl + o10); l11 = *(const V8*)(xl + o11);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a00 = (float)v00[e], a01 = (float)v01[e], a10 = (float)v10[e], a11 = (float)v11[e];
      if (xl) { a00 += (float)l00[e]; a01 += (float)l01[e]; a10 += (float)l10[e]; a11 += (float)l11[e]; }
      const float r = bilerp(a00, a01, a10, a11, lx, ly);
      // value by value (not planes.hpp on all 8): with the 8 results live at once the kernel takes 64 -> 72 VGPRs and loses a wave
      if (yl) { T a, b2; split_rtz(r, a, b2); o[e] = a; ol[e] = b2; }
      else o[e] = (T)r;
    }
    *(V8*)(y + i * 8) = o;
    if (yl) *(V8*)(yl + i * 8) = ol;
  }
}

__global__ __launch_bounds__(256) void upsample_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int B,
                                                           int IH, int IW, int OH, int OW, int relu) {
  const size_t total = (size_t)B * OH * OW;
  const float sy = ac_scale(IH, OH), sx = ac_scale(IW, OW);
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    const size_t t = i / OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    y[i] = ac_sample_f32(x + (size_t)b * IH * IW, IH, IW, oy, ox, sy, sx, relu);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img,
                                                       typename Half<DT>::T* __restrict__ rows,
                                                       typename Half<DT>::T* __restrict__ rows_lo, int B, int H, int W,
                                                       int ldk) {
  using T = typename Half<DT>::T;
  using V8 = typename Half<DT>::V8;
  const int ph = H / 14, pw = W / 14;
  const int kv = ldk >> 3;
  const size_t total = (size_t)B * ph * pw * kv;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k8 = (int)(i % kv);
    size_t row = i / kv;
    const int px = (int)(row % pw);
    const size_t t = row / pw;
    const int py = (int)(t % ph);
    const int b = (int)(t / ph);
    V8 o, ol;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k8 * 8 + e;
      float v = 0.f;
      if (k < 588) {
        const int c = k / 196, rem = k - c * 196;
        const int ky = rem / 14, kx = rem - ky * 14;
        v = img[(((size_t)b * 3 + c) * H + py * 14 + ky) * W + px * 14 + kx];
      }
      // value by value (not planes.hpp on all 8): with the 8 values live at once the fp16 kernel takes 30 -> 32 VGPRs
      if (rows_lo) { T a, b2; split_rtz(v, a, b2); o[e] = a; ol[e] = b2; }
      else o[e] = (T)v;
    }
    *(V8*)(rows + i * 8) = o;
    if (rows_lo) *(V8*)(rows_lo + i * 8) = ol;
  }
}

__global__ void fill_row_kernel(float* __restrict__ x, const float* __restrict__ vec, int B, int rows_per_b, int row,
                                int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  x[((size_t)b * rows_per_b + row) * C + c] = vec[c];
}

// torch upsample_bicubic2d (A = -0.75), align_corners=False with an explicit scale factor: src = (dst + 0.5) / scale - 0.5
// (hp_src), border-clamped taps.
__global__ void bicubic_kernel(const float* __restrict__ src, float* __restrict__ dst, int ih, int iw, int oh, int ow,
                               int C, float inv_sy, float inv_sx) {
  const size_t total = (size_t)oh * ow * C;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int ox = (int)(p % ow), oy = (int)(p / ow);
    const float fy = hp_src(oy, inv_sy), fx = hp_src(ox, inv_sx);
    const int iy = (int)floorf(fy), ix = (int)floorf(fx);
    float wy[4], wx[4];
    const CubicTaps ty = cubic_taps(iy, fy - (float)iy, ih, wy), tx = cubic_taps(ix, fx - (float)ix, iw, wx);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float rowv = 0.f;
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) rowv += wx[bq] * src[((size_t)ty.idx(a) * iw + tx.idx(bq)) * C + c];
      acc += wy[a] * rowv;
    }
    dst[i] = acc;
  }
}

// vdn_preprocess: the whole pre-processing of a batch of frames in one launch — u8 [n,h,w,3] (RGB, or BGR with swap_rb) ->
// /255 -> cubic resize to (H, W) (same taps as bicubic_kernel: A = -0.75, half-pixel centres, border clamp; identity-sized
// inputs hit the weights {0,1,0,0} exactly) -> (v - mean[c]) / std[c] -> f32 NCHW. One thread per output pixel, 3 channels.
struct PrepNorm { float mean[3], inv_std[3]; };
__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int n, int ih, int iw,
                                                         int oh, int ow, int swap_rb, PrepNorm nm) {
  const size_t per = (size_t)oh * ow, total = per * n;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int f = (int)(i / per);
    const size_t p = i - (size_t)f * per;
    const int ox = (int)(p % ow), oy = (int)(p / ow);
    int iy, ix;
    float ty, tx;
    halfpixel_coord(oy, ih, oh, iy, ty);
    halfpixel_coord(ox, iw, ow, ix, tx);
    float wy[4], wx[4];
    const CubicTaps cy = cubic_taps(iy, ty, ih, wy), cx = cubic_taps(ix, tx, iw, wx);
    const uint8_t* img = src + (size_t)f * ih * iw * 3;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float rowv[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) {
        const uint8_t* px = img + ((size_t)cy.idx(a) * iw + cx.idx(bq)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) rowv[c] += wx[bq] * ((float)px[c] / 255.0f);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wy[a] * rowv[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int sc = swap_rb ? 2 - c : c;   // output channel c reads source channel sc
      dst[((size_t)f * 3 + c) * per + p] = (acc[sc] - nm.mean[c]) * nm.inv_std[c];
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void head_out_kernel(const typename Half<DT>::T* __restrict__ feat,
                                                       const typename Half<DT>::T* __restrict__ feat_lo,
                                                       const float* __restrict__ w, float bias,
                                                       float* __restrict__ depth, int M, int C, int act, float out_scale) {
  using V8 = typename Half<DT>::V8;
  __shared__ float sw[64];
  if (threadIdx.x < C) sw[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  for (size_t m = blockIdx.x * (size_t)256 + threadIdx.x; m < (size_t)M; m += (size_t)gridDim.x * 256) {
    float acc = bias;
    for (int c = 0; c < C; c += 8) {
      const V8 v = *(const V8*)(feat + m * C + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += sw[c + e] * (float)v[e];
      if (feat_lo) {
        const V8 vl = *(const V8*)(feat_lo + m * C + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += sw[c + e] * (float)vl[e];
      }
    }
    // `act` is the same for the whole grid; the sum in front of it is the same instructions for all three
    depth[m] = act == VDN_OUT_SIGMOID ? scaled_sigmoid(acc, out_scale) : act == VDN_OUT_RELU ? fmaxf(acc, 0.f) : acc;
  }
}

// sigmoid -> conv3x3 s2 p1 (1->4) -> LayerNorm2d(4, eps 1e-6) -> GELU -> conv1x1 (4->1)
// w: [conv w 4x9 | conv b 4 | ln w 4 | ln b 4 | proj w 4 | proj b 1]
__global__ __launch_bounds__(256) void mask_down1_kernel(const float* __restrict__ depth, float* __restrict__ out,
                                                         int B, int H, int W, int OH, int OW,
                                                         const float* __restrict__ w) {
  __shared__ float sw[53];
  if (threadIdx.x < 53) sw[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  const size_t total = (size_t)B * OH * OW;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    const size_t t = i / OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    float in[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
        float v = 0.f;  // zero padding applies to sigmoid(depth), i.e. the padded value is 0
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = 1.f / (1.f + expf(-depth[((size_t)b * H + iy) * W + ix]));
        in[ky * 3 + kx] = v;
      }
    float ch[4], mean = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float a = sw[36 + c];
#pragma unroll
      for (int k = 0; k < 9; ++k) a += sw[c * 9 + k] * in[k];
      ch[c] = a;
      mean += a;
    }
    mean *= 0.25f;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) var += (ch[c] - mean) * (ch[c] - mean);
    const float rstd = 1.f / sqrtf(var * 0.25f + 1e-6f);
    float o = sw[52];
#pragma unroll
    for (int c = 0; c < 4; ++c) o += sw[48 + c] * gelu_erf((ch[c] - mean) * rstd * sw[40 + c] + sw[44 + c]);
    out[i] = o;
  }
}

// conv7x7 s7 (1->49) -> LayerNorm2d(49) -> GELU -> conv1x1 (49->1)
// w: [conv w 49x49 | conv b 49 | ln w 49 | ln b 49 | proj w 49 | proj b 1]
__global__ __launch_bounds__(128) void mask_down2_kernel(const float* __restrict__ in, float* __restrict__ out, int B,
                                                         int H, int W, int OH, int OW, const float* __restrict__ w) {
  __shared__ float sw[2598];
  for (int i = threadIdx.x; i < 2598; i += 128) sw[i] = w[i];
  __syncthreads();
  const size_t i = blockIdx.x * (size_t)128 + threadIdx.x;
  if (i >= (size_t)B * OH * OW) return;
  const int ox = (int)(i % OW);
  const size_t t = i / OW;
  const int oy = (int)(t % OH);
  const int b = (int)(t / OH);
  float px[49];
#pragma unroll
  for (int ky = 0; ky < 7; ++ky)
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) px[ky * 7 + kx] = in[((size_t)b * H + oy * 7 + ky) * W + ox * 7 + kx];
  float ch[49], mean = 0.f;
#pragma unroll
  for (int c = 0; c < 49; ++c) {
    float a = sw[2401 + c];
#pragma unroll
    for (int k = 0; k < 49; ++k) a += sw[c * 49 + k] * px[k];
    ch[c] = a;
    mean += a;
  }
  mean *= (1.f / 49.f);
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < 49; ++c) var += (ch[c] - mean) * (ch[c] - mean);
  const float rstd = 1.f / sqrtf(var * (1.f / 49.f) + 1e-6f);
  float o = sw[2597];
#pragma unroll
  for (int c = 0; c < 49; ++c)
    o += sw[2548 + c] * gelu_erf((ch[c] - mean) * rstd * sw[2450 + c] + sw[2499 + c]);
  out[i] = o;
}

// Depthwise 7x7 (pad 3) on f32 NHWC (sam2/modeling/memory_encoder.py:99-117 CXBlock.dwconv). One workgroup owns
// 8 output rows x all columns x 32 channels: the 14 input rows it needs and the 49 x 32 weights are staged in LDS once
// (round 1 read every input 49 times through L2: 1.3 GB for a 45 MB tensor), then a thread produces runs of 4 adjacent
// outputs for 4 channels, re-using each staged input row segment (10 values) for 28 multiply-adds.
constexpr int DW_TH = 8, DW_CB = 32, DW_PS = 36;  // rows per tile, channels per block, padded pixel stride (floats)
__global__ __launch_bounds__(256) void dwconv7_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H,
                                                      int W, int C, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int WT) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sw = (float*)smem;                 // [49][32]
  float* sx = sw + 49 * DW_CB;              // [DW_TH + 6][WT + 6][DW_PS]  (halo of 3 columns on both sides, zero outside the image)
  // WT: columns per tile (the whole row when it fits the LDS, else 64-column tiles: maps wider than 72 pixels)
  const int cblocks = C / DW_CB, rtiles = (H + DW_TH - 1) / DW_TH, ctiles = (W + WT - 1) / WT;
  int bid = blockIdx.x;
  const int cb = (bid % cblocks) * DW_CB;
  bid /= cblocks;
  const int x0 = (bid % ctiles) * WT;
  bid /= ctiles;
  const int oy0 = (bid % rtiles) * DW_TH, b = bid / rtiles;
  const int Wt = (W - x0) < WT ? (W - x0) : WT;   // columns of this tile
  const int WP = WT + 6;
  for (int i = threadIdx.x; i < 49 * (DW_CB / 4); i += 256) {
    const int t = i / (DW_CB / 4), v = i - t * (DW_CB / 4);
    *(f32x4*)(sw + t * DW_CB + v * 4) = *(const f32x4*)(w + (size_t)t * C + cb + v * 4);
  }
  for (int i = threadIdx.x; i < (DW_TH + 6) * WP * (DW_CB / 4); i += 256) {
    const int v = i % (DW_CB / 4);
    const int p = i / (DW_CB / 4);
    const int r = p / WP, cx = p - r * WP;
    const int iy = oy0 - 3 + r, ix = x0 + cx - 3;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) val = *(const f32x4*)(x + (((size_t)b * H + iy) * W + ix) * C + cb + v * 4);
    *(f32x4*)(sx + (size_t)(r * WP + cx) * DW_PS + v * 4) = val;
  }
  __syncthreads();
  const int v = threadIdx.x & 7, pl = threadIdx.x >> 3;  // 8 channel quads x 32 run lanes
  const int runs_per_row = (Wt + 3) / 4;
  const f32x4 bv = *(const f32x4*)(bias + cb + v * 4);
  for (int run = pl; run < DW_TH * runs_per_row; run += 32) {
    const int ry = run / runs_per_row, ox0 = (run - ry * runs_per_row) * 4;   // tile-local column
    if (oy0 + ry >= H) break;
    f32x4 acc[4] = {bv, bv, bv, bv};
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const float* row = sx + (size_t)((ry + ky) * WP + ox0) * DW_PS + v * 4;
      f32x4 in[10], wk[7];
#pragma unroll
      for (int i = 0; i < 10; ++i) in[i] = (ox0 + i < WP) ? *(const f32x4*)(row + i * DW_PS) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) wk[kx] = *(const f32x4*)(sw + (ky * 7 + kx) * DW_CB + v * 4);
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) acc[o] += in[o + kx] * wk[kx];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (ox0 + o < Wt) *(f32x4*)(y + (((size_t)b * H + oy0 + ry) * W + x0 + ox0 + o) * C + cb + v * 4) = acc[o];
  }
}

// vdn_oc1_combine: conv3x3(pad 1) of a 2x bilinear up-sampling, with the channel mixing already done at the LOW resolution.
// z [B, IH, IW, 9, Co] holds per source pixel the nine tap images Z_t (tap bias included); an output value is the sum over
// the taps that stay inside the OH x OW map of Z_t sampled bilinearly at the tap's position — ac_coord, the expression
// upsample_kernel uses, so the sample positions are those of the materialised map. One workgroup owns OC_T x OC_T output
// pixels x CS channels and stages the source patch those read (11 x 11 pixels at scale 1/2) in LDS once: z crosses the
// memory system about twice (halo) instead of 36 times.
constexpr int OC_T = 16, OC_NT = 512;  // output tile side, threads per workgroup
template <int CS>
__global__ __launch_bounds__(OC_NT) void oc1_combine_kernel(const float* __restrict__ z, const float* __restrict__ bias,
                                                          float* __restrict__ out, int IH, int IW, int OH, int OW, int Co,
                                                          int max_pix) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sz = (float*)smem;  // [patch pixel][tap][CS]
  constexpr int V = CS / 4;
  const float sy = ac_scale(IH, OH), sx = ac_scale(IW, OW);
  const int slices = Co / CS, txn = (OW + OC_T - 1) / OC_T, tyn = (OH + OC_T - 1) / OC_T;
  int bid = blockIdx.x;
  const int cs = (bid % slices) * CS;
  bid /= slices;
  const int ox0 = (bid % txn) * OC_T;
  bid /= txn;
  const int oy0 = (bid % tyn) * OC_T, b = bid / tyn;
  // source rows / columns that the tile's sample positions [o0 - 1, o0 + OC_T] (clipped to the map) touch
  const int ylast = oy0 + OC_T < OH - 1 ? oy0 + OC_T : OH - 1, xlast = ox0 + OC_T < OW - 1 ? ox0 + OC_T : OW - 1;
  constexpr AcWeight R = AcWeight::rounded;  // the materialised map's flavour
  const int py0 = ac_coord<R>(oy0 > 0 ? oy0 - 1 : 0, sy, IH).i0, px0 = ac_coord<R>(ox0 > 0 ? ox0 - 1 : 0, sx, IW).i0;
  const int py1 = ac_coord<R>(ylast, sy, IH).i1, px1 = ac_coord<R>(xlast, sx, IW).i1;
  const int nph = py1 - py0 + 1, npw = px1 - px0 + 1;
  if (nph * npw > max_pix) return;  // the host sized the LDS for every tile of this shape: never taken
  const float* zb = z + ((size_t)b * IH * IW) * 9 * Co + cs;
  const int total = nph * npw * 9 * V;
  constexpr int U = 9;  // loads in flight per thread before the first LDS write: the 11 x 11 patch in one pass
  for (int base = threadIdx.x; base < total; base += OC_NT * U) {
    f32x4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * OC_NT;
      if (i < total) {
        const int v = i % V, t = (i / V) % 9, p = i / (9 * V);
        const int pr = p / npw, pc = p - pr * npw;
        r[u] = *(const f32x4*)(zb + ((size_t)(py0 + pr) * IW + px0 + pc) * 9 * Co + t * Co + v * 4);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * OC_NT;
      if (i < total) *(f32x4*)(sz + (size_t)i * 4) = r[u];  // i = (p * 9 + t) * V + v
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < OC_T * OC_T * V; i += OC_NT) {
    const int v = i % V, pix = i / V;
    const int oy = oy0 + pix / OC_T, ox = ox0 + pix % OC_T;
    if (oy >= OH || ox >= OW) continue;
    int xa[3], xb[3];
    float xl[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = ox + kx - 1;
      AcCoord cx = {0, 0, 0.f};
      if (xx >= 0 && xx < OW) cx = ac_coord<R>(xx, sx, IW);
      xa[kx] = (cx.i0 - px0) * 9 * CS;
      xb[kx] = (cx.i1 - px0) * 9 * CS;
      xl[kx] = cx.l1;
    }
    f32x4 acc = *(const f32x4*)(bias + cs + v * 4);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = oy + ky - 1;
      if (yy < 0 || yy >= OH) continue;
      const auto [y0, y1, ly] = ac_coord<R>(yy, sy, IH);
      const float* r0 = sz + (size_t)(y0 - py0) * npw * 9 * CS + v * 4;
      const float* r1 = sz + (size_t)(y1 - py0) * npw * 9 * CS + v * 4;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = ox + kx - 1;
        if (xx < 0 || xx >= OW) continue;
        const int t = (ky * 3 + kx) * CS;
        const float lx = xl[kx];
        const f32x4 a00 = *(const f32x4*)(r0 + xa[kx] + t), a01 = *(const f32x4*)(r0 + xb[kx] + t);
        const f32x4 a10 = *(const f32x4*)(r1 + xa[kx] + t), a11 = *(const f32x4*)(r1 + xb[kx] + t);
        // not bilerp, on purpose: the four corner weights once per tap instead of three lerps per channel (VALU- and LDS-heavy)
        const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
        acc += w00 * a00 + w01 * a01 + (w10 * a10 + w11 * a11);
      }
    }
    *(f32x4*)(out + (((size_t)b * OH + oy) * OW + ox) * Co + cs + v * 4) = acc;
  }
}

}  // namespace

extern "C" int vdn_upsample_bilinear(int dt, const void* x, const void* x_lo, void* y, void* y_lo, int B, int IH,
                                     int IW, int OH, int OW, int C, vdn_stream stream) {
  if (!x || !y || B <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || C <= 0) return VDN_EINVAL;
  if ((C & 7) || (((uintptr_t)x | (uintptr_t)y) & 15)) return VDN_EALIGN;
  const unsigned g = grid_for((size_t)B * OH * OW * (C >> 3), 16384);
  hipStream_t s = (hipStream_t)stream;
  return with_half(dt, [&](auto t) -> int {
    using T = typename Half<decltype(t)::value>::T;
    hipLaunchKernelGGL(upsample_kernel<decltype(t)::value>, dim3(g), dim3(256), 0, s, (const T*)x, (const T*)x_lo, (T*)y, (T*)y_lo, B,
                       IH, IW, OH, OW, C);
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
}

extern "C" int vdn_upsample_bilinear_f32(const float* x, float* y, int B, int IH, int IW, int OH, int OW, int relu,
                                         vdn_stream stream) {
  if (!x || !y || B <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return VDN_EINVAL;
  hipLaunchKernelGGL(upsample_f32_kernel, dim3(grid_for((size_t)B * OH * OW, 4096)), dim3(256), 0, (hipStream_t)stream, x, y,
                     B, IH, IW, OH, OW, relu);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_oc1_combine(const float* z, const float* bias, float* out, int B, int IH, int IW, int OH, int OW, int Co,
                               vdn_stream stream) {
  if (!z || !bias || !out || B <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || Co <= 0) return VDN_EINVAL;
  if ((Co & 15) || (((uintptr_t)z | (uintptr_t)bias | (uintptr_t)out) & 15)) return VDN_EALIGN;
  // the largest source patch any tile stages, with the kernel's own expressions
  auto span = [](int O, int I) {
    const float s = ac_scale(I, O);
    int worst = 0;
    for (int o0 = 0; o0 < O; o0 += OC_T) {
      const int last = o0 + OC_T < O - 1 ? o0 + OC_T : O - 1;
      const int n = ac_coord<AcWeight::rounded>(last, s, I).i1 - ac_coord<AcWeight::rounded>(o0 > 0 ? o0 - 1 : 0, s, I).i0 + 1;
      worst = n > worst ? n : worst;
    }
    return worst;
  };
  const int max_pix = span(OH, IH) * span(OW, IW);
  constexpr int CS = 16;  // 11 x 11 pixels x 9 taps x 16 channels x 4 B = 68 KiB: two workgroups per CU
  const size_t lds = (size_t)max_pix * 9 * CS * sizeof(float);
  if (lds > 160 * 1024) return VDN_EUNSUPPORTED;  // scale well above 1/2: not a 2x up-sampling
  const size_t blocks = (size_t)B * ((OH + OC_T - 1) / OC_T) * ((OW + OC_T - 1) / OC_T) * (Co / CS);
  if (blocks >= (1u << 31)) return VDN_EUNSUPPORTED;
  static const hipError_t attr = hipFuncSetAttribute((const void*)oc1_combine_kernel<CS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr != hipSuccess) return -(1000 + (int)attr);
  hipLaunchKernelGGL(oc1_combine_kernel<CS>, dim3((unsigned)blocks), dim3(OC_NT), lds, (hipStream_t)stream, z, bias, out, IH, IW, OH,
                     OW, Co, max_pix);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_patchify(int dt, const float* img, void* rows, void* rows_lo, int B, int H, int W, int ldk,
                            vdn_stream stream) {
  if (!img || !rows || B <= 0 || H <= 0 || W <= 0 || H % 14 || W % 14) return VDN_EINVAL;
  if (ldk < 588 || (ldk & 63) || ((uintptr_t)rows & 15)) return VDN_EALIGN;
  const unsigned g = grid_for((size_t)B * (H / 14) * (W / 14) * (ldk >> 3), 8192);
  hipStream_t s = (hipStream_t)stream;
  return with_half(dt, [&](auto t) -> int {
    using T = typename Half<decltype(t)::value>::T;
    hipLaunchKernelGGL(patchify_kernel<decltype(t)::value>, dim3(g), dim3(256), 0, s, img, (T*)rows, (T*)rows_lo, B, H, W, ldk);
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
}

extern "C" int vdn_fill_row(float* x, const float* vec, int B, int rows_per_b, int row, int C, vdn_stream stream) {
  if (!x || !vec || B <= 0 || rows_per_b <= 0 || row < 0 || row >= rows_per_b || C <= 0) return VDN_EINVAL;
  hipLaunchKernelGGL(fill_row_kernel, dim3((B * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, vec, B,
                     rows_per_b, row, C);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_bicubic(const float* src, float* dst, int ih, int iw, int oh, int ow, int C, float scale_rows,
                           float scale_cols, vdn_stream stream) {
  if (!src || !dst || ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0 || C <= 0 || scale_rows <= 0.f || scale_cols <= 0.f)
    return VDN_EINVAL;
  hipLaunchKernelGGL(bicubic_kernel, dim3(grid_for((size_t)oh * ow * C, 4096)), dim3(256), 0, (hipStream_t)stream, src, dst,
                     ih, iw, oh, ow, C, 1.0f / scale_rows, 1.0f / scale_cols);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_preprocess(const uint8_t* frames, int n, int h, int w, int swap_rb, float* out, int H, int W, const float* mean3,
                              const float* std3, vdn_stream stream) {
  if (!frames || !out || !mean3 || !std3 || n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return VDN_EINVAL;
  PrepNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return VDN_EINVAL;
    nm.mean[c] = mean3[c];
    nm.inv_std[c] = 1.0f / std3[c];
  }
  hipLaunchKernelGGL(preprocess_kernel, dim3(grid_for((size_t)n * H * W, 4096)), dim3(256), 0, (hipStream_t)stream, frames, out,
                     n, h, w, H, W, swap_rb, nm);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_head_out_act(int dt, const void* feat, const void* feat_lo, const float* w, float bias, float* depth,
                                int M, int C, int act, float out_scale, vdn_stream stream) {
  if (!feat || !w || !depth || M <= 0 || C <= 0 || C > 64) return VDN_EINVAL;
  if (act != VDN_OUT_NONE && act != VDN_OUT_RELU && act != VDN_OUT_SIGMOID) return VDN_EINVAL;
  if ((C & 7) || ((uintptr_t)feat & 15)) return VDN_EALIGN;
  const unsigned g = grid_for((size_t)M, 8192);
  hipStream_t s = (hipStream_t)stream;
  return with_half(dt, [&](auto t) -> int {
    using T = typename Half<decltype(t)::value>::T;
    hipLaunchKernelGGL(head_out_kernel<decltype(t)::value>, dim3(g), dim3(256), 0, s, (const T*)feat, (const T*)feat_lo, w, bias, depth,
                       M, C, act, out_scale);
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
}

extern "C" int vdn_head_out(int dt, const void* feat, const void* feat_lo, const float* w, float bias, float* depth,
                            int M, int C, int relu, vdn_stream stream) {
  return vdn_head_out_act(dt, feat, feat_lo, w, bias, depth, M, C, relu ? VDN_OUT_RELU : VDN_OUT_NONE, 1.f, stream);
}

extern "C" int vdn_mask_down1(const float* depth, float* out, int B, int H, int W, int OH, int OW, const float* w,
                              vdn_stream stream) {
  if (!depth || !out || !w || B <= 0 || OH != (H + 2 - 3) / 2 + 1 || OW != (W + 2 - 3) / 2 + 1) return VDN_EINVAL;
  hipLaunchKernelGGL(mask_down1_kernel, dim3(grid_for((size_t)B * OH * OW, 4096)), dim3(256), 0, (hipStream_t)stream, depth,
                     out, B, H, W, OH, OW, w);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_mask_down2(const float* in, float* out, int B, int H, int W, int OH, int OW, const float* w,
                              vdn_stream stream) {
  if (!in || !out || !w || B <= 0 || OH != (H - 7) / 7 + 1 || OW != (W - 7) / 7 + 1 || OH <= 0 || OW <= 0)
    return VDN_EINVAL;
  const size_t total = (size_t)B * OH * OW;
  hipLaunchKernelGGL(mask_down2_kernel, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, (hipStream_t)stream, in,
                     out, B, H, W, OH, OW, w);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_dwconv7(const float* x, float* y, int B, int H, int W, int C, const float* w, const float* bias,
                           vdn_stream stream) {
  if (!x || !y || !w || !bias || B <= 0 || H <= 0 || W <= 0 || C <= 0) return VDN_EINVAL;
  if (C % DW_CB) return VDN_EALIGN;
  // the whole row per tile while it fits the 160 KiB of LDS (W <= 72, which takes 163 520 of its 163 840 bytes: the 37 x 37 grid of 518 x 518 inputs), else 64-column tiles
  const int WT = ((size_t)49 * DW_CB + (size_t)(DW_TH + 6) * (W + 6) * DW_PS) * sizeof(float) <= 160 * 1024 ? W : 64;
  const size_t lds = ((size_t)49 * DW_CB + (size_t)(DW_TH + 6) * (WT + 6) * DW_PS) * sizeof(float);
  static const hipError_t attr = hipFuncSetAttribute((const void*)dwconv7_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr != hipSuccess) return -(1000 + (int)attr);
  hipLaunchKernelGGL(dwconv7_kernel, dim3(B * ((H + DW_TH - 1) / DW_TH) * ((W + WT - 1) / WT) * (C / DW_CB)), dim3(256), lds,
                     (hipStream_t)stream, x, y, B, H, W, C, w, bias, WT);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" size_t vdn_sizeof_gemm_desc(void) { return sizeof(vdn_gemm_desc); }
extern "C" size_t vdn_offsetof_gemm_zeros(void) { return offsetof(vdn_gemm_desc, zeros); }
extern "C" size_t vdn_offsetof_gemm_res2_lo(void) { return offsetof(vdn_gemm_desc, res2_lo); }

extern "C" const char* vdn_version(void) { return "vdn-hip 0.1 (gfx950)"; }

extern "C" int vdn_arch_ok(void) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 0;
  const char* a = prop.gcnArchName;
  return (a[0] == 'g' && a[1] == 'f' && a[2] == 'x' && a[3] == '9' && a[4] == '5' && a[5] == '0') ? 1 : 0;
}
