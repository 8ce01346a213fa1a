// Source coordinates and blends of every resize in the library, each written once. Four coordinate rules:
//   align-corners         ac_scale + ac_coord<AcWeight>   torch's bilinear, align_corners=True (two weight flavours)
//   half-pixel, fp32      hp_src, hp_source               torch's bilinear / bicubic, align_corners=False
//   half-pixel, exact     halfpixel_coord                 integer split of the same coordinate, for the cubic preprocess
//   cubic taps            cubic_w, cubic_taps             torch's upsample_bicubic2d (A = -0.75), border-clamped
// A function here is compiled under the contraction mode in force HERE, not at its call site: the ones whose roundings
// matter set their own mode, so neither the including file's pragma nor a build flag changes them.
#pragma once
#include <math.h>

// scale = (in - 1) / (out - 1) in float, 0 for a single output: PyTorch's area_pixel_compute_scale, align_corners=True.
__host__ __device__ inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// PyTorch's align_corners=True source position src = fl(scale * dst): i0 = its integer part clamped to the map, i1 the
// next pixel, l1 the weight of i1. The weight comes in two flavours, named at every call site:
//   rounded  fl(src - i0), from the ROUNDED product, under contract(off): torch's fp32 CPU arithmetic, bit for bit.
//            upsample_kernel, upsample_f32_kernel, oc1_combine_kernel, dn_tail_kernel. Pinned by test_gpu_geometry.py
//            (UPSAMPLE BAR) and test_gpu_resample.py.
//   fused    the same two statements under contract(fast), which hipcc turns into v_fma_f32(scale, dst, -i0) in
//            depth_tail_kernel, its only user: one rounding, the more exact weight, up to 2^-24 src away from torch's (4e-4 of
//            a depth of 10 at a 1080-row frame). Pinned by test_gpu_resample.py, which fails if the weight stops being fused.
//            (Written as fmaf() the weight is the same, but hipcc then packs that kernel's blend differently, fuses other
//            products of it, and the depth moves in its last bit: profiles/resample_refactor.md.)
enum class AcWeight { rounded, fused };
struct AcCoord { int i0, i1; float l1; };
template <AcWeight W>
__host__ __device__ __forceinline__ AcCoord ac_coord(int o, float scale, int in) {
  int i0;
  float l1;
  if constexpr (W == AcWeight::rounded) {
#pragma clang fp contract(off)
    const float src = scale * (float)o;
    i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;
    l1 = src - (float)i0;
  } else {
#pragma clang fp contract(fast)
    const float src = scale * (float)o;
    i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;
    l1 = src - (float)i0;
  }
  return {i0, i0 < in - 1 ? i0 + 1 : i0, l1};
}

// (1 - ly) ((1 - lx) a00 + lx a01) + ly ((1 - lx) a10 + lx a11) on floats, under contract(fast): which products are
// fused into the sums is the compiler's choice per call site. upsample_kernel only (ac_sample_f32 below is the fp32 map's,
// with the roundings pinned): in
// depth_tail_kernel and dn_tail_kernel a call of this function changes that choice and with it the last bit of the result,
// so they keep the expression in place; oc1_combine_kernel's four corner weights and resize_bilinear_hp_kernel's separately
// rounded products are other expressions, on purpose.
template <class T>
__device__ __forceinline__ T bilerp(T a00, T a01, T a10, T a11, float lx, float ly) {
#pragma clang fp contract(fast)
  const T top = (1.f - lx) * a00 + lx * a01;
  const T bot = (1.f - lx) * a10 + lx * a11;
  return (1.f - ly) * top + ly * bot;
}

// One output pixel (oy, ox) of the align-corners bilinear resize of the fp32 map xb [IH, IW], rounded weights, rectified when
// relu != 0 (fmaxf: a NaN sample becomes 0): the pixel of upsample_f32_kernel, and of refine_window_tail_kernel, which
// samples the head's map where it finishes a window and never stores the resized one. sy, sx = ac_scale of the two axes.
// The blend is bilerp's expression with its roundings WRITTEN OUT, under contract(off): the ones hipcc chose for
// upsample_f32_kernel while that kernel held a call of bilerp (it packs the two rows into one v_pk_fma_f32 pair, hence the
// mirrored rows: the upper row rounds its left product, the lower row its right one, and both products of the last line are
// rounded). A second caller of bilerp gets other fusions (measured: one v_fmac per line), so the two kernels would differ
// in the last bit; written out, both give the bits upsample_f32_kernel has always given (profiles/refine_clip.md).
__device__ __forceinline__ float ac_sample_f32(const float* __restrict__ xb, int IH, int IW, int oy, int ox, float sy, float sx,
                                               int relu) {
#pragma clang fp contract(off)
  const auto [y0, y1, ly] = ac_coord<AcWeight::rounded>(oy, sy, IH);
  const auto [x0, x1, lx] = ac_coord<AcWeight::rounded>(ox, sx, IW);
  const float a00 = xb[y0 * IW + x0], a01 = xb[y0 * IW + x1], a10 = xb[y1 * IW + x0], a11 = xb[y1 * IW + x1];
  const float mx = 1.f - lx, my = 1.f - ly;
  const float top = fmaf(lx, a01, mx * a00);
  const float bot = fmaf(mx, a10, lx * a11);
  float v = my * top + ly * bot;
  if (relu) v = fmaxf(v, 0.f);
  return v;
}

// Half-pixel source position (dst + 0.5) * scale - 0.5 with scale = in / out (or 1 / scale_factor), fused: the float32
// arithmetic of F.interpolate(align_corners=False), whose builds contract this expression; a separately rounded product
// moves a weight by an ulp of the coordinate, 1e-6 of the result. Pinned by test_gpu_eval.py's resize tests.
__device__ __forceinline__ float hp_src(int dst, float scale) {
#pragma clang fp contract(off)
  return fmaf(scale, (float)dst + 0.5f, -0.5f);
}

// Half-pixel bilinear: hp_src clamped at 0, the two pixels and their weights; the weights then match torch's bit for bit.
__device__ __forceinline__ void hp_source(int dst, float scale, int in, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
  float src = hp_src(dst, scale);
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  w1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  w0 = 1.f - w1;
}

// Half-pixel source coordinate (o + 0.5) * in / out - 0.5 = num / den with num = (2 o + 1) in - out, den = 2 out, split
// EXACTLY into its floor and its fraction: an fp32 product with a rounded in / out is off by up to 2^-24 of the coordinate,
// which at a 1080-row frame moves the fraction (and with it every cubic weight) by 1e-4. 64-bit: num reaches 2 in out.
// The fraction's numerator is below den, so both conversions are exact while out < 2^23 and the quotient is rounded once.
// Pinned by test_gpu_geometry.py (PREPROCESS BAR).
__device__ __forceinline__ void halfpixel_coord(int o, int in, int out, int& i, float& t) {
  const long long den = 2ll * out, num = (2ll * o + 1) * in - out;
  long long q = num / den, r = num - q * den;
  if (r < 0) { r += den; --q; }   // floor, not truncation: num < 0 left of / above the first source centre when up-scaling
  i = (int)q;
  t = (float)r / (float)den;
}

// torch upsample_bicubic2d (A = -0.75): the weights of the taps i - 1 .. i + 2 at fraction t.
__device__ __forceinline__ void cubic_w(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// One axis of a cubic resize: the weights of the four taps i - 1 .. i + 2 at fraction t, into the caller's w, and the
// taps' border-clamped source indices. The caller keeps its own pixel fetch and its own summation order. (The weights stay
// a plain local array: held in this struct, hipcc packs two of preprocess_kernel's products into one multiply and they lose
// their fused add, which moves the result's last bit.)
struct CubicTaps {
  int i, in;
  __device__ __forceinline__ int idx(int a) const {   // a = 0 .. 3
    const int v = i - 1 + a;
    return v < 0 ? 0 : (v > in - 1 ? in - 1 : v);
  }
};
__device__ __forceinline__ CubicTaps cubic_taps(int i, float t, int in, float w[4]) {
  cubic_w(t, w);
  return {i, in};
}
