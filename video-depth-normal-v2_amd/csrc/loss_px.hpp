// What the passes of the depth criterion share (loss.hip forward, loss_grad.hip backward): the blocks per frame, the aligned
// prediction, the trimmed criterion's residuals, the gradient through the fit (which ssim.hip shares) and a lane's pixels (swept, loaded and summed as frame_sums.hpp states). Include it AFTER the unit's `#pragma clang fp contract(off)`: aligned()
// is a multiply that feeds an add, and both units must round it twice.
#pragma once
#include "common.hpp"
#include "frame_sums.hpp"

namespace {

constexpr int DL_BPF = 32;        // blocks per frame, fixed so that the workspace depends on B and T alone
constexpr int DL_MAX_SCALES = 4;  // the reference's default, and all its scripts construct

struct MinOp {
  __device__ __forceinline__ float operator()(float a, float b) const { return b < a ? b : a; }
};
struct MaxOp {
  __device__ __forceinline__ float operator()(float a, float b) const { return b > a ? b : a; }
};

// Two roundings. Plain operators, which the unit's pragma keeps apart: the bodies of __fmul_rn and __fadd_rn are compiled under
// the header's contraction mode, and once inlined the pair becomes one v_fma_f32.
__device__ __forceinline__ float aligned(float scale, float p, float shift) {
  const float m = scale * p;
  return m + shift;
}

// The trimmed criterion (vdn_depth_loss_trimmed and its backward): the three residuals |r| it selects among, in fp64 exactly
// as the untrimmed passes sum them, and the selection key of one. The forward's select, its sums and the backward's weights
// all come through these, so they decide on the same bits.
enum { TR_DATA = 0, TR_STABLE = 1, TR_ABSREL = 2, TR_TERMS = 3 };
__device__ __forceinline__ double res_data(float a, float t, double mp, double sp, double mt, double st) {
  return fabs(((double)a - mp) / sp - ((double)t - mt) / st);
}
__device__ __forceinline__ double res_stable(float pg, float tg) { return fabs((double)pg - (double)tg); }
__device__ __forceinline__ double res_absrel(float a, float t) { return fabs(((double)a - (double)t) / (double)t); }
// The float32 rounding of |r| >= 0: its bit pattern is ordered. Every NaN is the one key above +inf's, as torch.sort puts it.
__device__ __forceinline__ uint32_t trim_key(double r) {
  const float v = (float)r;
  return v != v ? 0x7FC00000u : __builtin_bit_cast(uint32_t, v);
}
// The weight of a counted element with key `key`: 1 below the threshold, w at it, 0 above. tr = out + 20 + 5 * term:
// k | n_less | n_tied | thr | w; k == 0 keeps nothing.
__device__ __forceinline__ double trim_weight(const double* __restrict__ tr, uint32_t key) {
  if (!(tr[0] > 0.0)) return 0.0;
  const uint32_t thr = __builtin_bit_cast(uint32_t, (float)tr[3]);
  return key < thr ? 1.0 : (key == thr ? tr[4] : 0.0);
}

// The gradient through the fit at a kept pixel of an item (loss_grad.hip's write pass, ssim.hip's): from g_a of the aligned
// prediction, g_p = sc g_a + (G0 (dN0 - sc dD) + G1 (dN1 - sh dD)) / D with G0 = sum g_a p, G1 = sum g_a over the pixels the
// criterion sums, a01 .. b1 the masked sums of the fit, D = det + 1e-6 (include/vdn.h, vdn_depth_loss_backward).
struct FitGrad {
  double a01, a11, b0, b1, D, G0, G1, sc, sh;
  __device__ __forceinline__ double operator()(double g, double pd, double td) const {
    const double dN0 = a11 * td - b1, dN1 = -b0 - a01 * td + 2.0 * pd * b1, dD = 2.0 * (pd * a11 - a01);
    const double fit = (G0 * (dN0 - sc * dD) + G1 * (dN1 - sh * dD)) / D;
    return sc * g + fit;
  }
};

// PPL consecutive pixels of a frame, loaded as frame_sums.hpp loads them (VEC: one 16-byte load per float plane and one 4-byte
// load of the mask, which the bases must allow; the lane owns the same pixels either way), and which of them the mask keeps.
template <int PPL, bool VEC = (PPL == 4)>
struct Px {
  float p[PPL], t[PPL];
  bool k[PPL];
  __device__ __forceinline__ Px(const float* __restrict__ pf, const float* __restrict__ tf, const uint8_t* __restrict__ mf, int i) {
    load_px<PPL, VEC>(pf + i, p);
    load_px<PPL, VEC>(tf + i, t);
    const uint32_t m = load_mask<PPL, VEC>(mf + i);
#pragma unroll
    for (int j = 0; j < PPL; ++j) k[j] = mask_byte(m, j) != 0;
  }
};

}  // namespace
