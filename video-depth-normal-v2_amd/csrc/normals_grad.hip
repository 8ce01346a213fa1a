// The gradient of the normal criterion (normals.hip, vdn_normal_eval) with respect to its prediction, on the device: what
// autograd computes for g * normal_loss of the reference's VideoNormalLoss. include/vdn.h (vdn_normal_loss_backward) states it.
// F.cosine_similarity clamps the two norms outside the graph, so with n = max(|p|, 1e-8), that = t / max(|t|, 1e-8) and N the
// pixels the erosion keeps over the whole batch, a kept pixel gets
//     dL/dp_c = -(g / N) * (that_c - ((p . that) / n) * (p_c / |p|)) / n          (p_c / |p| := 0 where |p| = 0)
// on both sides of the clamp, a dropped pixel +0.0, and everything +0.0 when N = 0.
// One pass: a lane owns the pixels the forward gives it (four consecutive ones with 16-byte loads and stores where the planes
// allow, one otherwise: frame_sums.hpp), reads the forward's count and the incoming coefficient from device memory and writes its pixels'
// three components once. No sums, no atomics, no workspace: a component depends on its own pixel (and, for a depth target,
// on the pixel's stencil) alone, so the two load shapes and two runs give the same bits. fp64 from the f32 samples,
// contraction off, one rounding to float32 at the store.
// profiles/normal_eval.md found the forward bound by its fp64 divisions and square roots, not by memory, so the divisions are
// counted here: 1 / n and 1 / max(|t|, 1e-8) are formed once per pixel and multiplied into the three channels (two divisions
// where dividing per channel would take nine); 1 / |p| is 1 / n except under the clamp, where a third division is taken.
#include "common.hpp"

#pragma clang fp contract(off)
#include "normal_px.hpp"

namespace {

template <int PPL, bool DEPTH>
__global__ __launch_bounds__(256) void normal_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, int H, int W,
                                                          const double* __restrict__ count, const double* __restrict__ coeff,
                                                          float* __restrict__ grad) {
  const int f = blockIdx.x / NE_BPF, b = blockIdx.x % NE_BPF;
  const int hw = H * W;
  const float* pf = pred + (size_t)f * 3 * hw;
  const float* tf = target + (size_t)f * (DEPTH ? 1 : 3) * hw;
  const uint8_t* mf = mask ? mask + (size_t)f * hw : nullptr;
  float* gf = grad + (size_t)f * 3 * hw;
  const double N = count[0];
  const bool live = N > 0.0;                     // nothing kept: the loss is sum * 0 and its gradient +0.0 everywhere
  const double k = live ? -(coeff[0] / N) : 0.0;
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<NE_BPF, PPL>()) {
    const int p0 = (int)q0;
    float pv[3][PPL], tv[3][PPL], r[3][PPL];
    load3<PPL>(pf, hw, p0, pv);
    if (!DEPTH) load3<PPL>(tf, hw, p0, tv);
    RowWalk at(p0, W);
    const Hood<PPL, DEPTH> hood(tf, mf, at.y, at.x, H, W);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      r[0][j] = r[1][j] = r[2][j] = 0.f;
      if (live && hood.keep(mf, j, at.y, at.x, H, W)) {  // a dropped pixel is skipped: nothing under it is read
        const double a[3] = {(double)pv[0][j], (double)pv[1][j], (double)pv[2][j]};
        double t[3];
        if (DEPTH) hood.normal(tf, j, at.y, at.x, H, W, t);
        else t[0] = (double)tv[0][j], t[1] = (double)tv[1][j], t[2] = (double)tv[2][j];
        const double na = norm3(a);
        const double inv_n = 1.0 / clamp_norm(na), inv_nt = 1.0 / clamp_norm(norm3(t));
        const double inv_na = na >= 1e-8 ? inv_n : (na > 0.0 ? 1.0 / na : 0.0);  // d max(|p|, eps) / dp = p / |p|, 0 at the origin
        const double th[3] = {t[0] * inv_nt, t[1] * inv_nt, t[2] * inv_nt};
        const double d = ((a[0] * th[0] + a[1] * th[1]) + a[2] * th[2]) * inv_n;
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c][j] = (float)(k * ((th[c] - d * (a[c] * inv_na)) * inv_n));
      }
      at.step(W);
    }
    store3<PPL>(gf, hw, p0, r);
  }
}

}  // namespace

extern "C" int vdn_normal_loss_backward_trip(int wide) { return (int)(wide ? sweep_stride<NE_BPF, 4>() : sweep_stride<NE_BPF, 1>()); }

extern "C" int vdn_normal_loss_backward(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int frames,
                                        int H, int W, const double* count, const double* coeff, float* grad_pred, vdn_stream stream) {
  if (!pred || !target || !count || !coeff || !grad_pred) return VDN_EINVAL;
  if (frames <= 0 || H < 2 || W < 2) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX) return VDN_EUNSUPPORTED;
  if (frames > INT32_MAX / NE_BPF) return VDN_EINVAL;
  if (misaligned(4, pred, target, grad_pred) || misaligned(8, count, coeff)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)frames * NE_BPF), block(256);
  // a depth target is read through its stencil, never by quads
  with_ppl(wide_ok((size_t)H * W, {pred, grad_pred, target_is_depth ? nullptr : target}), [&](auto ppl) {
    with_bool(target_is_depth != 0, [&](auto depth) {
      hipLaunchKernelGGL((normal_grad_kernel<decltype(ppl)::value, decltype(depth)::value>), grid, block, 0, s, pred, target, mask,
                         H, W, count, coeff, grad_pred);
    });
  });
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
