// Normal evaluation on the device: the reference's normal_vector / sobel_ix_iy (utils/normal_utils.py:4-52) and its
// VideoNormalLoss (loss/loss.py:370-409), for tensors that already sit in HBM.
//   vdn_sobel_ix_iy, vdn_normal_vector  the Sobel stencil on the reflect-padded depth and the unit normals made from it
//   vdn_erode_mask3                     the 3 x 3 erosion of the loss's mask
//   vdn_normal_eval                     one pass: erode, (make the target normal from depth,) cosine, per-block partial
//                                       sums; then a one-block finalise
// The stencil, the normalisation and the cosine are fp64 computed from the f32 samples, with separate multiply and add
// roundings (contraction is off for this file). Sums have the fixed order of frame_sums.hpp, with NE_BPF blocks per frame. No
// atomics: two runs give the same bits. Any 4-byte-aligned pointer is accepted; vdn_normal_eval reads pred (and a stored
// target) four floats per lane where the planes are 16-byte aligned, one per lane otherwise. Stencil and erosion neighbours
// that belong to other lanes or blocks are read through the cache, as refine_pack_kernel does; the four pixels of a lane share theirs.
#include "common.hpp"
#include "frame_sums.hpp"

#pragma clang fp contract(off)
#include "normal_px.hpp"

namespace {

// workspace, in 8-byte slots: [T] frame sums | [T] frame counts (i64) | [T][NE_BPF] block sums | [T][NE_BPF] block counts
struct Ws {
  double* fsum;
  int64_t* fcnt;
  double* bsum;
  int64_t* bcnt;
  __host__ __device__ Ws(void* p, int T) {
    fsum = (double*)p;
    fcnt = (int64_t*)(fsum + T);
    bsum = (double*)(fcnt + T);
    bcnt = (int64_t*)(bsum + (size_t)T * NE_BPF);
  }
};

// F.cosine_similarity(a, b, dim, eps = 1e-8) of torch 2.x: sum_c (a_c / max(|a|, eps)) * (b_c / max(|b|, eps)), evaluated as
// (a . b) / (max(|a|, eps) * max(|b|, eps)): the same number in exact arithmetic with one fp64 division in place of six
// (the kernel is bound by its fp64 divisions and square roots, not by memory: profiles/normal_eval.md). Neither form can
// overflow from float32 inputs, and inf or NaN components give NaN in both. The comparison (not fmax) keeps a NaN norm.
__device__ __forceinline__ double cosine3(const double (&a)[3], const double (&b)[3]) {
  const double na = clamp_norm(norm3(a)), nb = clamp_norm(norm3(b));
  return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (na * nb);
}

// ------------------------------------------------------------------------------------------------ stencil outputs
// MODE 0: o0, o1 = Ix, Iy planes [F, H, W]; MODE 1: o0 = normals [F, 3, H, W]
template <int MODE>
__global__ __launch_bounds__(256) void normal_vector_kernel(const float* __restrict__ d, float* __restrict__ o0, float* __restrict__ o1,
                                                            int F, int H, int W, double k, double sxy, double sz, double eps) {
  const size_t hw = (size_t)H * W, total = (size_t)F * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t f = i / hw;
    const int p = (int)(i - f * hw);
    const int y = p / W, x = p - y * W;
    float a[3][3];
    window_at(d + f * hw, y, x, H, W, a);
    double ix, iy;
    sobel(a, k, ix, iy);
    if (MODE == 0) {
      o0[i] = (float)ix;
      o1[i] = (float)iy;
    } else {
      double n[3];
      unit_normal(ix, iy, sxy, sz, eps, n);
      float* of = o0 + f * 3 * hw;
      of[p] = (float)n[0];
      of[hw + p] = (float)n[1];
      of[2 * hw + p] = (float)n[2];
    }
  }
}

__global__ __launch_bounds__(256) void erode_mask3_kernel(const uint8_t* __restrict__ m, uint8_t* __restrict__ out, int F, int H, int W) {
  const size_t hw = (size_t)H * W, total = (size_t)F * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t f = i / hw;
    const int p = (int)(i - f * hw);
    const int y = p / W;
    out[i] = kept_at(m + f * hw, y, p - y * W, H, W) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ fused loss
// PPL pixels per lane, consecutive in the frame: 4 (16-byte loads of the pred / target planes; needs hw % 4 == 0 and
// 16-byte-aligned bases) or 1. DEPTH: target is a depth map and the target normal is made here.
template <int PPL, bool DEPTH>
__global__ __launch_bounds__(256) void normal_eval_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const uint8_t* __restrict__ mask, int T, int H, int W,
                                                                  void* __restrict__ workspace) {
  const Ws ws(workspace, T);
  const int f = blockIdx.x / NE_BPF, b = blockIdx.x % NE_BPF;
  const int hw = H * W;
  const float* pf = pred + (size_t)f * 3 * hw;
  const float* tf = target + (size_t)f * (DEPTH ? 1 : 3) * hw;
  const uint8_t* mf = mask ? mask + (size_t)f * hw : nullptr;
  Tuple<double, 1> sum = {{0.0}};
  Tuple<int, 1> cnt = {{0}};
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<NE_BPF, PPL>()) {
    const int p0 = (int)q0;
    float pv[3][PPL], tv[3][PPL];
    load3<PPL>(pf, hw, p0, pv);
    if (!DEPTH) load3<PPL>(tf, hw, p0, tv);
    RowWalk at(p0, W);
    const Hood<PPL, DEPTH> hood(tf, mf, at.y, at.x, H, W);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (hood.keep(mf, j, at.y, at.x, H, W)) {  // a dropped pixel is skipped: nothing under it is read into the sums
        const double a[3] = {(double)pv[0][j], (double)pv[1][j], (double)pv[2][j]};
        double t[3];
        if (DEPTH) hood.normal(tf, j, at.y, at.x, H, W, t);
        else t[0] = (double)tv[0][j], t[1] = (double)tv[1][j], t[2] = (double)tv[2][j];
        sum.v[0] += cosine3(a, t);
        cnt.v[0] += 1;
      }
      at.step(W);
    }
  }
  block_row<1, 1>(sum, cnt, ws.bsum, ws.bcnt);
}

// One block: the fold of frame_sums.hpp.
__global__ __launch_bounds__(256) void normal_eval_finalise_kernel(void* __restrict__ workspace, int T, double* __restrict__ frame_sums,
                                                                   int64_t* __restrict__ frame_counts, double* __restrict__ out) {
  const Ws ws(workspace, T);
  for (int f = threadIdx.x; f < T; f += 256) {
    double s;
    int64_t n;
    fold_blocks<1, 1, NE_BPF>(ws.bsum, ws.bcnt, f, &s, &n);
    store_row<1, 1>(ws.fsum, ws.fcnt, (size_t)f, &s, &n);
    if (frame_sums) frame_sums[f] = s;
    if (frame_counts) frame_counts[f] = n;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s;
  int64_t n;
  fold_frames<1, 1>(ws.fsum, ws.fcnt, 0, T, &s, &n);
  out[0] = n > 0 ? 1.0 - s / (double)n : 1.0;  // reduction_batch_based: sum * 0 when nothing is kept
  out[1] = (double)n;
}

// the shared argument checks of the stencil entries; VDN_OK when the call may launch
inline int check_frames(int frames, int H, int W) {
  if (frames <= 0 || H < 2 || W < 2) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX) return VDN_EUNSUPPORTED;
  return VDN_OK;
}

}  // namespace

extern "C" size_t vdn_normal_eval_workspace_bytes(int frames) {
  if (frames <= 0) return 0;
  return sizeof(double) * (size_t)frames * (2 + 2 * (size_t)NE_BPF);
}

extern "C" int vdn_sobel_ix_iy(const float* depth, float* ix, float* iy, int frames, int H, int W, int normalize_kernel,
                               vdn_stream stream) {
  if (!depth || !ix || !iy) return VDN_EINVAL;
  if (const int rc = check_frames(frames, H, W)) return rc;
  if (misaligned(4, depth, ix, iy)) return VDN_EALIGN;
  hipLaunchKernelGGL(normal_vector_kernel<0>, dim3(grid_for((size_t)frames * H * W, 16384)), dim3(256), 0, (hipStream_t)stream,
                     depth, ix, iy, frames, H, W, normalize_kernel ? 0.125 : 1.0, 1.0, 1.0, 0.0);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_normal_vector(const float* depth, float* out, int frames, int H, int W, int normalize_kernel, float scale_xy,
                                 float scale_z, float eps, vdn_stream stream) {
  if (!depth || !out) return VDN_EINVAL;
  if (const int rc = check_frames(frames, H, W)) return rc;
  if (misaligned(4, depth, out)) return VDN_EALIGN;
  hipLaunchKernelGGL(normal_vector_kernel<1>, dim3(grid_for((size_t)frames * H * W, 16384)), dim3(256), 0, (hipStream_t)stream,
                     depth, out, (float*)nullptr, frames, H, W, normalize_kernel ? 0.125 : 1.0, (double)scale_xy, (double)scale_z,
                     (double)eps);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_erode_mask3(const uint8_t* mask, uint8_t* out, int frames, int H, int W, vdn_stream stream) {
  if (!mask || !out) return VDN_EINVAL;
  if (const int rc = check_frames(frames, H, W)) return rc;
  hipLaunchKernelGGL(erode_mask3_kernel, dim3(grid_for((size_t)frames * H * W, 16384)), dim3(256), 0, (hipStream_t)stream, mask,
                     out, frames, H, W);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_normal_eval(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int frames, int H,
                               int W, void* workspace, double* frame_sums, int64_t* frame_counts, double* out, vdn_stream stream) {
  if (!pred || !target || !workspace || !out) return VDN_EINVAL;
  if (const int rc = check_frames(frames, H, W)) return rc;
  if (frames > INT32_MAX / NE_BPF) return VDN_EINVAL;
  if (misaligned(4, pred, target) || misaligned(8, workspace, frame_sums, frame_counts, out)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)frames * NE_BPF), block(256);
  // a depth target is read through its stencil, never by quads
  with_ppl(wide_ok((size_t)H * W, {pred, target_is_depth ? nullptr : target}), [&](auto ppl) {
    with_bool(target_is_depth != 0, [&](auto depth) {
      hipLaunchKernelGGL((normal_eval_partial_kernel<decltype(ppl)::value, decltype(depth)::value>), grid, block, 0, s, pred, target,
                         mask, frames, H, W, workspace);
    });
  });
  hipLaunchKernelGGL(normal_eval_finalise_kernel, dim3(1), dim3(256), 0, s, workspace, frames, frame_sums, frame_counts, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
