// Normal evaluation on the device: the reference's normal_vector / sobel_ix_iy (utils/normal_utils.py:4-52) and its
// VideoNormalLoss (loss/loss.py:370-409), for tensors that already sit in HBM.
//   vdn_sobel_ix_iy, vdn_normal_vector  the Sobel stencil on the reflect-padded depth and the unit normals made from it
//   vdn_erode_mask3                     the 3 x 3 erosion of the loss's mask
//   vdn_normal_eval                     one pass: erode, (make the target normal from depth,) cosine, per-block partial
//                                       sums; then a one-block finalise
// The stencil, the normalisation and the cosine are fp64 computed from the f32 samples, with separate multiply and add
// roundings (contraction is off for this file). Sums have a fixed order: a lane's stride through its block's share, the
// wave and the block as reduce.hpp states them, a frame's NE_BPF blocks in index order, the frames in index order. No
// atomics: two runs give the same bits. Any 4-byte-aligned pointer is accepted; vdn_normal_eval reads pred (and a stored
// target) four floats per lane where the planes are 16-byte aligned, one per lane otherwise. Stencil and erosion neighbours
// that belong to other lanes or blocks are read through the cache, as refine_pack_kernel does; the four pixels of a lane share theirs.
#include "common.hpp"
#include "reduce.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int NE_BPF = 64;  // blocks per frame, fixed so that the workspace depends on the frame count alone

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

// cross-correlation with kx = [[1,0,-1],[2,0,-2],[1,0,-1]], ky = [[1,2,1],[0,0,0],[-1,-2,-1]] (times 1/8 = k), in fp64.
// a[r][c] is the 3 x 3 window; its centre is not used.
__device__ __forceinline__ void sobel(const float (&a)[3][3], double k, double& ix, double& iy) {
  const double a00 = a[0][0], a01 = a[0][1], a02 = a[0][2], a10 = a[1][0], a12 = a[1][2], a20 = a[2][0], a21 = a[2][1],
               a22 = a[2][2];
  ix = ((a00 - a02) + 2.0 * (a10 - a12) + (a20 - a22)) * k;
  iy = ((a00 - a20) + 2.0 * (a01 - a21) + (a02 - a22)) * k;
}

// n = (-sxy Ix, -sxy Iy, sz) / sqrt(nx^2 + ny^2 + nz^2 + eps)
__device__ __forceinline__ void unit_normal(double ix, double iy, double sxy, double sz, double eps, double (&n)[3]) {
  const double nx = -sxy * ix, ny = -sxy * iy;
  const double norm = sqrt(((nx * nx + ny * ny) + sz * sz) + eps);
  n[0] = nx / norm;
  n[1] = ny / norm;
  n[2] = sz / norm;
}

__device__ __forceinline__ void window_at(const float* __restrict__ df, int y, int x, int H, int W, float (&a)[3][3]) {
  const int ys[3] = {refl_lo(y), y, refl_hi(y, H)}, xs[3] = {refl_lo(x), x, refl_hi(x, W)};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) a[r][c] = (r == 1 && c == 1) ? 0.f : df[(size_t)ys[r] * W + xs[c]];
}

// erosion at (y, x): the pixel and its neighbours inside the image are all non-zero
__device__ __forceinline__ bool kept_at(const uint8_t* __restrict__ mf, int y, int x, int H, int W) {
  bool k = true;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) k = k && mf[(size_t)yy * W + xx] != 0;
    }
  return k;
}

// F.cosine_similarity(a, b, dim, eps = 1e-8) of torch 2.x: sum_c (a_c / max(|a|, eps)) * (b_c / max(|b|, eps)), evaluated as
// (a . b) / (max(|a|, eps) * max(|b|, eps)): the same number in exact arithmetic with one fp64 division in place of six
// (the kernel is bound by its fp64 divisions and square roots, not by memory: profiles/normal_eval.md). Neither form can
// overflow from float32 inputs, and inf or NaN components give NaN in both. The comparison (not fmax) keeps a NaN norm.
__device__ __forceinline__ double cosine3(const double (&a)[3], const double (&b)[3]) {
  double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  double nb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  na = na < 1e-8 ? 1e-8 : na;
  nb = nb < 1e-8 ? 1e-8 : nb;
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
  const double eps = (double)1e-8f;  // normal_vector's default, as vdn_normal_vector receives it
  double sum = 0.0;
  int cnt = 0;
  for (int64_t q0 = (int64_t)(b * 256 + (int)threadIdx.x) * PPL; q0 < hw; q0 += (int64_t)NE_BPF * 256 * PPL) {
    const int p0 = (int)q0;
    float pv[3][PPL], tv[3][PPL];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (PPL == 4) {
        const f32x4 v = *(const f32x4*)(pf + (size_t)c * hw + p0);
#pragma unroll
        for (int j = 0; j < PPL; ++j) pv[c][j] = v[j];
        if (!DEPTH) {
          const f32x4 w = *(const f32x4*)(tf + (size_t)c * hw + p0);
#pragma unroll
          for (int j = 0; j < PPL; ++j) tv[c][j] = w[j];
        }
      } else {
        pv[c][0] = pf[(size_t)c * hw + p0];
        if (!DEPTH) tv[c][0] = tf[(size_t)c * hw + p0];
      }
    }
    int y = p0 / W, x = p0 - y * W;
    // A quad that lies in one row with a column to spare on either side shares its neighbours: per row six columns serve
    // the four erosion tests and the four stencils (18 + 18 loads in place of 36 + 32). Other quads go pixel by pixel.
    const bool fast = PPL == 4 && x >= 1 && x + PPL < W;
    bool keepq[PPL];
    float dq[3][PPL + 2];
    if (fast) {
#pragma unroll
      for (int j = 0; j < PPL; ++j) keepq[j] = true;
      if (mf) {
        bool v[PPL + 2];  // the column's pixels in rows y - 1 .. y + 1 inside the image are all non-zero
#pragma unroll
        for (int c = 0; c < PPL + 2; ++c) {
          const size_t o = (size_t)y * W + (x - 1 + c);
          bool k = mf[o] != 0;
          if (y > 0) k &= mf[o - W] != 0;
          if (y < H - 1) k &= mf[o + W] != 0;
          v[c] = k;
        }
#pragma unroll
        for (int j = 0; j < PPL; ++j) keepq[j] = v[j] & v[j + 1] & v[j + 2];
      }
      bool any = false;
#pragma unroll
      for (int j = 0; j < PPL; ++j) any |= keepq[j];
      if (DEPTH && any) {
        const int ys[3] = {refl_lo(y), y, refl_hi(y, H)};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < PPL + 2; ++c) dq[r][c] = tf[(size_t)ys[r] * W + (x - 1 + c)];
      }
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const bool keep = fast ? keepq[j] : (!mf || kept_at(mf, y, x, H, W));
      if (keep) {  // a dropped pixel is skipped: nothing under it is read into the sums
        const double a[3] = {(double)pv[0][j], (double)pv[1][j], (double)pv[2][j]};
        double t[3];
        if (DEPTH) {
          float win[3][3];
          if (fast) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int c = 0; c < 3; ++c) win[r][c] = dq[r][j + c];
          } else {
            window_at(tf, y, x, H, W, win);
          }
          double ix, iy;
          sobel(win, 0.125, ix, iy);
          unit_normal(ix, iy, 1.0, 1.0, eps, t);
        } else {
          t[0] = (double)tv[0][j], t[1] = (double)tv[1][j], t[2] = (double)tv[2][j];
        }
        sum += cosine3(a, t);
        cnt += 1;
      }
      if (++x == W) x = 0, ++y;
    }
  }
  __shared__ WaveSlots<double> rs;
  __shared__ WaveSlots<int> rc;
  rs.put(sum, SumOp{});
  rc.put(cnt, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    ws.bsum[blockIdx.x] = rs.get(SumOp{});
    ws.bcnt[blockIdx.x] = (int64_t)rc.get(SumOp{});
  }
}

// One block: every frame's blocks in index order, then the frames in index order.
__global__ __launch_bounds__(256) void normal_eval_finalise_kernel(void* __restrict__ workspace, int T, double* __restrict__ frame_sums,
                                                                   int64_t* __restrict__ frame_counts, double* __restrict__ out) {
  const Ws ws(workspace, T);
  for (int f = threadIdx.x; f < T; f += 256) {
    double s = 0.0;
    int64_t n = 0;
    for (int b = 0; b < NE_BPF; ++b) {
      s += ws.bsum[(size_t)f * NE_BPF + b];
      n += ws.bcnt[(size_t)f * NE_BPF + b];
    }
    ws.fsum[f] = s;
    ws.fcnt[f] = n;
    if (frame_sums) frame_sums[f] = s;
    if (frame_counts) frame_counts[f] = n;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  int64_t n = 0;
  for (int f = 0; f < T; ++f) {
    s += ws.fsum[f];
    n += ws.fcnt[f];
  }
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
  if (((uintptr_t)depth & 3) || ((uintptr_t)ix & 3) || ((uintptr_t)iy & 3)) return VDN_EALIGN;
  hipLaunchKernelGGL(normal_vector_kernel<0>, dim3(grid_for((size_t)frames * H * W, 16384)), dim3(256), 0, (hipStream_t)stream,
                     depth, ix, iy, frames, H, W, normalize_kernel ? 0.125 : 1.0, 1.0, 1.0, 0.0);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_normal_vector(const float* depth, float* out, int frames, int H, int W, int normalize_kernel, float scale_xy,
                                 float scale_z, float eps, vdn_stream stream) {
  if (!depth || !out) return VDN_EINVAL;
  if (const int rc = check_frames(frames, H, W)) return rc;
  if (((uintptr_t)depth & 3) || ((uintptr_t)out & 3)) return VDN_EALIGN;
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
  if (((uintptr_t)pred & 3) || ((uintptr_t)target & 3)) return VDN_EALIGN;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)frame_sums & 7) || ((uintptr_t)frame_counts & 7) || ((uintptr_t)out & 7))
    return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)frames * NE_BPF), block(256);
  // four floats per lane when every plane of every frame starts on 16 bytes and holds whole quads
  const bool wide = ((size_t)H * W) % 4 == 0 && !((uintptr_t)pred & 15) && (target_is_depth || !((uintptr_t)target & 15));
  if (target_is_depth) {
    if (wide) hipLaunchKernelGGL((normal_eval_partial_kernel<4, true>), grid, block, 0, s, pred, target, mask, frames, H, W, workspace);
    else hipLaunchKernelGGL((normal_eval_partial_kernel<1, true>), grid, block, 0, s, pred, target, mask, frames, H, W, workspace);
  } else {
    if (wide) hipLaunchKernelGGL((normal_eval_partial_kernel<4, false>), grid, block, 0, s, pred, target, mask, frames, H, W, workspace);
    else hipLaunchKernelGGL((normal_eval_partial_kernel<1, false>), grid, block, 0, s, pred, target, mask, frames, H, W, workspace);
  }
  hipLaunchKernelGGL(normal_eval_finalise_kernel, dim3(1), dim3(256), 0, s, workspace, frames, frame_sums, frame_counts, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
