// Clip evaluation on the device: the reference's eval_single_by_data (eval_depthcrafter/eval.py:55-151) and its seven
// metrics (eval_depthcrafter/metric.py), for a prediction that already sits in HBM.
//   vdn_eval_fit      one pass: masked sums of the least-squares scale/shift alignment, then a one-block solve
//   vdn_eval_metrics  one pass: align, clip and accumulate the per-frame sums of all seven metrics; a one-block finalise
//   vdn_resize_bilinear_hp  half-pixel bilinear resize of the prediction to the ground truth's size
// Everything the reference computes in float64 is fp64 here, with its roundings (separate multiply and add: contraction
// is off for this file); what it computes in float32 (the valid test, the TGM gradient of gt and its threshold, the three
// delta accuracies) is float32 here. Sums have the fixed order of frame_sums.hpp, with EVAL_BPF blocks per frame. No atomics:
// two runs give the same bits. Loads are one float per lane (coalesced), so any 4-byte-aligned pointer is accepted.
// The two kernels of vdn_eval_metrics keep their interleaved row (MET_SLOTS) and spell that header's block row and block fold
// out; keep them equal to block_row and fold_blocks (profiles/criteria_refactor.md says why they are not calls).
#include "common.hpp"
#include "frame_sums.hpp"
#include "resample.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int EVAL_BPF = 32;   // blocks per frame, fixed so that the workspace depends on the frame count alone
constexpr int FIT_SLOTS = 7;   // sum p*p, sum p, sum p*t, sum t, count (i64), min p, max p
constexpr int MET_SLOTS = 9;   // n (i64), sum |d|, sum |d|/g, sum d*d, 3 delta counts (i64), TGM sum, TGM count (i64)
constexpr int FRAME_SLOTS = 2 + MET_SLOTS;  // valid count, next kept frame, the frame's reduced metric sums

// workspace, in 8-byte slots: [T] valid pixels per frame | [T] next kept frame or -1 | [T][MET_SLOTS] frame sums |
//                             [T][EVAL_BPF][FIT_SLOTS] | [T][EVAL_BPF][MET_SLOTS]
struct Ws {
  int64_t* nvalid;
  int64_t* next;
  double* frame;
  double* fit;
  double* met;
  __host__ __device__ Ws(void* p, int T) {
    nvalid = (int64_t*)p;
    next = nvalid + T;
    frame = (double*)(next + T);
    fit = frame + (size_t)T * MET_SLOTS;
    met = fit + (size_t)T * EVAL_BPF * FIT_SLOTS;
  }
};

struct Range {
  double lo, hi;
  float lo32, hi32;  // numpy compares the float32 gt with the bounds in float32
};

__device__ __forceinline__ bool is_valid(float g, const uint8_t* mask, size_t i, const Range& r) {
  return g > r.lo32 && g < r.hi32 && (!mask || mask[i] != 0);
}
__device__ __forceinline__ double clip_low(double v, double lo) { return v < lo ? lo : v; }  // np.maximum: NaN stays NaN
__device__ __forceinline__ double max_nan(double x, double y) { return (x > y || x != x) ? x : y; }  // torch.max: NaN wins

// what the fit reduces in fp64: sum p*p, sum p, sum p*t, sum t, min p, max p
struct FitSums {
  double s[4], pmin, pmax;
};
struct FitOp {
  __device__ __forceinline__ FitSums operator()(FitSums a, const FitSums& b) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.s[k] = a.s[k] + b.s[k];
    a.pmin = fmin(a.pmin, b.pmin);
    a.pmax = fmax(a.pmax, b.pmax);
    return a;
  }
};

// the aligned, clipped prediction the metrics compare with gt (eval.py:110-128)
__device__ __forceinline__ double aligned(float pred, double scale, double shift, int depth_domain, const Range& r) {
  double a = clip_low(scale * clip_low((double)pred, r.lo) + shift, r.lo);
  if (depth_domain) a = a > 0.0 ? 1.0 / a : 0.0;  // depth2disparity: zero where not positive
  a = clip_low(a, r.lo);
  return a > r.hi ? r.hi : a;
}

// ---------------------------------------------------------------------------------------------------- masked fit
__global__ __launch_bounds__(256) void eval_fit_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               const uint8_t* __restrict__ mask, size_t hw, Range r,
                                                               int depth_domain, double* __restrict__ partial) {
  const size_t f = blockIdx.x / EVAL_BPF, b = blockIdx.x % EVAL_BPF, base = f * hw;
  FitSums a = {{0, 0, 0, 0}, INFINITY, -INFINITY};
  int cnt = 0;
  for (size_t i = sweep_first<1>((int)b); i < hw; i += sweep_stride<EVAL_BPF, 1>()) {
    const float g = gt[base + i];
    if (!is_valid(g, mask, base + i, r)) continue;
    const double p = clip_low((double)pred[base + i], r.lo);
    const double t = depth_domain ? 1.0 / ((double)g + 1e-8) : (double)g;
    a.s[0] += p * p;
    a.s[1] += p;
    a.s[2] += p * t;
    a.s[3] += t;
    cnt += 1;
    a.pmin = fmin(a.pmin, p);
    a.pmax = fmax(a.pmax, p);
  }
  __shared__ WaveSlots<FitSums> rd;
  __shared__ WaveSlots<int> rc;
  rd.put(a, FitOp{});
  rc.put(cnt, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    a = rd.get(FitOp{});
    double* o = partial + (size_t)blockIdx.x * FIT_SLOTS;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = a.s[k];
    ((int64_t*)o)[4] = rc.get(SumOp{});
    o[5] = a.pmin;
    o[6] = a.pmax;
  }
}

// One block: the valid count of every frame, the chain of kept frames, the clip's sums and the 2 x 2 solve.
__global__ __launch_bounds__(256) void eval_fit_solve_kernel(void* __restrict__ workspace, int T, double* __restrict__ coef) {
  const Ws ws(workspace, T);
  for (int f = threadIdx.x; f < T; f += 256) {
    int64_t n = 0;
    for (const size_t o : frame_blocks<EVAL_BPF>(f)) n += ((const int64_t*)(ws.fit + o * FIT_SLOTS))[4];
    ws.nvalid[f] = n;
  }
  FitSums a = {{0, 0, 0, 0}, INFINITY, -INFINITY};
  for (size_t j = threadIdx.x; j < (size_t)T * EVAL_BPF; j += 256) {
    const double* q = ws.fit + j * FIT_SLOTS;
    for (int k = 0; k < 4; ++k) a.s[k] += q[k];
    a.pmin = fmin(a.pmin, q[5]);
    a.pmax = fmax(a.pmax, q[6]);
  }
  __shared__ WaveSlots<FitSums> rd;
  rd.put(a, FitOp{});
  __syncthreads();  // nvalid[] and the slots are visible to lane 0 below
  if (threadIdx.x != 0) return;
  int64_t total = 0, next = -1;
  for (int f = T - 1; f >= 0; --f) {
    ws.next[f] = next;
    if (ws.nvalid[f] > 0) next = f;
    total += ws.nvalid[f];
  }
  a = rd.get(FitOp{});
  const double pmin = a.pmin, pmax = a.pmax;
  const double n = (double)total, spp = a.s[0], sp = a.s[1], spt = a.s[2], st = a.s[3];
  if (total == 0) {  // no valid pixel: nothing to align to, and every metric is NaN
    coef[0] = coef[1] = NAN;
  } else if (pmin == pmax) {  // all p equal: A = [c 1] has rank 1, lstsq returns the minimum-norm solution
    const double c = pmin, k = (st / n) / (c * c + 1.0);
    coef[0] = c * k;
    coef[1] = k;
  } else {
    const double det = spp * n - sp * sp;
    coef[0] = (n * spt - sp * st) / det;
    coef[1] = (spp * st - sp * spt) / det;
  }
}

// ---------------------------------------------------------------------------------------------------- fused metrics
// tgm_stride: the distance of the TGM gradient in elements, W (the next row of the same frame: what the reference
// computes on [T, H, W]) or 0 for "the same pixel of the next kept frame" (metric.py as written for [B, S, H, W]).
__global__ __launch_bounds__(256) void eval_metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                   const uint8_t* __restrict__ mask, int T, size_t hw,
                                                                   size_t row_stride, Range r, int depth_domain,
                                                                   const double* __restrict__ coef, void* __restrict__ workspace) {
  const Ws ws(workspace, T);
  const size_t f = blockIdx.x / EVAL_BPF, b = blockIdx.x % EVAL_BPF, base = f * hw;
  if (ws.nvalid[f] == 0) return;  // a dropped frame: the finalise pass never reads its partials
  const double scale = coef[0], shift = coef[1];
  const int64_t nf = ws.next[f];
  // neighbour of pixel i for the gradient: base + i + row_stride inside the frame, or pixel i of frame nf
  const bool over_time = row_stride == 0;
  const size_t nb_off = over_time ? (nf >= 0 ? (size_t)nf * hw - base : 0) : row_stride;
  const size_t nb_end = over_time ? (nf >= 0 ? hw : 0) : (hw > row_stride ? hw - row_stride : 0);
  Tuple<double, 4> s = {{0, 0, 0, 0}};  // |d|, |d|/g, d*d, TGM
  Tuple<int, 5> c = {{0, 0, 0, 0, 0}};  // n, delta1..3, TGM count
  for (size_t i = sweep_first<1>((int)b); i < hw; i += sweep_stride<EVAL_BPF, 1>()) {
    const float g32 = gt[base + i];
    if (!is_valid(g32, mask, base + i, r)) continue;  // the TGM mask also needs the first pixel of the pair valid
    const double g = (double)g32;
    const double a = aligned(pred[base + i], scale, shift, depth_domain, r);
    const double d = a - g, ad = fabs(d);
    s.v[0] += ad;
    s.v[1] += ad / g;
    s.v[2] += d * d;
    const double q = max_nan(a / g, g / a);
    c.v[0] += 1;
    c.v[1] += q < 1.25;
    c.v[2] += q < 1.5625;
    c.v[3] += q < 1.953125;
    if (i < nb_end) {
      const float dg = gt[base + i + nb_off] - g32;  // float32, as the reference's gt tensor
      if (dg < 0.05f) {
        const double da = aligned(pred[base + i + nb_off], scale, shift, depth_domain, r) - a;
        s.v[3] += fabs(da - (double)dg);
        c.v[4] += 1;
      }
    }
  }
  __shared__ WaveSlots<Tuple<double, 4>> rd;
  __shared__ WaveSlots<Tuple<int, 5>> rc;
  rd.put(s, SumOp{});
  rc.put(c, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    s = rd.get(SumOp{});
    c = rc.get(SumOp{});
    double* o = ws.met + (size_t)blockIdx.x * MET_SLOTS;
    int64_t* oi = (int64_t*)o;
    oi[0] = c.v[0];
    o[1] = s.v[0];
    o[2] = s.v[1];
    o[3] = s.v[2];
    oi[4] = c.v[1];
    oi[5] = c.v[2];
    oi[6] = c.v[3];
    o[7] = s.v[3];
    oi[8] = c.v[4];
  }
}

// out[7] in eval_metrics order: abs_relative_difference, delta1_acc, temporal_gradient_matching_error, abs_difference,
// rmse_linear, delta2_acc, delta3_acc. Frames without a valid pixel are dropped; 0/0 stays NaN.
__global__ __launch_bounds__(256) void eval_finalise_kernel(void* __restrict__ workspace, int T, int over_time,
                                                            double* __restrict__ out) {
  const Ws ws(workspace, T);
  for (int f = threadIdx.x; f < T; f += 256) {
    if (ws.nvalid[f] == 0) continue;
    double sd[MET_SLOTS] = {0};
    int64_t si[MET_SLOTS] = {0};
    for (int b = 0; b < EVAL_BPF; ++b) {
      const double* q = ws.met + ((size_t)f * EVAL_BPF + b) * MET_SLOTS;
      const int64_t* qi = (const int64_t*)q;
      sd[1] += q[1], sd[2] += q[2], sd[3] += q[3], sd[7] += q[7];
      si[0] += qi[0], si[4] += qi[4], si[5] += qi[5], si[6] += qi[6], si[8] += qi[8];
    }
    double* o = ws.frame + (size_t)f * MET_SLOTS;
    int64_t* oi = (int64_t*)o;
    o[1] = sd[1], o[2] = sd[2], o[3] = sd[3], o[7] = sd[7];
    oi[0] = si[0], oi[4] = si[4], oi[5] = si[5], oi[6] = si[6], oi[8] = si[8];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double absdiff = 0, absrel = 0, rmse = 0, tgm = 0;
  float delta[3] = {0.f, 0.f, 0.f};  // the reference's delta accuracies are float32: quotient and mean
  int64_t kept = 0, pairs = 0;
  for (int f = 0; f < T; ++f) {
    if (ws.nvalid[f] == 0) continue;
    const double* q = ws.frame + (size_t)f * MET_SLOTS;
    const int64_t* qi = (const int64_t*)q;
    const double n = (double)qi[0];
    ++kept;
    absdiff += q[1] / n;
    absrel += q[2] / n;
    rmse += sqrt(q[3] / n);
    for (int k = 0; k < 3; ++k) delta[k] += (float)qi[4 + k] / (float)qi[0];
    if (!over_time || ws.next[f] >= 0) {
      ++pairs;
      tgm += q[7] / (double)qi[8];
    }
  }
  const double k = (double)kept;
  out[0] = absrel / k;
  out[1] = (double)(delta[0] / (float)kept);
  out[2] = tgm / (double)pairs;
  out[3] = absdiff / k;
  out[4] = rmse / k;
  out[5] = (double)(delta[1] / (float)kept);
  out[6] = (double)(delta[2] / (float)kept);
}

// ---------------------------------------------------------------------------------------------------- resize
// Half-pixel bilinear with hp_source's coordinates (resample.hpp); no antialiasing when shrinking (cv2.INTER_LINEAR has none
// either). The blend below is separately rounded products under this file's contract(off), not resample.hpp's bilerp.
__global__ __launch_bounds__(256) void resize_bilinear_hp_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total,
                                                                 int IH, int IW, int OH, int OW) {
  const float sh = (float)IH / (float)OH, sw = (float)IW / (float)OW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const size_t f = i / ((size_t)OW * OH);
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    hp_source(oy, sh, IH, y0, y1, hy0, hy1);
    hp_source(ox, sw, IW, x0, x1, wx0, wx1);
    const float* p = x + f * (size_t)IH * IW;
    const float top = wx0 * p[(size_t)y0 * IW + x0] + wx1 * p[(size_t)y0 * IW + x1];
    const float bot = wx0 * p[(size_t)y1 * IW + x0] + wx1 * p[(size_t)y1 * IW + x1];
    y[i] = hy0 * top + hy1 * bot;
  }
}

inline bool make_range(double dmin, double dmax, Range& r) {
  if (!(dmin < dmax)) return false;
  r = Range{dmin, dmax, (float)dmin, (float)dmax};
  return true;
}

}  // namespace

extern "C" size_t vdn_eval_workspace_bytes(int frames) {
  if (frames <= 0) return 0;
  return sizeof(double) * (size_t)frames * (FRAME_SLOTS + (size_t)EVAL_BPF * (FIT_SLOTS + MET_SLOTS));
}

extern "C" int vdn_eval_fit(const float* pred, const float* gt, const uint8_t* mask, int frames, size_t hw, double dmin,
                            double dmax, int domain, void* workspace, double* coef, vdn_stream stream) {
  Range r;
  if (!pred || !gt || !workspace || !coef || frames <= 0 || hw == 0 || !make_range(dmin, dmax, r)) return VDN_EINVAL;
  if (domain != VDN_EVAL_DEPTH && domain != VDN_EVAL_DISP) return VDN_EINVAL;
  if (frames > INT32_MAX / EVAL_BPF) return VDN_EINVAL;
  if (misaligned(4, pred, gt) || misaligned(8, workspace, coef)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const Ws ws(workspace, frames);
  hipLaunchKernelGGL(eval_fit_partial_kernel, dim3((unsigned)frames * EVAL_BPF), dim3(256), 0, s, pred, gt, mask, hw, r,
                     domain == VDN_EVAL_DEPTH, ws.fit);
  hipLaunchKernelGGL(eval_fit_solve_kernel, dim3(1), dim3(256), 0, s, workspace, frames, coef);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_eval_metrics(const float* pred, const float* gt, const uint8_t* mask, int frames, int H, int W, double dmin,
                                double dmax, int domain, int tgm, const double* coef, void* workspace, double* out,
                                vdn_stream stream) {
  Range r;
  if (!pred || !gt || !workspace || !coef || !out || frames <= 0 || H <= 0 || W <= 0 || !make_range(dmin, dmax, r))
    return VDN_EINVAL;
  if (domain != VDN_EVAL_DEPTH && domain != VDN_EVAL_DISP) return VDN_EINVAL;
  if (tgm != VDN_EVAL_TGM_ROWS && tgm != VDN_EVAL_TGM_FRAMES) return VDN_EINVAL;
  if (frames > INT32_MAX / EVAL_BPF) return VDN_EINVAL;
  if (misaligned(4, pred, gt) || misaligned(8, workspace, coef, out)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const size_t hw = (size_t)H * W;
  hipLaunchKernelGGL(eval_metrics_partial_kernel, dim3((unsigned)frames * EVAL_BPF), dim3(256), 0, s, pred, gt, mask, frames, hw,
                     tgm == VDN_EVAL_TGM_ROWS ? (size_t)W : (size_t)0, r, domain == VDN_EVAL_DEPTH, coef, workspace);
  hipLaunchKernelGGL(eval_finalise_kernel, dim3(1), dim3(256), 0, s, workspace, frames, tgm == VDN_EVAL_TGM_FRAMES, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_resize_bilinear_hp(const float* x, float* y, int frames, int IH, int IW, int OH, int OW, vdn_stream stream) {
  if (!x || !y || frames <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return VDN_EINVAL;
  if (misaligned(4, x, y)) return VDN_EALIGN;
  const size_t total = (size_t)frames * OH * OW;
  hipLaunchKernelGGL(resize_bilinear_hp_kernel, dim3(grid_for(total, 16384)), dim3(256), 0, (hipStream_t)stream, x, y, total,
                     IH, IW, OH, OW);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
