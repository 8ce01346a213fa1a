// The metric-depth branch's criterion and scores on the device: metric_depth/util/loss.py (SiLogLoss, with its gradient with
// respect to the prediction), metric_depth/util/metric.py (eval_depth's nine metrics) and what the validation loop of
// metric_depth/train.py:160-177 does around them (the align-corners resize of the prediction to the ground truth's size and
// the mask (valid_mask == 1) & (depth >= min_depth) & (depth <= max_depth)). include/vdn.h (vdn_metric_eval, vdn_silog_loss,
// vdn_silog_loss_backward) states the arithmetic.
//   eval      pass 1 leaves the fp64 sums and the counts of each block's share of an item in the workspace, MT_BPI partials
//             per item; pass 2 is one block per item that takes the item's MT_BPI partials one per lane through the block
//             reduction of reduce.hpp and writes the item's row. With a prediction of another size a lane samples it at its
//             pixel (four loads that hit the cache: the prediction is a fraction of the ground truth) and the resized map is
//             never written. 9 bytes per pixel cross the memory bus (4 + 4 + 1), at most.
//   loss      the same two passes over one flat run of `count` floats: count, sum dl, sum dl^2.
//   backward  one elementwise pass: 9 bytes read and 4 written per pixel.
// What decides something in float32 in the reference (the mask's comparisons, the resampled prediction, thresh and the three
// quotients d_k) is the same float32 operation here, one rounding each; everything else is fp64 from the float32 inputs on.
// Contraction is off: a product and the sum it feeds are rounded separately. Sums have a fixed order (a lane's stride through
// its block's share and the block's row as frame_sums.hpp states them, the MT_BPI partials one per lane through the same block
// reduction): no atomics, two runs give the same bits.
// A lane owns four consecutive elements (16-byte loads, one 4-byte load of the mask) where the item's length is a multiple of
// 4 and the bases allow it, one element otherwise; the values do not depend on which. It issues the loads of MT_INFLIGHT
// trips of the grid before it uses the first (sweep below): an item has only MT_BPI blocks, and the validation loop has one
// item per launch.
#include "common.hpp"
#include "frame_sums.hpp"
#include "resample.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int MT_BPI = 256;      // blocks per item: pass 2 reduces an item's partials one per lane
constexpr int MT_INFLIGHT = 4;   // trips of the grid whose loads a lane issues before it uses the first
constexpr int EV_D = 6;          // fp64 sums of eval: |d|/t, d^2/t, d^2, dl^2, |log10 p - log10 t|, dl
constexpr int EV_C = 4;          // counts of eval: kept, thresh < 1.25, < 1.25^2, < 1.25^3
constexpr int EV_SLOTS = EV_D + EV_C / 2;  // 8-byte slots per partial: the doubles, then the four ints
constexpr int SL_SLOTS = 3;      // 8-byte slots per partial of the loss: sum dl, sum dl^2, kept (int64)

// (mask == 1) & (t >= lo) & (t <= hi), the bounds compared in float32; `on` == 0: the mask alone. A NaN t fails the bounds.
struct Keep {
  float lo, hi;
  int on;
  __device__ __forceinline__ bool operator()(uint32_t m, float t) const { return m == 1u && (!on || (t >= lo && t <= hi)); }
};

// what a lane loaded at one visit
template <int PPL>
struct Elems {
  float p[PPL], t[PPL];
  uint32_t m;  // PPL mask bytes, the first in the low byte
};

// A lane's share of an item of n elements: the PPL elements at (b * 256 + lane) * PPL + k * trip, k = 0, 1, ..., trip =
// MT_BPI * 256 * PPL. body(i, px) gets the element index and what was loaded there: the target, the mask bytes (all 1 without
// a mask) and, with LOAD_P, the prediction. This is the sweep of frame_sums.hpp with MT_INFLIGHT visits taken at a time, so that
// the loads of all of them stand before the first use.
// load_px of frame_sums.hpp for a plane and an index, spelled out: keep it equal to load_px. Through load_px the two resampling
// kernels compile to other, longer code (profiles/criteria_refactor.md).
template <int PPL>
__device__ __forceinline__ void load_f(const float* p, int i, float (&v)[PPL]) {
  if (PPL == 4) {
    const f32x4 q = *(const f32x4*)(p + i);
#pragma unroll
    for (int j = 0; j < PPL; ++j) v[j] = q[j];
  } else {
    v[0] = p[i];
  }
}

template <int PPL, bool LOAD_P, typename Body>
__device__ __forceinline__ void sweep(const float* pf, const float* tf, const uint8_t* mf, int b, int n, Body body) {
  const int64_t trip = sweep_stride<MT_BPI, PPL>();
  for (int64_t q0 = sweep_first<PPL>(b); q0 < n; q0 += trip * MT_INFLIGHT) {
    Elems<PPL> v[MT_INFLIGHT];
#pragma unroll
    for (int u = 0; u < MT_INFLIGHT; ++u)
      if (q0 + u * trip < n) {
        const int i = (int)(q0 + u * trip);
        load_f<PPL>(tf, i, v[u].t);
        if (LOAD_P) load_f<PPL>(pf, i, v[u].p);
        v[u].m = 0x01010101u;
        if (mf) v[u].m = load_mask<PPL>(mf + i);
      }
#pragma unroll
    for (int u = 0; u < MT_INFLIGHT; ++u)
      if (q0 + u * trip < n) body((int)(q0 + u * trip), v[u]);
  }
}

__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }  // torch.max: a NaN wins

// The prediction at pixel (y, x) of the ground truth's grid: align-corners bilinear, every product and sum rounded on its own.
struct Sampler {
  const float* p;
  int ph, pw;
  float sy, sx;
  __device__ __forceinline__ float operator()(int y, int x) const {
    const AcCoord cy = ac_coord<AcWeight::rounded>(y, sy, ph), cx = ac_coord<AcWeight::rounded>(x, sx, pw);
    const float* r0 = p + (size_t)cy.i0 * pw;
    const float* r1 = p + (size_t)cy.i1 * pw;
    const float a00 = r0[cx.i0], a01 = r0[cx.i1], a10 = r1[cx.i0], a11 = r1[cx.i1];
    const float wx0 = 1.f - cx.l1, wy0 = 1.f - cy.l1;
    const float top = wx0 * a00 + cx.l1 * a01;
    const float bot = wx0 * a10 + cx.l1 * a11;
    return wy0 * top + cy.l1 * bot;
  }
};

// ---------------------------------------------------------------------------------------------------- the nine metrics
template <int PPL, bool RESAMPLE>
__global__ __launch_bounds__(256) void metric_partial_kernel(const float* __restrict__ pred, const float* __restrict__ depth,
                                                             const uint8_t* __restrict__ valid, int ph, int pw, int H, int W,
                                                             Keep keep, double* __restrict__ partial) {
  const int it = blockIdx.x / MT_BPI, b = blockIdx.x % MT_BPI;
  const int n = H * W;
  const float* pf = pred + (size_t)it * ph * pw;
  const float* tf = depth + (size_t)it * n;
  const uint8_t* mf = valid ? valid + (size_t)it * n : nullptr;
  const Sampler sample{pf, ph, pw, ac_scale(ph, H), ac_scale(pw, W)};
  Tuple<double, EV_D> s = {{0, 0, 0, 0, 0, 0}};
  Tuple<int, EV_C> c = {{0, 0, 0, 0}};
  sweep<PPL, !RESAMPLE>(pf, tf, mf, b, n, [&](int i, Elems<PPL>& v) {
    int y = 0, x = 0;
    if (RESAMPLE) y = i / W, x = i - y * W;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (keep(mask_byte(v.m, j), v.t[j])) {  // a dropped pixel is skipped: nothing under it reaches a sum
        const float t32 = v.t[j], p32 = RESAMPLE ? sample(y, x) : v.p[j];
        const float q = max_nan(__fdiv_rn(t32, p32), __fdiv_rn(p32, t32));
        c.v[0] += 1;
        c.v[1] += q < 1.25f;
        c.v[2] += q < 1.5625f;
        c.v[3] += q < 1.953125f;
        const double p = (double)p32, t = (double)t32;
        const double d = p - t, d2 = d * d, dl = log(p) - log(t);
        s.v[0] += fabs(d) / t;
        s.v[1] += d2 / t;
        s.v[2] += d2;
        s.v[3] += dl * dl;
        s.v[4] += fabs(log10(p) - log10(t));
        s.v[5] += dl;
      }
      if (RESAMPLE && ++x == W) x = 0, ++y;  // the next element of the lane begins the next row
    }
  });
  // The block's row, spelled out: a partial keeps its counts behind its own sums, in EV_SLOTS slots, and the finish kernel
  // reads it whole. Keep it equal to block_row of frame_sums.hpp (profiles/criteria_refactor.md).
  __shared__ WaveSlots<Tuple<double, EV_D>> rd;
  __shared__ WaveSlots<Tuple<int, EV_C>> rc;
  rd.put(s, SumOp{});
  rc.put(c, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    s = rd.get(SumOp{});
    c = rc.get(SumOp{});
    double* o = partial + (size_t)blockIdx.x * EV_SLOTS;
#pragma unroll
    for (int k = 0; k < EV_D; ++k) o[k] = s.v[k];
    int* oc = (int*)(o + EV_D);
#pragma unroll
    for (int k = 0; k < EV_C; ++k) oc[k] = c.v[k];
  }
}

// One block per item. out[it][10] = n | d1 d2 d3 abs_rel sq_rel rmse rmse_log log10 silog. n == 0: 0 / 0, nine NaN.
__global__ __launch_bounds__(256) void metric_finish_kernel(const double* __restrict__ partial, double* __restrict__ out) {
  const double* q = partial + ((size_t)blockIdx.x * MT_BPI + threadIdx.x) * EV_SLOTS;  // MT_BPI = 256 partials, one per lane
  const int* qc = (const int*)(q + EV_D);
  Tuple<double, EV_D> s;
  Tuple<int, EV_C> c;
#pragma unroll
  for (int k = 0; k < EV_D; ++k) s.v[k] = q[k];
#pragma unroll
  for (int k = 0; k < EV_C; ++k) c.v[k] = qc[k];
  __shared__ WaveSlots<Tuple<double, EV_D>> rd;
  __shared__ WaveSlots<Tuple<int, EV_C>> rc;
  rd.put(s, SumOp{});
  rc.put(c, SumOp{});
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = rd.get(SumOp{});
  c = rc.get(SumOp{});
  double* o = out + (size_t)blockIdx.x * 10;
  const double n = (double)c.v[0];
  const float n32 = (float)c.v[0];
  o[0] = n;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[1 + k] = (double)__fdiv_rn((float)c.v[1 + k], n32);  // the reference's float32 quotient
  o[4] = s.v[0] / n;
  o[5] = s.v[1] / n;
  o[6] = sqrt(s.v[2] / n);
  const double m2 = s.v[3] / n, m1 = s.v[5] / n;
  o[7] = sqrt(m2);
  o[8] = s.v[4] / n;
  o[9] = sqrt(m2 - 0.5 * (m1 * m1));
}

// ---------------------------------------------------------------------------------------------------- SiLogLoss
template <int PPL>
__global__ __launch_bounds__(256) void silog_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                            const uint8_t* __restrict__ mask, int n, Keep keep,
                                                            double* __restrict__ partial) {
  Tuple<double, 2> s = {{0, 0}};
  int cnt = 0;
  sweep<PPL, true>(pred, target, mask, (int)blockIdx.x, n, [&](int, Elems<PPL>& v) {
#pragma unroll
    for (int j = 0; j < PPL; ++j)
      if (keep(mask_byte(v.m, j), v.t[j])) {
        const double dl = log((double)v.t[j]) - log((double)v.p[j]);
        s.v[0] += dl;
        s.v[1] += dl * dl;
        cnt += 1;
      }
  });
  // the block's row, spelled out as in metric_partial_kernel: the count behind the block's own sums
  __shared__ WaveSlots<Tuple<double, 2>> rd;
  __shared__ WaveSlots<int> rc;
  rd.put(s, SumOp{});
  rc.put(cnt, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    s = rd.get(SumOp{});
    double* o = partial + (size_t)blockIdx.x * SL_SLOTS;
    o[0] = s.v[0];
    o[1] = s.v[1];
    ((int64_t*)o)[2] = rc.get(SumOp{});
  }
}

// One block. out[4] = loss | n | sum dl | sum dl^2.
__global__ __launch_bounds__(256) void silog_finish_kernel(const double* __restrict__ partial, double lambd,
                                                           double* __restrict__ out) {
  const double* q = partial + (size_t)threadIdx.x * SL_SLOTS;
  __shared__ WaveSlots<Tuple<double, 2>> rd;
  __shared__ WaveSlots<int> rc;
  rd.put(Tuple<double, 2>{{q[0], q[1]}}, SumOp{});
  rc.put((int)((const int64_t*)q)[2], SumOp{});
  __syncthreads();
  if (threadIdx.x != 0) return;
  const Tuple<double, 2> s = rd.get(SumOp{});
  const double n = (double)rc.get(SumOp{});
  const double m1 = s.v[0] / n, m2 = s.v[1] / n;
  out[0] = sqrt(m2 - lambd * (m1 * m1));
  out[1] = n;
  out[2] = s.v[0];
  out[3] = s.v[1];
}

// grad = coeff * -(dl - lambd * mean) / (n * loss * pred) on kept pixels, in fp64 and rounded once; +0 on dropped ones.
template <int PPL>
__global__ __launch_bounds__(256) void silog_backward_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const uint8_t* __restrict__ mask, int n, Keep keep, double lambd,
                                                             const double* __restrict__ state, const float* __restrict__ coeff,
                                                             float* __restrict__ grad) {
  const double loss = state[0], cnt = state[1];
  const double shift = lambd * (state[2] / cnt), den = cnt * loss, co = (double)coeff[0];
  sweep<PPL, true>(pred, target, mask, (int)blockIdx.x, n, [&](int i, Elems<PPL>& v) {
    float g[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      g[j] = 0.f;
      if (keep(mask_byte(v.m, j), v.t[j])) {
        const double p = (double)v.p[j];
        const double dl = log((double)v.t[j]) - log(p);
        g[j] = (float)(co * (-(dl - shift) / (den * p)));
      }
    }
    store_px<PPL>(grad + i, g);
  });
}

inline bool make_keep(int bounded, double min_depth, double max_depth, Keep& k) {
  k = Keep{(float)min_depth, (float)max_depth, bounded != 0};
  return !bounded || (min_depth == min_depth && max_depth == max_depth);
}

}  // namespace

static_assert(MT_BPI == 256, "the finishing kernels read one partial per lane of a 256-lane block");
static_assert(EV_C % 2 == 0, "the counts of a partial fill whole 8-byte slots");

extern "C" int vdn_metric_trip(int wide) { return (int)(wide ? sweep_stride<MT_BPI, 4>() : sweep_stride<MT_BPI, 1>()); }

extern "C" size_t vdn_metric_workspace_bytes(int items) {
  if (items <= 0) return 0;
  return sizeof(double) * (size_t)items * MT_BPI * EV_SLOTS;
}

extern "C" size_t vdn_silog_loss_workspace_bytes(void) { return sizeof(double) * (size_t)MT_BPI * SL_SLOTS; }

extern "C" int vdn_metric_eval(const float* pred, const float* depth, const uint8_t* valid, int items, int ph, int pw, int H,
                               int W, int bounded, double min_depth, double max_depth, void* workspace, double* out,
                               vdn_stream stream) {
  Keep keep;
  if (!pred || !depth || !workspace || !out) return VDN_EINVAL;
  if (items <= 0 || ph <= 0 || pw <= 0 || H <= 0 || W <= 0 || !make_keep(bounded, min_depth, max_depth, keep)) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX || (int64_t)ph * pw > INT32_MAX || items > 65535) return VDN_EUNSUPPORTED;
  if (misaligned(4, pred, depth) || misaligned(8, workspace, out)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const bool resample = ph != H || pw != W;
  const int n = H * W;
  const dim3 grid((unsigned)items * MT_BPI), block(256);
  double* partial = (double*)workspace;
  // a prediction of another size is sampled, never read by quads
  with_ppl(wide_ok((size_t)n, {depth, resample ? nullptr : pred}, {valid}), [&](auto ppl) {
    with_bool(resample, [&](auto resampled) {
      hipLaunchKernelGGL((metric_partial_kernel<decltype(ppl)::value, decltype(resampled)::value>), grid, block, 0, s, pred, depth, valid,
                         ph, pw, H, W, keep, partial);
    });
  });
  hipLaunchKernelGGL(metric_finish_kernel, dim3((unsigned)items), block, 0, s, (const double*)partial, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_silog_loss(const float* pred, const float* target, const uint8_t* mask, int64_t count, double lambd,
                              int bounded, double min_depth, double max_depth, void* workspace, double* out,
                              vdn_stream stream) {
  Keep keep;
  if (!pred || !target || !workspace || !out) return VDN_EINVAL;
  if (count <= 0 || !make_keep(bounded, min_depth, max_depth, keep)) return VDN_EINVAL;
  if (count > INT32_MAX) return VDN_EUNSUPPORTED;
  if (misaligned(4, pred, target) || misaligned(8, workspace, out)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(MT_BPI), block(256);
  double* partial = (double*)workspace;
  with_ppl(wide_ok((size_t)count, {pred, target}, {mask}), [&](auto ppl) {
    hipLaunchKernelGGL(silog_partial_kernel<decltype(ppl)::value>, grid, block, 0, s, pred, target, mask, (int)count, keep, partial);
  });
  hipLaunchKernelGGL(silog_finish_kernel, dim3(1), block, 0, s, (const double*)partial, lambd, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_silog_loss_backward(const float* pred, const float* target, const uint8_t* mask, int64_t count, double lambd,
                                       int bounded, double min_depth, double max_depth, const double* state, const float* coeff,
                                       float* grad, vdn_stream stream) {
  Keep keep;
  if (!pred || !target || !state || !coeff || !grad) return VDN_EINVAL;
  if (count <= 0 || !make_keep(bounded, min_depth, max_depth, keep)) return VDN_EINVAL;
  if (count > INT32_MAX) return VDN_EUNSUPPORTED;
  if (misaligned(4, pred, target, grad, coeff) || misaligned(8, state)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(MT_BPI), block(256);
  with_ppl(wide_ok((size_t)count, {pred, target, grad}, {mask}), [&](auto ppl) {
    hipLaunchKernelGGL(silog_backward_kernel<decltype(ppl)::value>, grid, block, 0, s, pred, target, mask, (int)count, keep, lambd, state,
                       coeff, grad);
  });
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
