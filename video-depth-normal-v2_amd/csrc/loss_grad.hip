// The gradient of the depth criterion (loss.hip) with respect to its prediction, on the device: what autograd computes for
//   L = c_sp * spatial_loss + c_st * stable_loss + c_ar * absRel_loss
// of the reference's VideoDepthLoss (d1 is piecewise constant), from the state the forward left: the float32 fit, the
// per-frame medians, scales and counts, and out[20]. include/vdn.h (vdn_depth_loss_backward) states the arithmetic.
//   stats      per frame in DL_BPF blocks: sum g_x, sum g_x x, sum |a - m| (for the clamp's branch), sigma = sum sign(a - m),
//              the lowest index of a kept pixel with a == m, the masked min / max of the target, and the four sums of the fit
//   solve 1    one block: g_s, g_m, the median's holder and the float32 temporal threshold per frame; the fit's sums per item
//   fit sums   g_a per kept pixel; per frame in DL_BPF blocks sum g_a p and sum g_a
//   solve 2    one block: an item's frames in index order
//   write      g_p = sc g_a + keep * (fit correction) (FitGrad, loss_px.hpp), rounded to float32 once; +0.0 at a dropped pixel
// g_x is a gather: a pixel reads its left, right, upper and lower neighbour at stride 2^k on every grid it belongs to, inside
// its own frame, and no lane writes another lane's pixel. There are no atomics; sums have the fixed order of frame_sums.hpp.
// Pass 1 leaves g_x in an fp64 plane of the workspace, pass 3 turns it into g_a in place and pass 5 reads it, so the stencil is
// evaluated once. The alternative, every pass recomputing g_x from the inputs with a workspace that depends on B and T alone,
// was measured and dropped: 679 against 380 us for the launch at [1, 32, 518, 518] (profiles/depth_loss_grad.md).
// A lane owns four consecutive pixels whenever H * W is a multiple of 4, with 16-byte loads where the bases allow and a load
// per pixel otherwise, so the sums and the gradient's bits do not depend on the tensors' alignment; one pixel per lane else.
// Everything is fp64 computed from the float32 samples, contraction off; a dropped pixel is skipped by a branch.
// The trimmed criterion (vdn_depth_loss_trimmed_backward) runs the same five passes: the data part of g_x and the temporal and
// absRel parts of g_a carry the weight 1, w or 0 that the forward's selection gives their residual (loss_px.hpp), the key
// recomputed from the inputs and compared with the threshold in out[20..34]. Untrimmed, every weight is an exact 1.
#include "common.hpp"
#include "frame_sums.hpp"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)
#include "loss_px.hpp"

namespace {

constexpr int NSUM = 7;  // sum g_x, sum g_x x, sum |a - m|, sum p^2, sum p, sum p t, sum t; the row's one count is sigma
enum { I_A00 = 0, I_A01, I_A11, I_B0, I_B1, I_D, I_OK, I_G0, I_G1, I_SLOTS };

struct IntMinOp {
  __device__ __forceinline__ int operator()(int a, int b) const { return b < a ? b : a; }
};

// workspace, in 8-byte slots; a pass's rows (frame_sums.hpp) are a sums array and a counts array
struct Gw {
  double* sum_b;     // [F][DL_BPF][NSUM]
  int64_t* sig_b;    // [F][DL_BPF] their counts: sigma
  int64_t* hold_b;   // [F][DL_BPF] lowest index with a == m, INT_MAX for none
  float* mm_b;       // [F][DL_BPF][2] block min, max of the kept target
  double* G_b;       // [F][DL_BPF][2] block sums g_a p, g_a
  double* fit_f;     // [F][4]
  double* gsm;       // [F][2] g_s, g_m
  int64_t* hold_f;   // [F] the holder's index in the frame, -1 for nobody
  float* th;         // [F] (a slot each)
  double* item;      // [B][I_SLOTS]
  double* plane;     // [F][H W] g_x, then g_a
  __host__ __device__ static size_t slots(size_t B, size_t F) { return F * DL_BPF * (NSUM + 1 + 1 + 1 + 2) + F * (4 + 2 + 1 + 1) + B * I_SLOTS; }
  __host__ __device__ Gw(void* p, int B, int T) {
    const size_t F = (size_t)B * T, FB = F * DL_BPF;
    double* q = (double*)p;
    sum_b = q, q += FB * NSUM;
    sig_b = (int64_t*)q, q += FB;
    hold_b = (int64_t*)q, q += FB;
    mm_b = (float*)q, q += FB;
    G_b = q, q += FB * 2;
    fit_f = q, q += F * 4;
    gsm = q, q += F * 2;
    hold_f = (int64_t*)q, q += F;
    th = (float*)q, q += F;
    item = q, q += (size_t)B * I_SLOTS;
    plane = q;
  }
};

__device__ __forceinline__ int sgn(double v) { return (v > 0.0) - (v < 0.0); }  // 0 for 0 and for NaN

// What every pass knows about its frame. The forward's results are read, never redone: sc, sh (scale_shift), the medians and
// scales (frame_stats), the counts (frame_counts, out).
struct FrameCtx {
  const float* pf;
  const float* tf;
  const uint8_t* mf;
  int H, W, hw, scales;
  float sc, sh;
  double mp, sp, mt, st, cnt;
  double alpha, c_sp, c_st, c_ar, Mtot, Mk[DL_MAX_SCALES], Mt, Mar;
  const double* tr;  // out + 20 of vdn_depth_loss_trimmed: per term k | n_less | n_tied | thr | w; nullptr: every weight is 1
  bool has_prev, has_next;  // a frame of the same item before / after this one, when the temporal term is on
  __device__ FrameCtx(const float* pred, const float* target, const uint8_t* mask, int T, int H_, int W_, double alpha_, int scales_,
                      int temporal, const float* __restrict__ ss, const double* __restrict__ fs, const int64_t* __restrict__ fc,
                      const double* __restrict__ out, const float* __restrict__ coeff, int trimmed, int f) {
    tr = trimmed ? out + 20 : nullptr;
    H = H_, W = W_, hw = H_ * W_, scales = scales_, alpha = alpha_;
    pf = pred + (size_t)f * hw, tf = target + (size_t)f * hw, mf = mask + (size_t)f * hw;
    sc = ss[(f / T) * 2], sh = ss[(f / T) * 2 + 1];
    mp = fs[(size_t)f * 4], sp = fs[(size_t)f * 4 + 1], mt = fs[(size_t)f * 4 + 2], st = fs[(size_t)f * 4 + 3];
    cnt = (double)fc[f];
    c_sp = (double)coeff[0], c_st = temporal ? (double)coeff[1] : 0.0, c_ar = (double)coeff[2];
    Mtot = out[7], Mt = temporal ? out[16] : 0.0, Mar = out[17];
#pragma unroll
    for (int k = 0; k < DL_MAX_SCALES; ++k) Mk[k] = out[12 + k];
    has_prev = temporal && (f % T) > 0;
    has_next = temporal && (f % T) + 1 < T;
  }
  // the difference of the normalised maps at one pixel, exactly as the forward takes it
  __device__ __forceinline__ double diff(float a, float t) const { return ((double)a - mp) / sp - ((double)t - mt) / st; }
  __device__ __forceinline__ double diff_at(size_t o) const { return diff(aligned(sc, pf[o], sh), tf[o]); }
  // the weight u of a counted element of `term` with residual r (loss_px.hpp): 1 when nothing is trimmed
  __device__ __forceinline__ double weight(int term, double r) const { return tr ? trim_weight(tr + 5 * term, trim_key(r)) : 1.0; }
  // g_x of the kept pixel p = (y, x) whose difference is d: the data term's sign and, per grid, the integer sum of
  // sign(d_self - d_nb) over the kept neighbours, divided by the grid's kept points; grids in ascending order
  __device__ __forceinline__ double gx(int p, int y, int x, double d) const {
    double reg = 0.0;
    bool on = true;
#pragma unroll
    for (int k = 0; k < DL_MAX_SCALES; ++k) {
      const int step = 1 << k;
      on = on && k < scales && ((x | y) & (step - 1)) == 0;
      if (on && Mk[k] > 0.0) {
        int n = 0;
        if (x + step < W && mf[p + step] != 0) n += sgn(d - diff_at((size_t)p + step));
        if (x >= step && mf[p - step] != 0) n += sgn(d - diff_at((size_t)p - step));
        if (y + step < H) {
          const size_t o = (size_t)p + (size_t)step * W;
          if (mf[o] != 0) n += sgn(d - diff_at(o));
        }
        if (y >= step) {
          const size_t o = (size_t)p - (size_t)step * W;
          if (mf[o] != 0) n += sgn(d - diff_at(o));
        }
        reg += (double)n / Mk[k];
      }
    }
    return c_sp * (weight(TR_DATA, fabs(d)) * (double)sgn(d) / Mtot + alpha * reg);
  }
  // g_a of the kept pixel p with aligned prediction a and target t, from its g_x; gs, gm, holder, th_self and th_next are
  // solve 1's results for this frame (th_next: of the next frame)
  __device__ __forceinline__ double ga(int p, float a, float t, double gxv, double gs, double gm, int64_t holder, float th_self,
                                       float th_next) const {
    double g = gxv / sp + gs * (double)sgn((double)a - mp) / cnt;
    if ((int64_t)p == holder) g += gm;
    if (Mt > 0.0) {
      double later = 0.0, earlier = 0.0;
      if (has_prev && mf[(ptrdiff_t)p - hw] != 0) {  // the pair (f - 1, f): this frame is the later one
        const float tq = tf[(ptrdiff_t)p - hw], tg = t - tq;
        if (fabsf(tg) < th_self) {
          const float pg = a - aligned(sc, pf[(ptrdiff_t)p - hw], sh);
          later = weight(TR_STABLE, res_stable(pg, tg)) * (double)sgn((double)pg - (double)tg);
        }
      }
      if (has_next && mf[(size_t)p + hw] != 0) {     // the pair (f, f + 1): this frame is the earlier one
        const float tq = tf[(size_t)p + hw], tg = tq - t;
        if (fabsf(tg) < th_next) {
          const float pg = aligned(sc, pf[(size_t)p + hw], sh) - a;
          earlier = weight(TR_STABLE, res_stable(pg, tg)) * (double)sgn((double)pg - (double)tg);
        }
      }
      g += c_st * (later - earlier) / Mt;
    }
    if (Mar > 0.0 && t > 1e-3f && t < 70.f) g += c_ar * (weight(TR_ABSREL, res_absrel(a, t)) * (double)sgn((double)a - (double)t)) / ((double)t * Mar);
    return g;
  }
};

#define GRAD_ARGS                                                                                                              \
  const float *__restrict__ pred, const float *__restrict__ target, const uint8_t *__restrict__ mask, int B, int T, int H, int W, \
      double alpha, int scales, int temporal, const float *__restrict__ ss, const double *__restrict__ fs,                      \
      const int64_t *__restrict__ fc, const double *__restrict__ out, const float *__restrict__ coeff, int trimmed, void *__restrict__ workspace
#define GRAD_CTX FrameCtx c(pred, target, mask, T, H, W, alpha, scales, temporal, ss, fs, fc, out, coeff, trimmed, f)

// ------------------------------------------------------------------------------------------------ pass 1
template <int PPL, bool VEC>
__global__ __launch_bounds__(256) void grad_stats_kernel(GRAD_ARGS) {
  const Gw ws(workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const GRAD_CTX;
  const float mpf = (float)c.mp;  // the median is a float32 sample or 0
  Tuple<double, NSUM> s;
#pragma unroll
  for (int i = 0; i < NSUM; ++i) s.v[i] = 0.0;
  Tuple<int, 1> sigma = {{0}};
  int hold = INT_MAX;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t q0 = sweep_first<PPL>(b); q0 < c.hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL, VEC> q(c.pf, c.tf, c.mf, p0);
    RowWalk at(p0, W);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      double g = 0.0;
      if (q.k[j]) {
        const float a = aligned(c.sc, q.p[j], c.sh), t = q.t[j];
        g = c.gx(p0 + j, at.y, at.x, c.diff(a, t));
        const double dev = (double)a - c.mp, pd = (double)q.p[j], td = (double)t;
        s.v[0] += g;
        s.v[1] += g * (dev / c.sp);
        s.v[2] += fabs(dev);
        s.v[3] += pd * pd;
        s.v[4] += pd;
        s.v[5] += pd * td;
        s.v[6] += td;
        sigma.v[0] += sgn(dev);
        if (a == mpf) hold = IntMinOp{}(hold, p0 + j);
        mn = MinOp{}(mn, t);
        mx = MaxOp{}(mx, t);
      }
      ws.plane[(size_t)f * c.hw + p0 + j] = g;
      at.step(W);
    }
  }
  __shared__ WaveSlots<int> rh;
  __shared__ WaveSlots<float> rmn, rmx;
  rh.put(hold, IntMinOp{});
  rmn.put(mn, MinOp{});
  rmx.put(mx, MaxOp{});
  block_row<NSUM, 1>(s, sigma, ws.sum_b, ws.sig_b);
  if (threadIdx.x == 0) {
    ws.hold_b[blockIdx.x] = (int64_t)rh.get(IntMinOp{});
    ws.mm_b[(size_t)blockIdx.x * 2] = rmn.get(MinOp{});
    ws.mm_b[(size_t)blockIdx.x * 2 + 1] = rmx.get(MaxOp{});
  }
}

// One block: the fold of frame_sums.hpp, a lane per frame and then a lane per item.
__global__ __launch_bounds__(256) void grad_solve1_kernel(void* __restrict__ workspace, int B, int T, int hw, const double* __restrict__ fs,
                                                          const int64_t* __restrict__ fc) {
  const Gw ws(workspace, B, T);
  const int F = B * T;
  for (int f = threadIdx.x; f < F; f += 256) {
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t sigma = 0, hold = INT_MAX;
    float mn = INFINITY, mx = -INFINITY;
    for (const size_t o : frame_blocks<DL_BPF>(f)) {
      add_row<NSUM, 1>(ws.sum_b, ws.sig_b, o, s, &sigma);
      hold = ws.hold_b[o] < hold ? ws.hold_b[o] : hold;
      mn = MinOp{}(mn, ws.mm_b[o * 2]);
      mx = MaxOp{}(mx, ws.mm_b[o * 2 + 1]);
    }
    const int64_t n = fc[f];
    const double m = fs[(size_t)f * 4], sp = fs[(size_t)f * 4 + 1];
    double gs = 0.0, gm = 0.0;
    if (n > 0) {
      if (s[2] / (double)n >= 1e-6) gs = -s[1] / sp;  // the clamp passes no gradient below its bound
      gm = -s[0] / sp - gs * (double)sigma / (double)n;
    }
    ws.gsm[(size_t)f * 2] = gs;
    ws.gsm[(size_t)f * 2 + 1] = gm;
    // a median of 0 in a frame with a dropped pixel is taken to be a dropped pixel's 0: mask * a has the derivative 0 there
    ws.hold_f[f] = (n == 0 || hold == INT_MAX || (m == 0.0 && n < (int64_t)hw)) ? -1 : hold;
    ws.th[f] = (mx - mn) * 0.05f;  // -inf for a frame without a kept pixel: nothing is below it
    store_row<4, 0>(ws.fit_f, nullptr, (size_t)f, s + 3, nullptr);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) {
    double s[4];
    int64_t n;  // the forward's kept pixels, beside the fit's sums
    fold_frames<4, 1>(b * T, T, s, &n, [&](int f, double* row_s, int64_t* row_n) {
      load_row<4, 0>(ws.fit_f, nullptr, (size_t)f, row_s, nullptr);
      row_n[0] = fc[f];
    });
    const double a00 = s[0], a01 = s[1], b0 = s[2], b1 = s[3], a11 = (double)n, det = a00 * a11 - a01 * a01;
    double* it = ws.item + (size_t)b * I_SLOTS;
    it[I_A00] = a00, it[I_A01] = a01, it[I_A11] = a11, it[I_B0] = b0, it[I_B1] = b1, it[I_D] = det + 1e-6;
    it[I_OK] = det != 0.0 ? 1.0 : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ pass 2
template <int PPL, bool VEC>
__global__ __launch_bounds__(256) void grad_fit_partial_kernel(GRAD_ARGS) {
  const Gw ws(workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const GRAD_CTX;
  const double gs = ws.gsm[(size_t)f * 2], gm = ws.gsm[(size_t)f * 2 + 1];
  const int64_t holder = ws.hold_f[f];
  const float th_self = ws.th[f], th_next = c.has_next ? ws.th[f + 1] : 0.f;
  Tuple<double, 2> s = {{0.0, 0.0}};
  for (int64_t q0 = sweep_first<PPL>(b); q0 < c.hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL, VEC> q(c.pf, c.tf, c.mf, p0);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (q.k[j]) {
        const float a = aligned(c.sc, q.p[j], c.sh), t = q.t[j];
        const size_t o = (size_t)f * c.hw + p0 + j;
        const double g = c.ga(p0 + j, a, t, ws.plane[o], gs, gm, holder, th_self, th_next);
        ws.plane[o] = g;  // g_x becomes g_a in place: the lane that wrote the slot reads and rewrites it
        s.v[0] += g * (double)q.p[j];
        s.v[1] += g;
      }
    }
  }
  block_row<2>(s, ws.G_b);
}

// One block, a lane per item: the fold of frame_sums.hpp (every frame's blocks in index order, the frames in index order),
// spelled out; keep it equal to fold_frames over fold_blocks (profiles/criteria_refactor.md says why it is not a call).
__global__ __launch_bounds__(256) void grad_solve2_kernel(void* __restrict__ workspace, int B, int T) {
  const Gw ws(workspace, B, T);
  for (int b = threadIdx.x; b < B; b += 256) {
    double G0 = 0.0, G1 = 0.0;
    for (int t = 0; t < T; ++t) {
      double f0 = 0.0, f1 = 0.0;
      for (int k = 0; k < DL_BPF; ++k) {
        const size_t o = ((size_t)b * T + t) * DL_BPF + k;
        f0 += ws.G_b[o * 2], f1 += ws.G_b[o * 2 + 1];
      }
      G0 += f0, G1 += f1;
    }
    ws.item[(size_t)b * I_SLOTS + I_G0] = G0;
    ws.item[(size_t)b * I_SLOTS + I_G1] = G1;
  }
}

// ------------------------------------------------------------------------------------------------ pass 3
template <int PPL, bool VEC>
__global__ __launch_bounds__(256) void grad_write_kernel(GRAD_ARGS, float* __restrict__ grad) {
  const Gw ws(workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const GRAD_CTX;
  const double* it = ws.item + (size_t)(f / T) * I_SLOTS;
  const FitGrad fit{it[I_A01], it[I_A11], it[I_B0], it[I_B1], it[I_D], it[I_G0], it[I_G1], (double)c.sc, (double)c.sh};
  const bool ok = it[I_OK] != 0.0;
  float* gf = grad + (size_t)f * c.hw;
  // the start IS sweep_first<PPL>(b) of frame_sums.hpp, spelled out, and must stay equal to it (profiles/criteria_refactor.md
  // says why it is not a call)
  for (int64_t q0 = (int64_t)(b * 256 + (int)threadIdx.x) * PPL; q0 < c.hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL, VEC> q(c.pf, c.tf, c.mf, p0);
    float r[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      r[j] = 0.f;
      if (q.k[j] && ok) {
        r[j] = (float)fit(ws.plane[(size_t)f * c.hw + p0 + j], (double)q.p[j], (double)q.t[j]);
      }
    }
    store_px<PPL, VEC>(gf + p0, r);
  }
}

}  // namespace

extern "C" size_t vdn_depth_loss_backward_workspace_bytes(int B, int T, int H, int W) {
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
  const size_t F = (size_t)B * T;
  return sizeof(double) * (Gw::slots((size_t)B, F) + F * (size_t)H * W);
}

// trimmed: out is the f64 [40] of vdn_depth_loss_trimmed and out[20..34] weigh the three trimmed terms
static int depth_loss_backward(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                               double alpha, int scales, double stable_scale, const float* scale_shift, const double* frame_stats,
                               const int64_t* frame_counts, const double* out, const float* coeff, int trimmed, void* workspace,
                               float* grad_prediction, vdn_stream stream) {
  if (!prediction || !target || !mask || !workspace || !scale_shift || !frame_stats || !frame_counts || !out || !coeff || !grad_prediction)
    return VDN_EINVAL;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || scales < 0) return VDN_EINVAL;
  if (stable_scale > 0.0 && T < 2) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX || (int64_t)B * T > 65535 || scales > DL_MAX_SCALES) return VDN_EUNSUPPORTED;
  if (trimmed && (uint64_t)B * T * (uint64_t)H * W > UINT32_MAX) return VDN_EUNSUPPORTED;  // as the trimmed forward
  if (misaligned(4, prediction, target, scale_shift, coeff, grad_prediction) || misaligned(8, workspace, frame_stats, frame_counts, out))
    return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int F = B * T, hw = H * W;
  const dim3 grid((unsigned)F * DL_BPF), block(256);
  // A lane owns four consecutive pixels whenever a frame holds whole quads, so the sums do not depend on where the tensors
  // start; the 16-byte loads and stores are taken when wide_ok allows them.
  const bool quads = hw % 4 == 0;
  const bool vec = wide_ok((size_t)hw, {prediction, target, grad_prediction}, {mask});
  const int eff_scales = alpha > 0.0 ? scales : 0;  // as the forward: the regulariser is skipped
  const int temporal = stable_scale > 0.0;
  auto launch = [&](auto ppl, auto v) {
    constexpr int PPL = decltype(ppl)::value;
    constexpr bool VEC = decltype(v)::value != 0;
    hipLaunchKernelGGL((grad_stats_kernel<PPL, VEC>), grid, block, 0, s, prediction, target, mask, B, T, H, W, alpha, eff_scales,
                       temporal, scale_shift, frame_stats, frame_counts, out, coeff, trimmed, workspace);
    hipLaunchKernelGGL(grad_solve1_kernel, dim3(1), block, 0, s, workspace, B, T, hw, frame_stats, frame_counts);
    hipLaunchKernelGGL((grad_fit_partial_kernel<PPL, VEC>), grid, block, 0, s, prediction, target, mask, B, T, H, W, alpha, eff_scales,
                       temporal, scale_shift, frame_stats, frame_counts, out, coeff, trimmed, workspace);
    hipLaunchKernelGGL(grad_solve2_kernel, dim3(1), block, 0, s, workspace, B, T);
    hipLaunchKernelGGL((grad_write_kernel<PPL, VEC>), grid, block, 0, s, prediction, target, mask, B, T, H, W, alpha, eff_scales,
                       temporal, scale_shift, frame_stats, frame_counts, out, coeff, trimmed, workspace, grad_prediction);
  };
  if (vec) launch(IC<4>{}, IC<1>{});
  else with_ppl(quads, [&](auto ppl) { launch(ppl, IC<0>{}); });  // quads on unaligned bases: a load per pixel
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_depth_loss_backward(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                                       double alpha, int scales, double stable_scale, const float* scale_shift,
                                       const double* frame_stats, const int64_t* frame_counts, const double* out, const float* coeff,
                                       void* workspace, float* grad_prediction, vdn_stream stream) {
  return depth_loss_backward(prediction, target, mask, B, T, H, W, alpha, scales, stable_scale, scale_shift, frame_stats, frame_counts,
                             out, coeff, 0, workspace, grad_prediction, stream);
}

extern "C" size_t vdn_depth_loss_trimmed_backward_workspace_bytes(int B, int T, int H, int W) {
  return vdn_depth_loss_backward_workspace_bytes(B, T, H, W);
}

extern "C" int vdn_depth_loss_trimmed_backward(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H,
                                               int W, double alpha, int scales, double stable_scale, const float* scale_shift,
                                               const double* frame_stats, const int64_t* frame_counts, const double* out,
                                               const float* coeff, void* workspace, float* grad_prediction, vdn_stream stream) {
  return depth_loss_backward(prediction, target, mask, B, T, H, W, alpha, scales, stable_scale, scale_shift, frame_stats, frame_counts,
                             out, coeff, 1, workspace, grad_prediction, stream);
}
