// The depth criterion of the reference's validate on the device: VideoDepthLoss of loss/loss.py:326-367 (trim = 0,
// batch-based reduction, no SSIM term), forward only, for [B, T, H, W] tensors that already sit in HBM. The trimmed criterion
// (trim > 0: vdn_depth_loss_trimmed) runs these passes and then its own, in the last section of the namespace.
//   fit        per item, the masked sums of compute_scale_and_shift (fp64), per-frame counts and the masked min / max of
//              the target; a one-block solve rounds scale and shift to float32 once
//   select     the lower medians of keep ? aligned : 0 and keep ? target : 0 per frame (select.hpp, two slots)
//   scale      per frame, sum over kept pixels of |x - m| for both
//   fused      one pass: data term, the gradient terms of the grids [::2^k, ::2^k], absRel, d1 and the temporal term;
//              then a one-block finalise
// The aligned prediction a = fl32(fl32(scale * p) + shift) is never stored: every pass recomputes it bit for bit, so
// thresholds, medians and differences are taken on the float32 numbers the reference holds. Everything else is fp64
// computed from the float32 samples with separate multiply and add roundings (contraction is off for this file). A dropped
// pixel is skipped by a branch: NaN or inf under it reaches nothing. Sums have the fixed order of frame_sums.hpp, with DL_BPF
// blocks per frame. The only atomics are the integer ones of the select's histograms: two runs give the same bits.
// Any 4-byte-aligned pointer is accepted; where H * W is a multiple of 4, prediction and target are 16-byte aligned and the
// mask 4-byte aligned, a lane reads four consecutive pixels with one load per plane, one pixel otherwise. Neighbours
// (x + 2^k, y + 2^k) that belong to other lanes are read through the cache; the right-hand neighbour of the finest grid
// comes from the lane's own quad, and the next frame's pixels are read like the frame's own.
#include "common.hpp"
#include "frame_sums.hpp"
#include "select.hpp"
#include <math.h>

#pragma clang fp contract(off)
#include "loss_px.hpp"

namespace {

constexpr int NACC = 3 + DL_MAX_SCALES;
// accumulator slots of the fused pass: doubles {data, absRel, temporal, g_0 .. g_3 numerators}, integers {absRel count,
// d1 hits, temporal count, M_0 .. M_3}
enum { A_DATA = 0, A_ABSREL = 1, A_TEMP = 2, A_G = 3 };

// workspace, in 8-byte slots; a pass's rows (frame_sums.hpp) are a sums array and a counts array
struct Ws {
  double* fit_b;     // [F][DL_BPF][4] block sums p^2, p, p t, t
  int64_t* cnt_b;    // [F][DL_BPF] their counts: kept pixels
  float* mm_b;       // [F][DL_BPF][2] block min, max of the kept target
  double* fit_f;     // [F][4]
  int64_t* cnt_f;    // [F]
  float* th;         // [F] (a slot each)
  float* ss;         // [B][2] scale, shift
  float* med;        // [F][2] lower median of the aligned prediction, of the target
  double* dev_b;     // [F][DL_BPF][2] block sums |a - m|, |t - m|
  double* acc_b;     // [F][DL_BPF][NACC]
  int64_t* cnt_acc_b;  // [F][DL_BPF][NACC]
  double* acc_f;     // [F][NACC]
  int64_t* cnt_acc_f;  // [F][NACC]
  void* select;
  __host__ __device__ static size_t slots(size_t B, size_t F) {
    return F * DL_BPF * (4 + 1 + 1 + 2 + 2 * NACC) + F * (4 + 1 + 1 + 1 + 2 * NACC) + B;
  }
  __host__ __device__ Ws(void* p, int B, int T) {
    const size_t F = (size_t)B * T, FB = F * DL_BPF;
    double* q = (double*)p;
    fit_b = q, q += FB * 4;
    cnt_b = (int64_t*)q, q += FB;
    mm_b = (float*)q, q += FB;
    dev_b = q, q += FB * 2;
    acc_b = q, q += FB * NACC;
    cnt_acc_b = (int64_t*)q, q += FB * NACC;
    fit_f = q, q += F * 4;
    cnt_f = (int64_t*)q, q += F;
    th = (float*)q, q += F;
    med = (float*)q, q += F;
    acc_f = q, q += F * NACC;
    cnt_acc_f = (int64_t*)q, q += F * NACC;
    ss = (float*)q, q += B;
    select = q;
  }
};

// ------------------------------------------------------------------------------------------------ fit
template <int PPL>
__global__ __launch_bounds__(256) void fit_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, int B, int T, int hw,
                                                          void* __restrict__ workspace) {
  const Ws ws(workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const float* pf = pred + (size_t)f * hw;
  const float* tf = target + (size_t)f * hw;
  const uint8_t* mf = mask + (size_t)f * hw;
  Tuple<double, 4> s = {{0.0, 0.0, 0.0, 0.0}};
  Tuple<int, 1> cnt = {{0}};
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL> q(pf, tf, mf, p0);
#pragma unroll
    for (int j = 0; j < PPL; ++j)
      if (q.k[j]) {
        const double p = (double)q.p[j], t = (double)q.t[j];
        s.v[0] += p * p;
        s.v[1] += p;
        s.v[2] += p * t;
        s.v[3] += t;
        cnt.v[0] += 1;
        mn = MinOp{}(mn, q.t[j]);
        mx = MaxOp{}(mx, q.t[j]);
      }
  }
  __shared__ WaveSlots<float> rmn, rmx;
  rmn.put(mn, MinOp{});
  rmx.put(mx, MaxOp{});
  block_row<4, 1>(s, cnt, ws.fit_b, ws.cnt_b);
  if (threadIdx.x == 0) {
    ws.mm_b[(size_t)blockIdx.x * 2] = rmn.get(MinOp{});
    ws.mm_b[(size_t)blockIdx.x * 2 + 1] = rmx.get(MaxOp{});
  }
}

// One block: the fold of frame_sums.hpp, a lane per frame and then a lane per item, then the 2 x 2 solve.
__global__ __launch_bounds__(256) void fit_solve_kernel(void* __restrict__ workspace, int B, int T, int64_t* __restrict__ frame_counts,
                                                        float* __restrict__ scale_shift) {
  const Ws ws(workspace, B, T);
  const int F = B * T;
  for (int f = threadIdx.x; f < F; f += 256) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t n = 0;
    float mn = INFINITY, mx = -INFINITY;
    for (const size_t o : frame_blocks<DL_BPF>(f)) {
      add_row<4, 1>(ws.fit_b, ws.cnt_b, o, s, &n);
      mn = MinOp{}(mn, ws.mm_b[o * 2]);
      mx = MaxOp{}(mx, ws.mm_b[o * 2 + 1]);
    }
    store_row<4, 1>(ws.fit_f, ws.cnt_f, (size_t)f, s, &n);
    ws.th[f] = (mx - mn) * 0.05f;  // -inf for a frame without a kept pixel: nothing is below it
    if (frame_counts) frame_counts[f] = n;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) {
    double s[4];
    int64_t n;
    fold_frames<4, 1>(ws.fit_f, ws.cnt_f, b * T, T, s, &n);
    const double a00 = s[0], a01 = s[1], b0 = s[2], b1 = s[3], a11 = (double)n;
    const double det = a00 * a11 - a01 * a01;
    double scale = 0.0, shift = 0.0;
    if (det != 0.0) {
      scale = (a11 * b0 - a01 * b1) / (det + 1e-6);
      shift = (-a01 * b0 + a00 * b1) / (det + 1e-6);
    }
    ws.ss[b * 2] = (float)scale;
    ws.ss[b * 2 + 1] = (float)shift;
    if (scale_shift) scale_shift[b * 2] = (float)scale, scale_shift[b * 2 + 1] = (float)shift;
  }
}

// ------------------------------------------------------------------------------------------------ medians
// slot 0: keep ? aligned prediction : 0; slot 1: keep ? target : 0 (torch.median of mask * x counts dropped pixels as zeros)
struct LossKey {
  const float* pred;
  const float* target;
  const uint8_t* mask;
  const float* ss;
  size_t hw;
  int T;
  static constexpr int SLOTS = 2, PER = 1;
  __device__ __forceinline__ uint32_t operator()(int f, size_t i, uint32_t (&key)[1][2]) const {
    const size_t o = (size_t)f * hw + i;
    float a = 0.f, t = 0.f;
    if (mask[o] != 0) {
      const int b = f / T;
      a = aligned(ss[b * 2], pred[o], ss[b * 2 + 1]);
      t = target[o];
    }
    key[0][0] = ordered_key(a);
    key[0][1] = ordered_key(t);
    return 3u;
  }
};

__global__ void median_store_kernel(const SelState* __restrict__ st, int F, float* __restrict__ med) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F * 2) med[i] = key_value(st[i].prefix) + 0.f;  // + 0: a median of -0.0 is stored as +0.0
}

template <int PPL>
__global__ __launch_bounds__(256) void deviation_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                const uint8_t* __restrict__ mask, int B, int T, int hw,
                                                                void* __restrict__ workspace) {
  const Ws ws(workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const float* pf = pred + (size_t)f * hw;
  const float* tf = target + (size_t)f * hw;
  const uint8_t* mf = mask + (size_t)f * hw;
  const float sc = ws.ss[(f / T) * 2], sh = ws.ss[(f / T) * 2 + 1];
  const double mp = (double)ws.med[f * 2], mt = (double)ws.med[f * 2 + 1];
  Tuple<double, 2> s = {{0.0, 0.0}};
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL> q(pf, tf, mf, p0);
#pragma unroll
    for (int j = 0; j < PPL; ++j)
      if (q.k[j]) {
        s.v[0] += fabs((double)aligned(sc, q.p[j], sh) - mp);
        s.v[1] += fabs((double)q.t[j] - mt);
      }
  }
  block_row<2>(s, ws.dev_b);
}

// s of normalize_prediction_robust: max(sum |x - m| / n, 1e-6), 1 for a frame without a kept pixel; which = 0 prediction, 1 target
__device__ double frame_scale(const Ws& ws, int f, int which) {
  const int64_t n = ws.cnt_f[f];
  if (n == 0) return 1.0;
  double s = 0.0;
  for (const size_t o : frame_blocks<DL_BPF>(f)) s += ws.dev_b[o * 2 + which];
  s = s / (double)n;
  return s < 1e-6 ? 1e-6 : s;
}

// ------------------------------------------------------------------------------------------------ fused pass
template <int PPL>
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const uint8_t* __restrict__ mask, int B, int T, int H, int W, int scales,
                                                           int temporal, void* __restrict__ workspace) {
  const Ws ws(workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const int hw = H * W;
  const float* pf = pred + (size_t)f * hw;
  const float* tf = target + (size_t)f * hw;
  const uint8_t* mf = mask + (size_t)f * hw;
  __shared__ double fs[2];
  if (threadIdx.x < 2) fs[threadIdx.x] = frame_scale(ws, f, threadIdx.x);
  __syncthreads();
  const float sc = ws.ss[(f / T) * 2], sh = ws.ss[(f / T) * 2 + 1];
  const double mp = (double)ws.med[f * 2], mt = (double)ws.med[f * 2 + 1], sp = fs[0], st = fs[1];
  const bool has_next = temporal && (f % T) + 1 < T;  // the next frame of the same item
  const float th = has_next ? ws.th[f + 1] : 0.f;
  // the difference of the normalised maps at one pixel
  auto diff = [&](float a, float t) { return ((double)a - mp) / sp - ((double)t - mt) / st; };
  Tuple<double, NACC> acc;
  Tuple<int, NACC> cnt;
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc.v[i] = 0.0, cnt.v[i] = 0;
  // The start below IS sweep_first<PPL>(b) of frame_sums.hpp, spelled out, and must stay equal to it (the lane owns the pixels
  // every other pass gives it). With the call the compiler leaves neighbour loads and their addresses of this kernel unmerged
  // (profiles/criteria_refactor.md).
  for (int64_t q0 = (int64_t)(b * 256 + (int)threadIdx.x) * PPL; q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL> q(pf, tf, mf, p0);
    // the same pixels of the next frame: frames are hw apart, so these are the same kind of load as q's
    const Px<PPL> qn(pf + (has_next ? hw : 0), tf + (has_next ? hw : 0), mf + (has_next ? hw : 0), p0);
    RowWalk at(p0, W);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (q.k[j]) {  // a dropped pixel is skipped: nothing under it is read into the sums
        const int p = p0 + j;
        const float a = aligned(sc, q.p[j], sh), t = q.t[j];
        const double d = diff(a, t);
        acc.v[A_DATA] += fabs(d);
        if (t > 1e-3f && t < 70.f) {
          acc.v[A_ABSREL] += fabs(((double)a - (double)t) / (double)t);
          cnt.v[A_ABSREL] += 1;
        }
        if (__fdiv_rn(a, t) < 1.25f && __fdiv_rn(t, a) < 1.25f) cnt.v[A_DATA] += 1;  // max(a / t, t / a) < 1.25; NaN is false
        if (has_next && qn.k[j]) {
          const float tg = qn.t[j] - t;
          if (fabsf(tg) < th) {
            const float pg = aligned(sc, qn.p[j], sh) - a;
            acc.v[A_TEMP] += fabs((double)pg - (double)tg);
            cnt.v[A_TEMP] += 1;
          }
        }
        bool on = true;
#pragma unroll
        for (int k = 0; k < DL_MAX_SCALES; ++k) {
          const int step = 1 << k;
          on = on && k < scales && ((at.x | at.y) & (step - 1)) == 0;  // a point of the grid [::step, ::step]
          if (on) {
            cnt.v[A_G + k] += 1;
            if (at.x + step < W) {
              const int jn = (j + 1) % PPL;
              if (PPL == 4 && k == 0 && jn > 0) {  // the next pixel of the quad, in the same row
                if (q.k[jn]) acc.v[A_G + k] += fabs(diff(aligned(sc, q.p[jn], sh), q.t[jn]) - d);
              } else if (mf[p + step] != 0) {
                acc.v[A_G + k] += fabs(diff(aligned(sc, pf[p + step], sh), tf[p + step]) - d);
              }
            }
            if (at.y + step < H) {
              const size_t o = (size_t)p + (size_t)step * W;
              if (mf[o] != 0) acc.v[A_G + k] += fabs(diff(aligned(sc, pf[o], sh), tf[o]) - d);
            }
          }
        }
      }
      at.step(W);
    }
  }
  block_row<NACC, NACC>(acc, cnt, ws.acc_b, ws.cnt_acc_b);
}

// One block: the fold of frame_sums.hpp. The integer slot of A_DATA holds the d1 hits.
__global__ __launch_bounds__(256) void loss_finalise_kernel(void* __restrict__ workspace, int B, int T, double alpha, int scales,
                                                            double stable_scale, double* __restrict__ frame_stats,
                                                            double* __restrict__ out) {
  const Ws ws(workspace, B, T);
  const int F = B * T;
  for (int f = threadIdx.x; f < F; f += 256) {
    // fold_blocks, with one row per trip: unrolled, the 2 * NACC accumulators and two rows in flight cost this kernel a wave
    // of occupancy
    double s[NACC] = {};
    int64_t n[NACC] = {};
#pragma unroll 1
    for (const size_t o : frame_blocks<DL_BPF>(f)) add_row<NACC, NACC>(ws.acc_b, ws.cnt_acc_b, o, s, n);
    store_row<NACC, NACC>(ws.acc_f, ws.cnt_acc_f, (size_t)f, s, n);
    if (frame_stats) {
      frame_stats[(size_t)f * 4] = (double)ws.med[f * 2];
      frame_stats[(size_t)f * 4 + 1] = frame_scale(ws, f, 0);
      frame_stats[(size_t)f * 4 + 2] = (double)ws.med[f * 2 + 1];
      frame_stats[(size_t)f * 4 + 3] = frame_scale(ws, f, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s[NACC];
  int64_t n[NACC + 1];  // the fused pass's counts, and the fit's kept pixels beside them
  fold_frames<NACC, NACC + 1>(0, F, s, n, [&](int f, double* fs, int64_t* fn) {
    load_row<NACC, NACC>(ws.acc_f, ws.cnt_acc_f, (size_t)f, fs, fn);
    fn[NACC] = ws.cnt_f[f];
  });
  const int64_t kept = n[NACC];
  const double data = kept > 0 ? s[A_DATA] / (double)kept : 0.0;
  double reg = 0.0;
  for (int k = 0; k < DL_MAX_SCALES; ++k) {
    const double g = k < scales && n[A_G + k] > 0 ? s[A_G + k] / (double)n[A_G + k] : 0.0;
    out[8 + k] = g;
    out[12 + k] = (double)n[A_G + k];
    reg += g;
  }
  const double spatial = alpha > 0.0 ? data + alpha * reg : data;
  const double stable = n[A_TEMP] > 0 ? s[A_TEMP] / (double)n[A_TEMP] : 0.0;
  out[0] = spatial;
  out[1] = stable;
  out[2] = n[A_ABSREL] > 0 ? s[A_ABSREL] / (double)n[A_ABSREL] : 0.0;
  out[3] = kept > 0 ? (double)n[A_DATA] / (double)kept : 0.0;
  out[4] = stable_scale > 0.0 ? spatial + stable_scale * stable : spatial;
  out[5] = data;
  out[6] = reg;
  out[7] = (double)kept;
  out[16] = (double)n[A_TEMP];
  out[17] = (double)n[A_ABSREL];
  out[18] = (double)n[A_DATA];
  out[19] = 0.0;
}

// ------------------------------------------------------------------------------------------------ trimmed criterion
// vdn_depth_loss_trimmed: the untrimmed launch above runs first and leaves the fit, the medians, the deviation sums, g_k, d1
// and all counts, none of which trim changes. Then
//   prepare    one block: the per-frame scales once, and per term k = floor(n * keep) from the counts in out (on the device);
//   select     one set of all frames, three slots (data, stable, absRel), rank k - 1 each: the thresholds (select.hpp);
//   sums       per frame in DL_BPF blocks and per term: sum and count of the residuals below the threshold and of those at it;
//   finalise   one block: the fold of frame_sums.hpp, w = (k - n_less) / n_tied, the five values and out[20..39].
// The residuals are recomputed from the inputs by every pass (loss_px.hpp: the same expressions, so the same bits). One sweep
// that writes float32 key planes for the select's passes, and three selects of one slot, were measured and dropped (DESIGN
// 5.14, profiles/depth_loss_trim.md: 883 and 1209 against 824 us for the launch at [2, 32, 518, 518]).
constexpr int NTR = 2 * TR_TERMS;            // per term {below the threshold, at it}: a sum (double) and a count (integer)

struct Tw {  // the trimmed launch's own workspace, after the untrimmed one; in 8-byte slots
  double* fsc;      // [F][2] s of the aligned prediction, of the target
  uint32_t* rank;   // [3] (two slots)
  double* sum_b;    // [F][DL_BPF][NTR]
  int64_t* cnt_b;   // [F][DL_BPF][NTR]
  double* sum_f;    // [F][NTR]
  int64_t* cnt_f;   // [F][NTR]
  void* select;     // one set of three slots
  __host__ __device__ static size_t slots(size_t F) { return F * 2 + 2 + F * DL_BPF * 2 * NTR + F * 2 * NTR; }
  __host__ __device__ Tw(void* p, int B, int T) {
    const size_t F = (size_t)B * T, FB = F * DL_BPF;
    double* q = (double*)p;
    fsc = q, q += F * 2;
    rank = (uint32_t*)q, q += 2;
    sum_b = q, q += FB * NTR;
    cnt_b = (int64_t*)q, q += FB * NTR;
    sum_f = q, q += F * NTR;
    cnt_f = (int64_t*)q, q += F * NTR;
    select = q;
  }
};

// What a pass of the trimmed criterion knows about frame f, and the residuals of a lane's pixels.
struct TrimFrame {
  const float* pf;
  const float* tf;
  const uint8_t* mf;
  float sc, sh, th;
  double mp, sp, mt, st;
  int next;  // hw when the next frame belongs to the same item and the temporal term is on, else 0
  __device__ __forceinline__ TrimFrame(const float* pred, const float* target, const uint8_t* mask, int T, int hw, int temporal,
                                       const Ws& ws, const double* __restrict__ fsc, int f) {
    pf = pred + (size_t)f * hw, tf = target + (size_t)f * hw, mf = mask + (size_t)f * hw;
    sc = ws.ss[(f / T) * 2], sh = ws.ss[(f / T) * 2 + 1];
    mp = (double)ws.med[f * 2], mt = (double)ws.med[f * 2 + 1], sp = fsc[(size_t)f * 2], st = fsc[(size_t)f * 2 + 1];
    next = temporal && (f % T) + 1 < T ? hw : 0;
    th = next ? ws.th[f + 1] : 0.f;
  }
  // r[j][term] of pixels p0 .. p0 + PPL - 1; bit j * TR_TERMS + term of the result: the forward counts the pixel for the term
  template <int PPL>
  __device__ __forceinline__ uint32_t residuals(int p0, double (&r)[PPL][TR_TERMS]) const {
    const Px<PPL> q(pf, tf, mf, p0);
    const Px<PPL> qn(pf + next, tf + next, mf + next, p0);
    uint32_t on = 0;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      r[j][TR_DATA] = r[j][TR_STABLE] = r[j][TR_ABSREL] = 0.0;
      if (q.k[j]) {
        const float a = aligned(sc, q.p[j], sh), t = q.t[j];
        r[j][TR_DATA] = res_data(a, t, mp, sp, mt, st);
        on |= 1u << (j * TR_TERMS + TR_DATA);
        if (t > 1e-3f && t < 70.f) {
          r[j][TR_ABSREL] = res_absrel(a, t);
          on |= 1u << (j * TR_TERMS + TR_ABSREL);
        }
        if (next && qn.k[j]) {
          const float tg = qn.t[j] - t;
          if (fabsf(tg) < th) {
            r[j][TR_STABLE] = res_stable(aligned(sc, qn.p[j], sh) - a, tg);
            on |= 1u << (j * TR_TERMS + TR_STABLE);
          }
        }
      }
    }
    return on;
  }
};

#define TRIM_ARGS                                                                                                              \
  const float *__restrict__ pred, const float *__restrict__ target, const uint8_t *__restrict__ mask, int B, int T, int hw, \
      int temporal, void *__restrict__ workspace, void *__restrict__ trim_workspace

// the select's keys, recomputed from the inputs
template <int PPL>
struct TrimKey {
  static constexpr int SLOTS = TR_TERMS, PER = PPL;
  const float* pred;
  const float* target;
  const uint8_t* mask;
  int B, T, hw, temporal;
  void* workspace;
  void* trim_workspace;
  __device__ __forceinline__ uint32_t operator()(int f, size_t i, uint32_t (&key)[PPL][TR_TERMS]) const {
    const Ws ws(workspace, B, T);
    const Tw tw(trim_workspace, B, T);
    const TrimFrame fr(pred, target, mask, T, hw, temporal, ws, tw.fsc, f);
    double r[PPL][TR_TERMS];
    const uint32_t on = fr.residuals<PPL>((int)i, r);
#pragma unroll
    for (int j = 0; j < PPL; ++j)
#pragma unroll
      for (int k = 0; k < TR_TERMS; ++k) key[j][k] = trim_key(r[j][k]);
    return on;
  }
};

// One block. out[7], out[16] and out[17] are the counts the untrimmed finalise just wrote.
__global__ __launch_bounds__(256) void trim_prepare_kernel(void* __restrict__ workspace, void* __restrict__ trim_workspace, int B, int T,
                                                           double keep, double* __restrict__ out) {
  const Ws ws(workspace, B, T);
  const Tw tw(trim_workspace, B, T);
  const int F = B * T;
  for (int i = threadIdx.x; i < F * 2; i += 256) tw.fsc[i] = frame_scale(ws, i >> 1, i & 1);
  if (threadIdx.x < TR_TERMS) {
    const double n = out[threadIdx.x == TR_DATA ? 7 : (threadIdx.x == TR_STABLE ? 16 : 17)];
    const uint64_t k = (uint64_t)floor(n * keep);  // Python's int(n * (1.0 - trim)); n < 2^32 is exact in a double
    out[20 + 5 * threadIdx.x] = (double)k;
    tw.rank[threadIdx.x] = k ? (uint32_t)(k - 1) : 0u;
  }
}

template <int PPL>
__global__ __launch_bounds__(256) void trim_sum_kernel(TRIM_ARGS, const SelState* __restrict__ st) {
  const Ws ws(workspace, B, T);
  const Tw tw(trim_workspace, B, T);
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const TrimFrame fr(pred, target, mask, T, hw, temporal, ws, tw.fsc, f);
  const uint32_t thr[TR_TERMS] = {st[0].prefix, st[1].prefix, st[2].prefix};
  Tuple<double, NTR> acc;
  Tuple<int, NTR> cnt;
#pragma unroll
  for (int i = 0; i < NTR; ++i) acc.v[i] = 0.0, cnt.v[i] = 0;
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    double r[PPL][TR_TERMS];
    const uint32_t on = fr.residuals<PPL>(p0, r);
#pragma unroll
    for (int j = 0; j < PPL; ++j)
#pragma unroll
      for (int k = 0; k < TR_TERMS; ++k)
        if ((on >> (j * TR_TERMS + k)) & 1u) {
          const uint32_t key = trim_key(r[j][k]);
          if (key < thr[k]) acc.v[2 * k] += r[j][k], cnt.v[2 * k] += 1;
          else if (key == thr[k]) acc.v[2 * k + 1] += r[j][k], cnt.v[2 * k + 1] += 1;
        }
  }
  block_row<NTR, NTR>(acc, cnt, tw.sum_b, tw.cnt_b);
}

// One block: the fold of frame_sums.hpp; then the trimmed values over the untrimmed.
__global__ __launch_bounds__(256) void trim_finalise_kernel(void* __restrict__ trim_workspace, int B, int T, double alpha,
                                                            double stable_scale, const SelState* __restrict__ st,
                                                            double* __restrict__ out) {
  const Tw tw(trim_workspace, B, T);
  const int F = B * T;
  for (int f = threadIdx.x; f < F; f += 256) {
    double s[NTR];
    int64_t n[NTR];
    fold_blocks<NTR, NTR, DL_BPF>(tw.sum_b, tw.cnt_b, f, s, n);
    store_row<NTR, NTR>(tw.sum_f, tw.cnt_f, (size_t)f, s, n);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s[NTR];
  int64_t n[NTR];
  fold_frames<NTR, NTR>(tw.sum_f, tw.cnt_f, 0, F, s, n);
  const uint32_t thr[TR_TERMS] = {st[0].prefix, st[1].prefix, st[2].prefix};
  const double count[TR_TERMS] = {out[7], out[16], out[17]};
  double term[TR_TERMS];
  for (int i = 0; i < TR_TERMS; ++i) {
    double* tr = out + 20 + 5 * i;  // tr[0] = k, from the prepare kernel
    term[i] = 0.0, tr[1] = tr[2] = tr[3] = tr[4] = 0.0;
    if (tr[0] > 0.0) {              // k >= 1 means count >= 1 and at least one key at the threshold
      const double w = (tr[0] - (double)n[2 * i]) / (double)n[2 * i + 1];
      const double tied = w * s[2 * i + 1];
      term[i] = (s[2 * i] + tied) / count[i];
      tr[1] = (double)n[2 * i], tr[2] = (double)n[2 * i + 1], tr[3] = (double)__builtin_bit_cast(float, thr[i]), tr[4] = w;
    }
  }
  const double spatial = alpha > 0.0 ? term[TR_DATA] + alpha * out[6] : term[TR_DATA];
  out[0] = spatial;
  out[1] = term[TR_STABLE];
  out[2] = term[TR_ABSREL];
  out[4] = stable_scale > 0.0 ? spatial + stable_scale * term[TR_STABLE] : spatial;
  out[5] = term[TR_DATA];
  for (int i = 35; i < 40; ++i) out[i] = 0.0;
}

}  // namespace

extern "C" int vdn_depth_loss_trip(int wide) { return (int)(wide ? sweep_stride<DL_BPF, 4>() : sweep_stride<DL_BPF, 1>()); }

extern "C" size_t vdn_depth_loss_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return sizeof(double) * Ws::slots((size_t)B, (size_t)B * T) + select_workspace_bytes(B * T, 2);
}

// the errors of vdn_depth_loss, which the trimmed entry point shares; nothing is launched
static int depth_loss_check(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W, int scales,
                            double stable_scale, void* workspace, float* scale_shift, double* frame_stats, int64_t* frame_counts,
                            double* out) {
  if (!prediction || !target || !mask || !workspace || (!out && !scale_shift)) return VDN_EINVAL;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || scales < 0) return VDN_EINVAL;
  if (out && stable_scale > 0.0 && T < 2) return VDN_EINVAL;  // the reference divides by a count of zero strides
  if ((int64_t)H * W > INT32_MAX || (int64_t)B * T > 65535 || scales > DL_MAX_SCALES) return VDN_EUNSUPPORTED;
  if (misaligned(4, prediction, target, scale_shift) || misaligned(8, workspace, frame_stats, frame_counts, out)) return VDN_EALIGN;
  return VDN_OK;
}

extern "C" int vdn_depth_loss(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                              double alpha, int scales, double stable_scale, void* workspace, float* scale_shift,
                              double* frame_stats, int64_t* frame_counts, double* out, vdn_stream stream) {
  const int err = depth_loss_check(prediction, target, mask, B, T, H, W, scales, stable_scale, workspace, scale_shift, frame_stats,
                                   frame_counts, out);
  if (err != VDN_OK) return err;
  hipStream_t s = (hipStream_t)stream;
  const int F = B * T, hw = H * W;
  const dim3 grid((unsigned)F * DL_BPF), block(256);
  const Ws ws(workspace, B, T);
  with_ppl(wide_ok((size_t)hw, {prediction, target}, {mask}), [&](auto ppl) {
    constexpr int PPL = decltype(ppl)::value;
    hipLaunchKernelGGL(fit_partial_kernel<PPL>, grid, block, 0, s, prediction, target, mask, B, T, hw, workspace);
    hipLaunchKernelGGL(fit_solve_kernel, dim3(1), block, 0, s, workspace, B, T, frame_counts, scale_shift);
    if (!out) return;
    const uint32_t rank = (uint32_t)((hw - 1) / 2);  // torch.median: the lower of the two middle values
    select_launch(LossKey{prediction, target, mask, ws.ss, (size_t)hw, T}, F, 1, (size_t)hw, SelRanks<2>{{rank, rank}, nullptr}, ws.select, s);
    hipLaunchKernelGGL(median_store_kernel, dim3(grid_for((size_t)F * 2, 1024)), block, 0, s, select_state(ws.select, F, 2), F, ws.med);
    const int eff_scales = alpha > 0.0 ? scales : 0;  // the regulariser is skipped, as TrimmedProcrustesLoss skips it
    const int temporal = stable_scale > 0.0;
    hipLaunchKernelGGL(deviation_partial_kernel<PPL>, grid, block, 0, s, prediction, target, mask, B, T, hw, workspace);
    hipLaunchKernelGGL(loss_partial_kernel<PPL>, grid, block, 0, s, prediction, target, mask, B, T, H, W, eff_scales, temporal, workspace);
    hipLaunchKernelGGL(loss_finalise_kernel, dim3(1), block, 0, s, workspace, B, T, alpha, eff_scales, stable_scale, frame_stats, out);
  });
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" size_t vdn_depth_loss_trimmed_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return vdn_depth_loss_workspace_bytes(B, T) + sizeof(double) * Tw::slots((size_t)B * T) + select_workspace_bytes(1, TR_TERMS);
}

extern "C" int vdn_depth_loss_trimmed(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                                      double alpha, int scales, double stable_scale, double keep, void* workspace, float* scale_shift,
                                      double* frame_stats, int64_t* frame_counts, double* out, vdn_stream stream) {
  if (!out || !(keep > 0.0 && keep <= 1.0)) return VDN_EINVAL;  // a NaN fails both comparisons
  int err = depth_loss_check(prediction, target, mask, B, T, H, W, scales, stable_scale, workspace, scale_shift, frame_stats,
                             frame_counts, out);
  if (err != VDN_OK) return err;
  if ((uint64_t)B * T * (uint64_t)H * W > UINT32_MAX) return VDN_EUNSUPPORTED;  // the select's counters are 32-bit
  err = vdn_depth_loss(prediction, target, mask, B, T, H, W, alpha, scales, stable_scale, workspace, scale_shift, frame_stats,
                       frame_counts, out, stream);
  if (err != VDN_OK) return err;
  hipStream_t s = (hipStream_t)stream;
  const int F = B * T, hw = H * W, temporal = stable_scale > 0.0;
  const dim3 grid((unsigned)F * DL_BPF), block(256);
  void* tws = (char*)workspace + vdn_depth_loss_workspace_bytes(B, T);
  const Tw tw(tws, B, T);
  const SelState* st = select_state(tw.select, 1, TR_TERMS);
  hipLaunchKernelGGL(trim_prepare_kernel, dim3(1), block, 0, s, workspace, tws, B, T, keep, out);
  with_ppl(wide_ok((size_t)hw, {prediction, target}, {mask}), [&](auto ppl) {
    constexpr int PPL = decltype(ppl)::value;
    select_launch(TrimKey<PPL>{prediction, target, mask, B, T, hw, temporal, workspace, tws}, F, F, (size_t)hw,
                  SelRanks<TR_TERMS>{{0, 0, 0}, tw.rank}, tw.select, s);
    hipLaunchKernelGGL(trim_sum_kernel<PPL>, grid, block, 0, s, prediction, target, mask, B, T, hw, temporal, workspace, tws, st);
  });
  hipLaunchKernelGGL(trim_finalise_kernel, dim3(1), block, 0, s, tws, B, T, alpha, stable_scale, st, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
