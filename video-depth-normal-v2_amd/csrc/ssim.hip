// The SSIM term of the depth criterion on the device: the reference's DepthShallowSSIMLoss (loss/loss.py:296-323) with the
// weights [1, 0, 0, 0, 0] its VideoDepthLoss constructs it with, forward and the gradient with respect to the prediction.
// include/vdn.h (vdn_ssim_loss, vdn_ssim_loss_backward) states the arithmetic. The forward:
//   max        per frame in DL_BPF blocks: the largest kept aligned prediction and its lowest index, the largest kept target,
//              the lowest index of a dropped pixel
//   max solve  one block, a lane per item: max_val, who holds it and where
//   tile       one block per 16 x 32 tile of a frame's (H - 10) x (W - 10) outputs: x = a / max_val and y = t / max_val (the
//              reference's float32 division) staged in LDS with the halo, the five moments filtered along H into LDS and
//              along W into registers, cs = A / D per output, the tile's sums of cs and of (A - D) / D^2. No plane is written.
//   fold       a block per frame: the frame's tiles, a lane's in strides of 256 and the lanes as reduce.hpp states
//   finish     one block: the frames, in the same fixed order
// and the backward:
//   fit sums   (with a fit) the four masked sums of the fit, in the order loss_grad.hip sums them
//   tile       the forward's kernel again, which also leaves P = 1 / D, Q = A / D^2 and N = mu1 Q - mu2 P per output
//   fold       the forward's, over the tiles' sums of (A - D) / D^2
//   solve 1    one block, a lane per item: the term the item's holder receives
//   adjoint    one block per 16 x 32 tile of a frame's pixels: P, Q, N staged with the halo, filtered by the transposed
//              window along H into LDS and along W into registers; g_a into an fp64 plane, the tile's sums of g_a p and g_a
//   fold       the same over the adjoint's tiles
//   solve 2    one block: a lane per frame the fit's blocks, then a lane per item G0, G1 and the fit's determinant
//   write      g_p = sc g_a + keep * (fit correction) (loss_px.hpp), added to the prior gradient when asked, rounded once
// Everything from x and y on is fp64 with separate multiply and add roundings (contraction is off for this file); the taps are
// the eleven float32 values of the library's window widened to double, as literals. There are no atomics: a tile's sum has the
// order of reduce.hpp (a lane's two outputs, the wave's butterfly, the four waves), a frame's tiles are added by a block in
// that order too (one lane per frame and item walking every tile in turn was measured first: 1.4 and 1.6 ms of dependent loads
// in the two solves at [1, 32, 518, 518], against 0.2 ms for the stencil; profiles/ssim_loss.md), an item's frames in index
// order. Two runs give the same bits.
// LDS. The float tile is read with consecutive lanes on consecutive floats, the fp64 rows with consecutive lanes on consecutive
// doubles (a 32-lane half on the 64 banks that ds_read_b64 sees: conflict-free); a row of 42 doubles keeps the two halves of
// a wave on different rows. The forward's tile holds 2 x 26 x 42 floats and 5 x 16 x 42 doubles, 35.6 KB, the adjoint's
// 3 x (26 + 16) x 42 doubles, 42.3 KB: four and three blocks (sixteen and twelve waves) per CU.
#include "common.hpp"
#include "frame_sums.hpp"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)
#include "loss_px.hpp"

namespace {

constexpr int TH = 16, TW = 32;            // a tile's outputs (forward) or pixels (adjoint)
constexpr int HALO = 10;                   // window 11
constexpr int IH = TH + HALO, IW = TW + HALO;
constexpr double C2 = 0.03 * 0.03;
// torch.exp(-(k - 5)^2 / (2 * 1.5^2)) / sum in float32, k = 0 .. 10 (vdn.loss.SSIM_WINDOW)
__device__ constexpr double G[11] = {0x1.0d9570p-10, 0x1.f1fe02p-8, 0x1.26eb18p-5, 0x1.bff0fep-4, 0x1.b43c3ep-3, 0x1.106560p-2,
                                     0x1.b43c3ep-3, 0x1.bff0fep-4, 0x1.26eb18p-5, 0x1.f1fe02p-8, 0x1.0d9570p-10};
enum { H_PRED = 0, H_TARGET = 1, H_DROPPED = 2, H_CLAMP = 3, H_TIE = 4 };  // who holds an item's maximum (item_max[b][1])
enum { I_A01 = 0, I_A11, I_B0, I_B1, I_D, I_OK, I_G0, I_G1, I_HOLD, I_SLOTS };

__host__ __device__ inline int tiles_of(int h, int w) { return ((h + TH - 1) / TH) * ((w + TW - 1) / TW); }

// a float and the lowest index it was seen at; Best keeps the larger value and, among equal ones, the lower index
struct ValIdx {
  float v;
  int i;
};
struct BestOp {
  __device__ __forceinline__ ValIdx operator()(ValIdx a, ValIdx b) const { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
};
struct IntMinOp {
  __device__ __forceinline__ int operator()(int a, int b) const { return b < a ? b : a; }
};

// workspace of the forward, in 8-byte slots
struct Fw {
  ValIdx* pm_b;    // [F][DL_BPF] the largest kept aligned prediction of the block and its lowest index in the frame
  float* tm_b;     // [F][DL_BPF] the largest kept target (a slot each)
  int64_t* drop_b; // [F][DL_BPF] the lowest index of a dropped pixel, INT_MAX for none
  ValIdx* pm_f;    // [F] the same three per frame
  float* tm_f;     // [F]
  int64_t* drop_f; // [F]
  double* cs_f;    // [F][2] a frame's sums of cs and of (A - D) / D^2
  double* cs_b;    // [F][tiles][2] a tile's
  __host__ __device__ static size_t slots(size_t F, size_t tiles) { return F * DL_BPF * 3 + F * 5 + F * tiles * 2; }
  __host__ __device__ Fw(void* p, int F) {
    const size_t FB = (size_t)F * DL_BPF;
    double* q = (double*)p;
    pm_b = (ValIdx*)q, q += FB;
    tm_b = (float*)q, q += FB;
    drop_b = (int64_t*)q, q += FB;
    pm_f = (ValIdx*)q, q += F;
    tm_f = (float*)q, q += F;
    drop_f = (int64_t*)q, q += F;
    cs_f = q, q += (size_t)F * 2;
    cs_b = q;
  }
};

// ------------------------------------------------------------------------------------------------ the item's maximum
template <int PPL, bool VEC>
__global__ __launch_bounds__(256) void max_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, const float* __restrict__ ss, int T, int hw,
                                                          void* __restrict__ workspace) {
  const Fw ws(workspace, (int)(gridDim.x / DL_BPF));
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const float* pf = pred + (size_t)f * hw;
  const float* tf = target + (size_t)f * hw;
  const uint8_t* mf = mask + (size_t)f * hw;
  const float sc = ss ? ss[(f / T) * 2] : 1.f, sh = ss ? ss[(f / T) * 2 + 1] : 0.f;
  ValIdx pm = {-INFINITY, INT_MAX};
  float tm = -INFINITY;
  int drop = INT_MAX;
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL, VEC> q(pf, tf, mf, p0);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      if (q.k[j]) {
        const float a = ss ? aligned(sc, q.p[j], sh) : q.p[j];
        pm = BestOp{}(pm, ValIdx{a, p0 + j});
        tm = MaxOp{}(tm, q.t[j]);
      } else {
        drop = IntMinOp{}(drop, p0 + j);
      }
    }
  }
  __shared__ WaveSlots<ValIdx> rp;
  __shared__ WaveSlots<float> rt;
  __shared__ WaveSlots<int> rd;
  rp.put(pm, BestOp{});
  rt.put(tm, MaxOp{});
  rd.put(drop, IntMinOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    ws.pm_b[blockIdx.x] = rp.get(BestOp{});
    ws.tm_b[(size_t)blockIdx.x * 2] = rt.get(MaxOp{});
    ws.drop_b[blockIdx.x] = (int64_t)rd.get(IntMinOp{});
  }
}

// One block: a lane per frame takes the frame's blocks, then a lane per item its frames (the fold of frame_sums.hpp, for a
// maximum and two lowest indices, which no order changes). item_max[b] = {max_val, holder code, the weight of the prediction's
// path, the index in the item of the kept prediction that holds the prediction's maximum or -1}.
__global__ __launch_bounds__(256) void max_solve_kernel(void* __restrict__ workspace, int B, int T, int hw, double* __restrict__ item_max) {
  const Fw ws(workspace, B * T);
  for (int f = threadIdx.x; f < B * T; f += 256) {
    ValIdx pm = {-INFINITY, INT_MAX};
    float tm = -INFINITY;
    int64_t drop = INT_MAX;
    for (const size_t o : frame_blocks<DL_BPF>(f)) {
      pm = BestOp{}(pm, ws.pm_b[o]);  // a block's pixels are not a range of indices: among equal values the lower index wins
      tm = MaxOp{}(tm, ws.tm_b[o * 2]);
      drop = ws.drop_b[o] < drop ? ws.drop_b[o] : drop;
    }
    ws.pm_f[f] = pm, ws.tm_f[(size_t)f * 2] = tm, ws.drop_f[f] = drop;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) {
    float pm = -INFINITY, tm = -INFINITY;
    int64_t at = -1, drop = -1;
    for (int t = 0; t < T; ++t) {  // frames in index order: an equal value in a later frame has a higher index
      const int f = b * T + t;
      const ValIdx v = ws.pm_f[f];
      if (v.i != INT_MAX && (at < 0 || v.v > pm)) pm = v.v, at = (int64_t)t * hw + v.i;
      tm = MaxOp{}(tm, ws.tm_f[(size_t)f * 2]);
      if (drop < 0 && ws.drop_f[f] != INT_MAX) drop = (int64_t)t * hw + ws.drop_f[f];
    }
    // torch.max of prediction * mask: a dropped pixel is a 0 that takes part, and holds the maximum when it comes first
    bool kept_holds = at >= 0;
    if (drop >= 0) {
      if (!(pm >= 0.f)) kept_holds = false;
      else if (pm == 0.f) kept_holds = at < drop;
      pm = MaxOp{}(pm, 0.f);
      tm = MaxOp{}(tm, 0.f);
    }
    const float m = MaxOp{}(pm, tm);
    const float mv = MaxOp{}(m, 1e-8f);
    int code;
    double weight = 0.0;
    if (tm > pm) code = m < 1e-8f ? H_CLAMP : H_TARGET;
    else if (!kept_holds) code = H_DROPPED;  // a maximum of 0, which the clamp then raises: no gradient either way
    else if (m < 1e-8f) code = H_CLAMP;
    else if (tm == pm) code = H_TIE, weight = 0.5;
    else code = H_PRED, weight = 1.0;
    double* it = item_max + (size_t)b * 4;
    it[0] = (double)mv, it[1] = (double)code, it[2] = weight, it[3] = kept_holds ? (double)at : -1.0;
  }
}

// ------------------------------------------------------------------------------------------------ the tile
// x and y of pixel (yy, xx) of frame f, 0 outside the frame (such a value reaches no output that is summed)
struct Frame {
  const float* pf;
  const float* tf;
  int H, W;
  float sc, sh, mv;
  bool fit;
  __device__ Frame(const float* pred, const float* target, const float* __restrict__ ss, const double* __restrict__ item_max, int T,
                   int H_, int W_, int f) {
    H = H_, W = W_;
    pf = pred + (size_t)f * H * W, tf = target + (size_t)f * H * W;
    fit = ss != nullptr;
    sc = fit ? ss[(f / T) * 2] : 1.f, sh = fit ? ss[(f / T) * 2 + 1] : 0.f;
    mv = (float)item_max[(size_t)(f / T) * 4];
  }
  __device__ __forceinline__ float a_of(float p) const { return fit ? aligned(sc, p, sh) : p; }
  __device__ __forceinline__ float x_of(float p) const { return __fdiv_rn(a_of(p), mv); }
  __device__ __forceinline__ float y_of(float t) const { return __fdiv_rn(t, mv); }
};

// MAPS: also P, Q, N per output into maps [F][3][OH * OW] (the backward), and a frame that relu gates is skipped.
template <bool MAPS>
__global__ __launch_bounds__(256) void tile_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                   const float* __restrict__ ss, const double* __restrict__ item_max, int T, int H, int W,
                                                   int tiles_x, int tiles, double* __restrict__ cs_b, const double* __restrict__ frame_cs,
                                                   double* __restrict__ maps) {
  __shared__ float xs[IH * IW], ys[IH * IW];
  __shared__ double v[5][TH * IW];
  const int f = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  if (MAPS && !(frame_cs[f] > 0.0)) return;  // the whole block: no barrier is skipped by a part of it
  const int oy0 = (tile / tiles_x) * TH, ox0 = (tile % tiles_x) * TW, OH = H - HALO, OW = W - HALO;
  const Frame fr(pred, target, ss, item_max, T, H, W, f);
  for (int i = threadIdx.x; i < IH * IW; i += 256) {
    const int yy = oy0 + i / IW, xx = ox0 + i % IW;
    float xv = 0.f, yv = 0.f;
    if (yy < H && xx < W) {
      const size_t o = (size_t)yy * W + xx;
      xv = fr.x_of(fr.pf[o]), yv = fr.y_of(fr.tf[o]);
    }
    xs[i] = xv, ys[i] = yv;
  }
  __syncthreads();
  // along H: row r of the tile's outputs, column c of the staged tile
  for (int i = threadIdx.x; i < TH * IW; i += 256) {
    double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double xv = (double)xs[i + k * IW], yv = (double)ys[i + k * IW];
      m1 += G[k] * xv;
      m2 += G[k] * yv;
      e11 += G[k] * (xv * xv);
      e22 += G[k] * (yv * yv);
      e12 += G[k] * (xv * yv);
    }
    v[0][i] = m1, v[1][i] = m2, v[2][i] = e11, v[3][i] = e22, v[4][i] = e12;
  }
  __syncthreads();
  // along W: a lane's two outputs (r, c) and (r + 8, c)
  Tuple<double, 2> s = {{0.0, 0.0}};
  const int c = threadIdx.x % TW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = threadIdx.x / TW + half * (TH / 2);
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 11; ++l) {
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += G[l] * v[q][r * IW + c + l];
    }
    const int oy = oy0 + r, ox = ox0 + c;
    if (oy < OH && ox < OW) {
      const double A = 2.0 * (m[4] - m[0] * m[1]) + C2;
      const double D = (m[2] - m[0] * m[0]) + (m[3] - m[1] * m[1]) + C2;
      s.v[0] += A / D;
      s.v[1] += (A - D) / (D * D);
      if (MAPS) {
        double* mp = maps + (size_t)f * 3 * OH * OW + (size_t)oy * OW + ox;
        const double P = 1.0 / D, Q = A / (D * D);
        mp[0] = P;
        mp[(size_t)OH * OW] = Q;
        mp[(size_t)2 * OH * OW] = m[0] * Q - m[1] * P;
      }
    }
  }
  block_row<2>(s, cs_b);
}

// A block per frame: the frame's `rows` rows of ND sums (its tiles') into one row. A lane adds the rows lane, lane + 256, .. in
// this order, the lanes as reduce.hpp states. gate: frames whose gate[f] is not above 0 are left alone (the backward's gated
// frames, whose tiles were not written).
template <int ND>
__global__ __launch_bounds__(256) void frame_fold_kernel(const double* __restrict__ rows_in, int rows, const double* __restrict__ gate,
                                                         double* __restrict__ out) {
  const int f = blockIdx.x;
  if (gate && !(gate[f] > 0.0)) return;
  Tuple<double, ND> s;
  for (int i = 0; i < ND; ++i) s.v[i] = 0.0;
  for (int k = threadIdx.x; k < rows; k += 256)
    for (int i = 0; i < ND; ++i) s.v[i] += rows_in[((size_t)f * rows + k) * ND + i];
  block_row<ND>(s, out);
}

// One block: frame_cs, then the frames: a lane's in its stride order, the lanes as reduce.hpp states.
// out = {loss, mean relu(cs_f), gated frames, frames}.
__global__ __launch_bounds__(256) void finish_kernel(const double* __restrict__ cs_f, int F, double n_out, double* __restrict__ frame_cs,
                                                     double* __restrict__ out) {
  Tuple<double, 1> s = {{0.0}};
  Tuple<int, 1> gated = {{0}};
  for (int f = threadIdx.x; f < F; f += 256) {
    const double cs = cs_f[(size_t)f * 2] / n_out;
    frame_cs[f] = cs;
    if (cs > 0.0) s.v[0] += cs;
    else gated.v[0] += 1;
  }
  __shared__ WaveSlots<Tuple<double, 1>> rs;
  __shared__ WaveSlots<Tuple<int, 1>> rg;
  rs.put(s, SumOp{});
  rg.put(gated, SumOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mean = rs.get(SumOp{}).v[0] / (double)F;
    out[0] = 1.0 - mean, out[1] = mean, out[2] = (double)rg.get(SumOp{}).v[0], out[3] = (double)F;
  }
}

// ------------------------------------------------------------------------------------------------ the backward
struct Bw {
  double* fit_b;    // [F][DL_BPF][4] block sums p^2, p, p t, t over the kept pixels
  int64_t* cnt_b;   // [F][DL_BPF] kept pixels
  double* fit_f;    // [F][4] the same per frame
  int64_t* cnt_f;   // [F]
  double* cs_f;     // [F][2] as the forward's
  double* G_f;      // [F][2] a frame's sums g_a p, g_a
  double* cs_b;     // [F][tiles_out][2] as the forward's
  double* G_b;      // [F][tiles_in][2] a tile's sums g_a p, g_a
  double* item;     // [B][I_SLOTS]
  double* maps;     // [F][3][OH OW] P, Q, N
  double* plane;    // [F][H W] g_a
  __host__ __device__ static size_t slots(size_t B, size_t F, size_t t_out, size_t t_in, size_t n_out, size_t hw) {
    return F * DL_BPF * 5 + F * 9 + F * t_out * 2 + F * t_in * 2 + B * I_SLOTS + F * 3 * n_out + F * hw;
  }
  __host__ __device__ Bw(void* p, int B, int F, size_t t_out, size_t t_in, size_t n_out) {
    const size_t FB = (size_t)F * DL_BPF;
    double* q = (double*)p;
    fit_b = q, q += FB * 4;
    cnt_b = (int64_t*)q, q += FB;
    fit_f = q, q += (size_t)F * 4;
    cnt_f = (int64_t*)q, q += F;
    cs_f = q, q += (size_t)F * 2;
    G_f = q, q += (size_t)F * 2;
    cs_b = q, q += (size_t)F * t_out * 2;
    G_b = q, q += (size_t)F * t_in * 2;
    item = q, q += (size_t)B * I_SLOTS;
    maps = q, q += (size_t)F * 3 * n_out;
    plane = q;
  }
};

// the weight of frame f's cs_f in coeff * loss: -coeff / (F n_out) when relu passes it, else exactly nothing
__device__ __forceinline__ double frame_weight(const double* __restrict__ frame_cs, const float* __restrict__ coeff, int f, int F, double n_out) {
  return frame_cs[f] > 0.0 ? -(double)coeff[0] / ((double)F * n_out) : 0.0;
}

// the masked sums of the fit, as loss_grad.hip's first pass sums them again
template <int PPL, bool VEC>
__global__ __launch_bounds__(256) void fit_sums_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ mask, int hw, double* __restrict__ fit_b,
                                                       int64_t* __restrict__ cnt_b) {
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const float* pf = pred + (size_t)f * hw;
  const float* tf = target + (size_t)f * hw;
  const uint8_t* mf = mask + (size_t)f * hw;
  Tuple<double, 4> s = {{0.0, 0.0, 0.0, 0.0}};
  Tuple<int, 1> cnt = {{0}};
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const Px<PPL, VEC> q(pf, tf, mf, (int)q0);
#pragma unroll
    for (int j = 0; j < PPL; ++j)
      if (q.k[j]) {
        const double p = (double)q.p[j], t = (double)q.t[j];
        s.v[0] += p * p;
        s.v[1] += p;
        s.v[2] += p * t;
        s.v[3] += t;
        cnt.v[0] += 1;
      }
  }
  block_row<4, 1>(s, cnt, fit_b, cnt_b);
}

// One block, a lane per item: dL/dmax_val = -2 C2 sum_f w_f sum_o (A - D) / D^2 / max_val (the closed form of
// -sum_j (g_x x + g_y y)_j / max_val), times the weight of the prediction's path: what the holder receives.
__global__ __launch_bounds__(256) void hold_solve_kernel(void* __restrict__ workspace, int B, int T, int t_out, int t_in, double n_out,
                                                         const double* __restrict__ frame_cs, const double* __restrict__ item_max,
                                                         const float* __restrict__ coeff) {
  const Bw ws(workspace, B, B * T, (size_t)t_out, (size_t)t_in, (size_t)n_out);
  for (int b = threadIdx.x; b < B; b += 256) {
    double dm = 0.0;
    for (int t = 0; t < T; ++t) {
      const int f = b * T + t;
      const double w = frame_weight(frame_cs, coeff, f, B * T, n_out);
      if (w == 0.0) continue;  // a gated frame's tiles were not written, nor folded
      dm += w * ws.cs_f[(size_t)f * 2 + 1];
    }
    const double* im = item_max + (size_t)b * 4;
    ws.item[(size_t)b * I_SLOTS + I_HOLD] = im[2] != 0.0 ? im[2] * (-(2.0 * C2 * dm) / im[0]) : 0.0;
  }
}

__global__ __launch_bounds__(256) void adjoint_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      const float* __restrict__ ss, const double* __restrict__ item_max,
                                                      const double* __restrict__ frame_cs, const float* __restrict__ coeff, int B, int T,
                                                      int H, int W, int tiles_x, int t_out, int t_in, void* __restrict__ workspace) {
  __shared__ double ms[3][IH * IW];
  __shared__ double u[3][TH * IW];
  const int OH = H - HALO, OW = W - HALO, F = B * T;
  const Bw ws(workspace, B, F, (size_t)t_out, (size_t)t_in, (size_t)OH * OW);
  const int f = blockIdx.x / t_in, tile = blockIdx.x % t_in;
  const int iy0 = (tile / tiles_x) * TH, ix0 = (tile % tiles_x) * TW;
  const Frame fr(pred, target, ss, item_max, T, H, W, f);
  const double w = frame_weight(frame_cs, coeff, f, F, (double)OH * OW);  // the same for the whole block
  const double* im = item_max + (size_t)(f / T) * 4;
  const double mvd = im[0], hold = ws.item[(size_t)(f / T) * I_SLOTS + I_HOLD];
  const int64_t holder = im[2] != 0.0 ? (int64_t)im[3] - (int64_t)(f % T) * H * W : -1;  // in this frame's indices
  if (w != 0.0) {
    // outputs (iy0 - 10 + r, ix0 - 10 + c), zero outside the frame's outputs
    const double* mf = ws.maps + (size_t)f * 3 * OH * OW;
    for (int i = threadIdx.x; i < IH * IW; i += 256) {
      const int oy = iy0 - HALO + i / IW, ox = ix0 - HALO + i % IW;
      const bool in = oy >= 0 && oy < OH && ox >= 0 && ox < OW;
      const size_t o = in ? (size_t)oy * OW + ox : 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) ms[q][i] = in ? mf[(size_t)q * OH * OW + o] : 0.0;
    }
    __syncthreads();
    // along H: pixel row iy0 + r gathers the outputs iy0 + r - k, staged row r + 10 - k
    for (int i = threadIdx.x; i < TH * IW; i += 256) {
      double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 11; ++k) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a[q] += G[k] * ms[q][i + (HALO - k) * IW];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) u[q][i] = a[q];
    }
    __syncthreads();
  }
  Tuple<double, 2> s = {{0.0, 0.0}};
  const int c = threadIdx.x % TW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = threadIdx.x / TW + half * (TH / 2);
    const int iy = iy0 + r, ix = ix0 + c;
    if (iy < H && ix < W) {
      const size_t o = (size_t)iy * W + ix;
      const float p = fr.pf[o];
      double g = 0.0;
      if (w != 0.0) {
        double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int l = 0; l < 11; ++l) {
#pragma unroll
          for (int q = 0; q < 3; ++q) a[q] += G[l] * u[q][r * IW + c + HALO - l];
        }
        const double x = (double)fr.x_of(p), y = (double)fr.y_of(fr.tf[o]);
        g = (2.0 * w * ((y * a[0] - x * a[1]) + a[2])) / mvd;
      }
      if ((int64_t)o == holder) g += hold;
      ws.plane[(size_t)f * H * W + o] = g;
      s.v[0] += g * (double)p;
      s.v[1] += g;
    }
  }
  block_row<2>(s, ws.G_b);
}

// One block: a lane per frame folds the frame's blocks of the fit's sums, then a lane per item adds its frames' G0, G1 and fit
// sums in index order (frame_sums.hpp) and takes the determinant as the forward's solve does.
__global__ __launch_bounds__(256) void fit_solve_kernel(void* __restrict__ workspace, int B, int T, int t_out, int t_in, double n_out, int fit) {
  const Bw ws(workspace, B, B * T, (size_t)t_out, (size_t)t_in, (size_t)n_out);
  if (fit) {
    for (int f = threadIdx.x; f < B * T; f += 256) {
      double s[4];
      int64_t n;
      fold_blocks<4, 1, DL_BPF>(ws.fit_b, ws.cnt_b, f, s, &n);
      store_row<4, 1>(ws.fit_f, ws.cnt_f, (size_t)f, s, &n);
    }
    __syncthreads();
  }
  for (int b = threadIdx.x; b < B; b += 256) {
    double* it = ws.item + (size_t)b * I_SLOTS;
    double G[2];
    fold_frames<2, 0>(ws.G_f, nullptr, b * T, T, G, nullptr);
    it[I_G0] = G[0], it[I_G1] = G[1];
    if (!fit) continue;
    double s[4];
    int64_t n;
    fold_frames<4, 1>(ws.fit_f, ws.cnt_f, b * T, T, s, &n);
    const double a00 = s[0], a01 = s[1], b0 = s[2], b1 = s[3], a11 = (double)n, det = a00 * a11 - a01 * a01;
    it[I_A01] = a01, it[I_A11] = a11, it[I_B0] = b0, it[I_B1] = b1, it[I_D] = det + 1e-6, it[I_OK] = det != 0.0 ? 1.0 : 0.0;
  }
}

template <int PPL, bool VEC, bool ACC>
__global__ __launch_bounds__(256) void write_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                    const uint8_t* __restrict__ mask, const float* __restrict__ ss, int T, int hw,
                                                    const double* __restrict__ item, const double* __restrict__ plane,
                                                    float* __restrict__ grad) {
  const int f = blockIdx.x / DL_BPF, b = blockIdx.x % DL_BPF;
  const double* it = item + (size_t)(f / T) * I_SLOTS;
  const bool fit = ss != nullptr, ok = !fit || it[I_OK] != 0.0;
  FitGrad fg;
  if (fit) fg = FitGrad{it[I_A01], it[I_A11], it[I_B0], it[I_B1], it[I_D], it[I_G0], it[I_G1], (double)ss[(f / T) * 2], (double)ss[(f / T) * 2 + 1]};
  const float* pf = pred + (size_t)f * hw;
  const float* tf = target + (size_t)f * hw;
  const uint8_t* mf = mask + (size_t)f * hw;
  const double* gf = plane + (size_t)f * hw;
  float* out = grad + (size_t)f * hw;
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<DL_BPF, PPL>()) {
    const int p0 = (int)q0;
    const Px<PPL, VEC> q(pf, tf, mf, p0);
    float r[PPL];
    if (ACC) load_px<PPL, VEC>(out + p0, r);
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      double g = 0.0;
      if (ok) {
        g = gf[p0 + j];
        if (fit) g = q.k[j] ? fg(g, (double)q.p[j], (double)q.t[j]) : fg.sc * g;
      }
      r[j] = ACC ? (float)((double)r[j] + g) : (float)g;
    }
    store_px<PPL, VEC>(out + p0, r);
  }
}

int check(const float* prediction, const float* target, const uint8_t* mask, const float* scale_shift, int B, int T, int H, int W) {
  if (!prediction || !target || !mask) return VDN_EINVAL;
  if (B <= 0 || T <= 0 || H < HALO + 1 || W < HALO + 1) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX || (int64_t)B * T > 65535) return VDN_EUNSUPPORTED;
  if ((int64_t)B * T * tiles_of(H, W) > INT32_MAX) return VDN_EUNSUPPORTED;  // the tile kernels' grid
  if (misaligned(4, prediction, target, scale_shift)) return VDN_EALIGN;
  return VDN_OK;
}

}  // namespace

extern "C" int vdn_ssim_tile(int* th, int* tw) {
  if (!th || !tw) return VDN_EINVAL;
  *th = TH, *tw = TW;
  return VDN_OK;
}

extern "C" size_t vdn_ssim_loss_workspace_bytes(int B, int T, int H, int W) {
  if (B <= 0 || T <= 0 || H < HALO + 1 || W < HALO + 1) return 0;
  return sizeof(double) * Fw::slots((size_t)B * T, (size_t)tiles_of(H - HALO, W - HALO));
}

extern "C" int vdn_ssim_loss(const float* prediction, const float* target, const uint8_t* mask, const float* scale_shift, int B, int T,
                             int H, int W, void* workspace, double* out, double* frame_cs, double* item_max, vdn_stream stream) {
  if (const int rc = check(prediction, target, mask, scale_shift, B, T, H, W)) return rc;
  if (!workspace || !out || !frame_cs || !item_max) return VDN_EINVAL;
  if (misaligned(8, workspace, out, frame_cs, item_max)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int F = B * T, hw = H * W, OH = H - HALO, OW = W - HALO;
  const int tiles_x = (OW + TW - 1) / TW, tiles = tiles_of(OH, OW);
  const Fw ws(workspace, F);
  const dim3 block(256);
  with_ppl(wide_ok((size_t)hw, {prediction, target}, {mask}), [&](auto ppl) {
    constexpr int PPL = decltype(ppl)::value;
    hipLaunchKernelGGL((max_partial_kernel<PPL, PPL == 4>), dim3((unsigned)F * DL_BPF), block, 0, s, prediction, target, mask, scale_shift, T,
                       hw, workspace);
  });
  hipLaunchKernelGGL(max_solve_kernel, dim3(1), block, 0, s, workspace, B, T, hw, item_max);
  hipLaunchKernelGGL(tile_kernel<false>, dim3((unsigned)F * tiles), block, 0, s, prediction, target, scale_shift, item_max, T, H, W, tiles_x,
                     tiles, ws.cs_b, nullptr, nullptr);
  hipLaunchKernelGGL(frame_fold_kernel<2>, dim3((unsigned)F), block, 0, s, ws.cs_b, tiles, nullptr, ws.cs_f);
  hipLaunchKernelGGL(finish_kernel, dim3(1), block, 0, s, ws.cs_f, F, (double)OH * OW, frame_cs, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" size_t vdn_ssim_loss_backward_workspace_bytes(int B, int T, int H, int W) {
  if (B <= 0 || T <= 0 || H < HALO + 1 || W < HALO + 1) return 0;
  return sizeof(double) * Bw::slots((size_t)B, (size_t)B * T, (size_t)tiles_of(H - HALO, W - HALO), (size_t)tiles_of(H, W),
                                    (size_t)(H - HALO) * (W - HALO), (size_t)H * W);
}

extern "C" int vdn_ssim_loss_backward(const float* prediction, const float* target, const uint8_t* mask, const float* scale_shift, int B,
                                      int T, int H, int W, const double* out, const double* frame_cs, const double* item_max,
                                      const float* coeff, int accumulate, void* workspace, float* grad_prediction, vdn_stream stream) {
  if (const int rc = check(prediction, target, mask, scale_shift, B, T, H, W)) return rc;
  if (!workspace || !out || !frame_cs || !item_max || !coeff || !grad_prediction) return VDN_EINVAL;
  if (misaligned(4, coeff, grad_prediction) || misaligned(8, workspace, out, frame_cs, item_max)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int F = B * T, hw = H * W, OH = H - HALO, OW = W - HALO;
  const int t_out = tiles_of(OH, OW), t_in = tiles_of(H, W);
  const Bw ws(workspace, B, F, (size_t)t_out, (size_t)t_in, (size_t)OH * OW);
  const dim3 block(256), sweep((unsigned)F * DL_BPF);
  const bool quads = hw % 4 == 0;  // as loss_grad.hip: the sums' order depends on the shape alone
  const bool vec = wide_ok((size_t)hw, {prediction, target, grad_prediction}, {mask});
  auto sweeps = [&](auto ppl, auto v) {
    constexpr int PPL = decltype(ppl)::value;
    constexpr bool VEC = decltype(v)::value != 0;
    if (scale_shift)
      hipLaunchKernelGGL((fit_sums_kernel<PPL, VEC>), sweep, block, 0, s, prediction, target, mask, hw, ws.fit_b, ws.cnt_b);
    hipLaunchKernelGGL(tile_kernel<true>, dim3((unsigned)F * t_out), block, 0, s, prediction, target, scale_shift, item_max, T, H, W,
                       (OW + TW - 1) / TW, t_out, ws.cs_b, frame_cs, ws.maps);
    hipLaunchKernelGGL(frame_fold_kernel<2>, dim3((unsigned)F), block, 0, s, ws.cs_b, t_out, frame_cs, ws.cs_f);
    hipLaunchKernelGGL(hold_solve_kernel, dim3(1), block, 0, s, workspace, B, T, t_out, t_in, (double)OH * OW, frame_cs, item_max, coeff);
    hipLaunchKernelGGL(adjoint_kernel, dim3((unsigned)F * t_in), block, 0, s, prediction, target, scale_shift, item_max, frame_cs, coeff, B, T,
                       H, W, (W + TW - 1) / TW, t_out, t_in, workspace);
    hipLaunchKernelGGL(frame_fold_kernel<2>, dim3((unsigned)F), block, 0, s, ws.G_b, t_in, nullptr, ws.G_f);
    hipLaunchKernelGGL(fit_solve_kernel, dim3(1), block, 0, s, workspace, B, T, t_out, t_in, (double)OH * OW, scale_shift ? 1 : 0);
    with_bool(accumulate != 0, [&](auto acc) {
      hipLaunchKernelGGL((write_kernel<PPL, VEC, decltype(acc)::value>), sweep, block, 0, s, prediction, target, mask, scale_shift, T, hw,
                         ws.item, ws.plane, grad_prediction);
    });
  };
  if (vec) sweeps(IC<4>{}, IC<1>{});
  else with_ppl(quads, [&](auto ppl) { sweeps(ppl, IC<0>{}); });
  (void)out;  // the frames' number is B * T; the forward's values are not needed again
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
