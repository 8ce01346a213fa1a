// The batch preparation that the reference's scripts repeat between the loader and the model (scripts/train*.py and
// scripts/evaluate*.py: preprocess_rgb_sequences, preprocess_rgb_viz_sequences, preprocess_depth_sequences with its
// batch_wise_min_max_norm, and gt = 1. / torch.clamp(gt, min=1e-8)), on the device. include/vdn.h (vdn_prep_rgb,
// vdn_prep_depth) states it.
// Every operation is the reference's float32 operation, one IEEE rounding each: __fsub_rn and __fdiv_rn, and clamps written
// as comparisons so that a NaN stays a NaN (fmaxf / fminf would return the other operand). There is no multiply and no add
// next to one, so nothing can be contracted; contraction is off all the same.
// rgb      one launch: a lane clamps its elements and, when normalising, subtracts and divides by its channel's constants.
//          The channel is found per element, so a lane's elements may lie in two planes.
// depth    without the normalisation one launch. With it two: pass 1 leaves the (lo, hi, any) of each block's share of
//          the kept pixels in the workspace, PD_BPI partials per item; in pass 2 every block reduces its item's PD_BPI
//          partials itself, one per lane through the block reduction of reduce.hpp, and writes its share. Min and max are
//          exact in any order, so no order is promised. No finalise launch, no atomics. Pass 2 does not read the mask: the
//          result is written at every pixel, kept or not. 13 bytes per pixel cross the memory bus (4 + 1 read, 4 read, 4
//          written).
// A lane owns four consecutive elements (one 16-byte load and store, one 4-byte load of the mask) where the item's length is
// a multiple of 4 and the bases allow it, one element otherwise; the values do not depend on which. It issues the loads of
// several trips of the grid before it uses the first (sweep below).
#include "common.hpp"
#include "reduce.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int PD_BPI = 256;  // blocks per item (frame, for rgb): pass 2 reduces an item's partials one per lane

// torch.clamp(x, min = m), torch.clamp(x, max = m): a NaN fails the comparison and passes through
__device__ __forceinline__ float clamp_min(float x, float m) { return x < m ? m : x; }
__device__ __forceinline__ float clamp_max(float x, float m) { return x > m ? m : x; }
__device__ __forceinline__ float clamp01(float x) { return clamp_max(clamp_min(x, 0.f), 1.f); }

// reciprocal: the ground-truth line 1. / clamp(x, min = 1e-8); clamp0: the Lambda of preprocess_depth_sequences
template <bool RECIP, bool CLAMP0>
__device__ __forceinline__ float stage(float x) {
  if (RECIP) x = __fdiv_rn(1.f, clamp_min(x, 1e-8f));
  if (CLAMP0) x = clamp_min(x, 0.f);
  return x;
}

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
template <int PPL>
__device__ __forceinline__ void store_f(float* p, int i, const float (&v)[PPL]) {
  if (PPL == 4) *(f32x4*)(p + i) = f32x4{v[0], v[1 % PPL], v[2 % PPL], v[3 % PPL]};
  else p[i] = v[0];
}

// A lane's share of an item of n elements: the PPL elements at (b * 256 + lane) * PPL + k * trip, k = 0, 1, ..., trip =
// PD_BPI * 256 * PPL. The loads of PD_INFLIGHT trips are issued before the first is used: an item has only PD_BPI blocks, so
// at a small batch a compute unit holds a few waves and one load per lane in flight leaves the memory idle (measured,
// profiles/prep.md). body(i, v) gets the element index and the PPL values; it may store to i .. i + PPL - 1.
// rgb has a frame's worth of blocks per frame and many frames: two in flight keep its registers low.
constexpr int PD_INFLIGHT = 8, PD_INFLIGHT_RGB = 2;
template <int PPL, int INFLIGHT = PD_INFLIGHT, typename Body>
__device__ __forceinline__ void sweep(const float* xf, int b, int n, Body body) {
  const int64_t trip = (int64_t)PD_BPI * 256 * PPL;
  for (int64_t q0 = (int64_t)(b * 256 + (int)threadIdx.x) * PPL; q0 < n; q0 += trip * INFLIGHT) {
    float v[INFLIGHT][PPL];
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u)
      if (q0 + u * trip < n) load_f<PPL>(xf, (int)(q0 + u * trip), v[u]);
#pragma unroll
    for (int u = 0; u < INFLIGHT; ++u)
      if (q0 + u * trip < n) body((int)(q0 + u * trip), v[u]);
  }
}

// ------------------------------------------------------------------------------------------------ rgb
// in and out may be the same tensor: a lane reads its elements before it writes them, and nobody else touches them.
template <int PPL, bool NORM>
__global__ __launch_bounds__(256) void prep_rgb_kernel(const float* in, float* out, int hw) {
  const int f = blockIdx.x / PD_BPI, b = blockIdx.x % PD_BPI;
  const int n = 3 * hw;
  const float* xf = in + (size_t)f * n;
  float* of = out + (size_t)f * n;
  sweep<PPL, PD_INFLIGHT_RGB>(xf, b, n, [&](int i, float (&v)[PPL]) {
    int ch = i / hw, r = i - ch * hw;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      float c = clamp01(v[j]);
      if (NORM) {
        const float mean = ch == 0 ? 0.485f : ch == 1 ? 0.456f : 0.406f;
        const float sd = ch == 0 ? 0.229f : ch == 1 ? 0.224f : 0.225f;
        c = __fdiv_rn(__fsub_rn(c, mean), sd);
      }
      v[j] = c;
      if (++r == hw) r = 0, ++ch;  // the next element of the lane begins the next plane
    }
    store_f<PPL>(of, i, v);
  });
}

// ------------------------------------------------------------------------------------------------ depth
struct Partials {
  float* lo;      // [B][PD_BPI]
  float* hi;      // [B][PD_BPI]
  uint32_t* any;  // [B][PD_BPI]
  __host__ __device__ Partials(void* p, int B) {
    lo = (float*)p;
    hi = lo + (size_t)B * PD_BPI;
    any = (uint32_t*)(hi + (size_t)B * PD_BPI);
  }
};

template <int PPL, bool RECIP, bool CLAMP0>
__global__ __launch_bounds__(256) void prep_depth_stage_kernel(const float* in, float* out, int n) {
  const int it = blockIdx.x / PD_BPI, b = blockIdx.x % PD_BPI;
  const float* xf = in + (size_t)it * n;
  float* of = out + (size_t)it * n;
  sweep<PPL>(xf, b, n, [&](int i, float (&v)[PPL]) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) v[j] = stage<RECIP, CLAMP0>(v[j]);
    store_f<PPL>(of, i, v);
  });
}

template <int PPL, bool RECIP, bool CLAMP0>
__global__ __launch_bounds__(256) void prep_depth_partial_kernel(const float* __restrict__ in, const uint8_t* __restrict__ mask,
                                                                 int B, int n, void* __restrict__ workspace) {
  const Partials ws(workspace, B);
  const int it = blockIdx.x / PD_BPI, b = blockIdx.x % PD_BPI;
  const float* xf = in + (size_t)it * n;
  const uint8_t* mf = mask ? mask + (size_t)it * n : nullptr;
  float lo = INFINITY, hi = -INFINITY;
  uint32_t any = 0;
  sweep<PPL>(xf, b, n, [&](int i, float (&v)[PPL]) {
    uint32_t m = 0x01010101u;
    if (mf) m = PPL == 4 ? *(const uint32_t*)(mf + i) : (uint32_t)mf[i];
#pragma unroll
    for (int j = 0; j < PPL; ++j)
      if ((m >> (8 * j)) & 0xFFu) {  // a dropped pixel is skipped: nothing under it reaches lo or hi
        const float x = stage<RECIP, CLAMP0>(v[j]);
        lo = NanMinOp{}(lo, x);
        hi = NanMaxOp{}(hi, x);
        any = 1;
      }
  });
  __shared__ WaveSlots<float> rlo, rhi;
  __shared__ WaveSlots<uint32_t> rany;
  rlo.put(lo, NanMinOp{});
  rhi.put(hi, NanMaxOp{});
  rany.put(any, OrOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    ws.lo[blockIdx.x] = rlo.get(NanMinOp{});
    ws.hi[blockIdx.x] = rhi.get(NanMaxOp{});
    ws.any[blockIdx.x] = rany.get(OrOp{});
  }
}

template <int PPL, bool RECIP, bool CLAMP0>
__global__ __launch_bounds__(256) void prep_depth_norm_kernel(const float* in, float* out, int B, int n, const void* workspace,
                                                              float* minmax) {
  const Partials ws(const_cast<void*>(workspace), B);
  const int it = blockIdx.x / PD_BPI, b = blockIdx.x % PD_BPI;
  __shared__ WaveSlots<float> rlo, rhi;
  __shared__ WaveSlots<uint32_t> rany;
  rlo.put(ws.lo[(size_t)it * PD_BPI + threadIdx.x], NanMinOp{});  // the item's PD_BPI = 256 partials, one per lane
  rhi.put(ws.hi[(size_t)it * PD_BPI + threadIdx.x], NanMaxOp{});
  rany.put(ws.any[(size_t)it * PD_BPI + threadIdx.x], OrOp{});
  __syncthreads();
  const float lo = rlo.get(NanMinOp{}), hi = rhi.get(NanMaxOp{});
  const bool live = rany.get(OrOp{}) != 0;
  if (minmax && b == 0 && threadIdx.x == 0) minmax[it * 2] = lo, minmax[it * 2 + 1] = hi;
  const float d = clamp_min(__fsub_rn(hi, lo), 1e-8f);
  const float* xf = in + (size_t)it * n;
  float* of = out + (size_t)it * n;
  sweep<PPL>(xf, b, n, [&](int i, float (&v)[PPL]) {
#pragma unroll
    for (int j = 0; j < PPL; ++j)
      v[j] = live ? clamp01(__fdiv_rn(__fsub_rn(stage<RECIP, CLAMP0>(v[j]), lo), d)) : 0.f;  // no kept pixel: +0.0 everywhere
    store_f<PPL>(of, i, v);
  });
}

template <int PPL, bool RECIP, bool CLAMP0>
void launch_depth(const float* in, const uint8_t* mask, float* out, int B, int n, int normalize, void* workspace, float* minmax,
                  hipStream_t s) {
  const dim3 grid((unsigned)B * PD_BPI), block(256);
  if (!normalize) {
    hipLaunchKernelGGL((prep_depth_stage_kernel<PPL, RECIP, CLAMP0>), grid, block, 0, s, in, out, n);
    return;
  }
  hipLaunchKernelGGL((prep_depth_partial_kernel<PPL, RECIP, CLAMP0>), grid, block, 0, s, in, mask, B, n, workspace);
  hipLaunchKernelGGL((prep_depth_norm_kernel<PPL, RECIP, CLAMP0>), grid, block, 0, s, in, out, B, n, (const void*)workspace, minmax);
}

}  // namespace

static_assert(PD_BPI == 256, "pass 2 reads one partial per lane of a 256-lane block");

extern "C" int vdn_prep_trip(int wide) { return PD_BPI * 256 * (wide ? 4 : 1); }

extern "C" size_t vdn_prep_depth_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return (size_t)B * PD_BPI * (2 * sizeof(float) + sizeof(uint32_t));
}

extern "C" int vdn_prep_rgb(const float* in, float* out, int frames, int H, int W, int normalize, vdn_stream stream) {
  if (!in || !out) return VDN_EINVAL;
  if (frames <= 0 || H <= 0 || W <= 0) return VDN_EINVAL;
  if (3 * (int64_t)H * W > INT32_MAX || frames > 65535) return VDN_EUNSUPPORTED;
  if (((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int hw = H * W;
  const dim3 grid((unsigned)frames * PD_BPI), block(256);
  // four floats per lane when every plane of every frame starts on 16 bytes and holds whole quads
  const bool wide = hw % 4 == 0 && !((uintptr_t)in & 15) && !((uintptr_t)out & 15);
  if (normalize) {
    if (wide) hipLaunchKernelGGL((prep_rgb_kernel<4, true>), grid, block, 0, s, in, out, hw);
    else hipLaunchKernelGGL((prep_rgb_kernel<1, true>), grid, block, 0, s, in, out, hw);
  } else {
    if (wide) hipLaunchKernelGGL((prep_rgb_kernel<4, false>), grid, block, 0, s, in, out, hw);
    else hipLaunchKernelGGL((prep_rgb_kernel<1, false>), grid, block, 0, s, in, out, hw);
  }
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_prep_depth(const float* in, const uint8_t* mask, float* out, int B, int64_t n, int reciprocal, int clamp0,
                              int normalize, void* workspace, float* minmax, vdn_stream stream) {
  if (!in || !out || (normalize && !workspace)) return VDN_EINVAL;
  if (B <= 0 || n <= 0) return VDN_EINVAL;
  if (n > INT32_MAX || B > 65535) return VDN_EUNSUPPORTED;
  if (((uintptr_t)in & 3) || ((uintptr_t)out & 3) || ((uintptr_t)minmax & 3)) return VDN_EALIGN;
  if (normalize && ((uintptr_t)workspace & 7)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  // four floats per lane when every item starts on 16 bytes (its mask on 4) and holds whole quads
  const bool wide = n % 4 == 0 && !((uintptr_t)in & 15) && !((uintptr_t)out & 15) && !((uintptr_t)mask & 3);
  const int ni = (int)n;
#define VDN_PREP_GO(R, C)                                                                                   \
  do {                                                                                                      \
    if (wide) launch_depth<4, R, C>(in, mask, out, B, ni, normalize, workspace, minmax, s);                 \
    else launch_depth<1, R, C>(in, mask, out, B, ni, normalize, workspace, minmax, s);                      \
  } while (0)
  if (reciprocal && clamp0) VDN_PREP_GO(true, true);
  else if (reciprocal) VDN_PREP_GO(true, false);
  else if (clamp0) VDN_PREP_GO(false, true);
  else VDN_PREP_GO(false, false);
#undef VDN_PREP_GO
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
