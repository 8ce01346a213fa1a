// The colourised depth output of the reference's front ends, made on the device:
//   run.py:59-71, run_video.py:75-89, metric_depth/run.py:67-78   per frame: min/max of the frame, 0..255, truncate to
//                                 uint8, matplotlib palette (or a grey triple), BGR, optionally [raw | 50 white | depth]
//   utils/dc_utils.py:72-86 (save_video)   one min/max for the clip, the inferno palette (or one grey channel), RGB
//   vdn_minmax_f32   two stages through the workspace, no atomics: two runs give the same bits
//   vdn_colorize     index = (uint8)(((d - mn) / (mx - mn)) * 255.0f), each operation rounded to fp32 on its own as numpy
//                    does on a float32 array; table lookup; optional hconcat with the raw frame
// Both are memory traffic: 4 B in per pixel, 1 to 6 B out.
#include "common.hpp"
#include "reduce.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {

// 16-byte vectors that promise 4-byte alignment only: gfx950 global loads of any width need dword alignment alone
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int MM_MAX_BPG = 256;   // most blocks (partials) per group: the workspace depends on the group count alone
constexpr int MM_VEC_PER_BLOCK = 256 * 4;   // a block is worth launching for 4 vectors per lane

// numpy's min / max: a NaN anywhere makes the result NaN. v_min_f32 / v_max_f32 drop NaNs, so the NaN is carried beside them.
// A tie between +0.0 and -0.0 returns whichever zero v_min / v_max give: the one case where the bits may differ from numpy's.
struct MinMax {
  float lo, hi;
  int nan;
  __device__ __forceinline__ void take(float v) {
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
    nan |= (v != v);
  }
};
struct MinMaxOp {
  __device__ __forceinline__ MinMax operator()(MinMax a, const MinMax& b) const {
    return MinMax{fminf(a.lo, b.lo), fmaxf(a.hi, b.hi), a.nan | b.nan};
  }
};

// Stage 1: block b of group g takes every bpg-th run of 256 aligned float4 of the group's interior; block 0 also takes the
// (at most 3 + 3) elements before the first and after the last 16-byte boundary. partial[g][b] = {min, max}, both NaN if
// the block saw one.
__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ x, size_t n, int bpg,
                                                             float* __restrict__ partial) {
  const int g = blockIdx.x / bpg, b = blockIdx.x % bpg;
  const float* p = x + (size_t)g * n;
  size_t head = (4 - (((uintptr_t)p >> 2) & 3)) & 3;   // elements before the first 16-byte boundary
  head = head < n ? head : n;
  const size_t nv = (n - head) >> 2, tail0 = head + 4 * nv;
  const f32x4* v = (const f32x4*)(p + head);
  MinMax m{INFINITY, -INFINITY, 0};
  for (size_t i = (size_t)b * 256 + threadIdx.x; i < nv; i += (size_t)bpg * 256) {
    const f32x4 q = v[i];
    m.take(q[0]), m.take(q[1]), m.take(q[2]), m.take(q[3]);
  }
  if (b == 0) {
    if (threadIdx.x < head) m.take(p[threadIdx.x]);
    if (tail0 + threadIdx.x < n) m.take(p[tail0 + threadIdx.x]);
  }
  __shared__ WaveSlots<MinMax> red;
  red.put(m, MinMaxOp{});
  __syncthreads();
  if (threadIdx.x == 0) {
    m = red.get(MinMaxOp{});
    float* o = partial + ((size_t)g * MM_MAX_BPG + b) * 2;
    o[0] = m.nan ? NAN : m.lo;
    o[1] = m.nan ? NAN : m.hi;
  }
}

// Stage 2: one wave per group over its bpg partials.
__global__ __launch_bounds__(64) void minmax_final_kernel(const float* __restrict__ partial, int bpg, float* __restrict__ out) {
  const int g = blockIdx.x;
  MinMax m{INFINITY, -INFINITY, 0};
  for (int b = threadIdx.x; b < bpg; b += 64) {
    const float* q = partial + ((size_t)g * MM_MAX_BPG + b) * 2;
    m.lo = fminf(m.lo, q[0]);   // a block without elements left (+inf, -inf): harmless
    m.hi = fmaxf(m.hi, q[1]);
    m.nan |= (q[0] != q[0]);
  }
  m = wave_reduce(m, MinMaxOp{});
  if (threadIdx.x == 0) {
    out[2 * g] = m.nan ? NAN : m.lo;
    out[2 * g + 1] = m.nan ? NAN : m.hi;
  }
}

inline int minmax_bpg(size_t n) {
  const size_t want = (n / 4 + MM_VEC_PER_BLOCK - 1) / MM_VEC_PER_BLOCK;
  return (int)(want < 1 ? 1 : want > MM_MAX_BPG ? MM_MAX_BPG : want);
}

// ---------------------------------------------------------------------------------------------------- colourise
// Palette index of a depth value. Subtract, divide and multiply round to fp32 one by one (no reciprocal, no contraction),
// the conversion truncates. Departures, where the reference casts a NaN or an out-of-range value to uint8 (undefined):
// mx == mn -> 0; outside [mn, mx] -> 0 / 255; NaN (d, or the scaled value) -> 0.
__device__ __forceinline__ unsigned palette_index(float d, float mn, float mx) {
  if (mx == mn) return 0u;
  const float t = __fmul_rn(__fdiv_rn(__fsub_rn(d, mn), __fsub_rn(mx, mn)), 255.0f);
  if (!(t > 0.0f)) return 0u;   // negative, zero or NaN
  if (t >= 255.0f) return 255u;
  return (unsigned)t;
}

// Position of an output pixel: row R counts the rows of all frames (frame f = R / H, kept as f and y), column c runs over
// the Wout = Wraw + margin + W pixels of an output row; Wraw = margin = 0 without a raw frame, where the output pixels are
// the depth pixels in order.
struct Pos {
  unsigned f, y, c;
  size_t R;
  __device__ __forceinline__ void next(unsigned Wout, unsigned H) {
    if (++c == Wout) {
      c = 0, ++R;
      if (++y == H) y = 0, ++f;
    }
  }
};

struct VisArgs {
  const float* depth;
  const float* minmax;
  const uint8_t* lut;
  const uint8_t* raw;
  uint8_t* out;
  size_t pixels;          // N * H * Wout
  unsigned H, W, Wout, left;   // left = Wraw + margin: the first depth column of an output row
  int per_frame;
};

template <int CH, bool RAW>
__device__ __forceinline__ unsigned one_pixel(const VisArgs& a, const Pos& q, const unsigned* __restrict__ pal) {
  if (RAW && q.c < a.W) {
    const uint8_t* r = a.raw + 3 * (q.R * a.W + q.c);
    return (unsigned)r[0] | ((unsigned)r[1] << 8) | ((unsigned)r[2] << 16);
  }
  if (RAW && q.c < a.left) return 0x00FFFFFFu;
  const float* mm = a.minmax + (a.per_frame ? 2 * (size_t)q.f : 0);
  return pal[palette_index(a.depth[q.R * a.W + (q.c - a.left)], mm[0], mm[1])];
}

// 4 pixels of CH bytes -> CH dwords, little endian
template <int CH>
__device__ __forceinline__ void store4(uint8_t* dst, const unsigned (&v)[4]) {
  unsigned* o = (unsigned*)dst;
  if (CH == 1) {
    o[0] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
    o[0] = v[0] | (v[1] << 24);
    o[1] = (v[1] >> 8) | (v[2] << 16);
    o[2] = (v[2] >> 16) | (v[3] << 8);
  }
}

template <int CH>
__device__ __forceinline__ void store_bytes(uint8_t* dst, unsigned v) {
#pragma unroll
  for (int k = 0; k < CH; ++k) dst[k] = (uint8_t)(v >> (8 * k));
}

// The output is one flat run of pixels * CH bytes. Pixel `first` (0..3, chosen by the host from the output address) is the
// first whose byte address is a multiple of 4; from there every 4 pixels are CH whole dwords, whatever rows and frames
// they fall in. A lane makes such groups of 4; the (at most 3 + 3) pixels before `first` and after the last whole group
// are written byte by byte by block 0. The palette sits in LDS, one dword per entry.
template <int CH, bool RAW>
__global__ __launch_bounds__(256) void colorize_kernel(VisArgs a, unsigned first, size_t groups) {
  __shared__ unsigned pal[256];
  {
    unsigned e = 0;
#pragma unroll
    for (int k = 0; k < CH; ++k) e |= (unsigned)a.lut[threadIdx.x * CH + k] << (8 * k);
    pal[threadIdx.x] = e;
  }
  __syncthreads();
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    const size_t p0 = first + 4 * g;
    Pos q;
    q.R = p0 / a.Wout;
    q.c = (unsigned)(p0 - q.R * a.Wout);
    q.f = (unsigned)(q.R / a.H);
    q.y = (unsigned)(q.R - (size_t)q.f * a.H);
    unsigned v[4];
    // four depth pixels that are neighbours in memory and share a min/max: inside one row, or, without a raw frame (the
    // depth map is then as flat as the output), anywhere short of a frame's last three rows
    const bool one_row = q.c >= a.left && q.c + 3 < a.Wout;
    if (one_row || (!RAW && (!a.per_frame || q.y + 3 < a.H))) {
      const f32x4_a4 d = *(const f32x4_a4*)(a.depth + q.R * a.W + (q.c - a.left));
      const float* mm = a.minmax + (a.per_frame ? 2 * (size_t)q.f : 0);
      const float mn = mm[0], mx = mm[1];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = pal[palette_index(d[k], mn, mx)];
    } else {   // a row end, the margin or the raw frame inside the group
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = one_pixel<CH, RAW>(a, q, pal);
        q.next(a.Wout, a.H);
      }
    }
    store4<CH>(a.out + p0 * CH, v);
  }
  if (blockIdx.x == 0 && threadIdx.x < 6) {
    const size_t tail0 = first + 4 * groups;
    const size_t p = threadIdx.x < 3 ? threadIdx.x : tail0 + (threadIdx.x - 3);
    if (threadIdx.x < 3 ? p < first : p < a.pixels) {
      Pos q;
      q.R = p / a.Wout;
      q.c = (unsigned)(p - q.R * a.Wout);
      q.f = (unsigned)(q.R / a.H);
      q.y = 0;   // not read by one_pixel
      store_bytes<CH>(a.out + p * CH, one_pixel<CH, RAW>(a, q, pal));
    }
  }
}

}  // namespace

extern "C" size_t vdn_minmax_workspace_bytes(int groups) {
  if (groups <= 0) return 0;
  return (size_t)groups * MM_MAX_BPG * 2 * sizeof(float);
}

extern "C" int vdn_minmax_f32(const float* x, int groups, size_t n, void* workspace, float* out, vdn_stream stream) {
  if (!x || !workspace || !out || groups <= 0 || n == 0) return VDN_EINVAL;
  if (groups > INT32_MAX / MM_MAX_BPG) return VDN_EINVAL;
  if (((uintptr_t)x & 3) || ((uintptr_t)workspace & 3) || ((uintptr_t)out & 3)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int bpg = minmax_bpg(n);
  hipLaunchKernelGGL(minmax_partial_kernel, dim3((unsigned)groups * bpg), dim3(256), 0, s, x, n, bpg, (float*)workspace);
  hipLaunchKernelGGL(minmax_final_kernel, dim3((unsigned)groups), dim3(64), 0, s, (const float*)workspace, bpg, out);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_colorize(const float* depth, const float* minmax, int per_frame, const uint8_t* lut, int ch,
                            const uint8_t* raw, int margin, uint8_t* out, int N, int H, int W, vdn_stream stream) {
  if (!depth || !minmax || !lut || !out || N <= 0 || H <= 0 || W <= 0) return VDN_EINVAL;
  if (ch != 1 && ch != 3) return VDN_EINVAL;
  if (raw && (ch != 3 || margin < 0)) return VDN_EINVAL;
  const size_t wout = raw ? 2 * (size_t)W + (size_t)margin : (size_t)W;
  if (wout > UINT32_MAX || (size_t)N * H > UINT32_MAX) return VDN_EUNSUPPORTED;
  if (((uintptr_t)depth & 3) || ((uintptr_t)minmax & 3)) return VDN_EALIGN;
  VisArgs a;
  a.depth = depth, a.minmax = minmax, a.lut = lut, a.raw = raw, a.out = out;
  a.pixels = (size_t)N * H * wout;
  a.H = (unsigned)H, a.W = (unsigned)W, a.Wout = (unsigned)wout, a.left = (unsigned)(wout - W);
  a.per_frame = per_frame != 0;
  // byte address of pixel p is out + ch * p: with ch = 3 it is a multiple of 4 for p = (out & 3), with ch = 1 for p = -out & 3
  size_t first = ch == 3 ? ((uintptr_t)out & 3) : ((4 - ((uintptr_t)out & 3)) & 3);
  first = first < a.pixels ? first : a.pixels;
  const size_t groups = (a.pixels - first) / 4;
  const unsigned grid = grid_for(groups, 4096);  // groups may be 0: block 0 still writes the loose pixels
  hipStream_t s = (hipStream_t)stream;
  if (ch == 1) hipLaunchKernelGGL((colorize_kernel<1, false>), dim3(grid), dim3(256), 0, s, a, (unsigned)first, groups);
  else if (!raw) hipLaunchKernelGGL((colorize_kernel<3, false>), dim3(grid), dim3(256), 0, s, a, (unsigned)first, groups);
  else hipLaunchKernelGGL((colorize_kernel<3, true>), dim3(grid), dim3(256), 0, s, a, (unsigned)first, groups);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
