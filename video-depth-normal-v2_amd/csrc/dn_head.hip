// Depth + normal model (models/video_depth_model.py:64-119, models/video_depth_head_v2_sangyu.py:17-317):
// the three kernels of its path that the shared GEMM / LayerNorm / resize kernels do not cover.
//   dn_attn_kernel      grouped 8-head self-attention of the head's TransformerBlocks, head dim 12 / 24 / 48 / 96
//   dn_prologue_kernel  trunk-feature sum + the .view reinterpretation + APE -> frame-major token rows
//   dn_tail_kernel      conv3x3 48->3 + bias, bilinear resize, residual / ReLU, normal assembly
#include "common.hpp"

namespace {

template <int DT> __device__ __forceinline__ float ld_h(const typename Half<DT>::T* p, size_t i) { return (float)p[i]; }

template <int DT>
__device__ __forceinline__ void st_split(typename Half<DT>::T* hi, typename Half<DT>::T* lo, size_t i, float v) {
  using TT = typename Half<DT>::T;
  const TT h = (TT)v;   // round to nearest; lo = nearest(v - hi): value = hi + lo to ~2^-21 (HL.from_float)
  hi[i] = h;
  if (lo) lo[i] = (TT)(v - (float)h);
}

// ------------------------------------------------------------------------------------------------------------------
// dn_attn_kernel — softmax(scale q k^T) v for every (sequence, head), q | k | v read from the packed in_proj rows.
// A sequence is L rows of the token matrix: element j of sequence (g1, g0) is row g1 * s1 + g0 * s0 + j * estride.
// One wave per (64 queries, sequence, head); each lane owns one query row and keeps q, the output accumulator and the
// running (max, sum) of the online softmax in fp32 registers, so L is unbounded (3136 at level 0). Key / value tiles of
// 64 rows are staged in LDS as fp32 (hi + lo already summed in split mode) and every lane reads the same key row
// (an LDS broadcast). The head dim is a template argument, so 12 and 24 need no padding at all.
constexpr int KT = 64;

template <int DT, int DH>
__global__ __launch_bounds__(64) void dn_attn_kernel(const typename Half<DT>::T* __restrict__ qkv,
                                                     const typename Half<DT>::T* __restrict__ qkv_lo,
                                                     typename Half<DT>::T* __restrict__ out, typename Half<DT>::T* __restrict__ out_lo,
                                                     int C, int L, int estride, int n0, int s0, int s1, float sl2) {
  __shared__ float ks[KT][DH];
  __shared__ float vs[KT][DH];
  const int lane = threadIdx.x;
  const int head = blockIdx.y;
  const int seq = blockIdx.z;
  const size_t base = (size_t)(seq / n0) * s1 + (size_t)(seq % n0) * s0;
  const size_t ld = 3 * (size_t)C;
  const int qi = blockIdx.x * 64 + lane;
  const bool active = qi < L;
  float q[DH], o[DH];
  {
    const size_t r = (base + (size_t)(active ? qi : 0) * estride) * ld + head * DH;
#pragma unroll
    for (int e = 0; e < DH; ++e) {
      float v = ld_h<DT>(qkv, r + e);
      if (qkv_lo) v += ld_h<DT>(qkv_lo, r + e);
      q[e] = v * sl2;   // scale and log2(e) folded into q: exp2 below
      o[e] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < L; k0 += KT) {
    const int nk = min(KT, L - k0);
    __syncthreads();
    for (int i = lane; i < nk * DH; i += 64) {
      const int j = i / DH, e = i - j * DH;
      const size_t r = (base + (size_t)(k0 + j) * estride) * ld + head * DH + e;
      float kv = ld_h<DT>(qkv, r + C), vv = ld_h<DT>(qkv, r + 2 * C);
      if (qkv_lo) {
        kv += ld_h<DT>(qkv_lo, r + C);
        vv += ld_h<DT>(qkv_lo, r + 2 * C);
      }
      ks[j][e] = kv;
      vs[j][e] = vv;
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < DH; ++e) s = fmaf(q[e], ks[j][e], s);
      if (s > m) {   // rescale the accumulator only when the running max moves
        const float c = exp2f(m - s);
        l *= c;
#pragma unroll
        for (int e = 0; e < DH; ++e) o[e] *= c;
        m = s;
      }
      const float p = exp2f(s - m);
      l += p;
#pragma unroll
      for (int e = 0; e < DH; ++e) o[e] = fmaf(p, vs[j][e], o[e]);
    }
  }
  if (!active) return;
  const float inv = 1.f / l;
  const size_t r = (base + (size_t)qi * estride) * C + head * DH;
#pragma unroll
  for (int e = 0; e < DH; ++e) st_split<DT>(out, out_lo, r + e, o[e] * inv);
}

template <int DT, int DH>
int attn_launch(const void* qkv, const void* qkv_lo, void* out, void* out_lo, int C, int heads, int L, int estride, int n0,
                int s0, int nseq, int s1, float sl2, hipStream_t s) {
  using TT = typename Half<DT>::T;
  dim3 grid((L + 63) / 64, heads, nseq);
  hipLaunchKernelGGL((dn_attn_kernel<DT, DH>), grid, dim3(64), 0, s, (const TT*)qkv, (const TT*)qkv_lo, (TT*)out, (TT*)out_lo,
                     C, L, estride, n0, s0, s1, sl2);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

template <int DT>
int attn_dispatch(int dh, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int C, int heads, int L, int estride,
                  int n0, int s0, int nseq, int s1, float sl2, hipStream_t s) {
  switch (dh) {
    case 12: return attn_launch<DT, 12>(qkv, qkv_lo, out, out_lo, C, heads, L, estride, n0, s0, nseq, s1, sl2, s);
    case 24: return attn_launch<DT, 24>(qkv, qkv_lo, out, out_lo, C, heads, L, estride, n0, s0, nseq, s1, sl2, s);
    case 48: return attn_launch<DT, 48>(qkv, qkv_lo, out, out_lo, C, heads, L, estride, n0, s0, nseq, s1, sl2, s);
    case 96: return attn_launch<DT, 96>(qkv, qkv_lo, out, out_lo, C, heads, L, estride, n0, s0, nseq, s1, sl2, s);
  }
  return VDN_EUNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------------------------
// dn_prologue_kernel — token[(f hw + p), c] = a[f][c hw + p] (+ b[f][c hw + p]) (+ ape[f % S][c]). Each frame's input
// is read as a flat [C, hw] array: for the trunk's NHWC buffers that IS the `.view(B, S, D, H, W)` of
// video_depth_model.py:101-103, for the head's own [B, S, C, h, w] input it is the layout itself. One thread per input
// element (coalesced reads), scattered 2- / 4-byte stores.
template <int DT>
__global__ __launch_bounds__(256) void dn_prologue_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ ape, int S, int C, int hw, size_t n,
                                                          float* __restrict__ out_f, typename Half<DT>::T* __restrict__ out_h,
                                                          typename Half<DT>::T* __restrict__ out_lo) {
  const size_t per = (size_t)C * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t f = i / per;
    const int r = (int)(i - f * per);
    const int c = r / hw, p = r - c * hw;
    float v = a[i];
    if (b) v += b[i];
    if (ape) v += ape[(size_t)(f % S) * C + c];
    const size_t o = (f * hw + p) * C + c;
    if (out_f) out_f[o] = v;
    if (out_h) st_split<DT>(out_h, out_lo, o, v);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// dn_tail_kernel — one thread per output pixel (f, y, x) of the (OH, OW) grid. The 3-channel conv3x3 (pad 1) of the f32
// NHWC map x [F, IH, IW, Cin] is evaluated at the 1 (no resize) or 4 (bilinear, align_corners) source pixels the output
// needs; weights and bias sit in LDS. Outputs: raw [F, 3, OH, OW] (the head's own result) and / or depth [F, OH, OW] =
// relu?(ch0 + depth_in?) with normal [F, 3, OH, OW] = (-ch1, -ch2, 1).
constexpr int TAIL_MAXC = 128;

__device__ __forceinline__ void conv3_at(const float* __restrict__ x, const float* w, int IH, int IW, int Cin, int y, int xx,
                                         float acc[3]) {
  for (int ky = 0; ky < 3; ++ky) {
    const int sy = y + ky - 1;
    if (sy < 0 || sy >= IH) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int sx = xx + kx - 1;
      if (sx < 0 || sx >= IW) continue;
      const float* px = x + ((size_t)sy * IW + sx) * Cin;
      const float* wt = w + (ky * 3 + kx) * 3 * Cin;   // LDS layout [tap][co][ci]
      for (int ci = 0; ci < Cin; ++ci) {
        const float v = px[ci];
        acc[0] = fmaf(wt[ci], v, acc[0]);
        acc[1] = fmaf(wt[Cin + ci], v, acc[1]);
        acc[2] = fmaf(wt[2 * Cin + ci], v, acc[2]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void dn_tail_kernel(const float* __restrict__ x, int F, int IH, int IW, int Cin,
                                                      const float* __restrict__ w, const float* __restrict__ bias, int OH, int OW,
                                                      const float* __restrict__ depth_in, int relu, float* __restrict__ raw,
                                                      float* __restrict__ depth, float* __restrict__ normal) {
  __shared__ float ws[9 * 3 * TAIL_MAXC];
  for (int i = threadIdx.x; i < 27 * Cin; i += 256) {   // w is [3, Cin, 3, 3] (nn.Conv2d) -> [tap][co][ci]
    const int tap = i / (3 * Cin), r = i - tap * 3 * Cin, co = r / Cin, ci = r - co * Cin;
    ws[i] = w[(co * Cin + ci) * 9 + tap];
  }
  __syncthreads();
  const size_t hw = (size_t)OH * OW, n = (size_t)F * hw;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i / hw);
  const int pix = (int)(i - (size_t)f * hw);
  const int oy = pix / OW, ox = pix - oy * OW;
  const float* xf = x + (size_t)f * IH * IW * Cin;
  float v[3] = {bias[0], bias[1], bias[2]};
  if (IH == OH && IW == OW) {
    float acc[3] = {0.f, 0.f, 0.f};
    conv3_at(xf, ws, IH, IW, Cin, oy, ox, acc);
    for (int c = 0; c < 3; ++c) v[c] += acc[c];
  } else {   // F.interpolate(bilinear, align_corners=True): src = dst * (in - 1) / (out - 1)
    const float ry = OH > 1 ? (float)(IH - 1) / (float)(OH - 1) : 0.f;
    const float rx = OW > 1 ? (float)(IW - 1) / (float)(OW - 1) : 0.f;
    const float sy = ry * oy, sx = rx * ox;
    const int y0 = min((int)sy, IH - 1), x0 = min((int)sx, IW - 1);
    const int y1 = min(y0 + 1, IH - 1), x1 = min(x0 + 1, IW - 1);
    const float wy = sy - y0, wx = sx - x0;
    float a00[3] = {0.f, 0.f, 0.f}, a01[3] = {0.f, 0.f, 0.f}, a10[3] = {0.f, 0.f, 0.f}, a11[3] = {0.f, 0.f, 0.f};
    conv3_at(xf, ws, IH, IW, Cin, y0, x0, a00);
    conv3_at(xf, ws, IH, IW, Cin, y0, x1, a01);
    conv3_at(xf, ws, IH, IW, Cin, y1, x0, a10);
    conv3_at(xf, ws, IH, IW, Cin, y1, x1, a11);
    for (int c = 0; c < 3; ++c) {   // the bias is constant over the source pixels and the weights sum to 1
      const float top = (1.f - wx) * a00[c] + wx * a01[c], bot = (1.f - wx) * a10[c] + wx * a11[c];
      v[c] += (1.f - wy) * top + wy * bot;
    }
  }
  if (raw) {
    for (int c = 0; c < 3; ++c) raw[((size_t)f * 3 + c) * hw + pix] = v[c];
  }
  if (depth) {
    float d = v[0];
    if (depth_in) d += depth_in[i];
    if (relu) d = fmaxf(d, 0.f);
    depth[i] = d;
    normal[((size_t)f * 3 + 0) * hw + pix] = -v[1];
    normal[((size_t)f * 3 + 1) * hw + pix] = -v[2];
    normal[((size_t)f * 3 + 2) * hw + pix] = 1.f;
  }
}

}  // namespace

extern "C" int vdn_dn_attn(int dt, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int rows, int C, int heads,
                           int L, int estride, int n0, int s0, int n1, int s1, float scale, vdn_stream stream) {
  if (!qkv || !out || rows <= 0 || C <= 0 || heads <= 0 || C % heads || L <= 0 || estride <= 0 || n0 <= 0 || s0 < 0 ||
      n1 <= 0 || s1 < 0)
    return VDN_EINVAL;
  if ((qkv_lo == nullptr) != (out_lo == nullptr)) return VDN_EINVAL;
  const int64_t last = (int64_t)(n1 - 1) * s1 + (int64_t)(n0 - 1) * s0 + (int64_t)(L - 1) * estride;
  if (last >= rows) return VDN_EINVAL;   // every row a sequence touches lies inside the [rows, 3C] / [rows, C] buffers
  const int64_t nseq = (int64_t)n0 * n1;
  if (nseq > 65535 || heads > 65535) return VDN_EUNSUPPORTED;   // grid.z / grid.y
  const int dh = C / heads;
  if (dh != 12 && dh != 24 && dh != 48 && dh != 96) return VDN_EUNSUPPORTED;
  if (dt != VDN_F16 && dt != VDN_BF16) return VDN_EUNSUPPORTED;
  const float sl2 = scale * 1.44269504088896340736f;
  hipStream_t s = (hipStream_t)stream;
  if (dt == VDN_F16) return attn_dispatch<VDN_F16>(dh, qkv, qkv_lo, out, out_lo, C, heads, L, estride, n0, s0, (int)nseq, s1, sl2, s);
  return attn_dispatch<VDN_BF16>(dh, qkv, qkv_lo, out, out_lo, C, heads, L, estride, n0, s0, (int)nseq, s1, sl2, s);
}

extern "C" int vdn_dn_prologue(int dt, const float* a, const float* b, int frames, int C, int hw, const float* ape, int S,
                               float* out_f, void* out_h, void* out_lo, vdn_stream stream) {
  if (!a || frames <= 0 || C <= 0 || hw <= 0 || (!out_f && !out_h) || (out_lo && !out_h)) return VDN_EINVAL;
  if (ape && S <= 0) return VDN_EINVAL;
  if (out_h && dt != VDN_F16 && dt != VDN_BF16) return VDN_EUNSUPPORTED;
  if (!ape) S = 1;
  const size_t n = (size_t)frames * C * hw;
  const int blocks = (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
  hipStream_t s = (hipStream_t)stream;
  if (dt == VDN_BF16)
    hipLaunchKernelGGL(dn_prologue_kernel<VDN_BF16>, dim3(blocks), dim3(256), 0, s, a, b, ape, S, C, hw, n, out_f,
                       (__bf16*)out_h, (__bf16*)out_lo);
  else
    hipLaunchKernelGGL(dn_prologue_kernel<VDN_F16>, dim3(blocks), dim3(256), 0, s, a, b, ape, S, C, hw, n, out_f,
                       (_Float16*)out_h, (_Float16*)out_lo);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_dn_tail(const float* x, int F, int IH, int IW, int Cin, const float* w, const float* bias, int OH, int OW,
                           const float* depth_in, int relu, float* raw, float* depth, float* normal, vdn_stream stream) {
  if (!x || !w || !bias || F <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return VDN_EINVAL;
  if (Cin <= 0 || Cin > TAIL_MAXC) return VDN_EUNSUPPORTED;
  if ((!depth) != (!normal) || (!raw && !depth) || (depth_in && !depth)) return VDN_EINVAL;
  const size_t n = (size_t)F * OH * OW;
  if ((n + 255) / 256 > 0x7fffffff) return VDN_EUNSUPPORTED;
  hipLaunchKernelGGL(dn_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, F, IH, IW, Cin, w,
                     bias, OH, OW, depth_in, relu, raw, depth, normal);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
