// lane_attn_kernel — the one-query-per-lane attention, softmax(scale q k^T) v in fp32, behind both vdn_dn_attn (the grouped
// self-attention of the depth + normal head's TransformerBlocks, head dim 12 / 24 / 48 / 96) and vdn_hiera_attn (the
// mask-unit / global attention of every Hiera block, head dim 96, query max-pool fused on load). An MFMA version of this
// attention is the first thing to build for this model; it belongs here, once.
#include "common.hpp"

namespace {

// The L rows of a sequence inside the packed qkv [rows, 3C] (columns q | k | v, head h at columns h*DH.. of each) and the Lq
// rows of its result inside out [rows / qs, C]. Sequence (g1, g0), g0 < n0: element t is input row g1*s1 + g0*s0 + t*estride,
// query j is output row g1*os1 + g0*s0 + j*estride. With qs > 1, t = g*Lq + j and query j is the element-wise max of its qs
// elements (Hiera's query max-pool).
struct LaneAttnGeom {
  size_t s1, os1;
  int n0, s0, estride;
  int L, Lq, qs;   // keys, queries = L / qs, elements pooled into one query
};

constexpr int KT = 64;   // key rows per LDS tile

// One wave per (64 queries, head, sequence); SEQ_X puts the sequence on blockIdx.x and the query tile on blockIdx.z, else the
// other way round. Each lane owns one query row and keeps q, the output accumulator and the running (max, sum) of the online
// softmax in fp32 registers, so L is unbounded (3136 at level 0 of the head). Key / value tiles of 64 rows are staged in LDS as
// fp32 (hi + lo already summed in split mode) and every lane reads the same key row (an LDS broadcast). The head dim is a
// template argument, so 12 and 24 need no padding at all.
template <int DT, int DH, bool SEQ_X>
__global__ __launch_bounds__(64) void lane_attn_kernel(const typename Half<DT>::T* __restrict__ qkv,
                                                       const typename Half<DT>::T* __restrict__ qkv_lo,
                                                       typename Half<DT>::T* __restrict__ out, typename Half<DT>::T* __restrict__ out_lo,
                                                       int C, LaneAttnGeom g, float sl2) {
  __shared__ float ks[KT][DH];
  __shared__ float vs[KT][DH];
  const int lane = threadIdx.x;
  const int head = blockIdx.y;
  const int seq = SEQ_X ? blockIdx.x : blockIdx.z;
  const int qi = (SEQ_X ? blockIdx.z : blockIdx.x) * 64 + lane;
  const size_t off = (size_t)(seq % g.n0) * g.s0;
  const size_t base = (size_t)(seq / g.n0) * g.s1 + off;
  const size_t ld = 3 * (size_t)C;
  const bool active = qi < g.Lq;
  float q[DH], o[DH];
  {
    const int j = active ? qi : 0;
#pragma unroll
    for (int e = 0; e < DH; ++e) q[e] = -INFINITY;   // fmaxf(-inf, v) == v: qs = 1 loads q as it is
    for (int p = 0; p < g.qs; ++p) {
      const size_t r = (base + (size_t)(p * g.Lq + j) * g.estride) * ld + head * DH;
#pragma unroll
      for (int e = 0; e < DH; ++e) q[e] = fmaxf(q[e], load_half(qkv, qkv_lo, r + e));
    }
#pragma unroll
    for (int e = 0; e < DH; ++e) {
      q[e] *= sl2;   // scale and log2(e) folded into q: exp2 below
      o[e] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < g.L; k0 += KT) {
    const int nk = min(KT, g.L - k0);
    __syncthreads();
    for (int i = lane; i < nk * DH; i += 64) {
      const int j = i / DH, e = i - j * DH;
      const size_t r = (base + (size_t)(k0 + j) * g.estride) * ld + head * DH + e;
      ks[j][e] = load_half(qkv, qkv_lo, r + C);
      vs[j][e] = load_half(qkv, qkv_lo, r + 2 * C);
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
  const size_t r = ((size_t)(seq / g.n0) * g.os1 + off + (size_t)qi * g.estride) * C + head * DH;
#pragma unroll
  for (int e = 0; e < DH; ++e) store_half_nearest(out, out_lo, r + e, o[e] * inv);
}

template <int DT, int DH, bool SEQ_X>
bool launch_dh(const void* qkv, const void* qkv_lo, void* out, void* out_lo, int heads, int nseq, const LaneAttnGeom& g,
               float sl2, hipStream_t s) {
  using T = typename Half<DT>::T;
  const unsigned qtiles = (g.Lq + 63) / 64;
  const dim3 grid = SEQ_X ? dim3(nseq, heads, qtiles) : dim3(qtiles, heads, nseq);
  hipLaunchKernelGGL((lane_attn_kernel<DT, DH, SEQ_X>), grid, dim3(64), 0, s, (const T*)qkv, (const T*)qkv_lo, (T*)out, (T*)out_lo,
                     heads * DH, g, sl2);
  return true;
}

// the launch of both entry points, for the head dims DHS the caller instantiates; the caller has checked the grid limits
template <bool SEQ_X, int... DHS>
int lane_attn_launch(int dt, int dh, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int heads, int nseq,
                     const LaneAttnGeom& g, float scale, vdn_stream stream) {
  const float sl2 = scale * 1.44269504088896340736f;
  return with_half(dt, [&](auto t) -> int {
    if (!((dh == DHS && launch_dh<decltype(t)::value, DHS, SEQ_X>(qkv, qkv_lo, out, out_lo, heads, nseq, g, sl2, (hipStream_t)stream)) || ...))
      return VDN_EUNSUPPORTED;
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
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
  const LaneAttnGeom g{(size_t)s1, (size_t)s1, n0, s0, estride, L, L, 1};
  return lane_attn_launch<false, 12, 24, 48, 96>(dt, C / heads, qkv, qkv_lo, out, out_lo, heads, (int)nseq, g, scale, stream);
}

extern "C" int vdn_hiera_attn(int dt, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int frames, int heads, int W,
                              int Lkv, int q_stride, float scale, vdn_stream stream) {
  constexpr int DH = 96;   // head dim at every stage
  if (!qkv || !out || frames <= 0 || heads <= 0 || W <= 0 || Lkv <= 0 || q_stride <= 0 || Lkv % q_stride) return VDN_EINVAL;
  if ((qkv_lo == nullptr) != (out_lo == nullptr)) return VDN_EINVAL;
  const int64_t rows = (int64_t)frames * W * Lkv;
  if (rows * 3 * heads * DH > ((int64_t)1 << 40) || (int64_t)frames * W > 0x7fffffff || heads > 65535) return VDN_EUNSUPPORTED;
  const int Lq = Lkv / q_stride;
  if ((Lq + 63) / 64 > 65535) return VDN_EUNSUPPORTED;   // grid.z
  // token t of window w of frame f is row f*W*Lkv + t*W + w: sequence (f, w) with windows interleaved at stride 1
  const LaneAttnGeom g{(size_t)W * Lkv, (size_t)W * Lq, W, 1, W, Lkv, Lq, q_stride};
  return lane_attn_launch<true, DH>(dt, DH, qkv, qkv_lo, out, out_lo, heads, frames * W, g, scale, stream);
}
