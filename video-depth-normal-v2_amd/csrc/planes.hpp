// Output planes, written once: how fp32 values become the 16-bit hi / lo planes, the attention's e5m2 planes and the
// K-tile-major planes of the 8-bit GEMM. Used by the GEMM epilogues (gemm_kernels.hpp, gemm_x8.hip) and the element-wise
// producers of the same planes (norm.hip, pack.hip, tail.hip). The scalar pieces
// (split_rtz, split2_rtz, pk4_bf8, store_half*) are in common.hpp; include/vdn.h states the layouts for callers.
#pragma once
#include "common.hpp"

// ---- split: N values (a float array, or an f32x4 with N = 4, read in place) -> hi (toward zero) and lo (remainder) vectors
template <typename V> using plane_elem_t = std::remove_cv_t<std::remove_reference_t<decltype(V{}[0])>>;
template <int N, typename A, typename V>
__device__ __forceinline__ void split_n(const A& v, V& hi, V& lo) {
  static_assert(N % 2 == 0, "pairs");
#pragma unroll
  for (int e = 0; e < N; e += 2) {
    plane_elem_t<V> h0, h1, l0, l1;
    split2_rtz(v[e], v[e + 1], h0, h1, l0, l1);
    hi[e] = h0; hi[e + 1] = h1; lo[e] = l0; lo[e + 1] = l1;
  }
}
template <int N, typename V>
__device__ __forceinline__ void split_planes(const float (&v)[N], V& hi, V& lo) { split_n<N>(v, hi, lo); }
template <typename V>
__device__ __forceinline__ void split_planes(f32x4 a, V& hi, V& lo) { split_n<4>(a, hi, lo); }
// two accumulator groups -> one vector of 8 (a0: positions 0..3, a1: 4..7), a pair of each in turn
template <typename V>
__device__ __forceinline__ void split_planes(f32x4 a0, f32x4 a1, V& hi, V& lo) {
#pragma unroll
  for (int e = 0; e < 4; e += 2) {
    plane_elem_t<V> h0, h1, l0, l1;
    split2_rtz(a0[e], a0[e + 1], h0, h1, l0, l1);
    hi[e] = h0; hi[e + 1] = h1; lo[e] = l0; lo[e + 1] = l1;
    split2_rtz(a1[e], a1[e + 1], h0, h1, l0, l1);
    hi[4 + e] = h0; hi[5 + e] = h1; lo[4 + e] = l0; lo[5 + e] = l1;
  }
}
// the lo plane is optional: split, or hi alone rounded to NEAREST (lo is then left unset)
template <typename V>
__device__ __forceinline__ void split_or_round(bool split, f32x4 a, V& hi, V& lo) {
  if (split) return split_planes(a, hi, lo);
#pragma unroll
  for (int e = 0; e < 4; ++e) hi[e] = (plane_elem_t<V>)a[e];
}

// ---- store: the hi vector and the lo vector at one offset; a null lo plane is skipped
template <typename T, typename V>
__device__ __forceinline__ void store_planes(T* hi, T* lo, size_t o, const V& h, const V& l) {
  *(V*)(hi + o) = h;
  if (lo) *(V*)(lo + o) = l;
}
// the same for a GEMM's own output planes (LO_OPTIONAL = false: the flavour has p.out_lo by contract, no test)
template <bool LO_OPTIONAL = true, typename T, typename V>
__device__ __forceinline__ void store_out_planes(const vdn_gemm_desc& p, size_t o, const V& h, const V& l) {
  *(V*)((T*)p.out + o) = h;
  if (!LO_OPTIONAL || p.out_lo) *(V*)((T*)p.out_lo + o) = l;
}

// ---- K-tile-major planes (include/vdn.h: a_kt / out_kt): what the 8-bit cross-term GEMM reads per K step is contiguous.
//   16-bit plane: [N / 32][M][32] halves            6-bit rows: [N / 64][M][64] bytes, a row-slab = two 32-byte halves
// and row-major ([M][ld], the same bytes per row) when kt == 0. Producers and the consuming GEMM agree through these two.
// Offset in halves of column n of row m:
__device__ __forceinline__ size_t kt_half_offset(int kt, size_t m, int n, int M, int ld) {
  return kt ? ((size_t)(n >> 5) * M + m) * 32 + (n & 31) : m * ld + n;
}
// Offset in bytes of half `half` (0 / 1) of the row-slab that starts at column n64 (a multiple of 64) of row m:
__device__ __forceinline__ size_t kt_byte_offset(int kt, size_t m, int n64, int half, int M, int ld) {
  return (kt ? ((size_t)(n64 >> 6) * M + m) * 64 : m * ld + n64) + 32 * half;
}

// ---- the attention's e5m2 planes (include/vdn.h: dst8): N values as N bytes of e5m2(value) and, 64 bytes on, N bytes of
// e5m2(remainder * 2^10); `lo` holds the remainders of the fp16 split of v. pack_bf8 / pack_bf8_lo make the dwords, store_bf8 writes them.
template <int N, typename A>
__device__ __forceinline__ void pack_bf8(const A& v, uint32_t (&hi8)[N / 4]) {
#pragma unroll
  for (int q = 0; q < N / 4; ++q) hi8[q] = pk4_bf8(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
template <int N, typename V>
__device__ __forceinline__ void pack_bf8_lo(const V& lo, uint32_t (&lo8)[N / 4]) {
  const float k = VDN_LO8_SCALE;
#pragma unroll
  for (int q = 0; q < N / 4; ++q)
    lo8[q] = pk4_bf8(k * (float)lo[4 * q], k * (float)lo[4 * q + 1], k * (float)lo[4 * q + 2], k * (float)lo[4 * q + 3]);
}
template <int N, typename A, typename V>
__device__ __forceinline__ void store_bf8(uint8_t* d8, const A& v, const V& lo) {
  typedef uint32_t W __attribute__((ext_vector_type(N / 4)));
  uint32_t d[N / 4];
  W w;
  pack_bf8<N>(v, d);
#pragma unroll
  for (int q = 0; q < N / 4; ++q) w[q] = d[q];
  *(W*)d8 = w;
  pack_bf8_lo<N>(lo, d);
#pragma unroll
  for (int q = 0; q < N / 4; ++q) w[q] = d[q];
  *(W*)(d8 + 64) = w;
}

// ---- output tail of the generic GEMM stores (PLAIN / CONVT / GEGLU): 4 columns at offset o as f32, as split planes, or as
// the hi plane alone rounded to nearest. The split is element by element (the same bits as in pairs): in pairs the generic
// kernels allocate other registers (gemm_kernel<128, 32>: 66 -> 74 VGPRs).
template <int DT>
__device__ __forceinline__ void store_out4(const vdn_gemm_desc& p, size_t o, f32x4 a) {
  using T = typename Half<DT>::T;
  typename Half<DT>::V4 h, l;
  if (p.out_dt == VDN_F32) {
    *(f32x4*)((float*)p.out + o) = a;
  } else if (p.out_lo) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { T x0, x1; split_rtz(a[e], x0, x1); h[e] = x0; l[e] = x1; }
    store_out_planes<false, T>(p, o, h, l);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (T)a[e];
    *(typename Half<DT>::V4*)((T*)p.out + o) = h;
  }
}
