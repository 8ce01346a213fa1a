// The skeleton of the criteria (loss, loss_grad, normals, normals_grad, eval, metric), stated once: which pixels of a frame a
// lane owns and in which order it visits them, how a lane loads and stores them, the row a block leaves of its sums, the
// order in which one block folds those rows, and the host's choice between four pixels per lane and one.
// The ORDER OF EVERY SUM of these units is this header's and reduce.hpp's ("two runs give the same bits", include/vdn.h):
//   a lane      its pixels in the order of its sweep: p0 = (b * 256 + lane) * PPL + k * BPF * 256 * PPL, k = 0, 1, ...
//               (sweep_first, sweep_stride), and within a visit p0, p0 + 1, .., p0 + PPL - 1;
//   a block     the wave's butterfly and (w0 + w1) + (w2 + w3), as reduce.hpp states them (block_row);
//   a frame     its BPF blocks in index order (frame_blocks, fold_blocks);
//   the frames  in index order (fold_frames), all of them or an item's.
// A row is ND doubles and NI counts widened to int64_t; blocks and frames leave rows of the same form.
// Like reduce.hpp this header holds adds and index arithmetic only, and must never hold a multiply that feeds an add: the
// units include it under their own contraction mode, and the bits must not depend on where it is included. Its loops over a
// row's ND or NI members and a lane's PPL pixels have constant trip counts and are unrolled without being asked to.
#pragma once
#include "common.hpp"
#include "reduce.hpp"
#include <initializer_list>

// ------------------------------------------------------------------------------------------------ a lane's pixels
// A lane's visits to the n pixels of a frame that BPF blocks share, b the block's index in the frame: the pixels q0, q0 + 1, ..,
// q0 + PPL - 1 for q0 = sweep_first<PPL>(b); q0 < n; q0 += sweep_stride<BPF, PPL>(). The kernels write this `for` themselves, so
// that the loop's body is compiled as part of the kernel (profiles/criteria_refactor.md has what the other shapes cost).
template <int PPL>
__device__ __forceinline__ int64_t sweep_first(int b) {
  return (int64_t)(b * 256 + (int)threadIdx.x) * PPL;
}
template <int BPF, int PPL>
__host__ __device__ constexpr int64_t sweep_stride() {
  return (int64_t)BPF * 256 * PPL;
}

// (y, x) of pixel p0 in rows of W, and the step to the next pixel of the frame
struct RowWalk {
  int y, x;
  __device__ __forceinline__ RowWalk(int p0, int W) : y(p0 / W), x(p0 - (p0 / W) * W) {}
  __device__ __forceinline__ void step(int W) {
    if (++x == W) x = 0, ++y;
  }
};

// PPL consecutive floats at p: 4 or 1. VEC: the four by one 16-byte load (p must allow it); otherwise a load each.
template <int PPL, bool VEC = (PPL == 4)>
__device__ __forceinline__ void load_px(const float* __restrict__ p, float (&v)[PPL]) {
  static_assert(!VEC || PPL == 4, "the vector load takes four pixels");
  if (VEC) {
    const f32x4 q = *(const f32x4*)p;
    for (int j = 0; j < PPL; ++j) v[j] = q[j];
  } else {
    for (int j = 0; j < PPL; ++j) v[j] = p[j];
  }
}
// the PPL mask bytes at m, the first in the low byte. VEC: one 4-byte load.
template <int PPL, bool VEC = (PPL == 4)>
__device__ __forceinline__ uint32_t load_mask(const uint8_t* __restrict__ m) {
  if (VEC) return *(const uint32_t*)m;
  uint32_t r = 0;
  for (int j = 0; j < PPL; ++j) r |= (uint32_t)m[j] << (8 * j);
  return r;
}
__device__ __forceinline__ uint32_t mask_byte(uint32_t m, int j) { return (m >> (8 * j)) & 0xFFu; }
template <int PPL, bool VEC = (PPL == 4)>
__device__ __forceinline__ void store_px(float* __restrict__ p, const float (&v)[PPL]) {
  if (VEC) {
    *(f32x4*)p = f32x4{v[0], v[1 % PPL], v[2 % PPL], v[3 % PPL]};
  } else {
    for (int j = 0; j < PPL; ++j) p[j] = v[j];
  }
}

// ------------------------------------------------------------------------------------------------ a block's row
// A row is ND sums and NI counts. The rows of a pass lie in two dense arrays, sums[row][ND] (double) and counts[row][NI], not
// joined in one: the lanes of a one-block fold, one per frame, then lie half as far apart (profiles/criteria_refactor.md).
// Every lane of the block calls block_row with its own sums, ONCE PER KERNEL (its LDS slots belong to the instantiation, so a
// second call of the same one would reuse them across two barriers): row blockIdx.x gets the block's. It holds the block's
// single __syncthreads(): a kernel that reduces something else as well (a minimum, an index) puts it in a WaveSlots of its own before
// the call and gets it after. NI == 0: no counts, and c and counts are not looked at.
template <int ND, int NI>
__device__ __forceinline__ void block_row(const Tuple<double, ND>& s, const Tuple<int, (NI > 0 ? NI : 1)>& c, double* __restrict__ sums,
                                          int64_t* __restrict__ counts) {
  __shared__ WaveSlots<Tuple<double, ND>> rs;
  __shared__ WaveSlots<Tuple<int, (NI > 0 ? NI : 1)>> rc;
  rs.put(s, SumOp{});
  if (NI > 0) rc.put(c, SumOp{});
  __syncthreads();
  if (threadIdx.x != 0) return;
  const Tuple<double, ND> r = rs.get(SumOp{});
  for (int i = 0; i < ND; ++i) sums[(size_t)blockIdx.x * ND + i] = r.v[i];
  if (NI > 0) {
    const Tuple<int, (NI > 0 ? NI : 1)> n = rc.get(SumOp{});
    for (int i = 0; i < NI; ++i) counts[(size_t)blockIdx.x * NI + i] = (int64_t)n.v[i];
  }
}
template <int ND>
__device__ __forceinline__ void block_row(const Tuple<double, ND>& s, double* __restrict__ sums) {
  block_row<ND, 0>(s, Tuple<int, 1>{{0}}, sums, nullptr);
}

// s[ND], n[NI] = row o; row o = s[ND], n[NI]; s[ND], n[NI] += row o (counts and n are not looked at when NI == 0)
template <int ND, int NI>
__device__ __forceinline__ void load_row(const double* __restrict__ sums, const int64_t* __restrict__ counts, size_t o, double* s, int64_t* n) {
  for (int i = 0; i < ND; ++i) s[i] = sums[o * ND + i];
  for (int i = 0; i < NI; ++i) n[i] = counts[o * NI + i];
}
template <int ND, int NI>
__device__ __forceinline__ void store_row(double* __restrict__ sums, int64_t* __restrict__ counts, size_t o, const double* s, const int64_t* n) {
  for (int i = 0; i < ND; ++i) sums[o * ND + i] = s[i];
  for (int i = 0; i < NI; ++i) counts[o * NI + i] = n[i];
}
template <int ND, int NI>
__device__ __forceinline__ void add_row(const double* __restrict__ sums, const int64_t* __restrict__ counts, size_t o, double* s, int64_t* n) {
  for (int i = 0; i < ND; ++i) s[i] += sums[o * ND + i];
  for (int i = 0; i < NI; ++i) n[i] += counts[o * NI + i];
}

// ------------------------------------------------------------------------------------------------ the one-block fold
// o = at, at + 1, .. below stop: what `for (const size_t o : frame_blocks<BPF>(f))` walks
struct RowRange {
  size_t at, stop;
  struct End {};
  __device__ __forceinline__ RowRange begin() const { return *this; }
  __device__ __forceinline__ End end() const { return End{}; }
  __device__ __forceinline__ bool operator!=(End) const { return at < stop; }
  __device__ __forceinline__ void operator++() { ++at; }
  __device__ __forceinline__ size_t operator*() const { return at; }
};
// the rows o = f * BPF + b of frame f's blocks, b = 0 .. BPF - 1 in this order
template <int BPF>
__device__ __forceinline__ RowRange frame_blocks(int f) {
  return RowRange{(size_t)f * BPF, (size_t)f * BPF + BPF};
}
// s[ND], n[NI] = the sums of frame f's BPF rows, in index order. A kernel that folds something else over the same blocks (a
// minimum, an index) walks frame_blocks itself and calls add_row.
template <int ND, int NI, int BPF>
__device__ __forceinline__ void fold_blocks(const double* __restrict__ sums, const int64_t* __restrict__ counts, int f, double* s, int64_t* n) {
  for (int i = 0; i < ND; ++i) s[i] = 0.0;
  for (int i = 0; i < NI; ++i) n[i] = 0;
  for (const size_t o : frame_blocks<BPF>(f)) add_row<ND, NI>(sums, counts, o, s, n);
}
// s[ND], n[NI] = the sums over the frames f0 .. f0 + count - 1 in index order, where row(f, fs, fn) gives frame f's sums
// (a stored row, a fold_blocks, or a stored row with a count from elsewhere beside it: one walk, so one load latency per
// frame); for lane 0 over all frames, or for one lane per item over the item's
template <int ND, int NI, typename Row>
__device__ __forceinline__ void fold_frames(int f0, int count, double* s, int64_t* n, Row row) {
  for (int i = 0; i < ND; ++i) s[i] = 0.0;
  for (int i = 0; i < NI; ++i) n[i] = 0;
  for (int f = f0; f < f0 + count; ++f) {
    double fs[ND];
    int64_t fn[NI > 0 ? NI : 1];
    row(f, fs, fn);
    for (int i = 0; i < ND; ++i) s[i] += fs[i];
    for (int i = 0; i < NI; ++i) n[i] += fn[i];
  }
}
// the same over rows that a fold_blocks per frame stored (store_row)
template <int ND, int NI>
__device__ __forceinline__ void fold_frames(const double* __restrict__ sums, const int64_t* __restrict__ counts, int f0, int count, double* s,
                                            int64_t* n) {
  fold_frames<ND, NI>(f0, count, s, n, [&](int f, double* fs, int64_t* fn) { load_row<ND, NI>(sums, counts, (size_t)f, fs, fn); });
}

// ------------------------------------------------------------------------------------------------ the host side
// is any of the pointers off a multiple of `bytes` (a power of two); a null pointer is not
template <typename... P>
inline bool misaligned(uintptr_t bytes, P... ptrs) {
  return (... || (((uintptr_t)ptrs & (bytes - 1)) != 0));
}
// Four pixels per lane with vector loads and stores: runs of n pixels that are whole quads, every float plane on 16 bytes,
// every mask on 4. Null pointers are allowed (a plane the call does not have or does not load by quads).
inline bool wide_ok(size_t n, std::initializer_list<const void*> floats, std::initializer_list<const void*> masks = {}) {
  bool ok = n % 4 == 0;
  for (const void* p : floats) ok = ok && !misaligned(16, p);
  for (const void* p : masks) ok = ok && !misaligned(4, p);
  return ok;
}
// A run-time choice as a template argument of what the generic lambda f launches. Pixels per lane: f(IC<4>) or f(IC<1>).
template <typename F>
inline void with_ppl(bool wide, F&& f) {
  if (wide) f(IC<4>{});
  else f(IC<1>{});
}
// a flag: f(std::true_type) or f(std::false_type)
template <typename F>
inline void with_bool(bool c, F&& f) {
  if (c) f(std::true_type{});
  else f(std::false_type{});
}
