// The fixed-order reduction of a 256-lane block (4 waves of 64), stated once. The order is part of the contract of the
// kernels that use it (include/vdn.h: "two runs give the same bits"):
//   within a wave    the xor butterfly, lane distance 32, 16, 8, 4, 2, 1: v = op(v, value of lane ^ o); every lane ends
//                    with the wave's result;
//   across the waves lane 0 of each wave writes its slot in LDS, the CALLER places one __syncthreads(), then
//                    (w0 op w1) op (w2 op w3).
// A value is a scalar or a small struct of 32-bit words whose members op combines one by one (Tuple below, or a kernel's
// own): the members then go through the butterfly in lockstep, one round trip per step for all of them, and each member
// keeps exactly the order above. For min, max and or any order gives the same value (they are exact; v_min / v_max may
// pick either zero of a +0.0 / -0.0 tie); for sums this association is the result. Several WaveSlots may be put under one
// barrier: a kernel that reduces doubles and ints still has a single __syncthreads() between its puts and its gets.
// This header holds adds, min, max and or only, and must never hold a multiply that feeds an add: it is compiled under each
// unit's default contraction mode, before the `#pragma clang fp contract(off)` of the units that turn contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

template <typename T, int N>
struct Tuple {
  T v[N];
};

struct SumOp {
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
  template <typename T, int N> __device__ __forceinline__ Tuple<T, N> operator()(Tuple<T, N> a, const Tuple<T, N>& b) const {
#pragma unroll
    for (int k = 0; k < N; ++k) a.v[k] = a.v[k] + b.v[k];
    return a;
  }
};

// Minimum and maximum that keep a NaN, as torch.min / torch.max and numpy's do: once either side is a NaN the result is one,
// whatever the order. Written as comparisons (v_min / v_max and fminf / fmaxf return the other operand instead).
struct NanMinOp {
  __device__ __forceinline__ float operator()(float a, float b) const { return (b < a || b != b) ? b : a; }
};
struct NanMaxOp {
  __device__ __forceinline__ float operator()(float a, float b) const { return (b > a || b != b) ? b : a; }
};
struct OrOp {
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; }
};

template <typename T>
__device__ __forceinline__ T shfl_xor_words(T v, int o) {
  static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "a value of whole 32-bit words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = __shfl_xor(w[i], o);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, shfl_xor_words(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) { return wave_reduce(v, SumOp{}); }

// One value of type T per wave of a 256-lane block; declare it __shared__. put() is called by every lane of the block,
// get() after the caller's __syncthreads() by whichever lanes need the total.
template <typename T>
struct WaveSlots {
  T s[4];
  template <typename Op>
  __device__ __forceinline__ void put(T v, Op op) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  }
  template <typename Op>
  __device__ __forceinline__ T get(Op op) const {
    return op(op(s[0], s[1]), op(s[2], s[3]));
  }
};
