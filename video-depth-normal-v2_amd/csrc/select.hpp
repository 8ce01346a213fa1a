// The exact three-pass radix select on order-preserving 32-bit keys, stated once: per frame, TWO selections run in the
// same passes (slot 0 and slot 1). A key functor gives the two keys of element i of frame f; the two requested ranks
// (0-based, in the sorted order of the slot's n keys) are the same for every frame.
//   vdn_frame_median (refine.hip)  one key per element, ranks floor and ceil of (n - 1) / 2: both middle order statistics;
//   vdn_depth_loss   (loss.hip)    slot 0 the aligned prediction, slot 1 the target, both under the mask, one rank.
// Passes take the top 11, the next 11 and the last 10 bits: a histogram per (frame, slot) of the keys that match the
// prefix decided so far (integer atomics, in LDS and then in `hist`: counts do not depend on the order, so two runs give
// the same bits), then a one-block scan that finds the bin holding the rank, extends the prefix and clears the bins. After
// select2_launch, st[f * 2 + slot].prefix is the selected key.
#pragma once
#include "common.hpp"

namespace {

constexpr int BITS0 = 11, BITS1 = 11, BITS2 = 10, NBIN = 2048;

__device__ __forceinline__ uint32_t ordered_key(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return __builtin_bit_cast(float, u);
}

struct SelState {  // per (frame, slot)
  uint32_t prefix;  // key bits decided so far (right-aligned)
  uint32_t k;       // remaining rank inside the prefix
};

// the plain sample: both slots select among the same keys
struct SampleKey {
  const float* x;
  size_t n;
  __device__ __forceinline__ void operator()(int f, size_t i, uint32_t& k0, uint32_t& k1) const {
    k0 = k1 = ordered_key(x[(size_t)f * n + i]);
  }
};

__global__ void select_init_kernel(SelState* st, uint32_t* hist, int F, uint32_t rank0, uint32_t rank1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < F * 2) {
    st[i].prefix = 0;
    st[i].k = (i & 1) ? rank1 : rank0;
  }
  for (size_t j = i; j < (size_t)F * 2 * NBIN; j += (size_t)gridDim.x * blockDim.x) hist[j] = 0;
}

// PASS 0: top 11 bits; PASS 1: next 11 among keys whose top 11 equal the prefix; PASS 2: last 10
template <int PASS, typename KeyFn>
__global__ __launch_bounds__(256) void select_hist_kernel(const KeyFn key_of, size_t n, const SelState* __restrict__ st,
                                                          uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[2][NBIN];
  const int f = blockIdx.y;
  for (int i = threadIdx.x; i < 2 * NBIN; i += 256) (&h[0][0])[i] = 0;
  __syncthreads();
  const uint32_t p[2] = {st[f * 2].prefix, st[f * 2 + 1].prefix};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    uint32_t key[2];
    key_of(f, i, key[0], key[1]);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint32_t bin, pre;
      if (PASS == 0) { bin = key[s] >> (32 - BITS0); pre = 0; }
      else if (PASS == 1) { bin = (key[s] >> BITS2) & ((1u << BITS1) - 1); pre = key[s] >> (BITS1 + BITS2); }
      else { bin = key[s] & ((1u << BITS2) - 1); pre = key[s] >> BITS2; }
      if (PASS == 0 || pre == p[s]) atomicAdd(&h[s][bin], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * NBIN; i += 256) {
    const uint32_t v = (&h[0][0])[i];
    if (v) atomicAdd(hist + (size_t)f * 2 * NBIN + i, v);
  }
}

// One block of 256 lanes per (frame, slot): find the bin holding rank k, extend the prefix, clear the bins. The bin is the
// first one whose inclusive running count exceeds k (the last bin if none does). Each lane sums its own run of bins, the
// lane whose run holds the rank walks it: the same bin and the same remaining rank as one lane walking all bins (which took
// a dependent load per bin, and most of the select's time), found by integer adds in any order.
template <int PASS>
__global__ __launch_bounds__(256) void select_scan_kernel(SelState* st, uint32_t* hist) {
  constexpr int NB = PASS == 2 ? (1 << BITS2) : NBIN, PER = NB / 256;
  uint32_t* h = hist + (size_t)blockIdx.x * NBIN;
  __shared__ uint32_t part[256];
  // Every lane reads the state BEFORE the barrier and one lane writes it after: a read placed after the barrier could see
  // the holder's write (another wave may be that far ahead), and a second lane would then take the reduced rank for its own.
  SelState s = st[blockIdx.x];
  uint32_t v[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) v[i] = h[threadIdx.x * PER + i], sum += v[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  uint32_t before = 0;
  for (int j = 0; j < (int)threadIdx.x; ++j) before += part[j];
  const bool holds = before <= s.k && s.k - before < sum;
  if (holds || (threadIdx.x == 255 && s.k - before >= sum && before <= s.k)) {
    uint32_t cum = before;
    int b = threadIdx.x * PER;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      b = threadIdx.x * PER + i;
      if (b == NB - 1 || cum + v[i] > s.k) break;
      cum += v[i];
    }
    s.k -= cum;
    s.prefix = (s.prefix << (PASS == 0 ? BITS0 : (PASS == 1 ? BITS1 : BITS2))) | (uint32_t)b;
    st[blockIdx.x] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NBIN; i += 256) h[i] = 0;
}

inline size_t select2_workspace_bytes(int frames) { return (size_t)frames * 2 * (NBIN * sizeof(uint32_t) + sizeof(SelState)); }
inline SelState* select2_state(void* workspace, int frames) { return (SelState*)((uint32_t*)workspace + (size_t)frames * 2 * NBIN); }

// n < 2^32 keys per frame; workspace of select2_workspace_bytes(frames), 4-byte aligned. Seven launches on s.
template <typename KeyFn>
inline void select2_launch(const KeyFn& key_of, int frames, size_t n, uint32_t rank0, uint32_t rank1, void* workspace, hipStream_t s) {
  uint32_t* hist = (uint32_t*)workspace;
  SelState* st = select2_state(workspace, frames);
  const dim3 grid(grid_for(n, 64), frames), scan(frames * 2), block(256);
  hipLaunchKernelGGL(select_init_kernel, dim3(grid_for((size_t)frames * 2 * NBIN, 1024)), block, 0, s, st, hist, frames, rank0, rank1);
  hipLaunchKernelGGL((select_hist_kernel<0, KeyFn>), grid, block, 0, s, key_of, n, st, hist);
  hipLaunchKernelGGL(select_scan_kernel<0>, scan, block, 0, s, st, hist);
  hipLaunchKernelGGL((select_hist_kernel<1, KeyFn>), grid, block, 0, s, key_of, n, st, hist);
  hipLaunchKernelGGL(select_scan_kernel<1>, scan, block, 0, s, st, hist);
  hipLaunchKernelGGL((select_hist_kernel<2, KeyFn>), grid, block, 0, s, key_of, n, st, hist);
  hipLaunchKernelGGL(select_scan_kernel<2>, scan, block, 0, s, st, hist);
}

}  // namespace
