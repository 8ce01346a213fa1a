// The exact three-pass radix select on order-preserving 32-bit keys, stated once. A SET is `group` consecutive frames whose
// elements are selected among together; per set, SLOTS selections run in the same passes. A key functor states
//   static constexpr int SLOTS   selections per set;
//   static constexpr int PER     consecutive elements of a frame it takes per call (n must be a multiple of PER);
//   uint32_t operator()(int f, size_t i, uint32_t (&key)[PER][SLOTS]) const
//                                the keys of elements i .. i + PER - 1 of frame f; bit e * SLOTS + s of the result says that
//                                element i + e takes part in slot s. An element that does not is skipped: it has no key.
// The requested ranks (0-based, in the sorted order of the slot's keys) are the same for every set; they are given by value
// or read from device memory when the select starts (SelRanks), so a rank may be the result of an earlier kernel.
//   vdn_frame_median       (refine.hip)  a set per frame, one key per element, ranks floor and ceil of (n - 1) / 2;
//   vdn_depth_loss         (loss.hip)    a set per frame, slot 0 the aligned prediction, slot 1 the target, one rank;
//   vdn_depth_loss_trimmed (loss.hip)    one set of all frames, slots data / stable / absRel, ranks computed on the device.
// A caller whose ranks differ from set to set writes the states itself and starts select_passes:
//   vdn_normal_angle_stats (normal_metrics.hip)  frames, items and the batch as three selects over one plane, each set's
//                                        ranks floor and ceil of (m - 1) / 2 among its own m keys, written by its fold kernel.
// Passes take the top 11, the next 11 and the last 10 bits: a histogram per (set, slot) of the keys that match the prefix
// decided so far (integer atomics, in LDS and then in `hist`: counts do not depend on the order, so two runs give the same
// bits), then a one-block scan that finds the bin holding the rank, extends the prefix and clears the bins. After
// select_launch, st[set * SLOTS + slot].prefix is the selected key. A slot with fewer keys than its rank + 1 ends on its last
// bin; its prefix means nothing.
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

struct SelState {  // per (set, slot)
  uint32_t prefix;  // key bits decided so far (right-aligned)
  uint32_t k;       // remaining rank inside the prefix
};

template <int SLOTS>
struct SelRanks {
  uint32_t host[SLOTS];  // used when dev == nullptr
  const uint32_t* dev;   // [SLOTS] in device memory, read by the select's first kernel
};

template <int SLOTS>
__global__ void select_init_kernel(SelState* st, uint32_t* hist, int sets, SelRanks<SLOTS> ranks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < sets * SLOTS) {
    st[i].prefix = 0;
    st[i].k = ranks.dev ? ranks.dev[i % SLOTS] : ranks.host[i % SLOTS];
  }
  for (size_t j = i; j < (size_t)sets * SLOTS * NBIN; j += (size_t)gridDim.x * blockDim.x) hist[j] = 0;
}

// PASS 0: top 11 bits; PASS 1: next 11 among keys whose top 11 equal the prefix; PASS 2: last 10
template <int PASS, typename KeyFn>
__global__ __launch_bounds__(256) void select_hist_kernel(const KeyFn key_of, size_t n, int group, const SelState* __restrict__ st,
                                                          uint32_t* __restrict__ hist) {
  constexpr int S = KeyFn::SLOTS, E = KeyFn::PER;
  static_assert(S * E <= 32, "one bit per (element, slot)");
  __shared__ uint32_t h[S][NBIN];
  const int f = blockIdx.y, set = f / group;
  for (int i = threadIdx.x; i < S * NBIN; i += 256) (&h[0][0])[i] = 0;
  __syncthreads();
  uint32_t p[S];
#pragma unroll
  for (int s = 0; s < S; ++s) p[s] = st[set * S + s].prefix;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * E; i < n; i += (size_t)gridDim.x * 256 * E) {
    uint32_t key[E][S];
    const uint32_t on = key_of(f, i, key);
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        uint32_t bin, pre;
        if (PASS == 0) { bin = key[e][s] >> (32 - BITS0); pre = 0; }
        else if (PASS == 1) { bin = (key[e][s] >> BITS2) & ((1u << BITS1) - 1); pre = key[e][s] >> (BITS1 + BITS2); }
        else { bin = key[e][s] & ((1u << BITS2) - 1); pre = key[e][s] >> BITS2; }
        if (((on >> (e * S + s)) & 1u) && (PASS == 0 || pre == p[s])) atomicAdd(&h[s][bin], 1u);
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S * NBIN; i += 256) {
    const uint32_t v = (&h[0][0])[i];
    if (v) atomicAdd(hist + (size_t)set * S * NBIN + i, v);
  }
}

// One block of 256 lanes per (set, slot): find the bin holding rank k, extend the prefix, clear the bins. The bin is the
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

inline size_t select_workspace_bytes(int sets, int slots) { return (size_t)sets * slots * (NBIN * sizeof(uint32_t) + sizeof(SelState)); }
__host__ __device__ inline SelState* select_state(void* workspace, int sets, int slots) { return (SelState*)((uint32_t*)workspace + (size_t)sets * slots * NBIN); }

// The six launches of the three passes, for a workspace whose bins are zero and whose states hold prefix 0 and each
// (set, slot)'s own rank: what select_launch starts after its init kernel, and what a caller starts itself when the ranks
// differ from set to set (vdn_normal_angle_stats: the median of each set's own count, written by its fold kernel).
template <typename KeyFn>
inline void select_passes(const KeyFn& key_of, int frames, int group, size_t n, void* workspace, hipStream_t s) {
  constexpr int S = KeyFn::SLOTS;
  const int sets = frames / group;
  uint32_t* hist = (uint32_t*)workspace;
  SelState* st = select_state(workspace, sets, S);
  const dim3 grid(grid_for((n + KeyFn::PER - 1) / KeyFn::PER, 64), frames), scan(sets * S), block(256);
  hipLaunchKernelGGL((select_hist_kernel<0, KeyFn>), grid, block, 0, s, key_of, n, group, st, hist);
  hipLaunchKernelGGL(select_scan_kernel<0>, scan, block, 0, s, st, hist);
  hipLaunchKernelGGL((select_hist_kernel<1, KeyFn>), grid, block, 0, s, key_of, n, group, st, hist);
  hipLaunchKernelGGL(select_scan_kernel<1>, scan, block, 0, s, st, hist);
  hipLaunchKernelGGL((select_hist_kernel<2, KeyFn>), grid, block, 0, s, key_of, n, group, st, hist);
  hipLaunchKernelGGL(select_scan_kernel<2>, scan, block, 0, s, st, hist);
}

// `frames` frames of n elements each (n a multiple of KeyFn::PER, n < 2^32), `group` frames to a set (frames a multiple of
// group; fewer than 2^32 keys per set); workspace of select_workspace_bytes(frames / group, KeyFn::SLOTS), 4-byte aligned.
// Seven launches on s.
template <typename KeyFn>
inline void select_launch(const KeyFn& key_of, int frames, int group, size_t n, const SelRanks<KeyFn::SLOTS>& ranks, void* workspace,
                          hipStream_t s) {
  constexpr int S = KeyFn::SLOTS;
  const int sets = frames / group;
  hipLaunchKernelGGL(select_init_kernel<S>, dim3(grid_for((size_t)sets * S * NBIN, 1024)), dim3(256), 0, s,
                     select_state(workspace, sets, S), (uint32_t*)workspace, sets, ranks);
  select_passes(key_of, frames, group, n, workspace, s);
}

}  // namespace
