// The 64-key tile of the two MFMA flash-attention kernels, stated once: flash_attn_kernel (attn.hip, whose header describes
// the S^T = K Q^T / O^T = V^T P^T formulation, the row permutation and the LDS image) and flash_attn2_kernel
// (attn2_kernel.hpp). Everything here is common to both: the Q fragment loads, the LDS-DMA staging of K / V^T pieces, the
// fragment addresses, the mask of the ragged last tile, the pieces of the online softmax, the end of an iteration and the
// normalised output; the wave's place and the order of a run are stated here and spelled out by each kernel. What differs
// between the kernels is the instruction stream of one iteration (48 hand-placed slots in flash_attn_kernel, a generated
// stream in flash_attn2_kernel), which stays with each kernel.
// Both kernels are register-bound (occupancy 2 at 183..241 VGPRs) and their register allocation follows the order in which
// the prologue creates its values: these are plain inlined functions on values the kernels keep in locals, in the shapes
// with which every loop of every kernel compiles to the text it had before this header existed
// (profiles/attn_refactor.md, tools/asm_diff.py). Included by attn.hip after common.hpp, inside its anonymous namespace.

// Timing ablations for tools/attn_ablate.sh variant builds only (results are wrong with any bit set; the shipped
// library is built without the macro): 1 no LDS-DMA in the loop, 2 no workgroup barrier, 4 no softmax VALU, 8 no MFMA, 16 no fragment reads from LDS, 32 one workgroup per CU, 64 s_memtime stamps, 128 softmax without its fma
// (96 KB of LDS requested: one wave per SIMD).
#ifndef VDN_ATTN_ABL
#define VDN_ATTN_ABL 0
#endif

extern __shared__ __attribute__((aligned(16))) char attn_smem[];  // the LDS ring: 2 stages of NT tiles
constexpr int ATTN_TILE = 8192;      // one operand tile in LDS: 64 rows x 128 B
constexpr float ATTN_LAZY = 6.0f;    // the reference maximum moves only when a tile exceeds it by 2^ATTN_LAZY (lazy_reference)

__device__ __forceinline__ bool lane_hi() { return (threadIdx.x & 32) != 0; }
__device__ __forceinline__ int perm23(int i) {  // swap bits 2 and 3
  return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1);
}
// key offset (0..31) held by accumulator register `reg` of lane-half `h` after the row permutation
__device__ __forceinline__ int acc_key(int reg, int h) {
  return (reg & 3) + 4 * ((reg >> 2) & 1) + 8 * h + 16 * (reg >> 3);
}

// value held by the same row's lane in the other 32-lane half (v_permlane32_swap: VALU, no LDS round trip)
__device__ __forceinline__ float xhalf(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (lane_hi() ? r[0] : r[1]));
}

template <class F, int... J>
__device__ __forceinline__ void for_each_slot_impl(F& f, std::integer_sequence<int, J...>) {
  (f(std::integral_constant<int, J>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void for_each_slot(F& f) {
  for_each_slot_impl(f, std::make_integer_sequence<int, N>{});
}

// ---- the wave's place, spelled out by each kernel (the q-block count is `>> 7` in one and `/ QB` in the other, and behind
// a shared struct the tile loops of flash_attn_kernel changed): wave = tid >> 6 (made uniform), lane = tid & 63, row
// r = lane & 31 and half h = lane >> 5 of a 32 x 32 MFMA tile, and from the logical block id
//   bh = logical / nqb,  q0 = (logical - bh * nqb) * QB + wave * 32.
// 1-D grid, XCD-aware (xcd_remap): the q-blocks (QB queries) of one (batch, head) are consecutive logical ids and therefore
// run on ONE XCD, so its K / V^T tiles are fetched from HBM once and re-read by the other q-blocks from that XCD's L2
// (rocprofv3 FETCH_SIZE showed 7.6x over-fetch with a round-robin 2-D grid).

// Q fragments (B operand of S^T = K Q^T): Q[q][16 ks + 8 h + j] of the hi plane and, LO, of the lo plane; qo is the offset of
// Q[q][8 h] with q clamped to nq - 1 (lanes past the end read the last query; their output is not stored)
template <class HT, bool LO>
__device__ __forceinline__ void load_q(const typename HT::T* Q, const typename HT::T* Ql, size_t qo, typename HT::V8 (&qf)[4],
                                       typename HT::V8 (&ql)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qf[ks] = *(const typename HT::V8*)(Q + qo + 16 * ks);
    if constexpr (LO) ql[ks] = *(const typename HT::V8*)(Ql + qo + 16 * ks);
  }
}

// ---- staging: 8 pieces (1 KiB = 8 rows) per tile and operand, 8 / waves per wave, as `buffer_load_dwordx4 ... offen lds`:
// the (batch, head)'s plane is a buffer resource (4 SGPRs, hardware range check), the lane's place in a piece a
// loop-invariant 32-bit VGPR offset and the tile a SCALAR offset — no vector address arithmetic per tile (the flat
// global_load_lds form cost 16 v_lshl_add_u64 per tile and 16 VGPRs of per-lane 64-bit pointers). A stage of the LDS ring
// is NT tiles: K, V^T, second K plane, second V^T plane (the second planes are 128 B per key as well); the source chunk is
// XOR-swizzled with the row so that the ds_read_b128 fragment reads are bank-conflict free.
// Each kernel keeps the four resources and its offsets in locals of its own (as members of a struct they changed the tile
// loop of flash_attn_kernel's split forms).
template <class T>  // one plane of one (batch, head): K rows, V^T rows
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const void* base, int bh, int nk_pad) {
  const unsigned k_bytes = (unsigned)nk_pad * 64 * sizeof(T);
  return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + (size_t)bh * k_bytes), 0, (int)k_bytes, 0x00020000);
}
template <class T>  // byte offsets of the lane's 16 bytes of piece wave + 4 i in a K tile / in a V^T tile
__device__ __forceinline__ void stage_offsets(int wave, int lane, int i, int nk_pad, int& koff, int& voff) {
  const int row = (wave + 4 * i) * 8 + (lane >> 3);
  const int c = (lane & 7) ^ ((row >> 1) & 7);
  koff = (row * 64 + c * 8) * (int)sizeof(T);
  voff = (row * nk_pad + c * 8) * (int)sizeof(T);
}
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, int voffset, int soffset, char* dst) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voffset, soffset, 0, 0);
}
// piece wave + 4 i of tile t of K / of V^T, first or second plane (rs: its resource), into ring stage `buf`; the destination
// is formed whole and before the DMA call: the other orders move two scalar instructions of the tile loops
template <class T, int NT>
__device__ __forceinline__ void dma_k_piece(__amdgpu_buffer_rsrc_t rs, int koff, int buf, int t, int wave, int i, bool second) {
  char* dst = attn_smem + buf * NT * ATTN_TILE + (second ? 2 * ATTN_TILE : 0) + (wave + 4 * i) * 1024;
  lds_dma16(rs, koff, t * (64 * 64 * (int)sizeof(T)), dst);
}
template <class T, int NT>
__device__ __forceinline__ void dma_v_piece(__amdgpu_buffer_rsrc_t rs, int voff, int buf, int t, int wave, int i, bool second) {
  char* dst = attn_smem + buf * NT * ATTN_TILE + ATTN_TILE + (second ? 2 * ATTN_TILE : 0) + (wave + 4 * i) * 1024;
  lds_dma16(rs, voff, t * (64 * (int)sizeof(T)), dst);
}

// ---- fragment read offsets. Row `row` (+32 kb) of a tile, 16-byte chunk (2 ks + h) ^ swz(row): the kb / db
// term is a compile-time immediate and the ks / c term an XOR with (ks << 5), so ONE register per operand
// is kept (not 8) and the address of each fragment pair costs one v_xor (the loop is register-bound).
__device__ __forceinline__ int frag_base(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
struct FragAddr {
  int k_base, v_base;  // K rows go through perm23 so that the accumulator's k-order is the natural key order
  __device__ __forceinline__ FragAddr(int r, int h) : k_base(frag_base(perm23(r), h)), v_base(frag_base(r, h)) {}
  __device__ __forceinline__ int k(int kb, int ks) const { return kb * 4096 + (k_base ^ (ks << 5)); }
  __device__ __forceinline__ int v(int db, int c) const { return db * 4096 + (v_base ^ (c << 5)); }
};

// ---- the ragged last tile: scores of keys >= nk are -inf
__device__ __forceinline__ void mask_ragged(f32x16 (&s)[2], int t, int nk, int h) {
  if ((t + 1) * 64 > nk) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (t * 64 + kb * 32 + acc_key(i, h) >= nk) s[kb][i] = -INFINITY;
  }
}

// ---- pieces of the online softmax, in the order both streams issue them
// tile maximum, 8 scores per piece
template <int I>
__device__ __forceinline__ void max8(float& mx, const f32x16& s) {
  mx = fmaxf(fmaxf(mx, s[I]), s[I + 1]);
  mx = fmaxf(fmaxf(mx, s[I + 2]), s[I + 3]);
  mx = fmaxf(fmaxf(mx, s[I + 4]), s[I + 5]);
  mx = fmaxf(fmaxf(mx, s[I + 6]), s[I + 7]);
}
__device__ __forceinline__ void max_halves(float& mx) { mx = fmaxf(mx, xhalf(mx)); }
// Lazy rescale: the reference point m_run (RAW score domain; the scale is folded into the exp2 argument) moves only when
// some row's tile maximum exceeds it by more than 2^ATTN_LAZY (P stays <= 2^ATTN_LAZY: exact in fp32 / split fp16; the 1/l
// normalisation makes the result independent of the reference), so in steady state the O accumulators are never touched
// by the VALU. alpha rescales what was accumulated in the old reference, mb is the exp2 argument's offset in the new one.
__device__ __forceinline__ void lazy_reference(float mx, float scale_log2, float& m_run, bool& bump, float& alpha, float& mb) {
  bump = __builtin_amdgcn_ballot_w64((mx - m_run) * scale_log2 > ATTN_LAZY) != 0;  // wave-uniform
  const float m_new = bump ? fmaxf(m_run, mx) : m_run;
  alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2);  // == 1 when not bumped
  m_run = m_new;
  mb = -m_new * scale_log2;
}
// end of an iteration: O is in the old reference (it just received tile t-1): move it to the new one; then the stage's barrier
__device__ __forceinline__ void close_iteration(bool bump, float alpha, f32x16 (&o)[2]) {
  if (bump) {
    asm volatile("" ::: "memory");  // keep this a real (rarely taken) branch: if-converted it costs 16 v_pk_mul per tile
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
  }
  if constexpr (VDN_ATTN_ABL & 2) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  else stage_barrier();
}

// ---- a run, spelled out by each kernel in this order (its iteration is a lambda instantiated per position and parity):
//   K_0 (and K_1) in flight; stage_barrier; S(0) from stage 0; stage_barrier (every wave has read K_0 before iteration 0
//   lets K_2 overwrite it); then iteration t = 0 .. nt-1 with (has_prev, has_next) = (t > 0, t < nt-1), each computing
//   S(t+1), softmax(t) and O += V_{t-1} P(t-1) and ending in close_iteration; then O += V_{nt-1} P(nt-1), c outer (a P
//   fragment is dead after its MFMAs), per fragment V p [, V p_lo] [, V_lo p].

// ---- the output: O / l of the lane's query, 4 channels 8 g + 4 h .. + 3 of a 32-channel block at a time
__device__ __forceinline__ float inv_row_sum(float l_run) { return 1.0f / (l_run + __shfl_xor(l_run, 32)); }
struct OutRow {
  int hd;      // head
  size_t row;  // b * nq + q
  size_t oo;   // element offset of the head's 64 channels in [B, nq, H, 64]
};
__device__ __forceinline__ OutRow out_row(int bh, int H, int nq, int q) {
  const int b = bh / H, hd = bh - b * H;
  const size_t row = (size_t)b * nq + q;
  return {hd, row, (row * H + hd) * 64};
}
// planes: v = hi plane (rounded toward zero), vl = remainder; otherwise v = the rounded value
template <class HT>
__device__ __forceinline__ void out_quad(const f32x16& o, int g, float inv, bool planes, typename HT::V4& v, typename HT::V4& vl) {
  using T = typename HT::T;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = o[4 * g + e] * inv;
    if (planes) {
      T a, b;
      split_rtz(x, a, b);
      v[e] = a;
      vl[e] = b;
    } else {
      v[e] = (T)x;
    }
  }
}
