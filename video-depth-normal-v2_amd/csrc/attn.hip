// Attention kernels for gfx950 (wave64, v_mfma_f32_32x32x16_{f16,bf16}).
//
// flash_attn_kernel — head_dim 64, Nq x Nk scores never leave registers.
//   S^T = K Q^T is computed with the KEY on the accumulator row and the QUERY on the lane
//   (col = lane & 31), so a lane owns one query's scores: row max / sum are in-lane plus one
//   cross-half shuffle, and the exponentiated tile, converted pairwise to half, is directly the
//   B operand of O^T = V^T P^T (guide §3 'An accumulator tile as the next MFMA's operand').
//   The K rows are fed through the bit-2<->bit-3 row permutation so that the accumulator's
//   k-order is the natural key order and V^T fragments are one contiguous 16-byte LDS read.
//   K and V^T tiles (64 keys) arrive by LDS-DMA into a double buffer shared by the 4 waves
//   (4 x 32 = 128 queries per workgroup); chunk ^ ((row>>1)&7) source-side swizzle keeps the
//   ds_read_b128 fragment reads bank-conflict free.
//   SPLIT: every operand comes as (hi, lo) 16-bit planes and each product is accumulated as
//   hi*hi + hi*lo + lo*hi (fp32-faithful "x3" mode, see include/vdn.h).
//   PV2 (SPLIT only): P, which is born in registers, is rounded ONCE to 16 bits (p~) and O accumulates
//   p~ (V_hi + V_lo): 2 products instead of 3 and no lo split of P on the VALU. The row sum l is accumulated from the
//   SAME rounded p~ (one v_dot2 per pair), so O / l is an exact convex combination of the (21-bit) V rows with
//   weights p~ / sum p~: the rounding perturbs each weight by <= 2^-11 relative and any part of it common to a
//   row cancels in the normalisation (DESIGN.md §3 has the measured end-to-end effect).
//   The tile itself (staging, fragment addresses, softmax pieces, output) is attn_tile.hpp, shared with
//   flash_attn2_kernel (attn2_kernel.hpp), the kernel of the default mode: fp16 split planes with 8-bit Q / K planes.
//
// temporal_attn_kernel — <= 32 frames per (pixel, head): one wave per sequence, fragments loaded
//   straight from global memory (no LDS), same accumulator-as-operand chaining.
#include "common.hpp"
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace {

#include "attn_tile.hpp"

template <int DT, bool SPLIT, bool PV2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void flash_attn_kernel(const typename Half<DT>::T* __restrict__ Q,
                                                         const typename Half<DT>::T* __restrict__ K,
                                                         const typename Half<DT>::T* __restrict__ Vt,
                                                         typename Half<DT>::T* __restrict__ out,
                                                         const typename Half<DT>::T* __restrict__ Ql,
                                                         const typename Half<DT>::T* __restrict__ Kl,
                                                         const typename Half<DT>::T* __restrict__ Vtl,
                                                         typename Half<DT>::T* __restrict__ outl,
                                                         int H, int nq, int nq_pad, int nk, int nk_pad, float scale_log2) {
  using HT = Half<DT>;
  using T = typename HT::T;
  using V8 = typename HT::V8;
  constexpr int NT = SPLIT ? 4 : 2;  // tiles per stage: K, Vt (, K_lo, Vt_lo)
  // the wave's place (attn_tile.hpp states the order)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nqb = (nq + 127) >> 7;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = logical / nqb;
  const int q0 = (logical - bh * nqb) * 128 + wave * 32;
  const int r = lane & 31, h = lane >> 5;
  V8 qf[4], ql[4];
  {
    int q = q0 + r;
    q = q < nq ? q : nq - 1;
    load_q<HT, SPLIT>(Q, Ql, ((size_t)bh * nq_pad + q) * 64 + 8 * h, qf, ql);
  }
  // staging: 2 pieces per wave, tile and plane; the second planes are K_lo and V^T_lo
  const __amdgpu_buffer_rsrc_t rK = plane_rsrc<T>(K, bh, nk_pad), rV = plane_rsrc<T>(Vt, bh, nk_pad);
  const __amdgpu_buffer_rsrc_t rKl = plane_rsrc<T>(SPLIT ? Kl : K, bh, nk_pad), rVl = plane_rsrc<T>(SPLIT ? Vtl : Vt, bh, nk_pad);
  int koff[2], voff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) stage_offsets<T>(wave, lane, i, nk_pad, koff[i], voff[i]);
  auto stage_k_piece = [&](int buf, int t, int i, bool second) { dma_k_piece<T, NT>(second ? rKl : rK, koff[i], buf, t, wave, i, second); };
  auto stage_v_piece = [&](int buf, int t, int i, bool second) { dma_v_piece<T, NT>(second ? rVl : rV, voff[i], buf, t, wave, i, second); };
  auto stage_k = [&](int buf, int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_k_piece(buf, t, i, false);
      if constexpr (SPLIT) stage_k_piece(buf, t, i, true);
    }
  };
  auto stage_v = [&](int buf, int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_v_piece(buf, t, i, false);
      if constexpr (SPLIT) stage_v_piece(buf, t, i, true);
    }
  };
  const FragAddr fa(r, h);

  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;  // running max in the RAW score domain; the scale is folded into the exp2 argument

  // S^T of one 64-key tile from K buffer `buf`
  auto qk = [&](int buf, f32x16 (&sc)[2]) {
    const char* sK = attn_smem + buf * NT * ATTN_TILE;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[kb][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const V8 a = *(const V8*)(sK + fa.k(kb, ks));
        sc[kb] = HT::mfma32(a, qf[ks], sc[kb]);
        if constexpr (SPLIT) {
          const V8 al = *(const V8*)(sK + 2 * ATTN_TILE + fa.k(kb, ks));
          sc[kb] = HT::mfma32(a, ql[ks], sc[kb]);
          sc[kb] = HT::mfma32(al, qf[ks], sc[kb]);
        }
      }
    }
  };

  // Three-stage software pipeline, all in ONE basic block per iteration so the scheduler can slot the
  // softmax VALU work into the MFMA gaps of the SAME wave (an in-order wave only overlaps the two pipes
  // when they alternate in program order; PMC before: VALU busy 46 % + MFMA busy 53 % = 99 %, i.e. serial):
  //     iteration t:   S(t+1) = K_{t+1} Q^T   ||   P(t) = softmax-numerator(S(t))   ||   O += V_{t-1} P(t-1)
  // LDS ring (2 buffers each): iteration t reads K_{t+1} and V_{t-1}; its DMA fills K_{t+2} (buffer of K_t,
  // consumed in iteration t-1) and V_t (buffer of V_{t-2}, consumed in iteration t-1).
  const int nt = (nk + 63) >> 6;
  f32x16 s[2];
  V8 pf[2][2], pl[2][2];
  auto iter = [&](int t, auto has_prev_c, auto has_next_c) {
    constexpr bool HAS_PREV = decltype(has_prev_c)::value, HAS_NEXT = decltype(has_next_c)::value;
    const int cur = t & 1;
    if constexpr (!(VDN_ATTN_ABL & 1)) {
      stage_v(cur, t);
      if constexpr (HAS_NEXT) {
        if (t + 2 < nt) stage_k(cur, t + 2);
      }
    }
    if constexpr (!HAS_NEXT) mask_ragged(s, t, nk, h);  // only the last tile can be ragged
    const char* sKn = attn_smem + (cur ^ 1) * NT * ATTN_TILE;         // K_{t+1}
    const char* sVp = attn_smem + (cur ^ 1) * NT * ATTN_TILE + ATTN_TILE;  // V_{t-1}

    // ---- hand-placed stream: 48 slots = 16 MFMA triples (8 of PV(t-1), c outer; then 8 of QK(t+1)), each
    // slot = one small piece of softmax(t) + one MFMA, fenced by sched_barrier so the order survives the
    // scheduler (its own choice is all MFMAs first, then all VALU: no overlap inside the in-order wave;
    // sched_group_barrier pipelines were not honoured on this block). A 32x32x16 MFMA keeps the matrix pipe
    // 32 cycles and the issue port 8, so <= 24 cycles of VALU issue per slot are hidden.
    // S and P are updated IN PLACE (the loop is register-bound: O 32 + S 32 + Q 32 + P 32 + fragments):
    //   P fragment f is read by PV(t-1) in slots 6f..6f+5 and rewritten by softmax(t) in slots >= 7+8f;
    //   S[0] is last read in slot 20 and overwritten by QK(t+1) from slot 24, S[1] read in 36 (softmax piece
    //   first in the slot), overwritten from slot 36's MFMA on.
    V8 fr[2], fl[2];
    auto frag = [&](auto jc, V8& a, V8& al) {
      constexpr int j = decltype(jc)::value;
      if constexpr (VDN_ATTN_ABL & 16) {
        asm volatile("" : "+v"(a), "+v"(al));  // timing ablation: no fragment reads (operands stay what they were)
      } else if constexpr (j < 8) {
        if constexpr (HAS_PREV) {
          a = *(const V8*)(sVp + fa.v(j & 1, j >> 1));
          if constexpr (SPLIT) al = *(const V8*)(sVp + 2 * ATTN_TILE + fa.v(j & 1, j >> 1));
        }
      } else if constexpr (HAS_NEXT) {
        a = *(const V8*)(sKn + fa.k((j - 8) >> 2, (j - 8) & 3));
        if constexpr (SPLIT) al = *(const V8*)(sKn + 2 * ATTN_TILE + fa.k((j - 8) >> 2, (j - 8) & 3));
      }
    };
    auto mma = [&](auto jc, auto qc, const V8& a, const V8& al) {
      constexpr int j = decltype(jc)::value, q = decltype(qc)::value;
      if constexpr (!SPLIT && q > 0) return;
      if constexpr (j < 8) {
        if constexpr (HAS_PREV) {
          constexpr int c = j >> 1, db = j & 1;
          if constexpr (q == 0) o[db] = HT::mfma32(a, pf[c >> 1][c & 1], o[db]);
          if constexpr (q == 1 && !PV2) o[db] = HT::mfma32(a, pl[c >> 1][c & 1], o[db]);  // PV2: a VALU-only slot
          if constexpr (q == 2) o[db] = HT::mfma32(al, pf[c >> 1][c & 1], o[db]);
        }
      } else if constexpr (HAS_NEXT) {
        constexpr int kb = (j - 8) >> 2, ks = (j - 8) & 3;
        if constexpr (ks == 0 && q == 0) {
          f32x16 z;
#pragma unroll
          for (int i = 0; i < 16; ++i) z[i] = 0.f;
          s[kb] = HT::mfma32(a, qf[ks], z);
        } else {
          if constexpr (q == 0) s[kb] = HT::mfma32(a, qf[ks], s[kb]);
          if constexpr (q == 1) s[kb] = HT::mfma32(a, ql[ks], s[kb]);
          if constexpr (q == 2) s[kb] = HT::mfma32(al, qf[ks], s[kb]);
        }
      }
    };
    float mx = -1e30f, alpha = 1.f, mb = 0.f, ls = 0.f, px0 = 0.f, px1 = 0.f;
    bool bump = false;
    auto vstep = [&](auto kc) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k < 4) {
        max8<(k & 1) * 8>(mx, s[k >> 1]);
      } else if constexpr (k == 4) {
        max_halves(mx);
      } else if constexpr (k == 5) {
        lazy_reference(mx, scale_log2, m_run, bump, alpha, mb);
      } else if constexpr (k < 38) {
        constexpr int pi = (k - 6) >> 1, kb = pi >> 3, i = (pi & 7) * 2;
        if constexpr (((k - 6) & 1) == 0) {
          px0 = __builtin_amdgcn_exp2f(fmaf(s[kb][i], scale_log2, mb));
          px1 = __builtin_amdgcn_exp2f(fmaf(s[kb][i + 1], scale_log2, mb));
        } else if constexpr (SPLIT && PV2) {
          if constexpr (DT == VDN_F16) {  // one packed convert, one dot2 for the row sum of the ROUNDED weights
            const f16x2 pp = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(px0, px1));
            pf[kb][i >> 3][i & 7] = pp[0]; pf[kb][i >> 3][(i & 7) + 1] = pp[1];
            ls = __builtin_amdgcn_fdot2(pp, f16x2{(_Float16)1.f, (_Float16)1.f}, ls, false);
            asm volatile("" : "+v"(ls));  // or LLVM sinks all 16 dot2 behind the last MFMA of the iteration
          } else {
            const T a0 = (T)px0, a1 = (T)px1;
            pf[kb][i >> 3][i & 7] = a0; pf[kb][i >> 3][(i & 7) + 1] = a1;
            ls += (float)a0 + (float)a1;
          }
        } else {
          ls += px0 + px1;
          if constexpr (SPLIT) {
            T a0, a1, b0, b1;
            split2_rtz(px0, px1, a0, a1, b0, b1);
            pf[kb][i >> 3][i & 7] = a0; pf[kb][i >> 3][(i & 7) + 1] = a1;
            pl[kb][i >> 3][i & 7] = b0; pl[kb][i >> 3][(i & 7) + 1] = b1;
          } else {
            pf[kb][i >> 3][i & 7] = (T)px0; pf[kb][i >> 3][(i & 7) + 1] = (T)px1;
          }
        }
      } else if constexpr (k == 38) {
        l_run = l_run * alpha + ls;
      }
    };
    auto slot = [&](auto jc) {
      constexpr int j = decltype(jc)::value, tj = j / 3, q = j % 3;
      if constexpr (q == 0 && tj + 1 < 16) frag(std::integral_constant<int, tj + 1>{}, fr[(tj + 1) & 1], fl[(tj + 1) & 1]);
      if constexpr (!(VDN_ATTN_ABL & 4)) vstep(jc);
      if constexpr (!(VDN_ATTN_ABL & 8)) mma(std::integral_constant<int, tj>{}, std::integral_constant<int, q>{}, fr[tj & 1], fl[tj & 1]);
      __builtin_amdgcn_sched_barrier(0);
    };
    frag(std::integral_constant<int, 0>{}, fr[0], fl[0]);
    for_each_slot<48>(slot);

    // P(t) is only consumed by the next iteration's MFMAs: keep LLVM from sinking its computation there.
    asm volatile("" : "+v"(pf[0][0]), "+v"(pf[0][1]), "+v"(pf[1][0]), "+v"(pf[1][1]));
    if constexpr (SPLIT && !PV2) asm volatile("" : "+v"(pl[0][0]), "+v"(pl[0][1]), "+v"(pl[1][0]), "+v"(pl[1][1]));
    close_iteration(bump, alpha, o);
  };

  // The run, in the order attn_tile.hpp states it (spelled out in both kernels: as a shared function taking the
  // iteration it changed the tile loop's scalar code, profiles/attn_refactor.md).
  stage_k(0, 0);
  if (nt > 1) stage_k(1, 1);
  stage_barrier();
  qk(0, s);
  stage_barrier();  // every wave has read K_0 before iteration 0 lets K_2 overwrite it
  constexpr std::true_type Y{};
  constexpr std::false_type N{};
  if (nt == 1) {
    iter(0, N, N);
  } else {
    iter(0, N, Y);
    for (int t = 1; t + 1 < nt; ++t) iter(t, Y, Y);
    iter(nt - 1, Y, N);
  }
  // O^T += V^T P^T of the last tile (as a shared function it renamed the fragment registers of the bf16 3-product tile loop)
  {
    const char* sV = attn_smem + ((nt - 1) & 1) * NT * ATTN_TILE + ATTN_TILE;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const V8 a = *(const V8*)(sV + fa.v(db, c));
        o[db] = HT::mfma32(a, pf[c >> 1][c & 1], o[db]);
        if constexpr (SPLIT) {
          const V8 al = *(const V8*)(sV + 2 * ATTN_TILE + fa.v(db, c));
          if constexpr (!PV2) o[db] = HT::mfma32(a, pl[c >> 1][c & 1], o[db]);
          o[db] = HT::mfma32(al, pf[c >> 1][c & 1], o[db]);
        }
      }
  }

  const float inv = inv_row_sum(l_run);
  const int q = q0 + r;
  if (q < nq) {
    const size_t oo = out_row(bh, H, nq, q).oo;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // Must stay equal to out_quad (attn_tile.hpp), spelled out here: called with the quads by reference, the bf16
        // kernels kept them in scratch (24 bytes per lane, profiles/attn_refactor.md).
        typename HT::V4 v, vl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = o[db][4 * g + e] * inv;
          if (outl) {  // planes whenever the caller passes a lo plane (also in 1-product mode)
            T a, b2;
            split_rtz(x, a, b2);
            v[e] = a;
            vl[e] = b2;
          } else {
            v[e] = (T)x;
          }
        }
        *(typename HT::V4*)(out + oo + db * 32 + 8 * g + 4 * h) = v;
        if (outl) *(typename HT::V4*)(outl + oo + db * 32 + 8 * g + 4 * h) = vl;
      }
  }
}

#include "attn2_kernel.hpp"

template <int DT, bool SPLIT, int NB /*32-frame blocks: sequences of up to 32 NB frames*/>
__global__ __launch_bounds__(256) void temporal_attn_kernel(const typename Half<DT>::T* __restrict__ qkv,
                                                            typename Half<DT>::T* __restrict__ out,
                                                            const typename Half<DT>::T* __restrict__ qkv_lo,
                                                            typename Half<DT>::T* __restrict__ out_lo, int nseq,
                                                            int Tn, int D, int c, int heads, float scale_log2,
                                                            const float* __restrict__ rope_cs) {
  using HT = Half<DT>;
  using T = typename HT::T;
  using V8 = typename HT::V8;
  const int lane = threadIdx.x & 63;
  const int seq = blockIdx.x * 4 + (threadIdx.x >> 6);  // (b, d, head)
  if (seq >= nseq) return;
  const int head = seq % heads;
  const int bd = seq / heads;
  const int d = bd % D, b = bd / D;
  const int dh = c / heads;
  const int r = lane & 31, h = lane >> 5;
  const size_t rs = (size_t)D * 3 * c;  // stride between frames
  const size_t boff = ((size_t)b * Tn * D + d) * 3 * c + head * dh;
  const T* base = qkv + boff;
  const T* base_lo = SPLIT ? qkv_lo + boff : nullptr;
  const T* vb = base + 2 * c;
  const T* vb_lo = SPLIT ? base_lo + 2 * c : nullptr;
  const size_t ooff = ((size_t)b * Tn * D + d) * c + head * dh;
  T* ob = out + ooff;
  T* ob_lo = SPLIT ? out_lo + ooff : nullptr;
  const size_t os = (size_t)D * c;
  const int nks = (dh + 15) >> 4;
  const int neb = (dh + 31) >> 5;
  const int pk = perm23(r);

  for (int qb = 0; qb < NB; ++qb) {  // 32 query frames at a time (the v5 refiner runs 64-frame clips)
    if (qb * 32 >= Tn) break;
    const int tq = qb * 32 + r;
    const int fq = tq < Tn ? tq : Tn - 1;
    // ---- S^T = K Q^T, one 32 x 32 tile per key block
    f32x16 s[NB];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
      if (kb * 32 >= Tn) continue;
      const int tk = kb * 32 + pk;
      const int fk = tk < Tn ? tk : Tn - 1;
      for (int ks = 0; ks < nks; ++ks) {
        const int e0 = 16 * ks + 8 * h;
        V8 a, bq, al, bl;
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = (T)0.f; bq[j] = (T)0.f; al[j] = (T)0.f; bl[j] = (T)0.f; }
        if (e0 < dh) {
          bq = *(const V8*)(base + fq * rs + e0);
          a = *(const V8*)(base + fk * rs + c + e0);
          if constexpr (SPLIT) {
            bl = *(const V8*)(base_lo + fq * rs + e0);
            al = *(const V8*)(base_lo + fk * rs + c + e0);
          }
          if (rope_cs) {  // pe = 'rope' (motion_module.py:279-282): pairs (2i, 2i+1) of the c channels rotate with the frame index
            const size_t pair0 = (size_t)(head * dh + e0) >> 1;
            auto rot = [&](V8& hi, V8& lo, int frame) {
              const float* cs = rope_cs + ((size_t)frame * (c >> 1) + pair0) * 2;
#pragma unroll
              for (int j = 0; j < 8; j += 2) {
                const float x0 = (float)hi[j] + (SPLIT ? (float)lo[j] : 0.f), x1 = (float)hi[j + 1] + (SPLIT ? (float)lo[j + 1] : 0.f);
                const float cc = cs[j], ss = cs[j + 1];
                const float y0 = x0 * cc - x1 * ss, y1 = x0 * ss + x1 * cc;
                if constexpr (SPLIT) {
                  T h0, h1, l0, l1;
                  split2_rtz(y0, y1, h0, h1, l0, l1);
                  hi[j] = h0; hi[j + 1] = h1; lo[j] = l0; lo[j + 1] = l1;
                } else {
                  hi[j] = (T)y0; hi[j + 1] = (T)y1;
                }
              }
            };
            rot(bq, bl, fq);
            rot(a, al, fk);
          }
        }
        s[kb] = HT::mfma32(a, bq, s[kb]);
        if constexpr (SPLIT) {
          s[kb] = HT::mfma32(a, bl, s[kb]);
          s[kb] = HT::mfma32(al, bq, s[kb]);
        }
      }
    }
    float mx = -1e30f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = s[kb][i] * scale_log2;
        v = (kb * 32 + acc_key(i, h) < Tn) ? v : -INFINITY;
        s[kb][i] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float ls = 0.f;
    V8 pf[NB][2], pl[NB][2];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pv = __builtin_amdgcn_exp2f(s[kb][i] - mx);
        ls += pv;
        if constexpr (SPLIT) {
          T a2, b2;
          split_rtz(pv, a2, b2);
          pf[kb][i >> 3][i & 7] = a2;
          pl[kb][i >> 3][i & 7] = b2;
        } else {
          pf[kb][i >> 3][i & 7] = (T)pv;
        }
      }
    ls += __shfl_xor(ls, 32);
    const float inv = 1.0f / ls;

    // ---- O^T = V^T P^T, 32 output dims per pass; V^T fragments gathered element-wise (tiny op)
    for (int eb = 0; eb < neb; ++eb) {
      f32x16 o;
#pragma unroll
      for (int i = 0; i < 16; ++i) o[i] = 0.f;
      const int e = eb * 32 + r;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        if (kb * 32 >= Tn) continue;
#pragma unroll
        for (int sp = 0; sp < 2; ++sp) {
          V8 a, al;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int key = kb * 32 + 16 * sp + 8 * h + j;
            const bool ok = key < Tn && e < dh;
            a[j] = ok ? vb[key * rs + e] : (T)0.f;
            if constexpr (SPLIT) al[j] = ok ? vb_lo[key * rs + e] : (T)0.f;
          }
          o = HT::mfma32(a, pf[kb][sp], o);
          if constexpr (SPLIT) {
            o = HT::mfma32(a, pl[kb][sp], o);
            o = HT::mfma32(al, pf[kb][sp], o);
          }
        }
      }
      if (tq < Tn) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int e0 = eb * 32 + 8 * g + 4 * h;
          if (e0 < dh) {
            typename HT::V4 v, vl;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float x = o[4 * g + q] * inv;
              if constexpr (SPLIT) {
                T a2, b2;
                split_rtz(x, a2, b2);
                v[q] = a2;
                vl[q] = b2;
              } else {
                v[q] = (T)x;
              }
            }
            *(typename HT::V4*)(ob + tq * os + e0) = v;
            if constexpr (SPLIT) *(typename HT::V4*)(ob_lo + tq * os + e0) = vl;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// temporal_last_kernel — streaming mode (video_depth_stream.py:133-158, motion_module.py:255-277) with a
// PROJECTED key/value cache: every cached frame keeps its q|k|v projection WITHOUT the
// frame-position term (f32 [HW, 3c], the position is not known when the frame is cached: the window slides);
// by linearity  W (x + pe[t]) = W x + W pe[t],  so the position enters as three small tables
// (pe W_q^T, pe W_k^T, pe W_v^T: f32 [T, c] each) added on load. Only the NEWEST frame queries (the reference
// computes all T and keeps the last). One wave per pixel: lane owns c/64 consecutive channels, a head
// (c/8 channels) is 8 consecutive lanes; scores are reduced inside the 8-lane group, softmax over the
// <= 32 frames in registers, output written as operand planes for the out-projection GEMM. HBM-bound:
// T x 2c f32 per pixel are read once.
struct SlotTable { int s[32]; };  // ring slots of the window's frames, oldest first; passed BY VALUE (no table in HBM)

template <int DT, int CPL /*channels per lane: c / 64*/>
__global__ __launch_bounds__(256) void temporal_last_kernel(const float* __restrict__ pool, size_t slot_stride, SlotTable tab,
                                                            int T, int HW, int c,
                                                            const float* __restrict__ peq, const float* __restrict__ pek,
                                                            const float* __restrict__ pev, float scale,
                                                            typename Half<DT>::T* __restrict__ out,
                                                            typename Half<DT>::T* __restrict__ out_lo) {
  using Th = typename Half<DT>::T;
  const int lane = threadIdx.x & 63;
  const int px = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (px >= HW) return;
  const int ch = lane * CPL;
  const size_t row = (size_t)px * 3 * c;
  float q[CPL];
  {
    const float* qn = pool + (size_t)tab.s[T - 1] * slot_stride + row + ch;  // the newest frame is the query, at position T-1
#pragma unroll
    for (int e = 0; e < CPL; ++e) q[e] = (qn[e] + peq[(size_t)(T - 1) * c + ch + e]) * scale;
  }
  float sc[32];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 32; ++t) {
    sc[t] = -INFINITY;
    if (t < T) {
      const float* kt = pool + (size_t)tab.s[t] * slot_stride + row + c + ch;
      const float* pk = pek + (size_t)t * c + ch;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < CPL; ++e) d = fmaf(q[e], kt[e] + pk[e], d);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      sc[t] = d;
      mx = fmaxf(mx, d);
    }
  }
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < 32; ++t) {
    sc[t] = t < T ? __expf(sc[t] - mx) : 0.f;
    den += sc[t];
  }
  const float inv = 1.0f / den;
  float o[CPL];
#pragma unroll
  for (int e = 0; e < CPL; ++e) o[e] = 0.f;
#pragma unroll
  for (int t = 0; t < 32; ++t) {
    if (t < T) {
      const float* vt = pool + (size_t)tab.s[t] * slot_stride + row + 2 * c + ch;
      const float* pv = pev + (size_t)t * c + ch;
      const float p = sc[t] * inv;
#pragma unroll
      for (int e = 0; e < CPL; ++e) o[e] = fmaf(p, vt[e] + pv[e], o[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < CPL; ++e) store_half(out, out_lo, (size_t)px * c + ch + e, o[e]);
}

// pv: MFMA products per P V term in split mode (include/vdn.h): 1 (default), 2 or 3 — a per-call argument: the library keeps
// no selection state.
template <int DT>
int flash_launch(const void* Q, const void* K, const void* Vt, void* out, const void* Ql, const void* Kl, const void* Vtl,
                 void* outl, const void* Q8, const void* K8, void* out8, int out_kt, int B, int H, int nq, int nq_pad, int nk, int nk_pad,
                 float sl2, int pv, hipStream_t s) {
  using T = typename Half<DT>::T;
  const bool pv3 = pv == 3;  // the 3-product P V with P split into hi / lo planes
  const uint8_t* q8 = (const uint8_t*)Q8;
  const uint8_t* k8 = (const uint8_t*)K8;
  // the 8-bit / K-tile-major output planes and a lo-less output exist in the default kernel only (fp16 split planes + Q8 / K8)
  if ((out8 || out_kt || (Ql && !outl)) && !(Ql && !pv3 && q8 && k8 && DT == VDN_F16)) return VDN_EUNSUPPORTED;
  // flash_attn_kernel: 4 waves = 128 queries per workgroup, lds bytes of its two ring stages
  const auto grid = [&](int qb) { return dim3(((nq + qb - 1) / qb) * B * H); };  // 1-D: q-blocks of qb queries x (batch, head)
  auto launch = [&](auto kernel, int lds) {
    hipLaunchKernelGGL(kernel, grid(128), dim3(256), lds, s, (const T*)Q, (const T*)K, (const T*)Vt, (T*)out, (const T*)Ql,
                       (const T*)Kl, (const T*)Vtl, (T*)outl, H, nq, nq_pad, nk, nk_pad, sl2);
  };
  if (Ql && pv3)
    launch(flash_attn_kernel<DT, true, false>, 65536);
  else if (Ql && q8 && k8 && DT == VDN_F16) {
    if constexpr (DT == VDN_F16) {
#ifndef VDN_ATTN2_NW
#define VDN_ATTN2_NW 4
#endif
      constexpr int NW = VDN_ATTN2_NW;
      auto launch2 = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid(32 * NW), dim3(64 * NW), (VDN_ATTN_ABL & 32) ? 98304 : 65536, s, (const T*)Q,
                           (const T*)K, (const T*)Vt, (T*)out, (const T*)Kl, (const T*)Vtl, (T*)outl, q8, k8, H, nq, nq_pad, nk, nk_pad, sl2,
                           (uint8_t*)out8, out_kt, B * nq);
      };
      if (pv == 1) launch2(flash_attn2_kernel<1, NW>);
      else launch2(flash_attn2_kernel<2, NW>);
    }
  } else if (Ql)
    launch(flash_attn_kernel<DT, true, true>, 65536);
  else
    launch(flash_attn_kernel<DT, false, false>, 32768);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

template <int DT>
int temporal_launch(const void* qkv, void* out, const void* qkv_lo, void* out_lo, int nseq, int T, int D, int c, int heads,
                    float sl2, const float* rope_cs, hipStream_t s) {
  using TT = typename Half<DT>::T;
  const dim3 grid((nseq + 3) / 4);
#define VDN_TA(SP, NB_)                                                                                          \
  hipLaunchKernelGGL((temporal_attn_kernel<DT, SP, NB_>), grid, dim3(256), 0, s, (const TT*)qkv, (TT*)out,       \
                     (const TT*)(SP ? qkv_lo : nullptr), (TT*)(SP ? out_lo : nullptr), nseq, T, D, c, heads, sl2, rope_cs)
  if (qkv_lo) {
    if (T <= 32) VDN_TA(true, 1); else VDN_TA(true, 2);
  } else {
    if (T <= 32) VDN_TA(false, 1); else VDN_TA(false, 2);
  }
#undef VDN_TA
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

}  // namespace

extern "C" int vdn_flash_attn(int dt, const void* Q, const void* K, const void* Vt, void* out, const void* Q_lo,
                              const void* K_lo, const void* Vt_lo, void* out_lo, const void* Q8, const void* K8, void* out8,
                              int out_kt, int B, int H, int nq, int nq_pad, int nk, int nk_pad, float scale, int pv_products,
                              vdn_stream stream) {
  if (!Q || !K || !Vt || !out || B <= 0 || H <= 0 || nq <= 0 || nk <= 0) return VDN_EINVAL;
  if (pv_products < 0 || pv_products > 3) return VDN_EINVAL;
  const int pv = pv_products ? pv_products : 1;
  if (nq_pad < nq || nk_pad < nk || (nk_pad & 63)) return VDN_EALIGN;
  if (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)Vt | (uintptr_t)out) & 15) return VDN_EALIGN;
  const int nlo = (Q_lo != nullptr) + (K_lo != nullptr) + (Vt_lo != nullptr);
  if (nlo != 0 && nlo != 3) return VDN_EINVAL;  // operand planes are all-or-nothing; the output may be split either way
  if (nlo == 3 && !out_lo && !out8) return VDN_EINVAL;  // split operands: the output carries its remainder as a 16-bit or an 8-bit plane
  if (((uintptr_t)Q_lo | (uintptr_t)K_lo | (uintptr_t)Vt_lo | (uintptr_t)out_lo | (uintptr_t)Q8 | (uintptr_t)K8 | (uintptr_t)out8) & 15) return VDN_EALIGN;
  if ((Q8 == nullptr) != (K8 == nullptr) || (Q8 && (nlo != 3 || dt != VDN_F16))) return VDN_EINVAL;  // 8-bit planes come in pairs, split fp16 only
  const float sl2 = scale * 1.44269504088896340736f;
  hipStream_t s = (hipStream_t)stream;
  if (dt == VDN_F16)
    return flash_launch<VDN_F16>(Q, K, Vt, out, Q_lo, K_lo, Vt_lo, out_lo, Q8, K8, out8, out_kt, B, H, nq, nq_pad, nk, nk_pad, sl2, pv, s);
  if (dt == VDN_BF16)
    return flash_launch<VDN_BF16>(Q, K, Vt, out, Q_lo, K_lo, Vt_lo, out_lo, nullptr, nullptr, out8, out_kt, B, H, nq, nq_pad, nk, nk_pad, sl2, pv, s);
  return VDN_EUNSUPPORTED;
}

extern "C" int vdn_temporal_attn(int dt, const void* qkv, void* out, const void* qkv_lo, void* out_lo, int Bv, int T,
                                 int D, int c, int heads, float scale, const float* rope_cs, vdn_stream stream) {
  if (!qkv || !out || Bv <= 0 || T <= 0 || T > 64 || D <= 0 || heads <= 0 || c % heads) return VDN_EINVAL;
  if ((qkv_lo == nullptr) != (out_lo == nullptr)) return VDN_EINVAL;
  const int dh = c / heads;
  if ((dh & 7) || dh > 256 || (c & 7)) return VDN_EALIGN;
  if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)qkv_lo | (uintptr_t)out_lo) & 15) return VDN_EALIGN;
  const int nseq = Bv * D * heads;
  const float sl2 = scale * 1.44269504088896340736f;
  hipStream_t s = (hipStream_t)stream;
  return with_half(dt, [&](auto t) {
    return temporal_launch<decltype(t)::value>(qkv, out, qkv_lo, out_lo, nseq, T, D, c, heads, sl2, rope_cs, s);
  });
}

extern "C" int vdn_temporal_attn_last(int dt, const float* pool, size_t slot_stride, const int32_t* slots, int T, int HW,
                                      int c, const float* pe_q, const float* pe_k, const float* pe_v, float scale,
                                      void* out, void* out_lo, vdn_stream stream) {
  if (!pool || !slots || !pe_q || !pe_k || !pe_v || !out || T < 1 || T > 32 || HW <= 0) return VDN_EINVAL;
  if (slot_stride < (size_t)HW * 3 * c) return VDN_EINVAL;
  SlotTable tab;
  for (int t = 0; t < 32; ++t) {
    tab.s[t] = t < T ? slots[t] : 0;
    if (tab.s[t] < 0) return VDN_EINVAL;
  }
  if (c <= 0 || (c & 63) || c > 1024) return VDN_EUNSUPPORTED;  // 8 heads of c/8 = 8 lanes x c/64 channels
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((HW + 3) / 4), block(256);
#define VDN_TL(CPL_)                                                                                                     \
  hipLaunchKernelGGL((temporal_last_kernel<DT, CPL_>), grid, block, 0, s, pool, slot_stride, tab, T, HW, c, pe_q, pe_k, \
                     pe_v, scale, (typename Half<DT>::T*)out, (typename Half<DT>::T*)out_lo)
  return with_half(dt, [&](auto t) -> int {
    constexpr int DT = decltype(t)::value;
    switch (c) {
      case 64: VDN_TL(1); break;
      case 128: VDN_TL(2); break;
      case 192: VDN_TL(3); break;
      case 256: VDN_TL(4); break;
      case 384: VDN_TL(6); break;
      case 512: VDN_TL(8); break;
      case 768: VDN_TL(12); break;
      case 1024: VDN_TL(16); break;
      default: return VDN_EUNSUPPORTED;
    }
    VDN_CHECK_LAUNCH();
    return VDN_OK;
  });
#undef VDN_TL
}
