/* vdn.h — C-ABI of libvdn_hip.so: the MI355X (gfx950) kernels behind
 * DepthAnythingV2.forward / VideoDepthAnything.forward.
 *
 * The reference has no FFI for this path: callers hold a torch.nn.Module and every op below is a
 * torch.nn.functional call inside it. Each entry point therefore names the
 * reference call site(s) it replaces (paths relative to the reference root). The Python host
 * mirror (video-depth-normal-v2_amd/vdn) binds these with ctypes; INTEGRATION.md shows the stub
 * a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers + sizes only; every buffer is caller-owned device memory (hipMalloc'd by
 *    PyTorch-ROCm), the library allocates nothing and keeps no state;
 *  - every launch is asynchronous on `stream` (torch.cuda.current_stream().cuda_stream);
 *  - return 0 on success, a negative vdn_status on a rejected argument, or -(1000+hipError_t);
 *  - "half" = the 16-bit MFMA operand type chosen per call by `dt`: VDN_F16 (IEEE fp16, default:
 *    same MFMA rate as bf16 with 8x smaller rounding, and what the reference's own video driver
 *    autocasts to, video_depth_anything/video_depth.py:106) or VDN_BF16;
 *  - activations are channels-last: tokens [B, N, C] == NHWC feature maps [B, H, W, C].
 */
#ifndef VDN_H
#define VDN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vdn_stream; /* hipStream_t */

enum vdn_status { VDN_OK = 0, VDN_EINVAL = -1, VDN_EUNSUPPORTED = -2, VDN_EALIGN = -3 };
enum vdn_dtype { VDN_F16 = 0, VDN_BF16 = 1, VDN_F32 = 2, VDN_NONE = 3 };
enum vdn_act { VDN_ACT_NONE = 0, VDN_ACT_GELU = 1, VDN_ACT_RELU = 2,
               VDN_ACT_SILU = 3 /* only as the gate of VDN_ST_GEGLU: out = h * silu(gate) (SwiGLU, dinov2_layers/swiglu_ffn.py:29-33) */ };
enum vdn_amode { VDN_A_PLAIN = 0, VDN_A_CONV3X3 = 1,
                 VDN_A_PAD3X3 = 2 /* 3x3 stride-1 convolution on padded-row operand planes (cross-term kernel only; see pad_hi) */ };
enum vdn_store {
  VDN_ST_PLAIN = 0,   /* out[row(m) * ldc + n]                                                   */
  VDN_ST_HEADS = 1,   /* n -> (split, head, e<64); per-split buffer, token- or dim-major          */
  VDN_ST_CONVT = 2,   /* ConvTranspose2d with kernel == stride: pixel-shuffle scatter to NHWC      */
  VDN_ST_GEGLU = 3    /* weight rows packed as 16-row blocks [h | gate]; out = h * gelu(gate), or h * silu(gate) with act = VDN_ACT_SILU */
};

/* Kernel-selection knobs of vdn_gemm (which tile / pipeline / split-K variant a shape gets; never what is computed beyond
 * fp32 summation order). The library holds NO mutable selection state: the defaults are read from the environment variables
 * named below once, at the first use (vdn_gemm_get_tuning returns them), and a launch that wants other values points its
 * descriptor's `tuning` at a struct of its own (tests pin a tile with force_bm; tools run A/B experiments). Thread-safe.   */
typedef struct vdn_gemm_tuning {
  int force_bm;     /* VDN_GEMM_BM       0 = cost model; 128 | 192 | 256 force the 8-wave kernels' M tile                  */
  int p8;           /* VDN_GEMM_P8       1 = ping-pong 3-product kernel at BM 256 (default), 2 = also BM 192, 0 = never   */
  int no_splitk;    /* VDN_GEMM_NOSPLITK 1 = never split K                                                                */
  int no_pipe;      /* VDN_GEMM_NOPIPE   1 = lock-step loop without the phase shift                                       */
  int splitk_p8;    /* VDN_SPLITK_P8     >= 2: K slices for deep residual linears on the ping-pong kernel                 */
  int cus;          /* VDN_GEMM_CUS      > 0 overrides the CU count tiles are sized for (else desc.cu_hint / 256)          */
  int splitk_occ;   /* VDN_SPLITK_OCC    split K when the 128-row tile grid covers <= this percent of the CUs (50)         */
  int splitk_max;   /* VDN_SPLITK_MAX    most K slices (8)                                                                */
  int min_tiles;    /* VDN_GEMM_MIN_TILES plain-A problems with fewer 128x256 tiles use the 4-wave 128x128 kernel (96)     */
  float f128, f192; /* VDN_GEMM_F128/F192 cost factors of the smaller M tiles of the 3-product kernels (1.3, 1.2)          */
  int x8;           /* VDN_GEMM_X8       1 (default): launches that carry A8 / W8 planes run on the 8-bit cross-term kernel; 0: rejected */
} vdn_gemm_tuning;
int vdn_gemm_get_tuning(vdn_gemm_tuning* out);   /* the environment-derived defaults */

/* One descriptor drives every GEMM-shaped op on the path:
 *   out = epilogue( A[M,K] x W[N,K]^T ),  half operands, fp32 accumulate on MFMA.
 * Replaces F.linear / nn.Conv2d(1x1, 3x3 s1|s2 p1) / nn.ConvTranspose2d(k==s) at:
 *   depth_anything_v2/dinov2_layers/attention.py:51,60 (qkv, proj), mlp.py:36,39 (fc1, fc2),
 *   patch_embed.py:76 (14x14 s14 conv == GEMM on patchified rows),
 *   depth_anything_v2/dpt.py:129-130 (projects, resize_layers), util/blocks.py:68-74 (RCU convs),
 *   :146 (out_conv), dpt.py:135-138 (layerN_rn), :145,148 (output_conv1/2),
 *   video_depth_anything/motion_module/motion_module.py:116,131 (proj_in/out), :273,280-281
 *   (to_q/k/v), :315 (to_out), attention.py:383-384 (GEGLU), :329 (ff out),
 *   sam2/modeling/sam/transformer.py:279-281,309 (q/k/v/out_proj), memory_attention.py:96
 *   (linear1/2), memory_encoder.py:108-110 (pwconv1/2), :172 (pix_feat_proj).                   */
typedef struct vdn_gemm_desc {
  int32_t dt;            /* vdn_dtype of A and W (VDN_F16 | VDN_BF16)                             */
  int32_t M, N, K;       /* K = logical reduction length (conv: 9*Cin), multiple of 8             */
  /* A operand */
  const void* A;         /* plain: half [M, lda]; conv: half NHWC [cB, cH, cW, cC]                */
  int32_t a_mode;        /* vdn_amode                                                             */
  int32_t lda;           /* elements                                                              */
  int32_t relu_a;        /* apply ReLU to A on load (ResidualConvUnit's activation on its input)  */
  int32_t cB, cH, cW, cC, cOH, cOW, cstride; /* conv geometry (pad 1), M == cB*cOH*cOW            */
  /* W operand: half [N, ldb], K-contiguous, zero-padded to ldb (multiple of 64, >= K)            */
  const void* W;
  int32_t ldb;
  /* epilogue, applied in fp32 in this order:
   *   v = acc + bias[n] + rowadd[m];  v = act(v);  v *= gamma[n];
   *   v += tab[(m % tab_mod + tab_off), n];  v += res1[m,n];  v += res2[m,n]                     */
  const float* bias;     /* [N] or NULL                                                           */
  const float* rowadd;   /* [M] or NULL                                                           */
  int32_t act;           /* vdn_act                                                               */
  const float* gamma;    /* [N] or NULL (LayerScale / CXBlock gamma)                              */
  const float* tab;      /* f32 [*, N] or NULL (pos_embed)                                        */
  int32_t tab_mod, tab_off;
  const void* res1;      /* [M, ldr1] or NULL                                                     */
  int32_t res1_dt, ldr1;
  const void* res2;
  int32_t res2_dt, ldr2;
  /* store */
  int32_t store;         /* vdn_store                                                             */
  void* out;             /* PLAIN/CONVT/GEGLU destination                                         */
  int32_t out_dt;        /* VDN_F16|VDN_BF16|VDN_F32                                              */
  int32_t ldc;
  int32_t row_group, row_skip; /* PLAIN: out row = m + (m / row_group + 1) * row_skip if row_group>0
                                  (patch tokens land after each image's cls row)                 */
  /* HEADS: N == nsplit * heads * 64. split s goes to dst[s]:
   *   token-major  [Bt, heads, tpad, 64]  (transposed[s] == 0)
   *   dim-major    [Bt, heads, 64, tpad]  (transposed[s] == 1, the V^T image the attention
   *                                        kernel reads with contiguous keys)
   * with m -> (bt = m / tokens, t = m % tokens + tok_off).
   * rope[s] != 0 rotates adjacent pairs (2i,2i+1) of each head by rope_cs[(t % rope_mod), i]
   * = (cos, sin) (sam2/modeling/position_encoding.py:212-239); requires the weight rows of that
   * split to be packed pair-split (VDN_PACK_ROPE of vdn_pack_weight below).                      */
  void* dst[3];
  int32_t nsplit, heads, tokens, tok_off, tpad;
  int32_t transposed[3];
  int32_t rope[3];
  const float* rope_cs;  /* f32 [rope_mod, 32, 2]                                                 */
  int32_t rope_mod;
  /* CONVT: N == ck*ck*cout, n = (ky*ck + kx)*cout + co; m = (b, y, x) on a cB x cH x cW grid;
   * out NHWC [cB, cH*ck, cW*ck, cout]                                                            */
  int32_t ck, cout;
  const void* zeros;     /* >= 16 bytes of zeros (conv padding taps / K tail read from here)      */
  /* Split-precision ("x3") planes, all optional. A 16-bit tensor t may come with a second plane
   * t_lo = half(t_exact - float(t_hi)); the kernel then accumulates
   *     A_hi*W_hi  +  A_hi*W_lo (if W_lo)  +  A_lo*W_hi (if A_lo)
   * as extra K segments of the same MFMA loop (fp32-faithful to ~2^-21 instead of 2^-11), and
   * half outputs are written as (hi = round-toward-zero, lo = remainder) when out_lo / dst_lo is
   * given. hi and lo share their sign, so relu_a acts on each plane independently. TRANSPOSED head splits (V^T) are the
   * exception: hi is rounded to nearest, and their dst_lo may be NULL on its own (the one-product P V attention reads hi only). */
  const void* A_lo;
  const void* W_lo;
  void* out_lo;
  void* dst_lo[3];
  const void* res1_lo;
  const void* res2_lo;
  /* conv K order: 0 = (tap, ci) ; 1 = (ci/64, tap, ci%64) — requires cC % 64 == 0. With order 1
   * consecutive K steps read the same pixels' neighbouring taps / the two halves of one 128-byte
   * line, so the 9x re-read of the input map is served from L2 instead of HBM.                   */
  int32_t conv_korder;
  /* Tile-shape hint: how many CUs this launch can count on (0 = the whole chip, 256). A caller that keeps two
   * independent launch streams busy passes 128: the M tile is then chosen for the share of the machine one
   * kernel really gets while the other stream's kernels co-run (measured +3.6 % end to end). Never changes results. */
  int32_t cu_hint;
  /* Optional split-K workspace (f32, caller-owned, >= 16-byte aligned): a 3x3 convolution whose tile grid covers
   * only a fraction of the chip (low-resolution maps with 9*Cin = 9216-deep reductions) is cut into up to 8 K
   * slices that write partial sums here and a second kernel adds them in a fixed order and applies the epilogue
   * (deterministic). NULL / 0 disables. `ksplit` is set by the library and must be 0 on entry.                */
  void* splitk_ws;
  int64_t splitk_ws_bytes;
  int32_t ksplit;
  /* HEADS, split-plane mode, VDN_F16 only: optional 8-bit planes of a token-major split s (Q / K) for the attention
   * kernel's cross terms (vdn_flash_attn Q8 / K8): u8 [Bt, heads, tpad, 128], per token 64 bytes of e5m2(v) followed by
   * 64 bytes of e5m2((v - hi(v)) * 2^10), same token mapping as dst[s]. NULL = not written. Must be NULL for
   * transposed splits. A split with 8-bit planes may leave its dst_lo NULL (the attention then never reads the fp16 lo plane).                                                                                            */
  void* dst8[3];
  /* Cross-term planes of the GEMM operands themselves (plain A, VDN_F16, K % 64 == 0; all three optional). When A8 and W8 are
   * given, the kernel accumulates A_hi W_hi^T on fp16 MFMAs and the two cross terms A_hi W_lo^T + A_lo W_hi^T on the
   * block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, e3m2 operands: 4.2x the fp16 rate) instead of two more fp16
   * products; A_lo / W_lo are then not read.
   *   A8 u8 [2, M, K], W8 u8 [2, N, ldb]: plane 0 describes hi(v), plane 1 the remainder v - hi(v); same row-major shape
   *   as the fp16 operand (lda == K), in "x6 rows": per row and 64 of K a 64-byte row-slab of two 32-byte HALVES (one per
   *   K half of the MFMA), each [24 B: 32 e3m2 codes, 6-bit fields, little-endian][1 B: E8M0 scale byte s, value = code
   *   2^(s - 127)][7 B unused]; s = floor(log2 max|hi| of the half) - 4 + 127 for plane 0 and 10 less for plane 1.
   *   WHICH 32 columns of the slab a half holds, and in what order, is the producer's choice (vdn_pack_x8 `order`): the
   *   hardware only needs A and W to agree, so the weight planes are packed in the order of the kernel that writes A.
   *   out8: the same planes of a half-precision output of the bias + GELU flavour (u8 [2, M, ldc], N == ldc, N % 64 == 0),
   *   written next to out / out_lo for the GEMM that consumes it (order 1). vdn_pack_x8 / vdn_layernorm / vdn_flash_attn
   *   (their out8 arguments) produce the planes of weights and of the other activations.                             */
  const void* A8;
  const void* W8;
  void* out8;
  /* K-tile-major operand planes of the 8-bit cross-term kernel (all 0 = row-major). A 16-bit plane [rows, K] is stored as
   * [K / 32][rows][32] and a byte plane as [K / 64][rows][64]: the 16 rows x 64 bytes one LDS-DMA instruction moves are then
   * one contiguous KiB (8 full cache lines) instead of 16 half-used lines — 67 against 44 GB/s per CU of L2 -> LDS feed.
   *   a_kt:   A and A8 are K-tile-major (lda is ignored; rows = M);   w_kt: W and W8 (rows = N, K extent = ldb; vdn_pack_x8);
   *   out_kt: a 16-bit PLAIN output (out, out_lo if given, out8) is WRITTEN K-tile-major with rows = M, columns = N == ldc,
   *           i.e. as the a_kt operand of the next GEMM (bias + GELU / plain half-plane flavours of the 8-bit kernel only).
   * vdn_layernorm and vdn_flash_attn produce the same layout (their `kt` arguments).                                      */
  int32_t a_kt, w_kt, out_kt;
  /* 8-bit cross-term kernel: which cross terms this launch accumulates. 0 = both (fp32-faithful, the default);
   * 1 = without A_lo W_hi^T (A enters as its 16-bit hi plane alone: 2^-12 per activation element);
   * 2 = without A_hi W_lo^T (W as its hi plane alone). A per-launch precision knob for the per-layer budget of
   * DESIGN.md §3 / profiles/r03_precision_budget.md; the engines pass 0 unless VDN_X8_TERMS says otherwise.           */
  int32_t x8_terms;
  const vdn_gemm_tuning* tuning;   /* NULL = the library defaults (vdn_gemm_get_tuning); else this launch's own knobs */
  /* Sub-pixel convolution: Conv2d(3x3, pad 1, no bias) o ConvTranspose2d(kernel == stride == ck, bias) as ONE implicit GEMM on
   * the LOW-resolution map (depth_anything_v2/dpt.py:129 resize_layers[0|1] followed by :135-136 layer1_rn / layer2_rn; no
   * non-linearity in between). Output pixel (ck y + a, ck x + b) is phase (a, b) of source pixel (y, x); its 3x3 window on the
   * ck-times map touches only the source neighbours (y + sy, x + sx) with sy in {-1, 0} for a == 0, {0, 1} for a == ck - 1,
   * {0} otherwise (sx alike): 1, 2 or 4 neighbours per phase. subpix != 0 selects the mode:
   *   a_mode = VDN_A_CONV3X3 on the source map (cstride 1, cOH == cH, cOW == cW, cC % 64 == 0, conv_korder 1);
   *   store = VDN_ST_CONVT with ck in {2, 4}, cout % 256 == 0, N == ck*ck*cout, half output with out_lo (pixel-shuffle
   *   scatter into NHWC [cB, cH*ck, cW*ck, cout] planes); split planes A_lo / W_lo required; K == ldb == 4 * cC.
   *   W row n = (a*ck + b)*cout + co holds its phase's neighbours in the order (sy ascending, sx ascending) as
   *   K = (ci/64, neighbour slot, ci%64), stored RAGGED: the first cC * (neighbours of the phase) elements of the row, the rest
   *   of the row is never read. A workgroup walks only its phase's K.
   *   subpix_bias f32 [ck*ck, 4, cout]: the transposed convolution's bias seen through the taps that land in neighbour slot s
   *   of the phase (unused slots are not read). A neighbour outside the map drops out WHOLE, its bias share included (the
   *   high-resolution pixels it would produce lie in the 3x3 conv's zero padding), so the bias of a row is the sum over the
   *   slots whose neighbour is inside; `bias`, act, rowadd, gamma, tab, res1 / res2 must be unset.
   * vdn/pack.py subpixel_conv builds both from the reference's parameters.                                                */
  int32_t subpix;
  const float* subpix_bias;
  /* Padded-row operand planes: a 3x3, stride-1, pad-1 convolution F -> N as a cross-term GEMM whose nine taps are row shifts
   * (a_mode = VDN_A_PAD3X3; the ResidualConvUnit convolutions of the two high-resolution fusion blocks, util/blocks.py:68-74).
   * An operand map is NHWC with a one-pixel ZERO RING per frame: Mp = cB (cH + 2) (cW + 2) rows of cC channels, row
   * (b, y, x) = (b (cH + 2) + y) (cW + 2) + x with the image at y in 1..cH, x in 1..cW. It is stored as the K-tile-major planes of
   * a_kt above: fp16 hi [cC / 32][Mp][32] and the two planes of x6 rows [cC / 64][Mp][64] (A8; plane 1 follows plane 0), and
   * every allocation carries cW + 3 GUARD ROWS (64 bytes each) in front of its first plane and behind its last: tap (dy, dx) of
   * output row m is row m + dy (cW + 2) + dx of the same plane, for every row including the ring, a wave-uniform shift that
   * stays inside the allocation. Ring pixels hold zero bits in all three planes (a zero code is zero under any scale byte), so
   * the shifted rows ARE the convolution's zero padding; what a ring row itself accumulates is never stored.
   *   M = Mp, K = 9 cC = ldb, cC % 64 == 0 and <= 4096, a_kt = w_kt = 1; W / W8 from vdn_pack_x8 (order 1) of the weight in
   *   K = (tap, channel) order (VDN_PACK_CONV3X3_TAPS); fp16 only; cOH, cOW, cstride, lda, relu_a unused (0).
   * Two epilogues, both with N == ldc, N % 64 == 0:
   *   act = VDN_ACT_RELU, out_kt = 1, out + out8, no residual: relu(acc + bias) as the padded operand planes of the NEXT such
   *     convolution (out = its fp16 hi plane, out8 = its x6 rows, guards as above; ring rows are written as zero bits).
   *   act = VDN_ACT_NONE, out_kt = 0, out + out_lo, res1 (+ res2) with their lo planes: v = acc + bias + res1 [+ res2] on the
   *     UNPADDED rows (b cH + y - 1) cW + x - 1 of row-major split planes [cB cH cW, ld*] (ring rows read and store nothing
   *     there); when pad_hi and out8 are given, relu(v) is also written as padded operand planes (pad_hi = fp16 hi plane,
   *     out8 = x6 rows; ring rows zero bits).                                                                              */
  void* pad_hi;
} vdn_gemm_desc;

int vdn_gemm(const vdn_gemm_desc* d, vdn_stream stream);

/* LayerNorm over the last dim of [rows, C] (fp32 statistics, two-pass in registers).
 *   y = LN(x) * w + b;  y += alpha * addvec[c];  y += addtab[(row / tab_div) % tab_mod, c]
 * writes out_h (half, optional) and out_f (f32, optional).
 * Replaces nn.LayerNorm at dinov2_layers/block.py:84,87 + dinov2.py:310 (eps 1e-6),
 * memory_attention.py:60,74,93,162 (eps 1e-5), motion_module.py:179,189 (eps 1e-5, with the
 * sinusoidal PE add of :211 fused as addtab), LayerNorm2d sam2_utils.py:148-153 on NHWC rows.
 *   out_group > 0 drops the first row of every `out_group` rows (the cls token, dinov2.py:312)
 *   and writes the remaining rows compacted.
 *   out8 (VDN_F16, C % 64 == 0, optional): u8 [2, rows, C], the x6 rows of y (vdn_gemm_desc.A8; order 0): the A8 planes of the
 *   GEMM that consumes y (out_h_lo may then be NULL). kt != 0: out_h / out_h_lo / out8 are written K-tile-major (vdn_gemm_desc.a_kt). */
int vdn_layernorm(const void* x, int x_dt, int rows, int C, const float* w, const float* b, float eps,
                  const float* addvec, float alpha, const float* addtab, int tab_div, int tab_mod,
                  int out_group, void* out_h, void* out_h_lo, int h_dt, float* out_f, void* out8, int kt,
                  vdn_stream stream);

/* Fused attention forward, head_dim 64: out[b, q, h*64+e] = softmax(scale * Q K^T) V.
 *   Q  half [BH, nq_pad, 64] (rows >= nq never read), K half [BH, nk_pad, 64],
 *   Vt half [BH, 64, nk_pad] (dim-major; columns >= nk must be finite), nk_pad % 64 == 0.
 * Scores never touch HBM. Replaces dinov2_layers/attention.py:53-59 and
 * F.scaled_dot_product_attention at sam2/modeling/sam/transformer.py:306.
 *   Q8 / K8 (both or neither; split fp16 planes only): the 8-bit planes vdn_gemm wrote through dst8
 *   (u8 [BH, n_pad, 128]); the two cross terms K_hi Q_lo^T + K_lo Q_hi^T of the scores then run on the block-scaled
 *   8-bit MFMA (e5m2, 2.3x the fp16 rate) instead of two fp16 products; logits stay within ~1e-5. NULL = 3 fp16 products.
 *   out8 (with Q8 / K8 only, optional): u8 [2, B nq, H 64], the x6 rows of the output (vdn_gemm_desc.A8; order 2): the A8 planes of
 *   the projection that consumes the output (out_lo may then be NULL); out_kt != 0: out / out_lo / out8 are written K-tile-major
 *   with rows = B nq (vdn_gemm_desc.a_kt).                                                                                 */
int vdn_flash_attn(int dt, const void* Q, const void* K, const void* Vt, void* out, const void* Q_lo,
                   const void* K_lo, const void* Vt_lo, void* out_lo, const void* Q8, const void* K8, void* out8, int out_kt,
                   int B, int H, int nq, int nq_pad, int nk, int nk_pad, float scale, int pv_products, vdn_stream stream);
/* pv_products (split-plane mode only; 0 = the default, 1): MFMA products per P V term — a PER-CALL argument, the library keeps
 * no selection state. 2: the softmax weights, born in registers, are rounded once to 16 bits and the row sum uses the same
 * rounded weights (O = sum p~ V / sum p~, V at 21 bits): each weight is off by <= 2^-11 relative, common factors cancel.
 * 3: P is split into hi / lo planes too (every output within ~1e-6 of fp64 at ~13 % more kernel time; reads the fp16 lo
 * planes of Q and K, so their producer must write them). 1 (fp16 planes with Q8 / K8 only, else treated as 2): V enters as
 * its hi plane alone, which the producer rounds to nearest (vdn_gemm writes the hi plane of TRANSPOSED head splits that
 * way; lo = remainder): every output element is a convex combination of fp16-rounded V values, i.e. within 2^-12 relative of
 * the 2-product result at worst; 2e-5..9e-5 end to end on the fixtures against the 1e-3 tolerance (2: 7e-6..2e-5), 14-17 %
 * less kernel time. A memory bank keeps the V planes its producer wrote: use one value per model. */

/* Temporal attention over <=64 frames per (pixel, head) (32 in the 32-frame windows, 64 in the v5 refiner): qkv half [(b f), D, 3c] packed
 * [q | k | v], out half [(b f), D, c]. Replaces motion_module/attention.py:182-211 (_attention)
 * with the rearranges of motion_module.py:255,320. rope_cs (pe = 'rope', motion_module.py:236-240,279-282; NULL for 'ape',
 * whose position term enters before the projections): f32 [T, c/2, 2] = (cos, sin)(t * 10000^(-2i/c)); adjacent channel
 * pairs (2i, 2i+1) of q and k are rotated by their frame's angles on load (attention.py:403-429).                       */
int vdn_temporal_attn(int dt, const void* qkv, void* out, const void* qkv_lo, void* out_lo, int Bv, int T, int D,
                      int c, int heads, float scale, const float* rope_cs, vdn_stream stream);

/* GroupNorm over NHWC half [F, HW, C] (fp32 stats per (frame, group)); `partial` is
 * f32 [F, nsplit, groups, 2] scratch. Replaces motion_module.py:112 (32 groups, eps 1e-6).       */
int vdn_groupnorm(int dt, const void* x, const void* x_lo, void* y, void* y_lo, int F, int HW, int C, int groups,
                  const float* w, const float* b, float eps, float* partial, int nsplit, vdn_stream stream);

/* Bilinear resize, align_corners=True, NHWC half (C % 8 == 0) or single-channel f32.
 * Replaces F.interpolate at util/blocks.py:144, dpt.py:147, depth_anything_v2.py:63,
 * video_depth.py:63.                                                                             */
int vdn_upsample_bilinear(int dt, const void* x, const void* x_lo, void* y, void* y_lo, int B, int IH, int IW, int OH,
                          int OW, int C, vdn_stream stream);
int vdn_upsample_bilinear_f32(const float* x, float* y, int B, int IH, int IW, int OH, int OW, int relu,
                              vdn_stream stream);

/* f32 NCHW image [B,3,H,W] -> half rows [B*ph*pw, ldk] with k = (c*14+ky)*14+kx, zero tail.
 * (the im2col-free view of PatchEmbed's 14x14 stride-14 conv, patch_embed.py:76)                 */
int vdn_patchify(int dt, const float* img, void* rows, void* rows_lo, int B, int H, int W, int ldk,
                 vdn_stream stream);

/* x[b*rows_per_b + row, :] = vec[:] (cls_token + pos_embed[0], dinov2.py:219-220)                */
int vdn_fill_row(float* x, const float* vec, int B, int rows_per_b, int row, int C, vdn_stream stream);

/* Bicubic resample (A=-0.75, align_corners=False, src = (dst+0.5)/scale - 0.5, clamped taps) of a
 * channels-last f32 [ih, iw, C] grid to [oh, ow, C]: torch's scale-factor bicubic used on the
 * pos_embed grid (dinov2.py:193-203, scale_rows = sx, scale_cols = sy there) and the same
 * kernel cv2.INTER_CUBIC applies to frames (util/transform.py:113).                               */
int vdn_bicubic(const float* src, float* dst, int ih, int iw, int oh, int ow, int C, float scale_rows,
                float scale_cols, vdn_stream stream);

/* The whole pre-processing of a batch of frames in ONE launch (depth_anything_v2.py:67-92, util/transform.py:109-157,
 * video_depth.py:73-99): u8 [n, h, w, 3] HOST-ORDER RGB (swap_rb = 0) or BGR (swap_rb = 1: cv2.cvtColor(BGR2RGB)) -> /255 ->
 * cubic resize to (H, W) with the taps of vdn_bicubic (identity when (H, W) == (h, w)) -> (v - mean[c]) / std[c] ->
 * f32 [n, 3, H, W]. mean3 / std3: 3 HOST floats each (ImageNet: .485 .456 .406 / .229 .224 .225).                    */
int vdn_preprocess(const uint8_t* frames, int n, int h, int w, int swap_rb, float* out, int H, int W, const float* mean3,
                   const float* std3, vdn_stream stream);

/* y = x + alpha * vec[c]  (memory_attention.py:141)                                               */
int vdn_add_vec(const float* x, const float* vec, float alpha, float* y, int rows, int C, vdn_stream stream);

/* depth[m] = (relu?) (bias + sum_c w[c] * feat[m, c]), feat half [M, C<=64] already ReLU'd
 * (the 1x1 conv + ReLU closing output_conv2, dpt.py:111-112)                                      */
int vdn_head_out(int dt, const void* feat, const void* feat_lo, const float* w, float bias, float* depth, int M,
                 int C, int relu, vdn_stream stream);

/* Final activation of a DPT head's last 1x1 convolution (vdn_head_out_act, vdn_depth_tail_act):
 *   VDN_OUT_NONE     v                          (the signed map in front of the activation)
 *   VDN_OUT_RELU     max(v, 0), NaN passes      (depth_anything_v2/dpt.py:112)
 *   VDN_OUT_SIGMOID  out_scale * sigmoid(v)     (metric_depth/depth_anything_v2/dpt.py:112-113 composed with the
 *                    `* max_depth` of its callers: dpt.py:183, metric_depth/train.py:131,165-166), the sigmoid in fp32 and
 *                    ONE multiply by out_scale; v -> -inf gives exactly 0, v -> +inf exactly out_scale, NaN passes.
 * out_scale is read by VDN_OUT_SIGMOID only.                                                                              */
enum { VDN_OUT_NONE = 0, VDN_OUT_RELU = 1, VDN_OUT_SIGMOID = 2 };

/* vdn_head_out with the final activation `act` (the unfused end of the metric-depth head, metric_depth/depth_anything_v2/
 * dpt.py:112-113). vdn_head_out(relu) is this entry with act = relu ? VDN_OUT_RELU : VDN_OUT_NONE.                        */
int vdn_head_out_act(int dt, const void* feat, const void* feat_lo, const float* w, float bias, float* depth, int M,
                     int C, int act, float out_scale, vdn_stream stream);

/* MaskDownSampler stages of memory_block.py:72-75 (sam2/modeling/memory_encoder.py:36-58):
 * stage 1: sigmoid -> conv3x3 s2 p1 (1->4) -> LayerNorm2d -> GELU -> conv1x1 (4->1)
 * stage 2:            conv7x7 s7    (1->49) -> LayerNorm2d -> GELU -> conv1x1 (49->1)
 * w: packed f32 parameter block [conv w | conv b | ln w | ln b | proj w | proj b].                */
int vdn_mask_down1(const float* depth, float* out, int B, int H, int W, int OH, int OW, const float* w,
                   vdn_stream stream);
int vdn_mask_down2(const float* in, float* out, int B, int H, int W, int OH, int OW, const float* w,
                   vdn_stream stream);

/* Depthwise 7x7 pad 3 conv on f32 NHWC [B,H,W,C], w f32 [49, C], bias [C] (CXBlock.dwconv,
 * memory_encoder.py:101).                                                                         */
int vdn_dwconv7(const float* x, float* y, int B, int H, int W, int C, const float* w, const float* bias,
                vdn_stream stream);

/* y(half planes) = x(f32) + tab[(row / tab_div) % tab_mod]: the sinusoidal frame-position add of
 * motion_module.py:211 applied to a window assembled from cached (already LayerNorm-ed) states in the
 * streaming mode (video_depth_stream.py:133-144, motion_module.py:255-266).                        */
int vdn_addtab_cast(int dt, const float* x, const float* tab, int tab_div, int tab_mod, void* y, void* y_lo,
                    size_t rows, int C, vdn_stream stream);

/* Streaming temporal attention over a PROJECTED key/value cache (video_depth_stream.py:133-158,
 * motion_module.py:255-277). pool: a caller-owned ring of frame slots, f32 [slots, slot_stride >= HW*3c];
 * a slot holds one cached frame's [HW, 3c] = (q | k | v) projections of its LayerNorm-ed hidden state WITHOUT the
 * frame-position term. slots: HOST array of the T ring-slot indices of the window, oldest first (copied into the launch
 * arguments: no pointer table in HBM, nothing allocated per step). pe_q / pe_k / pe_v: f32 [>= T, c] =
 * PositionalEncoding.pe @ W_{q,k,v}^T (added on load: W(x + pe) = Wx + W pe). Only the newest frame (slots[T-1],
 * position T-1) queries; 8 heads of c/8; out: half planes [HW, c] (out_lo may be NULL).
 * c in {64, 128, 192, 256, 384, 512, 768, 1024}, T <= 32.                                                            */
int vdn_temporal_attn_last(int dt, const float* pool, size_t slot_stride, const int32_t* slots, int T, int HW, int c,
                           const float* pe_q, const float* pe_k, const float* pe_v, float scale, void* out, void* out_lo,
                           vdn_stream stream);

/* Device-side window stitcher of VideoDepthAnything.infer_video_depth (video_depth.py:118-156):
 * vdn_stitch_fit   — closed-form least-squares scale/shift of `pred` onto `target` over n f32 values with an all-ones
 *                    mask (compute_scale_and_shift_full, utils/util.py:40-62): coef[0..1] = {scale, shift}, {1, 0} when
 *                    the normal matrix is singular. Deterministic fp64 sums; `workspace` = vdn_stitch_workspace_bytes().
 * vdn_stitch_apply — for a window [T, hw] f32: frames align_len..overlap-1 are clamped-affine-mapped and cross-faded
 *                    into out_tail[overlap-align_len, hw] with weights 0, 1/(n-1), .., 1 (get_interpolate_frames,
 *                    utils/util.py:65-73), frames overlap..T-1 are mapped into out_new, and the mapped frame
 *                    `ref_frame` is also written to ref1 (the moving second alignment target, video_depth.py:150-152). */
size_t vdn_stitch_workspace_bytes(void);
int vdn_stitch_fit(const float* pred, const float* target, size_t n, void* workspace, float* coef, vdn_stream stream);
int vdn_stitch_apply(const float* window, const float* coef, float* out_tail, float* out_new, float* ref1, size_t hw,
                     int T, int align_len, int overlap, int ref_frame, vdn_stream stream);

/* Window stitcher of VideoDepthEstimationModel.infer_video (the depth + normal model's clip driver): one launch maps, blends
 * and stores one window's depth f32 [T, hw] and normal f32 [T, 3, hw] (nx, ny, nz planes) into the clip, whose frame `start`
 * out_depth [>= keep, hw] and out_normal [>= keep, 3, hw] point at. coef = {scale, shift} on the device (vdn_stitch_fit's,
 * or {1, 0}). With d' = d * scale + shift (a multiply, then an add: two float32 roundings), clamped as d' < 0 ? 0 : d' if and
 * only if clamp0 (a NaN stays a NaN), and n' = (scale * nx, scale * ny, 1), the gradient of the mapped depth, which the clamp
 * does not alter:
 *   frames t < overlap         : out = out * (1 - w_t) + new * w_t for depth, nx and ny, w = 0, 1 * (1 / (overlap-1)), .., 1
 *                                (get_interpolate_frames, utils/util.py:65-73), every operation rounded to float32; nz = 1
 *   frames overlap <= t < keep : out = new (nz = 1)
 *   frames t >= keep           : neither read nor written (the window's pad slots behind the end of the clip).
 * overlap = 0 is a first window: nothing of out_* is read. VDN_EINVAL, nothing written, for a NULL pointer, hw == 0, T < 1,
 * T > 8192, overlap < 0, overlap == 1 (no cross-fade has one frame), overlap > T / 2, keep < 1, keep > T, or keep <= overlap
 * when overlap > 0. No alignment is required: 16-byte accesses are used where hw % 4 == 0 and all four tensors are 16-byte
 * aligned, 4-byte ones otherwise. Launch grid: y = 4 * keep (frame, plane) pairs, x = min(ceil(groups / 256),
 * max(1, 2048 / (4 * keep))) blocks of 256 lanes striding over the plane's groups = hw / 4 (or hw) pixel groups.        */
int vdn_dn_stitch_apply(const float* depth, const float* normal, const float* coef, float* out_depth, float* out_normal,
                        size_t hw, int T, int overlap, int keep, int clamp0, vdn_stream stream);

/* Clip evaluation on the device: eval_single_by_data of eval_depthcrafter/eval.py:55-151 with the seven eval_metrics of
 * eval_depthcrafter/metric.py, for pred f32 [frames, H, W], gt f32 [frames, H, W] and an optional mask u8 [frames, H, W]
 * (NULL = all ones; non-zero = use). valid = gt > dmin && gt < dmax && mask, compared in float32 as numpy does for a
 * float32 gt. What the reference computes in float64 is fp64 here; sums have a fixed order and use no atomics, so two runs
 * give the same bits. Pointers need only their type's alignment (pred / gt 4 bytes, workspace / coef / out 8 bytes):
 * loads are one element per lane. VDN_EINVAL: a null pointer (mask excepted), a size <= 0, dmin >= dmax (or a NaN bound),
 * an unknown domain or TGM mode.
 * vdn_eval_fit     — coef[0..1] = (scale, shift) minimising sum over valid pixels of (scale * p + shift - t)^2,
 *                    p = max((double)pred, dmin), t = gt (VDN_EVAL_DISP) or 1 / ((double)gt + 1e-8) (VDN_EVAL_DEPTH);
 *                    closed form on the normal equations (eval.py:81-107 solves the same system by SVD). When every
 *                    valid p is the same value c the system has rank 1 and the result is lstsq's minimum-norm solution
 *                    (c, 1) * mean(t) / (c * c + 1); without any valid pixel coef = (NaN, NaN). Also leaves the per-frame
 *                    valid counts in `workspace` for vdn_eval_metrics.
 * vdn_eval_metrics — must follow vdn_eval_fit on the same pred / gt / mask / bounds / workspace. a = clip(aligned, dmin,
 *                    dmax) with aligned = max(scale * p + shift, dmin) (separate multiply and add roundings), inverted
 *                    first for VDN_EVAL_DEPTH. Per frame with a valid pixel: |a - g|, |a - g| / g, (a - g)^2 and the counts
 *                    of max(a / g, g / a) < 1.25, 1.25^2, 1.25^3 over its valid pixels; frames without one are dropped.
 *                    out[0..6] = abs_relative_difference, delta1_acc, temporal_gradient_matching_error, abs_difference,
 *                    rmse_linear, delta2_acc, delta3_acc: the mean over the kept frames of the per-frame quotient. The
 *                    three delta values are float32 quotients and a float32 mean (summed in frame order), widened.
 *                    TGM = mean of sum |da - dg| / count over valid[first] && dg < 0.05f, dg a float32 difference of gt:
 *                    VDN_EVAL_TGM_ROWS   the pair is (y, y + 1) of one frame, per kept frame over (H - 1) x W — what the
 *                                        reference computes, since it slices dim 1 of [T, H, W] tensors;
 *                    VDN_EVAL_TGM_FRAMES the pair is a kept frame and the next kept one, per pair over H x W —
 *                                        metric.py:3-33 as written for [B, S, H, W].
 *                    0 / 0 stays NaN (a kept frame with an empty TGM mask, H == 1, no kept frame).
 * vdn_resize_bilinear_hp — f32 [frames, IH, IW] -> [frames, OH, OW], half-pixel centres (align_corners=False, the
 *                    geometry of cv2.resize's default INTER_LINEAR, eval.py:42-53), no antialiasing.              */
enum vdn_eval_domain { VDN_EVAL_DEPTH = 0, VDN_EVAL_DISP = 1 };
enum vdn_eval_tgm { VDN_EVAL_TGM_ROWS = 0, VDN_EVAL_TGM_FRAMES = 1 };
size_t vdn_eval_workspace_bytes(int frames);
int vdn_eval_fit(const float* pred, const float* gt, const uint8_t* mask, int frames, size_t hw, double dmin, double dmax,
                 int domain, void* workspace, double* coef, vdn_stream stream);
int vdn_eval_metrics(const float* pred, const float* gt, const uint8_t* mask, int frames, int H, int W, double dmin,
                     double dmax, int domain, int tgm, const double* coef, void* workspace, double* out,
                     vdn_stream stream);
int vdn_resize_bilinear_hp(const float* x, float* y, int frames, int IH, int IW, int OH, int OW, vdn_stream stream);

/* Normal evaluation on the device: normal_vector / sobel_ix_iy of utils/normal_utils.py:4-52 and VideoNormalLoss of
 * loss/loss.py:370-409 (the one measure of normal quality the reference has; scripts/train*.py validate, and with
 * vdn_normal_loss_backward below the training step). f32 inputs,
 * frames are [H, W] row-major. Stateless, caller's stream, caller-owned buffers. The stencil, the normalisation and the
 * cosine are fp64 computed from the f32 samples (separate multiply and add roundings: contraction is off); sums have a
 * fixed order (a lane's stride through its block's share, the lanes of a wave by xor-shuffle, the four waves, a frame's
 * blocks in index order, the frames in index order) and use no atomics, so two runs give the same bits. Float pointers
 * need 4-byte alignment only (VDN_EALIGN otherwise; workspace, frame_sums, frame_counts and out 8 bytes); where pred and
 * target are 16-byte aligned and H * W is a multiple of 4, vdn_normal_eval reads them four floats per lane.
 * VDN_EINVAL: a null required pointer, frames <= 0, H < 2 or W < 2 (the reference's reflect pad raises there).
 * VDN_EUNSUPPORTED: H * W > INT32_MAX. All of these are returned before anything is launched.
 * The stencil: Ix, Iy = cross-correlation of the reflect-padded map (no edge repeat) with kx = [[1,0,-1],[2,0,-2],[1,0,-1]]
 * and ky = [[1,2,1],[0,0,0],[-1,-2,-1]], both divided by 8 when normalize_kernel != 0.
 * vdn_sobel_ix_iy     — ix, iy f32 [frames, H, W] = Ix, Iy, each rounded to f32 once.
 * vdn_normal_vector   — out f32 [frames, 3, H, W] = (-scale_xy Ix, -scale_xy Iy, scale_z) / sqrt(nx^2 + ny^2 + nz^2 + eps),
 *                       each component rounded to f32 once. scale_xy, scale_z and eps are the float32 values given (the
 *                       reference multiplies float32 tensors by them), widened.
 * vdn_erode_mask3     — out u8 [frames, H, W] = 1 where mask and all of its 3 x 3 neighbours inside the image are
 *                       non-zero, else 0: eroded_mask of loss.py:380-387, whose convolution zero-pads the inverted mask,
 *                       so positions outside the image never erode a border pixel.
 * vdn_normal_eval     — pred f32 [frames, 3, H, W]; target f32 [frames, 3, H, W] of any length (target_is_depth == 0) or a
 *                       depth map f32 [frames, H, W] (target_is_depth != 0), whose normal is computed per pixel as
 *                       vdn_normal_vector does with its defaults (kernel / 8, scales 1, eps 1e-8f), held in fp64 and never
 *                       written; mask u8 [frames, H, W], non-zero = use, NULL = all ones. Over the pixels the erosion
 *                       of vdn_erode_mask3 keeps: cos = sum_c (a_c / max(|a|, 1e-8)) * (b_c / max(|b|, 1e-8)), which is
 *                       F.cosine_similarity of torch 2.x; a NaN there is a NaN in the sums. A dropped pixel is selected
 *                       away, never multiplied by zero: NaN or inf under it reaches nothing.
 *                       frame_sums[f] = sum of cos, frame_counts[f] = kept pixels (both may be NULL);
 *                       out[0] = 1 - (sum over frames) / count, or 1.0 when count == 0 (reduction_batch_based returns
 *                       sum * 0 there); out[1] = count. One pass over the inputs, a frame's blocks leave partials in
 *                       `workspace` (vdn_normal_eval_workspace_bytes(frames)), a one-block finalise reduces them.       */
size_t vdn_normal_eval_workspace_bytes(int frames);
int vdn_sobel_ix_iy(const float* depth, float* ix, float* iy, int frames, int H, int W, int normalize_kernel,
                    vdn_stream stream);
int vdn_normal_vector(const float* depth, float* out, int frames, int H, int W, int normalize_kernel, float scale_xy,
                      float scale_z, float eps, vdn_stream stream);
int vdn_erode_mask3(const uint8_t* mask, uint8_t* out, int frames, int H, int W, vdn_stream stream);
int vdn_normal_eval(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int frames, int H,
                    int W, void* workspace, double* frame_sums, int64_t* frame_counts, double* out, vdn_stream stream);

/* The gradient of vdn_normal_eval's out[0] with respect to pred, times a coefficient: what autograd computes for
 * g * normal_loss of the reference's VideoNormalLoss. pred, target, target_is_depth, mask, frames, H and W as for
 * vdn_normal_eval; a target made from depth is a constant of the differentiation.
 *   count   device pointer to the forward's kept count N, the out[1] vdn_normal_eval wrote for the same inputs (fp64)
 *   coeff   device pointer to g, the gradient arriving at the loss (fp64)
 *   grad_pred f32 [frames, 3, H, W], every element written exactly once
 * F.cosine_similarity clamps both norms to 1e-8 outside the graph, so autograd differentiates sum_c (p_c / n) (t_c / n_t)
 * with n = max(|p|, 1e-8), n_t = max(|t|, 1e-8) as if dn/dp = p / |p| on both sides of the clamp, and 0 at |p| = 0. With
 * that = t / n_t:
 *   kept pixel     grad_c = -(g / N) * (that_c - ((p . that) / n) * (p_c / |p|)) / n        (p_c / |p| := 0 where |p| = 0)
 *   dropped pixel  +0.0 in all three channels; it is skipped, never multiplied by zero, so NaN or inf under it reaches nothing
 *                  (the reference writes NaN there)
 *   N == 0         +0.0 everywhere
 * fp64 from the f32 samples, contraction off, 1 / n and 1 / n_t formed once per pixel, one rounding to f32 at the store. One
 * launch, no workspace, no atomics, no host synchronisation; an element depends on its own pixel alone, so the two load shapes
 * (four pixels per lane with 16-byte loads and stores where pred, grad_pred and a stored target are 16-byte aligned and H * W
 * is a multiple of 4; one pixel per lane otherwise) and two runs give the same bits.
 * VDN_EINVAL: a null pointer other than mask, frames <= 0, H < 2 or W < 2. VDN_EUNSUPPORTED: H * W > INT32_MAX. VDN_EALIGN:
 * a float pointer off 4 bytes, count or coeff off 8. All returned before anything is launched.
 * vdn_normal_loss_backward_trip(wide): the pixels of a frame that one trip of the grid covers (64 blocks x 256 lanes x 4 or
 * 1); a larger frame sends the lanes round their stride loop again.                                                        */
int vdn_normal_loss_backward_trip(int wide);
int vdn_normal_loss_backward(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int frames,
                             int H, int W, const double* count, const double* coeff, float* grad_pred, vdn_stream stream);

/* Angular error of predicted normals, and normals as a picture. An extension beyond the reference, which has the criterion
 * above and nothing else for normals. pred, target, target_is_depth and mask as for vdn_normal_eval.
 * The angle of a pixel with prediction a and target b, three f32 components each, widened to fp64:
 *   b        the stored target, or with target_is_depth (-Ix, -Iy, 1) of the Sobel / 8 stencil on the reflect-padded depth;
 *            the division by sqrt(|.|^2 + 1e-8) of vdn_normal_vector does not change the direction and is not applied;
 *   angle    atan2(|a x b|, a . b) * 180 / pi, every product and sum rounded on its own (contraction is off). Not acos of a
 *            cosine: that loses half the digits near 0 and 180 degrees;
 *   NaN      when any of the six components is NaN or +-inf; otherwise 90 when |a|^2 == 0 or |b|^2 == 0, the angle whose
 *            cosine is the 0 that the clamped norms of F.cosine_similarity give the criterion.
 * Kept pixels: mask non-zero (NULL = all ones), after the erosion of vdn_erode_mask3 when erode != 0, which is what
 * vdn_normal_eval scores. A dropped pixel is selected away and never multiplied: NaN under it reaches nothing.
 * vdn_normal_angle_map   — out f32 [frames, H, W]: the angle rounded to f32 once, NaN at a dropped pixel.
 * vdn_normal_angle_stats — rows f64 [1 + B + B T][9]: row 0 all kept pixels of the batch, rows 1 .. B each item, rows 1 + B ..
 *                          each frame. Columns n, mean, median, rmse, a5, a7_5, a11_25, a22_5, a30: the kept pixels, the mean
 *                          angle, numpy.median of the angles rounded to f32 (the mean of the two middle values for even n,
 *                          taken in fp64), sqrt(mean(angle^2)), and the share of kept pixels with angle < 5, 7.5, 11.25,
 *                          22.5 and 30 degrees (strict, compared in fp64). A set with n == 0 has n = 0 and NaN elsewhere; a set
 *                          with a NaN angle under a kept pixel has NaN in every column but n, and the sets that do not
 *                          contain it are untouched.
 *                          One sweep over the inputs leaves per-block partial sums and the f32 angle plane in `workspace`
 *                          (vdn_normal_angle_stats_workspace_bytes(B, T, H, W); 8-byte aligned); a one-block fold makes the
 *                          sums of frames, items and batch and the two median ranks of every set; the exact three-pass
 *                          radix select runs over the plane for frames, items and batch. Sums are fp64 in a fixed order (a
 *                          lane's stride, the wave's xor-shuffle, the four waves, a frame's blocks, an item's frames and
 *                          the items, each in index order) without floating-point atomics; the select's integer
 *                          histograms are exact in any order: two runs give the same bits. A lane owns four consecutive
 *                          pixels whenever H * W is a multiple of 4 (by 16-byte loads where pred, a stored target and the
 *                          workspace are 16-byte aligned, a load per pixel otherwise), so the order depends on the shape
 *                          alone, not on where a tensor starts.
 * vdn_normal_colorize    — x f32 [N, 3, H, W] normals of any length, or with from_depth a depth map [N, H, W] whose normal
 *                          is made per pixel as above; out u8 [N, H, W, 3], no alignment needed.
 *                          v_c = ((a_c / |a|) * 0.5 + 0.5) * 255 in fp64 with separate roundings, byte = (uint8)floor(v_c +
 *                          0.5); x, y, z go to R, G, B, reversed when bgr != 0. A zero or non-finite vector gives 128, 128, 128.
 * VDN_EINVAL: a null required pointer, a size <= 0, H < 2 or W < 2 (vdn_normal_colorize: only with from_depth).
 * VDN_EUNSUPPORTED: H * W > INT32_MAX, frames or B * T > 65535, B * T * H * W >= 2^32 (vdn_normal_angle_stats: the batch is
 * one set of the select). VDN_EALIGN: a float pointer off 4 bytes, workspace or rows off 8. All returned before anything is
 * launched.                                                                                                              */
int vdn_normal_angle_map(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int erode, int frames,
                         int H, int W, float* out, vdn_stream stream);
size_t vdn_normal_angle_stats_workspace_bytes(int B, int T, int H, int W);
int vdn_normal_angle_stats(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int erode, int B, int T,
                           int H, int W, void* workspace, double* rows, vdn_stream stream);
int vdn_normal_colorize(const float* x, int from_depth, int bgr, uint8_t* out, int N, int H, int W, vdn_stream stream);

/* The depth criterion on the device: VideoDepthLoss of loss/loss.py:326-367 as the reference's scripts construct it
 * (trim = 0, batch-based reduction, no SSIM term), the forward (its gradient: vdn_depth_loss_backward below);
 * scripts/train*.py validate:
 *     loss_dict = criterion(prediction=pred, target=gt, mask=valid)      (all [B, T, H, W])
 * prediction, target f32 [B, T, H, W] row-major, mask u8 [B, T, H, W] (non-zero = keep, required). Stateless, caller's
 * stream, caller-owned buffers.
 * Arithmetic. Tests and sums are fp64 computed from the f32 samples (separate multiply and add roundings: contraction is
 * off), except the operations the reference's float32 tensors decide something with, which are the same float32
 * operations here:
 *   fit      per item b over its T * H * W pixels, masked fp64 sums a00 = sum p^2, a01 = sum p, a11 = count, b0 = sum p t,
 *            b1 = sum t; det = a00 a11 - a01^2; if det != 0 scale = (a11 b0 - a01 b1) / (det + 1e-6), shift = (-a01 b0 +
 *            a00 b1) / (det + 1e-6), else both 0; each rounded to f32 once (compute_scale_and_shift).
 *   align    a = fadd_rn(fmul_rn(scale, p), shift): two f32 roundings. Never stored; every pass recomputes it bit for bit.
 *   robust   per frame f, for x = a and x = target: n_f = kept pixels; m = the lower median (rank (H W - 1) / 2 of the
 *            sorted values) of keep ? x : 0, which is torch.median of mask * x and an input sample or 0, so exact (-0.0 is
 *            returned as +0.0); s = max(sum_keep |x - m| / n_f, 1e-6); m = 0, s = 1 when n_f == 0. xn = (x - m) / s.
 *   spatial  data = sum_keep |an - tn| / sum n_f (0 when nothing is kept); with d = an - tn, on each grid [::2^k, ::2^k],
 *            k < scales: g_k = (sum |d(y, x + 2^k) - d(y, x)| + sum |d(y + 2^k, x) - d(y, x)|) / M_k over the pairs of grid
 *            points that are both kept, inside one frame; M_k = kept grid points of all frames, g_k = 0 when M_k == 0.
 *            spatial_loss = data + alpha * sum_k g_k; alpha <= 0 skips the regulariser (g_k = M_k = 0).
 *   stable   per frame, th = fmul_rn(fsub_rn(max, min), 0.05f) of the kept target (-inf for an empty frame). For t = 1 ..
 *            T - 1 inside one item: pg = fsub_rn(a_t, a_{t-1}), tg = fsub_rn(t_t, t_{t-1}); a pixel counts when kept in
 *            both frames and |tg| < th[b, t]; stable_loss = sum |pg - tg| / count (0 when count == 0). Computed when
 *            stable_scale > 0, which needs T >= 2 (the reference divides by zero strides at T == 1).
 *   absRel   over keep && target > 1e-3f && target < 70f: sum |(a - t) / t| / count (0 when count == 0).
 *   d1       over the mask: the share of pixels with fdiv_rn(a, t) < 1.25f and fdiv_rn(t, a) < 1.25f (a NaN or inf quotient
 *            is no hit); 0 when nothing is kept.
 *   total    spatial_loss + stable_scale * stable_loss (the second term when stable_scale > 0).
 * A dropped pixel is skipped by a branch, never multiplied by zero: NaN or inf under it reaches nothing. (The reference
 * multiplies by the mask, so there a NaN under a dropped pixel poisons the sums.)
 * out f64 [20]: 0 spatial_loss | 1 stable_loss | 2 absRel_loss | 3 d1 | 4 total_loss | 5 data | 6 sum_k g_k | 7 kept pixels |
 *               8..11 g_0..g_3 | 12..15 M_0..M_3 | 16 pixels of stable_loss | 17 pixels of absRel_loss | 18 hits of d1 |
 *               19 zero. out == NULL: only the fit runs (scale_shift is then required and T may
 *               be 1): compute_scale_and_shift on [B, T * H * W].
 * scale_shift f32 [B][2] = {scale, shift}; frame_stats f64 [B * T][4] = {m of a, s of a, m of target, s of target};
 * frame_counts i64 [B * T] = n_f. Each may be NULL.
 * Determinism: sums have a fixed order (a lane's stride through its block's share, the lanes of a wave by xor-shuffle, the
 * four waves, a frame's blocks in index order, the frames in index order); the medians come from the exact radix select
 * that vdn_frame_median uses, whose integer atomics count and cannot reorder anything. Two runs give the same bits.
 * workspace: vdn_depth_loss_workspace_bytes(B, T) bytes (it depends on B and T alone), 8-byte aligned.
 * Float pointers need 4-byte alignment, workspace, frame_stats, frame_counts and out 8 (VDN_EALIGN otherwise). Where H * W
 * is a multiple of 4, prediction and target are 16-byte aligned and the mask is 4-byte aligned, a lane reads four pixels
 * per load; one otherwise. VDN_EINVAL: a null required pointer, a size <= 0, scales < 0, or T < 2 with stable_scale > 0.
 * VDN_EUNSUPPORTED: H * W > INT32_MAX, B * T > 65535, scales > 4. All of these are returned before anything is launched.
 * vdn_depth_loss_trip(wide): the pixels of a frame that one trip of a criterion's sweep covers (32 blocks x 256 lanes x 4 or
 * 1); a larger frame sends the lanes round their stride loop again. The sweeps of the backward, of the trimmed criterion and
 * of the SSIM term have the same blocks per frame, so the figure is theirs too.                                            */
int vdn_depth_loss_trip(int wide);
size_t vdn_depth_loss_workspace_bytes(int B, int T);
int vdn_depth_loss(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                   double alpha, int scales, double stable_scale, void* workspace, float* scale_shift,
                   double* frame_stats, int64_t* frame_counts, double* out, vdn_stream stream);

/* The gradient of that criterion with respect to `prediction`: what autograd computes in the training step of
 * scripts/train*.py (total_loss.backward()) for
 *     L = c_sp * spatial_loss + c_st * stable_loss + c_ar * absRel_loss
 * where coeff f32 [3] = {c_sp, c_st, c_ar} is read on the device (no host synchronisation): for upstream gradients g of the
 * dictionary's entries, c_sp = g_total + g_spatial, c_st = stable_scale * g_total + g_stable, c_ar = g_absRel. d1 is piecewise
 * constant: its gradient is zero. Gradients with respect to target, and second derivatives, are not computed.
 * prediction, target, mask, B .. stable_scale are the arguments of the vdn_depth_loss call whose outputs are passed here:
 * scale_shift f32 [B][2], frame_stats f64 [B * T][4], frame_counts i64 [B * T] and out f64 [20], all required. The fit's
 * solve, the select and the deviation pass are not run again; the four masked sums of the fit, which the forward does not
 * return, are summed again in the forward's order. grad_prediction f32 [B, T, H, W] is written everywhere.
 * Arithmetic (fp64 from the f32 samples, contraction off; the two f32 roundings of a have the derivative 1; sign(0) = 0, as
 * in the backward of torch.abs). With k the keep mask, (sc, sh) the forward's f32 pair, m, s the median and scale of a, cnt
 * = n_f, x = (a - m) / s and d = x - y the difference of the normalised maps:
 *   g_x     at a kept pixel: c_sp * (sign(d) / M + alpha * (n_0 / M_0 + n_1 / M_1 + ...)), M = out[7], M_k = out[12 + k],
 *           n_k = the sum over the pixel's kept neighbours at stride 2^k (left, right, upper, lower, inside its frame) on
 *           each grid k it belongs to of sign(d_self - d_nb), an integer; grids with M_k == 0 add nothing; k ascending.
 *           A gather: no lane writes another lane's pixel.
 *   frame   g_s = -sum g_x x / s when cnt > 0 and sum_keep |a - m| / cnt >= 1e-6 (the clamp passes nothing below its
 *           bound), else 0; sigma = sum_keep sign(a - m); g_m = -sum g_x / s - g_s * sigma / cnt (0 when cnt == 0).
 *   g_a     g_x / s + g_s * sign(a - m) / cnt
 *           + g_m at the median's holder: the kept pixel of lowest index whose a equals m. Nobody holds it when the frame
 *             keeps nothing, or when m == 0 and the frame has a dropped pixel: the median is then taken to be the 0 of a
 *             dropped pixel, where the reference's mask * a has the derivative 0.
 *           + c_st * (e_later - e_earlier) / out[16]: for a pair (t - 1, t) of one item that the forward counts (kept in both
 *             frames, |tg| < th[b, t], the same f32 decisions), e = sign(pg - tg) at the later frame's pixel and the same at
 *             the earlier frame's, where it is subtracted. Only when stable_scale > 0.
 *           + c_ar * sign(a - target) / (target * out[17]) where the forward counts the pixel for absRel.
 *   fit     per item G0 = sum_keep g_a p, G1 = sum_keep g_a, D = det + 1e-6;
 *           g_p = sc * g_a + (G0 * (dN0 - sc * dD) + G1 * (dN1 - sh * dD)) / D at a kept pixel, with dN0 = a11 t - b1,
 *           dN1 = -b0 - a01 t + 2 p b1, dD = 2 (p a11 - a01); rounded to f32 once. An item with det == 0 has gradient 0.
 * A dropped pixel's gradient is +0.0 and it is skipped by a branch: NaN or inf under it reaches nothing.
 * Passes: per-frame sums in 32 blocks per frame, a one-block solve (g_s, g_m, holder, threshold, the fit's sums), the sums
 * G0 and G1 in 32 blocks per frame, a one-block solve, the write. No atomics; sums have the forward's fixed order (the
 * holder is a minimum over indices): two runs give the same bits.
 * The first pass leaves g_x in an fp64 plane of the workspace, the second turns it into g_a in place and the third reads it,
 * so the workspace is vdn_depth_loss_backward_workspace_bytes(B, T, H, W) bytes: a part that depends on B and T alone plus
 * B * T * H * W * 8, 8-byte aligned. (Recomputing g_x in every pass instead was measured and dropped: DESIGN 5.14.)
 * Load shapes and bits. Where H * W is a multiple of 4 a lane owns four consecutive pixels, read with one 16-byte load per
 * plane (and written with one store) when prediction, target and grad_prediction are 16-byte aligned and the mask 4-byte
 * aligned, and with a load per pixel otherwise; else a lane owns one pixel. The order of every sum therefore depends on the
 * shape alone, never on where a tensor starts: for the same forward state the gradient has the same bits at any alignment.
 * (vdn_depth_loss itself sums a misaligned tensor one pixel per lane, so its fp64 per-frame scales may differ in the last
 * place between two alignments of the same data; the gradient inherits exactly that difference and adds none.)
 * Errors as vdn_depth_loss, returned before anything is launched: VDN_EINVAL for a null pointer (every pointer is
 * required), a size <= 0, scales < 0, or T < 2 with stable_scale > 0; VDN_EUNSUPPORTED for H * W > INT32_MAX, B * T > 65535,
 * scales > 4; VDN_EALIGN for a float pointer off 4 bytes or workspace, frame_stats, frame_counts or out off 8. */
size_t vdn_depth_loss_backward_workspace_bytes(int B, int T, int H, int W);
int vdn_depth_loss_backward(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                            double alpha, int scales, double stable_scale, const float* scale_shift,
                            const double* frame_stats, const int64_t* frame_counts, const double* out, const float* coeff,
                            void* workspace, float* grad_prediction, vdn_stream stream);

/* The trimmed depth criterion: VideoDepthLoss(alpha, scales, trim, stable_scale) of loss/loss.py:326-367 with trim > 0 (its
 * TrimmedMAELoss and TrimmedAbsRelLoss, loss/loss.py:164-219), batch-based reduction, no SSIM term. vdn_depth_loss and
 * vdn_depth_loss_backward are unchanged; these two entry points stand beside them.
 * The arguments are those of vdn_depth_loss plus keep = 1.0 - trim, computed once by the caller in double, in (0, 1]. The fit,
 * the alignment, the robust normalisation, the grids g_k, d1 and every count are exactly vdn_depth_loss's (its kernels run
 * first, on the same stream). Three terms change. Each has a set of counted residuals |r|, fp64, as vdn_depth_loss sums them:
 *   data    |an - tn| over the kept pixels                          n = out[7]
 *   stable  |pg - tg| over the temporal pairs that are counted      n = out[16]
 *   absRel  |(a - t) / t| over the pixels absRel counts             n = out[17]
 * and the reference sorts them, keeps the k smallest and divides their sum by n (not by k). Here, per term:
 *   rank    k = (uint64) floor((double) n * keep), which is Python's int(len * (1.0 - trim)). n exists only on the device, so
 *           k is computed there; no host synchronisation is added.
 *   key     the float32 rounding of |r|. It is non-negative, so its bit pattern is ordered. A NaN residual has the one key
 *           0x7FC00000 and sorts after +inf, as in torch.sort. Dropped and uncounted elements take no part: they are
 *           skipped, not given a key. thr = the key of rank k - 1 among the n keys (an exact radix select over the batch).
 *   value   n_less = #{key < thr}, n_tied = #{key == thr}, w = (k - n_less) / n_tied in fp64;
 *           term = (sum_{key < thr} |r| + w * sum_{key == thr} |r|) / n, the fp64 residuals in the fixed order below.
 *           term = 0 and k = n_less = n_tied = thr = w = 0 when k == 0 (which includes n == 0).
 *           The reference keeps an arbitrary k - n_less of the tied elements (its sort is not stable). They are equal to
 *           float32, so w gives its value to float32 rounding, and the same bits on every run.
 * spatial_loss = data + alpha * sum_k g_k and total_loss = spatial_loss + stable_scale * stable_loss are formed from the
 * trimmed terms as vdn_depth_loss forms them; g_k and d1 are not trimmed.
 * out f64 [40]: 0..19 as vdn_depth_loss, with the trimmed values in 0, 1, 2, 4 and 5; for term i (0 data, 1 stable, 2 absRel)
 *               20 + 5 i: k | n_less | n_tied | thr as f64 | w; 35..39 zero. out is required (there is no fit-only form).
 * Passes after vdn_depth_loss's: a one-block kernel (per-frame scales once, the three k); the select of csrc/select.hpp over
 * one set of all frames with three slots, so the three terms share one sweep of the inputs per radix pass, each rank read
 * from device memory; per frame in 32 blocks the sums and counts below and at each threshold; a one-block finalise. Every
 * pass recomputes the residuals from the inputs, by the expressions of vdn_depth_loss (one sweep writing float32 key planes
 * for the select's passes, and three selects of one slot, were measured and dropped: DESIGN 5.14). Load shapes as
 * vdn_depth_loss.
 * Determinism: the sums have vdn_depth_loss's fixed order (lane stride, wave, block, a frame's blocks, frames in index order);
 * the select's integer atomics count and cannot reorder anything. Two runs give the same bits.
 * workspace: vdn_depth_loss_trimmed_workspace_bytes(B, T) bytes (it depends on B and T alone), 8-byte aligned.
 * Errors as vdn_depth_loss, returned before anything is launched, and: VDN_EINVAL for out == NULL and for keep outside (0, 1]
 * or NaN; VDN_EUNSUPPORTED when B * T * H * W > UINT32_MAX, the limit of the select's counters.                          */
size_t vdn_depth_loss_trimmed_workspace_bytes(int B, int T);
int vdn_depth_loss_trimmed(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                           double alpha, int scales, double stable_scale, double keep, void* workspace, float* scale_shift,
                           double* frame_stats, int64_t* frame_counts, double* out, vdn_stream stream);
/* The gradient of the trimmed criterion with respect to `prediction`: the contract of vdn_depth_loss_backward, with out the
 * f64 [40] that vdn_depth_loss_trimmed wrote for the same inputs and arguments. The selection is piecewise constant, so each
 * counted element of a term carries the weight u = 1 where key < thr, w where key == thr and 0 otherwise (0 everywhere when
 * k == 0), the key recomputed from the inputs and compared with out[20 + 5 i + 3]. u multiplies three terms of the chain:
 *   the data part of g_x         c_sp * u * sign(d) / M
 *   the stable part of g_a       c_st * (u_later e_later - u_earlier e_earlier) / out[16], u of the pair each e belongs to
 *   the absRel part of g_a       c_ar * u * sign(a - target) / (target * out[17])
 * The regulariser, the frame chain (g_s, g_m, the median's holder) and the fit chain follow from these and do not change. With
 * no tie at a threshold this is what autograd gives through the reference's sort and slice; with ties it is the mean over the
 * reference's possible choices. No atomics; the sums have the forward's fixed order, so two runs give the same bits.
 * workspace: vdn_depth_loss_trimmed_backward_workspace_bytes(B, T, H, W) bytes (that of vdn_depth_loss_backward). Errors as
 * vdn_depth_loss_backward, and VDN_EUNSUPPORTED when B * T * H * W > UINT32_MAX, for which no forward can have run.        */
size_t vdn_depth_loss_trimmed_backward_workspace_bytes(int B, int T, int H, int W);
int vdn_depth_loss_trimmed_backward(const float* prediction, const float* target, const uint8_t* mask, int B, int T, int H, int W,
                                    double alpha, int scales, double stable_scale, const float* scale_shift,
                                    const double* frame_stats, const int64_t* frame_counts, const double* out,
                                    const float* coeff, void* workspace, float* grad_prediction, vdn_stream stream);

/* The SSIM term of the depth criterion: DepthShallowSSIMLoss of loss/loss.py:296-323 with reduction "batch-based" and the
 * weights [1, 0, 0, 0, 0] that VideoDepthLoss constructs it with (scripts/train*.py: --ssim_loss_scale), the forward.
 * pytorch_msssim's MS_SSIM is restated from its published algorithm (the library's own file is not pinned: DESIGN.md 5.18):
 * with those weights the four pooled levels enter its product as value ** 0 == 1 with a zero gradient and are not computed.
 * prediction, target f32 [B, T, H, W] row-major, mask u8 [B, T, H, W] (non-zero = keep, required; it takes part in the
 * maximum alone, as in the reference). scale_shift f32 [B][2] or NULL: with it the term is taken on the aligned prediction
 * a = fadd_rn(fmul_rn(scale, p), shift), vdn_depth_loss's alignment (the composite criterion); a = p without.
 *   max      per item over its T * H * W pixels: pm = max of the kept a, tm = max of the kept target; when the item drops a
 *            pixel 0 takes part in both (the reference multiplies by the mask; a dropped pixel's own value is never read);
 *            max_val = max(max(pm, tm), 1e-8f), all float32.
 *   scale    x = fdiv_rn(a, max_val), y = fdiv_rn(target, max_val) at every pixel, dropped or not. From here on fp64 computed
 *            from these float32 values, separate multiply and add roundings (contraction is off).
 *   window   g_k, k = 0 .. 10: the float32 values of exp(-(k - 5)^2 / 4.5) / sum as torch computes them, widened to double,
 *            kept as literals (vdn.loss.SSIM_WINDOW). "Valid" filtering, along H and then W, taps in ascending order:
 *            mu1, mu2, e11, e22, e12 = the filtered x, y, x^2, y^2, x y on the (H - 10) x (W - 10) outputs.
 *   map      A = 2 (e12 - mu1 mu2) + C2, D = (e11 - mu1^2) + (e22 - mu2^2) + C2, C2 = 0.03^2; cs = A / D.
 *   frame    cs_f = sum of cs over the frame's outputs / ((H - 10)(W - 10)); loss = 1 - sum_f relu(cs_f) / (B T).
 * out f64 [4] = {loss, mean_f relu(cs_f), frames with cs_f <= 0 or NaN (gated by relu), B * T}; frame_cs f64 [B * T] = cs_f;
 * item_max f64 [B][4] = {max_val, who holds it, the weight of the prediction's path, index}: who = 0 a kept prediction
 * (weight 1), 1 the target (0), 2 a dropped pixel's zero (0), 3 the clamp (0: max(pm, tm) < 1e-8f), 4 prediction and target
 * equally (1/2, torch.max's rule); index = the lowest index in the item's T * H * W pixels of a kept prediction equal to the
 * largest kept one, -1 when a dropped pixel's zero comes before it or nothing is kept. All three are required.
 * One block takes a 16 x 32 tile of a frame's outputs (vdn_ssim_tile): x and y with the halo of 10 in LDS, the moments along
 * H into LDS, along W into registers; no plane is written. Determinism: a tile's sum in the order of the block reduction (a
 * lane's two outputs, the wave's xor-shuffle, the four waves); a frame's tiles by one block, a lane adding the tiles lane,
 * lane + 256, .. and the lanes by the block reduction; the frames likewise by one block; no atomics. Two runs give the same
 * bits.
 * workspace: vdn_ssim_loss_workspace_bytes(B, T, H, W) bytes, 8-byte aligned.
 * VDN_EINVAL: a null pointer (scale_shift excepted), a size <= 0, H < 11 or W < 11 (the library's own rule, min(H, W) > 160,
 * belongs to the Python classes). VDN_EUNSUPPORTED: H * W > INT32_MAX, B * T > 65535, more than INT32_MAX tiles. VDN_EALIGN: a
 * float pointer off 4 bytes; workspace, out, frame_cs or item_max off 8. All returned before anything is launched.          */
int vdn_ssim_tile(int* tile_h, int* tile_w);
size_t vdn_ssim_loss_workspace_bytes(int B, int T, int H, int W);
int vdn_ssim_loss(const float* prediction, const float* target, const uint8_t* mask, const float* scale_shift, int B, int T,
                  int H, int W, void* workspace, double* out, double* frame_cs, double* item_max, vdn_stream stream);

/* The gradient of coeff * (that loss) with respect to `prediction`. coeff f32 [1] is read on the device (no host
 * synchronisation). prediction .. W are the arguments of the vdn_ssim_loss call that wrote out, frame_cs and item_max.
 * Gradients with respect to target, and second derivatives, are not computed; the float32 roundings of a, x and y have the
 * derivative of the exact operation. With T(.) the transpose of the valid filter (zero outside the outputs), P = 1 / D,
 * Q = A / D^2, N = mu1 Q - mu2 P, and per frame w = -coeff / (B T (H - 10)(W - 10)) when cs_f > 0, else nothing at all:
 *   g_x      = (2 w ((y T(P) - x T(Q)) + T(N))), the sum over the outputs of d cs / d x: the adjoint stencil; +0.0 in a frame
 *              that relu gates.
 *   max      dL / d max_val = -sum_j (g_x x + g_y y)_j / max_val over the item, g_y the mirror image of g_x. The adjoint turns
 *            the sum into outputs alone: sum_j (g_x x + g_y y)_j = 2 C2 w sum_o (A - D) / D^2 per frame (cs is invariant
 *            under a common scale but for C2), and that closed form is what is evaluated: it has no cancelling parts. It is
 *            given, times item_max's weight, to the pixel item_max's index names; to nobody when the weight is 0.
 *   g_a      = g_x / max_val + that term at the holder.
 *   fit      with scale_shift: g_p = sc g_a + keep * (G0 (dN0 - sc dD) + G1 (dN1 - sh dD)) / D as in
 *            vdn_depth_loss_backward (the same code), with G0 = sum g_a p and G1 = sum g_a over ALL the item's pixels (the
 *            term ignores the mask, the fit does not) and the fit's masked sums summed again in vdn_depth_loss_backward's
 *            order; 0 for an item with det == 0. Without scale_shift g_p = g_a.
 *   write    accumulate == 0: grad_prediction = (float)g_p. accumulate != 0: (float)((double)grad_prediction + g_p), one
 *            rounding: how the composite adds the term to vdn_depth_loss_backward's result.
 * Passes: the fit's sums (with scale_shift), the forward's tile kernel leaving P, Q, N as fp64 planes over the outputs, the
 * fold of a frame's tiles and a one-block solve, the adjoint in 16 x 32 tiles of pixels (g_a into an fp64 plane, the tile's
 * sums for G0 and G1), the same fold and a one-block solve (an item's frames in index order), the write. No atomics, fixed order: two runs give the same bits, and as in vdn_depth_loss_backward the
 * order depends on the shape alone, not on where a tensor starts.
 * workspace: vdn_ssim_loss_backward_workspace_bytes(B, T, H, W) bytes, 8-byte aligned: B T (3 (H - 10)(W - 10) + H W) doubles
 * and a part that depends on B, T and the number of tiles.
 * Errors as vdn_ssim_loss, returned before anything is launched; every pointer but scale_shift is required.               */
size_t vdn_ssim_loss_backward_workspace_bytes(int B, int T, int H, int W);
int vdn_ssim_loss_backward(const float* prediction, const float* target, const uint8_t* mask, const float* scale_shift, int B,
                           int T, int H, int W, const double* out, const double* frame_cs, const double* item_max,
                           const float* coeff, int accumulate, void* workspace, float* grad_prediction, vdn_stream stream);

/* The batch preparation that scripts/train.py, train_v2.py .. train_v4.py and scripts/evaluate.py, evaluate_v2.py ..
 * evaluate_v4.py repeat between the loader and the model: preprocess_rgb_sequences, preprocess_rgb_viz_sequences,
 * preprocess_depth_sequences (with its batch_wise_min_max_norm) and gt = 1. / torch.clamp(gt, min=1e-8). Stateless, caller's
 * stream, caller-owned buffers, no host synchronisation.
 * Arithmetic: the reference's float32 operations, one IEEE rounding per reference operation (fsub_rn, fdiv_rn), nothing
 * contracted or reassociated, so the results are the bits of the torch composition. The constants are the float32 nearest
 * to 1e-8, to the means 0.485, 0.456, 0.406 and to the stds 0.229, 0.224, 0.225 (timm's IMAGENET_DEFAULT_MEAN / _STD).
 * clamp(x, min = m) is x < m ? m : x and clamp(x, max = m) is x > m ? m : x: a NaN stays a NaN, as in torch.clamp. The sign
 * of a zero result is not part of the contract.
 * vdn_prep_rgb    in, out f32 [frames, 3, H, W]; in == out is allowed. c = clamp(x, 0, 1); normalize != 0:
 *                 out = fdiv(fsub(c, mean[ch]), std[ch]) (torchvision's Normalize: sub_(mean).div_(std)); else out = c. The
 *                 channel is found per element. One launch.
 * vdn_prep_depth  in, out f32 [B, n] (n = S * H * W; in == out is allowed), mask u8 [B, n], non-zero = keep, or NULL = all
 *                 kept (the reference's masks == None branch). Stages in this order, each optional:
 *                   reciprocal  x = fdiv(1, clamp(x, min = 1e-8f))                  the ground-truth line
 *                   clamp0      x = clamp(x, min = 0)
 *                   normalize   lo, hi = the item's min and max of the staged x over its kept pixels (a NaN at a kept pixel
 *                               makes both NaN, as torch's min / max do; a dropped pixel is skipped by a branch, so nothing
 *                               under it reaches them); d = clamp(fsub(hi, lo), min = 1e-8f);
 *                               out = clamp(fdiv(fsub(x, lo), d), 0, 1) at every pixel of the item, kept or not; an item
 *                               with no kept pixel gives +0.0 everywhere.
 *                 minmax f32 [B][2] (may be NULL) receives lo, hi (+inf, -inf for an item with no kept pixel); written only
 *                 when normalising. One launch without the normalisation. Two with it: pass 1 leaves 256 per-block (lo, hi,
 *                 any) partials of each item in `workspace` (vdn_prep_depth_workspace_bytes(B) bytes, a multiple of 8 that
 *                 depends on B alone); in pass 2 every block reduces its item's partials itself and writes its share. No
 *                 finalise launch, no atomics; min and max are exact in any order, so two runs give the same bits. Pass 2
 *                 does not read the mask: 13 bytes per pixel cross the bus (rgb: 8).
 * Load shapes: where n (H * W for rgb) is a multiple of 4, the float pointers are 16-byte aligned and the mask is 4-byte
 * aligned, a lane handles four floats per 16-byte load and store; one element otherwise. The values are the same either way.
 * vdn_prep_trip(wide): the elements of one item (frame) that one trip of the grid covers (256 blocks x 256 lanes x 4 or 1);
 * a longer item sends the lanes round their stride loop again.
 * Errors, all returned before anything is launched. VDN_EINVAL: a null required pointer, a size <= 0, normalize with a NULL
 * workspace. VDN_EUNSUPPORTED: n or 3 * H * W above INT32_MAX, B (frames) above 65535. VDN_EALIGN: a float pointer off 4
 * bytes, a workspace off 8.                                                                                              */
int vdn_prep_trip(int wide);
size_t vdn_prep_depth_workspace_bytes(int B);
int vdn_prep_rgb(const float* in, float* out, int frames, int H, int W, int normalize, vdn_stream stream);
int vdn_prep_depth(const float* in, const uint8_t* mask, float* out, int B, int64_t n, int reciprocal, int clamp0,
                   int normalize, void* workspace, float* minmax, vdn_stream stream);

/* The metric-depth branch's criterion and scores: metric_depth/util/loss.py (SiLogLoss), metric_depth/util/metric.py
 * (eval_depth) and the body of the validation loop of metric_depth/train.py:160-177. Stateless, caller's stream, caller-owned
 * buffers, no host synchronisation, no atomics: two runs give the same bits.
 * Kept pixels. A pixel is kept when its mask byte EQUALS 1 (the reference's valid_mask == 1: a byte of 2 drops, unlike the
 * "non-zero = keep" masks of vdn_depth_loss) and, with bounded != 0, depth >= min_depth and depth <= max_depth, the bounds
 * rounded to float32 and compared in float32 (torch's rule for a float32 tensor against a Python number); a NaN depth fails
 * them. mask NULL: every byte is 1. A dropped pixel is skipped by a branch, so nothing under it (a NaN, an inf) reaches a
 * sum, where the reference indexes with the mask: the two agree.
 * Arithmetic. float32, one IEEE rounding per operation, nothing contracted: the resampled prediction, thresh =
 * max(fdiv(t, p), fdiv(p, t)) (a NaN wins, as torch.max) compared with 1.25, 1.5625 and 1.953125, and d_k = fdiv((float)
 * count_k, (float)n). fp64 from the float32 inputs on, products and sums rounded separately: the differences, log and log10,
 * the per-pixel terms, every sum, the means and the square roots. A non-positive prediction under a kept pixel gives what
 * IEEE log gives. Sums have a fixed order: a lane's stride through its block's share, the wave and the block (four waves of
 * 64 lanes, a butterfly and ((w0 + w1) + (w2 + w3))), then the item's 256 per-block partials the same way.
 * vdn_metric_eval  pred f32 [items, ph, pw], depth f32 [items, H, W], valid u8 [items, H, W] or NULL -> out f64 [items][10] =
 *                  n | d1 d2 d3 abs_rel sq_rel rmse rmse_log log10 silog, n the item's kept pixels; an item with n == 0 gets
 *                  nine NaN (0 / 0), as the reference's eval_depth of an empty vector. (ph, pw) != (H, W): the prediction is
 *                  sampled at each ground-truth pixel as F.interpolate(mode='bilinear', align_corners=True) places it, scale
 *                  = (in - 1) / (out - 1) in float32 (0 for out == 1), src = fl(scale * dst), i0 = min((int)src, in - 1), l =
 *                  fl(src - i0), top = fl(fl(fl(1 - lx) a00) + fl(lx a01)), bot the same on the lower row, v = fl(fl(fl(1 -
 *                  ly) top) + fl(ly bot)); the resized map is never written. Two launches: per-block partials into
 *                  `workspace` (vdn_metric_workspace_bytes(items) bytes), then one block per item.
 * vdn_silog_loss   pred, target f32 [count], mask u8 [count] or NULL -> out f64 [4] = loss | n | sum dl | sum dl^2 over the
 *                  kept pixels, dl = log(target) - log(pred), loss = sqrt(sum dl^2 / n - lambd (sum dl / n)^2). `target` is
 *                  what the bounds test. Two launches; workspace of vdn_silog_loss_workspace_bytes() bytes.
 * vdn_silog_loss_backward  grad f32 [count] <- (float)(coeff[0] * -(dl - lambd * sum dl / n) / (n * loss * pred)) at kept
 *                  pixels, +0.0 at dropped ones; `state` is the out[4] that vdn_silog_loss wrote for the same inputs and
 *                  arguments, coeff f32 [1] on the device (the gradient of whatever follows with respect to the loss). One
 *                  launch, elementwise.
 *                    case                                          loss   gradient
 *                    no kept pixel                                 NaN    +0.0 everywhere
 *                    pred == target at every kept pixel (sqrt(0))  0      NaN at kept pixels, +0.0 at dropped ones
 *                    negative radicand                             NaN    NaN at kept pixels, +0.0 at dropped ones
 *                  as the reference's autograd gives them on the CPU.
 * Load shapes: where the item's length (count) is a multiple of 4, the float pointers are 16-byte aligned and the mask is
 * 4-byte aligned, a lane handles four floats per 16-byte load; one element otherwise. The values are the same either way.
 * vdn_metric_trip(wide): the elements of one item that one trip of the grid covers (256 blocks x 256 lanes x 4 or 1); a
 * lane issues the loads of four trips together, and a longer item sends it round its loop again.
 * Errors, all returned before anything is launched. VDN_EINVAL: a null required pointer, a size <= 0, bounded with a NaN
 * bound. VDN_EUNSUPPORTED: H * W, ph * pw or count above INT32_MAX, items above 65535. VDN_EALIGN: a float pointer off 4
 * bytes; workspace, out or state off 8.                                                                                  */
int vdn_metric_trip(int wide);
size_t vdn_metric_workspace_bytes(int items);
int vdn_metric_eval(const float* pred, const float* depth, const uint8_t* valid, int items, int ph, int pw, int H, int W,
                    int bounded, double min_depth, double max_depth, void* workspace, double* out, vdn_stream stream);
size_t vdn_silog_loss_workspace_bytes(void);
int vdn_silog_loss(const float* pred, const float* target, const uint8_t* mask, int64_t count, double lambd, int bounded,
                   double min_depth, double max_depth, void* workspace, double* out, vdn_stream stream);
int vdn_silog_loss_backward(const float* pred, const float* target, const uint8_t* mask, int64_t count, double lambd, int bounded,
                            double min_depth, double max_depth, const double* state, const float* coeff, float* grad,
                            vdn_stream stream);

/* The colourised depth the reference's front ends write to disk, made on the device. Replaces, per frame, run.py:59-71,
 * run_video.py:75-89 and metric_depth/run.py:67-78 (min/max of the frame, matplotlib palette or a grey triple, BGR,
 * optionally cv2.hconcat([raw, 50 white columns, depth])) and, per clip, save_video of utils/dc_utils.py:72-86 (one min/max
 * for the clip, the inferno palette or one grey channel, RGB). Stateless, caller's stream, caller-owned buffers.
 * VDN_EINVAL: a null required pointer, a size <= 0, ch other than 1 or 3, raw with ch != 3 or margin < 0. VDN_EALIGN: a
 * float or workspace pointer that is not 4-byte aligned. Limits: vdn_minmax_f32 takes groups <= INT32_MAX / 256 (VDN_EINVAL
 * beyond); vdn_colorize returns VDN_EUNSUPPORTED when N * H or the output width 2W + margin exceeds UINT32_MAX. All of these
 * are returned before anything is launched.
 * vdn_minmax_f32 — x f32 [groups, n] contiguous -> out f32 [groups][2] = {min, max} of each group (a frame, or groups = 1
 *                  for a clip). numpy semantics: a NaN anywhere in a group makes both of its results NaN; +-inf are
 *                  ordinary values; when +0.0 and -0.0 tie for an extreme the sign of the zero returned is not defined
 *                  (numpy's depends on element order). x needs 4-byte alignment only (interior by 16-byte loads, ragged ends per element).
 *                  Two stages through `workspace` (vdn_minmax_workspace_bytes(groups)), no atomics: the same bits every run.
 * vdn_colorize   — depth f32 [N, H, W]; minmax f32 [N][2] (per_frame != 0) or [1][2]; lut u8 [256][ch], ch = 1 or 3: the
 *                  channel order is the table's, so BGR and RGB need no mode. raw == NULL: out u8 [N, H, W, ch]. Else raw u8
 *                  [N, H, W, 3], ch = 3, margin >= 0 and out u8 [N, H, 2W + margin, 3]: the raw pixels verbatim, `margin`
 *                  pixels of 255, the palette pixels. out needs no alignment.
 *                  index = (uint8)(((d - mn) / (mx - mn)) * 255.0f): subtract, divide and multiply each rounded to fp32
 *                  (no reciprocal, no contraction), the conversion truncates — what numpy does on a float32 array, bit
 *                  for bit. Departures from the reference, which leaves these to an undefined NaN / out-of-range -> uint8
 *                  cast: (1) mx == mn gives index 0 for every pixel; (2) d outside [mn, mx] (a range the caller
 *                  supplied) clamps to 0 / 255; (3) a NaN d (or NaN bounds) gives index 0.                          */
size_t vdn_minmax_workspace_bytes(int groups);
int vdn_minmax_f32(const float* x, int groups, size_t n, void* workspace, float* out, vdn_stream stream);
int vdn_colorize(const float* depth, const float* minmax, int per_frame, const uint8_t* lut, int ch, const uint8_t* raw,
                 int margin, uint8_t* out, int N, int H, int W, vdn_stream stream);

/* Depth-refiner wrappers v2 .. v5 (models/video_depth_model_v5.py:63-87,160-192, models/video_depth_model_v4.py:117-148,
 * utils/normal_utils.py:4-51). f32 throughout, frames are [frames, n = H*W] row-major.
 * vdn_frame_median  — median[f] = torch.quantile(x[f], 0.5) (linear interpolation), exact radix select; a frame that
 *                     holds a NaN of either sign gets a NaN, as torch.quantile gives it, and leaves the other frames'
 *                     medians alone. workspace = vdn_frame_median_workspace_bytes(frames): the select's bins and state
 *                     and one 4-byte NaN flag per frame, which the entry zeroes itself (one memset on `stream`).
 * vdn_refine_scale  — out = x / max_depth * s_f, s_f = exp(tanh(w * median[f] / max_depth + b) * max_log_scale)
 *                     (GlobalScaleHead: quantile pool -> 1x1 conv -> TanhToExp); scale_out[f] = s_f (may be NULL).
 * vdn_refine_pack   — encoder input [frames,3,H,W] = (d, nx, ny); normals != 0: Sobel/8 on a reflect-padded map,
 *                     n = (-Ix,-Iy,1)/sqrt(Ix^2+Iy^2+1+1e-8); normals == 0: d broadcast to 3 channels.
 * vdn_refine_finish — out = (scaled + (w * depth + b)) * max_depth (residual != 0) or depth * max_depth.
 * The v3 wrapper (models/video_depth_model_v3.py:167-206) is the same four with max_depth = 65535 in front and
 * max_depth = 1 in vdn_refine_finish (its result stays normalised); v2 (models/video_depth_model_v2.py:75-100) has no
 * scale head and its own finish:
 * vdn_refine_normalize — out = x / max_depth over n floats, the correctly rounded fp32 division vdn_refine_scale applies
 *                     (video_depth_model_v2.py:77). An entry of its own rather than a mode of vdn_refine_scale: that one
 *                     reads a per-frame median, and v2 has none to compute.
 * vdn_refine_mix    — out = relu(a2 * relu(a0 * depth + a1 * x + c0) + c1) over n floats: final_res of
 *                     video_depth_model_v2.py:64-72,96-97 (Conv2d(2,1,1) - BatchNorm2d - ReLU - Conv2d(1,1,1) -
 *                     BatchNorm2d - ReLU on stack([depth, x])) with the eval-mode BatchNorms folded into five scalars by
 *                     the caller. relu is torch.relu's: NaN in, NaN out.
 * Both take any n >= 1 and any 4-byte-aligned pointers (16 bytes per lane where the arrays' alignments agree, one
 * float per lane at the ends and where they do not); out must not overlap an input.                               */
size_t vdn_frame_median_workspace_bytes(int frames);
int vdn_frame_median(const float* x, int frames, size_t n, float* median, void* workspace, vdn_stream stream);
int vdn_refine_scale(const float* x, const float* median, int frames, size_t n, float w, float b, float max_log_scale,
                     float max_depth, float* out, float* scale_out, vdn_stream stream);
int vdn_refine_pack(const float* d, float* out, int frames, int H, int W, int normals, vdn_stream stream);
int vdn_refine_finish(const float* scaled, const float* depth, float w, float b, float max_depth, int residual, float* out,
                      size_t n, vdn_stream stream);
int vdn_refine_normalize(const float* x, float max_depth, float* out, size_t n, vdn_stream stream);
int vdn_refine_mix(const float* depth, const float* x, float a0, float a1, float c0, float a2, float c1, float* out, size_t n,
                   vdn_stream stream);

/* The end of one window of the refiners' clip driver (refiner.refine_video_depth: models/video_depth_model_v5.py:215-283 on
 * depth windows), in one launch. A window's T slots show the clip frames slots[0..T): copies of the previous window's
 * keyframes, new frames, padding; the finish of slot t needs the scaled input of THAT frame, scaled[slots[t]], which the
 * driver keeps once per clip frame. For slot t and output pixel (oy, ox):
 *   d   = (IH, IW) == (OH, OW) ? net[t][oy][ox]
 *                              : max(bilinear align-corners sample of net[t] at (oy, ox), 0)   (v5:184-185; the pixel of
 *                                vdn_upsample_bilinear_f32(relu = 1), never stored at full resolution)
 *   out[t][oy][ox] =
 *     VDN_TAIL_SHIFT, residual != 0   (scaled[f] + (c0 * d + c1)) * c2      c0, c1 = the shift head's weight and bias, c2 =
 *                                     max_depth or 1 (v5:188-192, v4:144-148, v3:203-204): the pixel of vdn_refine_finish
 *     VDN_TAIL_SHIFT, residual == 0   d * c2; scaled is not read and may be NULL
 *     VDN_TAIL_MIX                    relu(c3 * relu(c0 * d + c1 * scaled[f] + c2) + c4), (c0 .. c4) = vdn_refine_mix's (a0, a1,
 *                                     c0, a2, c1) (v2:96-98); residual is ignored
 * with f = slots[t]. net f32 [T, IH, IW] is the head's rectified map, scaled f32 [frames, OH, OW], slots int32 [T] in device
 * memory with every entry in [0, frames) (the caller checks the table on the host before it uploads it; an entry outside the
 * range reads nothing and fills its slot with NaN), out f32 [T, OH, OW], overlapping no input. The pixel expressions are the
 * three entries' own device functions, so out has the bits of: gather scaled by slots, vdn_upsample_bilinear_f32(relu = 1) where
 * the sizes differ, vdn_refine_finish / vdn_refine_mix.
 * Load shapes: where OW is a multiple of 4 and the bases read or written in place are 16-byte aligned, a lane handles four
 * pixels of a row per 16-byte access; one pixel otherwise. The values are the same either way.
 * vdn_refine_window_tail_trip(wide): the pixels of one slot that one trip of the grid covers (64 blocks x 256 lanes x 4 or 1); a
 * larger frame sends the lanes round their stride loop again.
 * Errors, all returned before anything is launched. VDN_EINVAL: a null required pointer, a size <= 0, T > 65535, an unknown
 * kind. VDN_EUNSUPPORTED: OH * OW or IH * IW above INT32_MAX. VDN_EALIGN: a pointer off 4 bytes.                        */
enum { VDN_TAIL_SHIFT = 0, VDN_TAIL_MIX = 1 };
int vdn_refine_window_tail_trip(int wide);
int vdn_refine_window_tail(const float* net, int IH, int IW, const float* scaled, int frames, const int32_t* slots, int T,
                           int OH, int OW, int kind, int residual, float c0, float c1, float c2, float c3, float c4,
                           float* out, vdn_stream stream);

/* Fused depth tail (depth_anything_v2/dpt.py:146-151; video_depth_anything/dpt_temporal.py:106-111 runs the same ops
 * in micro-batches): bilinear resize (align_corners=True) of the fp32 NHWC map x [B, IH, IW, C] (output_conv1's result,
 * written as ONE fp32 plane) to (OH, OW), Conv3x3(C -> 32, pad 1) + bias2 + ReLU, Conv1x1(32 -> 1) + b1 [+ ReLU when
 * relu != 0] -> depth f32 [B, OH, OW]. The up-sampled map and the 32-channel map stay on chip. w / w_lo: split planes
 * [32, ldb] with K = tap * C + ci (tap = 3 ky + kx; VDN_PACK_CONV3X3_TAPS), ldb >= 9 C; C a multiple of 32; `dt` is
 * the 16-bit type of the weight planes and of the on-chip up-sampled fragments; 3 MFMA products per term. The scale
 * (IH-1)/(OH-1) must be <= 10/17 (a 13 x 13 source patch covers a tile's halo): VDN_EUNSUPPORTED otherwise.           */
int vdn_depth_tail(int dt, const float* x, int B, int IH, int IW, int C, const void* w, const void* w_lo, int ldb,
                   const float* bias2, const float* w1, float b1, float* depth, int OH, int OW, int relu,
                   vdn_stream stream);
/* The same with the final activation `act` (VDN_OUT_*): VDN_OUT_SIGMOID is the tail of the metric-depth head
 * (metric_depth/depth_anything_v2/dpt.py:146-147 with output_conv2 of :109-114, times max_depth as dpt.py:183 has it).
 * vdn_depth_tail(relu) is this entry with act = relu ? VDN_OUT_RELU : VDN_OUT_NONE, and runs the kernel it always ran.   */
int vdn_depth_tail_act(int dt, const float* x, int B, int IH, int IW, int C, const void* w, const void* w_lo, int ldb,
                       const float* bias2, const float* w1, float b1, float* depth, int OH, int OW, int act,
                       float out_scale, vdn_stream stream);

/* Point cloud of a metric depth map (metric_depth/depth_to_pointcloud.py:99-104), one launch: depth f32 [h, w] and
 * rgb u8 [h, w, 3] -> points f64 [h*w, 3] = (x z, y z, z) with x = (col - w / 2) / fx, y = (row - h / 2) / fy in float64
 * and z widened from float32, colors f64 [h*w, 3] = rgb / 255.0. Subtractions, divisions and products only, each
 * correctly rounded and none contracted: the bits numpy gives. points and colors 16-byte aligned; fx, fy non-zero.     */
int vdn_depth_to_points(const float* depth, const uint8_t* rgb, int h, int w, double fx, double fy, double* points,
                        double* colors, vdn_stream stream);

/* output_conv1 of a 2x up-sampled map without the up-sampled map (depth_anything_v2/dpt.py:145 on the path_1 of
 * util/blocks.py:144-146): Conv3x3(pad 1) o bilinear(align_corners=True) o Conv1x1 is linear with no activation in between,
 * so the channel mixing of all nine taps runs as ONE vdn_gemm at the low resolution (weight rows t*Co + c = W_t Wo, bias
 * W_t bo, t = 3 ky + kx; vdn/pack.py lowres_oc1) and this entry does what is left, which is memory traffic:
 *   z f32 [B, IH, IW, 9*Co] -> out f32 [B, OH, OW, Co],
 *   out[b, y, x, c] = bias[c] + sum over the taps t with (y + ky - 1, x + kx - 1) inside OH x OW of
 *                     bilinear(z[b, :, :, t*Co + c]; that position), source coordinates as vdn_upsample_bilinear computes them.
 * A tap in the zero padding drops out whole (its share of the 1x1 bias rides inside z). Co % 16 == 0. A workgroup stages the
 * source patch of its 16 x 16 output pixels in LDS, so (IH-1)/(OH-1) must be about 1/2 or less (VDN_EUNSUPPORTED when the
 * patch outgrows the LDS). No atomics: deterministic.                                                                     */
int vdn_oc1_combine(const float* z, const float* bias, float* out, int B, int IH, int IW, int OH, int OW, int Co,
                    vdn_stream stream);

/* Depth + normal model (models/video_depth_model.py:64-119 with the VideoDepthAnythingHeadV2 head of
 * models/video_depth_head_v2_sangyu.py). Tokens are frame-major channel-last rows [B*S*h*w, C].
 * vdn_dn_attn     — nn.MultiheadAttention(C, heads, batch_first) self-attention (video_depth_head_v2_sangyu.py:67,
 *                   with the rearranges of :120,:122 (spatial) and :173,:175 (temporal)): qkv half [rows, 3C] = the
 *                   packed in_proj output (q | k | v, head h at columns h*dh.. of each), out half [rows, C]. Sequence
 *                   (g1 < n1, g0 < n0) is the L rows g1*s1 + g0*s0 + j*estride, j < L: spatial = (L = h*w, estride 1,
 *                   n0 1, n1 B*S, s1 h*w), temporal = (L = S, estride h*w, n0 h*w, s0 1, n1 B, s1 S*h*w). Head dim
 *                   C/heads in {12, 24, 48, 96}; online softmax, any L. qkv_lo / out_lo: split planes (both or neither).
 *                   Shares lane_attn_kernel (csrc/lane_attn.hip) with vdn_hiera_attn: these arguments are its sequence
 *                   geometry as they stand, with output stride s1 and no query pooling (Lq = L).
 * vdn_dn_prologue — the features the head consumes, in one launch per level (video_depth_model.py:89-103,
 *                   video_depth_head_v2_sangyu.py:272-276): token[(f*hw + p), c] = a[f][c*hw + p] (+ b[f][c*hw + p])
 *                   (+ ape[f % S][c]); a / b f32 per frame [C*hw] (the trunk's NHWC buffers read flat = the `.view`
 *                   reinterpretation; the head's own [B,S,C,h,w] input), b / ape optional. Writes out_f (f32 [rows, C])
 *                   and / or the half planes out_h (+ out_lo) in `dt`.
 * vdn_dn_tail     — conv3x3 (Cin -> 3, pad 1) + bias of the f32 NHWC map x [F, IH, IW, Cin] (final_upscale_layer's
 *                   last conv, :249), bilinear resize (align_corners) to (OH, OW) when it differs (video_depth_model.py:
 *                   107-110), then raw f32 [F, 3, OH, OW] (optional, the head's result) and / or depth f32 [F, OH, OW]
 *                   = relu?(ch0 (+ depth_in)) with normal f32 [F, 3, OH, OW] = (-ch1, -ch2, 1) (:112-123).
 *                   w f32 [3, Cin, 3, 3] as nn.Conv2d stores it, bias f32 [3]; Cin <= 128.                          */
int vdn_dn_attn(int dt, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int rows, int C, int heads, int L,
                int estride, int n0, int s0, int n1, int s1, float scale, vdn_stream stream);
int vdn_dn_prologue(int dt, const float* a, const float* b, int frames, int C, int hw, const float* ape, int S, float* out_f,
                    void* out_h, void* out_lo, vdn_stream stream);
int vdn_dn_tail(const float* x, int F, int IH, int IW, int Cin, const float* w, const float* bias, int OH, int OW,
                const float* depth_in, int relu, float* raw, float* depth, float* normal, vdn_stream stream);

/* Hiera trunk of the depth + normal model (models/hiera_image_encoder.py:35,60: hiera_{tiny,small,base}_224 of the
 * published Hiera code, inference, no masking; a 224 x 224 frame gives 56 x 56 tokens, head dim 96 at every stage).
 * Tokens live in the model's UNROLLED order: with d_k = 2*sy_k + sx_k the three nested stride-2 levels of the grid,
 * u = ((d1*4 + d2)*4 + d3)*49 + Y*7 + X for position y = 8Y + 4 sy3 + 2 sy2 + sy1 (x alike), so every 2 x 2 max-pool is a
 * max over the 4 contiguous quarters of a frame's token axis; stage s keeps the last 3 - s digits.
 * vdn_hiera_embed  — the gather of patch_embed.proj (Conv2d 3 -> 96, 7 x 7, stride 4, pad 3) as GEMM rows, already in
 *                    unrolled order (the model's `unroll` costs no pass): rows half [frames*3136, ldk],
 *                    row f*3136 + u, k = (c*7 + ky)*7 + kx = img[f, c, 4y-3+ky, 4x-3+kx] (0 outside), zero tail to ldk
 *                    (>= 147, a multiple of 64); img f32 [frames, 3, 224, 224]. The projection is a vdn_gemm whose `tab`
 *                    adds pos_embed permuted to unrolled order.
 * vdn_hiera_attn   — MaskUnitAttention: qkv half [frames*W*Lkv, 3C] (C = heads*96, columns q | k | v, each [heads][96]);
 *                    token t of window w of frame f is row f*W*Lkv + t*W + w. q_stride > 1 (the width-changing blocks):
 *                    t = g*Lq + j, Lq = Lkv / q_stride, and query j is the element-wise max of its q_stride rows
 *                    (the query max-pool), fused on load. out half [frames*W*Lq, C], row f*W*Lq + j*W + w. fp32 softmax.
 *                    W = 49 windows for the mask-unit stages, 1 for global attention. qkv_lo / out_lo: both or neither.
 *                    Shares lane_attn_kernel with vdn_dn_attn: in that entry's terms L = Lkv, estride = W, n0 = W, s0 = 1,
 *                    n1 = frames, s1 = W*Lkv, with output stride W*Lq and q_stride elements pooled into a query.
 * vdn_hiera_pool   — y[f, j, :] = max over g < 4 of x[f, g*n + j, :]; x f32 [frames, 4n, C], y f32 [frames, n, C]
 *                    (the max-pool of a width-changing block's projected residual). C % 4 == 0. Departure from the
 *                    reference, whose pool is torch.max / MaxPool and hands a NaN on: the max is C's fmaxf, where a NaN
 *                    loses against a number, so a token's NaN reaches y only when all four groups hold one there.
 * vdn_hiera_reroll — the model's `reroll` + undo_windowing: unrolled tokens f32 [frames, (56 >> stage)^2, C] of stage
 *                    0..3 -> f32 NHWC map [frames, 56 >> stage, 56 >> stage, C] (what vdn_dn_prologue reads). C % 4 == 0. */
int vdn_hiera_embed(int dt, const float* img, void* rows, void* rows_lo, int frames, int ldk, vdn_stream stream);
int vdn_hiera_attn(int dt, const void* qkv, const void* qkv_lo, void* out, void* out_lo, int frames, int heads, int W, int Lkv,
                   int q_stride, float scale, vdn_stream stream);
int vdn_hiera_pool(const float* x, float* y, int frames, int n, int C, vdn_stream stream);
int vdn_hiera_reroll(const float* tokens, float* map, int frames, int stage, int C, vdn_stream stream);

/* One-time weight packing ON THE DEVICE, so that a host in any language can feed the library from the reference's
 * fp32 parameter tensors as torch.nn stores them (vdn/pack.py is a thin caller of these). `w` is the contiguous fp32
 * parameter, (hi, lo) the [rows, ldb] planes vdn_gemm reads (lo may be NULL for the 1-product modes): K contiguous,
 * zero padded to ldb = vdn_pack_ldb(..) (a multiple of 64); hi = nearest(w), lo = nearest(w - hi).
 *   kind                 parameter (d0, d1, d2)                rows              K order
 *   VDN_PACK_LINEAR      [N, K] (d0 = N, d1 = K); also 1x1 convs and the 14x14 patch embedding (K = 588)
 *   VDN_PACK_CONV3X3     [Co, Ci, 3, 3] (d0 = Co, d1 = Ci)      Co                (ci/64, tap, ci%64) if Ci % 64 == 0 else (tap, ci)
 *   VDN_PACK_CONV3X3_TAPS  same                                 Co                (tap, ci)            [vdn_depth_tail]
 *   VDN_PACK_CONVT       [Ci, Co, k, k], kernel == stride (d0 = Ci, d1 = Co, d2 = k)   k*k*Co rows (ky, kx, co); K = ci
 *   VDN_PACK_GEGLU       [2 Nh, K] = [h ; gate]                 2 Nh, 16-row blocks alternating h / gate   [VDN_ST_GEGLU]
 *   VDN_PACK_ROPE        [N, K], N % 64 == 0                    per head (2i, 2i+1) -> [re 0-15 | im 0-15 | re 16-31 | im 16-31]
 * Concatenated projections (q|k|v) are packed one after the other into row ranges of one plane (hi + row0 * ldb).
 * vdn_pack_bias writes the matching bias order (row permutation / ConvTranspose repeat) as fp32 [rows].
 * Reference layouts: nn.Linear / nn.Conv2d / nn.ConvTranspose2d weights of dinov2_layers/*.py, util/blocks.py,
 * dpt.py:55-83, motion_module/attention.py:370-384 (GEGLU), sam2/modeling/sam/transformer.py:279-281 (RoPE q/k).   */
enum { VDN_PACK_LINEAR = 0, VDN_PACK_CONV3X3 = 1, VDN_PACK_CONV3X3_TAPS = 2, VDN_PACK_CONVT = 3, VDN_PACK_GEGLU = 4,
       VDN_PACK_ROPE = 5 };
int vdn_pack_rows(int kind, int d0, int d1, int d2);  /* rows of the packed planes, or a negative vdn_status */
int vdn_pack_ldb(int kind, int d0, int d1, int d2);   /* plane stride in elements */
int vdn_pack_weight(int dt, int kind, const float* w, int d0, int d1, int d2, void* hi, void* lo, int ldb, vdn_stream stream);
int vdn_pack_bias(int kind, const float* b, int d0, int d1, int d2, float* out, vdn_stream stream);
/* Operand planes of the cross-term GEMM (vdn_gemm_desc.A8 / W8) from fp16 split planes (hi, lo) [rows, ld] as vdn_pack_weight
 * wrote them (ld % 64 == 0): planes8 = u8 [2, rows, ld], the x6 rows of hi and of lo; kt != 0 stores both K-tile-major
 * ([ld/64][rows][64] each) and, if hi_kt is given, the hi plane again as [ld/32][rows][32].
 * order = which columns of a 64-wide slab half h holds at stream position p (both operands of a GEMM must use the order of
 * the kernel that writes its A planes):
 *   0  col = 32 h + p                                            A from vdn_layernorm or from this function
 *   1  col = 32 (p >> 4) + 16 ((p >> 3) & 1) + 8 h + (p & 7)     A from vdn_gemm out8 (bias + GELU)
 *   2  col = 32 (p >> 4) + 8 ((p >> 2) & 3) + 4 h + (p & 3)      A from vdn_flash_attn out8                              */
int vdn_pack_x8(const void* hi, const void* lo, int rows, int ld, void* hi_kt, void* planes8, int kt, int order,
                vdn_stream stream);
/* The same from an fp32 activation x [rows, ld] (ld % 64 == 0) whose producer writes no half planes (a residual stream that
 * feeds a GEMM without a LayerNorm in between: the memory feature of memory_encoder.py:173-181 before the key / value
 * projections of memory_attention.py): hi_kt = fp16 hi plane toward zero, K-tile-major; planes8 = u8 [2][ld/64][rows][64], order 0. */
int vdn_pack_x8_f32(const float* x, int rows, int ld, void* hi_kt, void* planes8, vdn_stream stream);

/* Padded-row operand planes (vdn_gemm_desc.pad_hi) of relu(x): x = split planes hi / lo, row-major [B H W, C] (C % 64 == 0) ->
 * hi_pad fp16 [C / 32][Mp][32] and planes8 u8 [2][C / 64][Mp][64] (x6 rows, order 1: that of the epilogues), Mp = B (H + 2) (W + 2). Image rows get
 * the values, ring rows zero bits; the guard rows around the planes are not touched. The first convolution of a fusion
 * block's ResidualConvUnit reads these; the later ones get theirs from the GEMM epilogues.                            */
int vdn_pack_x8_relu_pad(const void* hi, const void* lo, int B, int H, int W, int C, void* hi_pad, void* planes8, vdn_stream stream);

/* Workspace sizing (the library allocates nothing): bytes of split-K scratch worth passing as vdn_gemm_desc.splitk_ws
 * for this descriptor (0 = the shape never splits), and the partial-sum buffer of vdn_groupnorm.
 * See also vdn_stitch_workspace_bytes / vdn_frame_median_workspace_bytes.                                       */
size_t vdn_gemm_workspace_bytes(const vdn_gemm_desc* d);
size_t vdn_groupnorm_workspace_bytes(int frames, int groups, int nsplit);

/* misc */
int vdn_cast(const void* x, int x_dt, void* y, int y_dt, size_t n, vdn_stream stream);
size_t vdn_sizeof_gemm_desc(void);      /* layout probes for FFI bindings */
size_t vdn_offsetof_gemm_zeros(void);
size_t vdn_offsetof_gemm_res2_lo(void);
const char* vdn_version(void);
int vdn_arch_ok(void); /* 1 if device 0 is gfx950 */

#ifdef __cplusplus
}
#endif
#endif
