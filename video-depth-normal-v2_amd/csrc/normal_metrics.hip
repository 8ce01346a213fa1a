// Angular error of predicted normals and the normal-map picture, for tensors that already sit in HBM. An extension beyond
// the reference, whose one measure of normal quality is VideoNormalLoss (normals.hip): DESIGN 5 has the definition.
//   vdn_normal_angle_map    the angle of every kept pixel, float32, NaN at a dropped one
//   vdn_normal_angle_stats  n, mean, median, rmse and the shares under 5, 7.5, 11.25, 22.5 and 30 degrees of the batch, of
//                           each item and of each frame
//   vdn_normal_colorize     normals (or the normals of a depth map) as RGB / BGR bytes
// The angle is atan2(|a x b|, a . b) in fp64 from the f32 samples, with separate multiply and add roundings (contraction is
// off for this file); never acos of a cosine, which loses half the digits near 0 and 180 degrees. Kept pixels, the erosion
// and a target made from depth are normals.hip's (normal_px.hpp), except that the depth's normal (-Ix, -Iy, 1) keeps its
// length: the angle does not depend on it.
// The statistics take one sweep over the inputs that leaves a block row per frame_sums.hpp (2 sums, 7 counts) and the float32
// angle plane in the workspace, a one-block fold (frames, items, batch, in index order) that also writes each set's two
// median ranks into the states of select.hpp, the select's three passes over the plane at each of the three levels
// (group = 1, T, B T), and a kernel that writes the rows. No floating-point atomics: two runs give the same bits. A lane owns
// four consecutive pixels whenever H W is a multiple of 4, read by one 16-byte load per plane where the planes are 16-byte
// aligned and by a load per pixel otherwise, so the order of every sum depends on the shape alone.
#include "common.hpp"
#include "frame_sums.hpp"
#include "select.hpp"

#pragma clang fp contract(off)
#include "normal_px.hpp"

namespace {

constexpr int NS = 2;  // sums of a row: angle, angle^2
constexpr int NC = 7;  // counts of a row: kept pixels, angle < 5, 7.5, 11.25, 22.5, 30, NaN angles
constexpr int NCOL = 9;
constexpr double DEG = 57.29577951308232;  // 180 / pi

// the workspace of the statistics, in 8-byte slots; S = 1 + B + F sets (batch, items, frames), F = B T frames
//   [F][NE_BPF] block sums | block counts | [S] set sums | set counts | the selects of the batch, the items and the frames
//   (select.hpp: bins, then states) | the float32 angle plane [F][hw]
struct Ws {
  double* bsum;
  int64_t* bcnt;
  double* ssum;
  int64_t* scnt;
  void* sel[3];  // 0: one set of all frames, 1: a set per item, 2: a set per frame
  float* plane;
  size_t sel_bytes, bytes;
  __host__ __device__ Ws(void* p, int B, int T, size_t hw) {
    const size_t F = (size_t)B * T, S = 1 + B + F;
    bsum = (double*)p;
    bcnt = (int64_t*)(bsum + F * NE_BPF * NS);
    ssum = (double*)(bcnt + F * NE_BPF * NC);
    scnt = (int64_t*)(ssum + S * NS);
    char* c = (char*)(scnt + ((S * NC + 1) & ~(size_t)1));  // an even number of slots so far: the plane keeps p's 16-byte alignment
    const size_t per_set = 2 * (NBIN * sizeof(uint32_t) + sizeof(SelState));  // select_workspace_bytes(1, 2): a multiple of 16
    sel[0] = c;
    sel[1] = c + per_set;
    sel[2] = c + per_set * (1 + (size_t)B);
    sel_bytes = per_set * S;
    plane = (float*)(c + sel_bytes);
    bytes = (size_t)((char*)plane - (char*)p) + ((F * hw * sizeof(float) + 7) & ~(size_t)7);
  }
};

// the angle between a and b in degrees; NaN when a component is not finite, 90 when either vector is zero (the angle whose
// cosine is the 0 that F.cosine_similarity's clamped norms give the loss). Products of f32 values are exact in fp64 and
// their squares stay under 1e155: nothing overflows.
__device__ __forceinline__ double angle_deg(const double (&a)[3], const double (&b)[3]) {
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) finite = finite && __builtin_isfinite(a[c]) && __builtin_isfinite(b[c]);
  if (!finite) return __builtin_nan("");
  const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
  if (aa == 0.0 || bb == 0.0) return 90.0;
  const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  const double d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
  return atan2(sqrt((cx * cx + cy * cy) + cz * cz), d) * DEG;
}

// (-Ix, -Iy, 1) of the Sobel / 8 stencil at (y, x) of the reflect-padded depth frame df
__device__ __forceinline__ void depth_normal(const float (&win)[3][3], double (&n)[3]) {
  double ix, iy;
  sobel(win, 0.125, ix, iy);
  n[0] = -ix;
  n[1] = -iy;
  n[2] = 1.0;
}

template <int PPL, bool VEC>
__device__ __forceinline__ void load3v(const float* __restrict__ f, int hw, int p0, float (&v)[3][PPL]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) load_px<PPL, VEC>(f + (size_t)c * hw + p0, v[c]);
}

// ------------------------------------------------------------------------------------------------ the sweep
// Block blockIdx.x = f * NE_BPF + b sweeps frame f as frame_sums.hpp states. plane f32 [F][hw] receives every pixel's angle
// (NaN at a dropped pixel). STATS: the block's row of sums and counts as well. VEC: 16-byte loads and stores (pred, a stored
// target and the plane are 16-byte aligned); the values and their order are the same without.
template <int PPL, bool VEC, bool DEPTH, bool STATS>
__global__ __launch_bounds__(256) void angle_sweep_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, int erode, int H, int W,
                                                          float* __restrict__ plane, double* __restrict__ bsum,
                                                          int64_t* __restrict__ bcnt) {
  const int f = blockIdx.x / NE_BPF, b = blockIdx.x % NE_BPF;
  const int hw = H * W;
  const float* pf = pred + (size_t)f * 3 * hw;
  const float* tf = target + (size_t)f * (DEPTH ? 1 : 3) * hw;
  const uint8_t* mf = mask ? mask + (size_t)f * hw : nullptr;
  float* of = plane + (size_t)f * hw;
  Tuple<double, NS> sum = {{0.0, 0.0}};
  Tuple<int, NC> cnt = {{0, 0, 0, 0, 0, 0, 0}};
  for (int64_t q0 = sweep_first<PPL>(b); q0 < hw; q0 += sweep_stride<NE_BPF, PPL>()) {
    const int p0 = (int)q0;
    float pv[3][PPL], tv[3][PPL], o[PPL];
    load3v<PPL, VEC>(pf, hw, p0, pv);
    if (!DEPTH) load3v<PPL, VEC>(tf, hw, p0, tv);
    RowWalk at(p0, W);
    const Hood<PPL, DEPTH> hood(tf, erode ? mf : nullptr, at.y, at.x, H, W);  // without erosion: the depth windows alone
    const uint32_t own = (!erode && mf) ? load_mask<PPL, false>(mf + p0) : 0x01010101u;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const bool keep = erode ? hood.keep(mf, j, at.y, at.x, H, W) : mask_byte(own, j) != 0;
      o[j] = __builtin_nanf("");
      if (keep) {  // a dropped pixel is skipped: nothing under it is read into the sums
        const double a[3] = {(double)pv[0][j], (double)pv[1][j], (double)pv[2][j]};
        double t[3];
        if (DEPTH) {
          float win[3][3];
          if (hood.fast) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int c = 0; c < 3; ++c) win[r][c] = hood.dq[r][j + c];
          } else {
            window_at(tf, at.y, at.x, H, W, win);
          }
          depth_normal(win, t);
        } else {
          t[0] = (double)tv[0][j], t[1] = (double)tv[1][j], t[2] = (double)tv[2][j];
        }
        const double ang = angle_deg(a, t);
        o[j] = (float)ang;
        if (STATS) {
          cnt.v[0] += 1;
          if (ang != ang) {
            cnt.v[6] += 1;  // the set's flag: its sums are not looked at
          } else {
            sum.v[0] += ang;
            sum.v[1] += ang * ang;
            cnt.v[1] += ang < 5.0;
            cnt.v[2] += ang < 7.5;
            cnt.v[3] += ang < 11.25;
            cnt.v[4] += ang < 22.5;
            cnt.v[5] += ang < 30.0;
          }
        }
      }
      at.step(W);
    }
    store_px<PPL, VEC>(of + p0, o);
  }
  if (STATS) block_row<NS, NC>(sum, cnt, bsum, bcnt);
}

// ------------------------------------------------------------------------------------------------ the fold
// One block: every frame's blocks in index order, every item's frames in index order, the items in index order; then each
// set's select states: prefix 0 and the ranks floor and ceil of (m - 1) / 2 among its m keys, the kept pixels whose angle
// is a number. The bins were zeroed by the entry's memset.
__global__ __launch_bounds__(256) void angle_fold_kernel(void* __restrict__ workspace, int B, int T, size_t hw) {
  const Ws ws(workspace, B, T, hw);
  const int F = B * T, S = 1 + B + F;
  double s[NS];
  int64_t n[NC];
  for (int f = threadIdx.x; f < F; f += 256) {
    fold_blocks<NS, NC, NE_BPF>(ws.bsum, ws.bcnt, f, s, n);
    store_row<NS, NC>(ws.ssum, ws.scnt, (size_t)(1 + B + f), s, n);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < B; i += 256) {
    fold_frames<NS, NC>(ws.ssum + (size_t)(1 + B) * NS, ws.scnt + (size_t)(1 + B) * NC, i * T, T, s, n);
    store_row<NS, NC>(ws.ssum, ws.scnt, (size_t)(1 + i), s, n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    fold_frames<NS, NC>(ws.ssum + NS, ws.scnt + NC, 0, B, s, n);
    store_row<NS, NC>(ws.ssum, ws.scnt, 0, s, n);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < S; r += 256) {
    const int level = r == 0 ? 0 : (r <= B ? 1 : 2), sets = level == 0 ? 1 : (level == 1 ? B : F);
    const int set = level == 0 ? 0 : (level == 1 ? r - 1 : r - 1 - B);
    const int64_t m = ws.scnt[(size_t)r * NC] - ws.scnt[(size_t)r * NC + 6];
    SelState* st = select_state(ws.sel[level], sets, 2) + (size_t)set * 2;
    st[0] = SelState{0u, (uint32_t)(m > 0 ? (m - 1) / 2 : 0)};
    st[1] = SelState{0u, (uint32_t)(m / 2)};
  }
}

// both slots select among the numbers of the plane: a NaN (a dropped pixel, or a NaN angle, which the set's count flags) has no key
struct AngleKey {
  static constexpr int SLOTS = 2, PER = 1;
  const float* plane;
  size_t n;
  __device__ __forceinline__ uint32_t operator()(int f, size_t i, uint32_t (&key)[1][2]) const {
    const float v = plane[(size_t)f * n + i];
    key[0][0] = key[0][1] = ordered_key(v);
    return v == v ? 3u : 0u;
  }
};

// rows f64 [S][9] = n, mean, median, rmse, a5, a7_5, a11_25, a22_5, a30
__global__ __launch_bounds__(256) void angle_rows_kernel(void* __restrict__ workspace, int B, int T, size_t hw, double* __restrict__ rows) {
  const Ws ws(workspace, B, T, hw);
  const int F = B * T, S = 1 + B + F;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= S) return;
  const int level = r == 0 ? 0 : (r <= B ? 1 : 2), sets = level == 0 ? 1 : (level == 1 ? B : F);
  const int set = level == 0 ? 0 : (level == 1 ? r - 1 : r - 1 - B);
  const int64_t* c = ws.scnt + (size_t)r * NC;
  double* o = rows + (size_t)r * NCOL;
  const double n = (double)c[0];
  o[0] = n;
  if (c[0] == 0 || c[6] != 0) {
#pragma unroll
    for (int k = 1; k < NCOL; ++k) o[k] = __builtin_nan("");
    return;
  }
  const SelState* st = select_state(ws.sel[level], sets, 2) + (size_t)set * 2;
  const double lo = (double)key_value(st[0].prefix), hi = (double)key_value(st[1].prefix);
  o[1] = ws.ssum[(size_t)r * NS] / n;
  o[2] = (lo + hi) / 2.0;  // numpy.median: the mean of the two middle values, the same one for odd n
  o[3] = sqrt(ws.ssum[(size_t)r * NS + 1] / n);
#pragma unroll
  for (int k = 0; k < 5; ++k) o[4 + k] = (double)c[1 + k] / n;
}

// ------------------------------------------------------------------------------------------------ the picture
// PPL consecutive pixels of the flattened [N][hw] per lane: 4 (hw a multiple of 4 and out 4-byte aligned: three 4-byte
// stores) or 1. VEC: the planes of x by 16-byte loads (x 16-byte aligned, !DEPTH).
template <int PPL, bool VEC, bool DEPTH>
__global__ __launch_bounds__(256) void normal_colorize_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, size_t total,
                                                              int H, int W, int bgr) {
  const size_t hw = (size_t)H * W;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * PPL; i < total; i += (size_t)gridDim.x * 256 * PPL) {
    const size_t f = i / hw;
    const int p0 = (int)(i - f * hw);
    float v[3][PPL];
    if (!DEPTH) load3v<PPL, VEC>(x + f * 3 * hw, (int)hw, p0, v);
    RowWalk at(p0, W);
    uint8_t px[PPL * 3];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      double a[3];
      if (DEPTH) {
        float win[3][3];
        window_at(x + f * hw, at.y, at.x, H, W, win);
        depth_normal(win, a);
      } else {
        a[0] = (double)v[0][j], a[1] = (double)v[1][j], a[2] = (double)v[2][j];
      }
      const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
      const bool ok = __builtin_isfinite(a[0]) && __builtin_isfinite(a[1]) && __builtin_isfinite(a[2]) && aa != 0.0;
      const double len = sqrt(aa);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double vc = ((a[c] / len) * 0.5 + 0.5) * 255.0;
        px[j * 3 + (bgr ? 2 - c : c)] = ok ? (uint8_t)floor(vc + 0.5) : (uint8_t)128;
      }
      at.step(W);
    }
    if constexpr (PPL == 4) {
      uint32_t* o = (uint32_t*)(out + i * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) out[i * 3 + k] = px[k];
    }
  }
}

// the argument checks the angle entries share; VDN_OK when the call may launch
inline int check_angle_args(const float* pred, const float* target, int frames, int H, int W) {
  if (!pred || !target || frames <= 0 || H < 2 || W < 2) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX || frames > 65535) return VDN_EUNSUPPORTED;
  if (misaligned(4, pred, target)) return VDN_EALIGN;
  return VDN_OK;
}

template <bool STATS>
inline void launch_sweep(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int erode, int frames, int H,
                         int W, float* plane, double* bsum, int64_t* bcnt, hipStream_t s) {
  const size_t hw = (size_t)H * W;
  const dim3 grid((unsigned)frames * NE_BPF), block(256);
  // a depth target is read through its stencil, never by quads
  const bool vec = wide_ok(hw, {pred, target_is_depth ? nullptr : target, plane});
  with_ppl(hw % 4 == 0, [&](auto ppl) {
    with_bool(vec, [&](auto v) {
      with_bool(target_is_depth != 0, [&](auto depth) {
        constexpr int PPL = decltype(ppl)::value;
        constexpr bool VEC = PPL == 4 && decltype(v)::value;
        hipLaunchKernelGGL((angle_sweep_kernel<PPL, VEC, decltype(depth)::value, STATS>), grid, block, 0, s, pred, target, mask, erode,
                           H, W, plane, bsum, bcnt);
      });
    });
  });
}

}  // namespace

extern "C" int vdn_normal_angle_map(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int erode,
                                    int frames, int H, int W, float* out, vdn_stream stream) {
  if (!out) return VDN_EINVAL;
  if (const int rc = check_angle_args(pred, target, frames, H, W)) return rc;
  if (misaligned(4, out)) return VDN_EALIGN;
  launch_sweep<false>(pred, target, target_is_depth, mask, erode != 0, frames, H, W, out, nullptr, nullptr, (hipStream_t)stream);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" size_t vdn_normal_angle_stats_workspace_bytes(int B, int T, int H, int W) {
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || (int64_t)B * T > 65535) return 0;
  return Ws(nullptr, B, T, (size_t)H * W).bytes;
}

extern "C" int vdn_normal_angle_stats(const float* pred, const float* target, int target_is_depth, const uint8_t* mask, int erode, int B,
                                      int T, int H, int W, void* workspace, double* rows, vdn_stream stream) {
  if (!workspace || !rows || B <= 0 || T <= 0) return VDN_EINVAL;
  if ((int64_t)B * T > 65535) return VDN_EUNSUPPORTED;
  const int F = B * T;
  if (const int rc = check_angle_args(pred, target, F, H, W)) return rc;
  const size_t hw = (size_t)H * W;
  if ((uint64_t)F * hw >= ((uint64_t)1 << 32)) return VDN_EUNSUPPORTED;  // the batch is one set of the select
  if (misaligned(8, workspace, rows)) return VDN_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const Ws ws(workspace, B, T, hw);
  const hipError_t e = hipMemsetAsync(ws.sel[0], 0, ws.sel_bytes, s);  // the bins of the three selects
  if (e != hipSuccess) return -(1000 + (int)e);
  launch_sweep<true>(pred, target, target_is_depth, mask, erode != 0, F, H, W, ws.plane, ws.bsum, ws.bcnt, s);
  hipLaunchKernelGGL(angle_fold_kernel, dim3(1), dim3(256), 0, s, workspace, B, T, hw);
  const AngleKey key{ws.plane, hw};
  select_passes(key, F, F, hw, ws.sel[0], s);
  select_passes(key, F, T, hw, ws.sel[1], s);
  select_passes(key, F, 1, hw, ws.sel[2], s);
  hipLaunchKernelGGL(angle_rows_kernel, dim3((1 + B + F + 255) / 256), dim3(256), 0, s, workspace, B, T, hw, rows);
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}

extern "C" int vdn_normal_colorize(const float* x, int from_depth, int bgr, uint8_t* out, int N, int H, int W, vdn_stream stream) {
  if (!x || !out || N <= 0 || H <= 0 || W <= 0 || (from_depth && (H < 2 || W < 2))) return VDN_EINVAL;
  if ((int64_t)H * W > INT32_MAX) return VDN_EUNSUPPORTED;
  if (misaligned(4, x)) return VDN_EALIGN;
  const size_t hw = (size_t)H * W, total = (size_t)N * hw;
  const bool quads = hw % 4 == 0 && !misaligned(4, out);
  with_ppl(quads, [&](auto ppl) {
    with_bool(!from_depth && !misaligned(16, x), [&](auto v) {
      with_bool(from_depth != 0, [&](auto depth) {
        constexpr int PPL = decltype(ppl)::value;
        constexpr bool VEC = PPL == 4 && decltype(v)::value;
        hipLaunchKernelGGL((normal_colorize_kernel<PPL, VEC, decltype(depth)::value>), dim3(grid_for(total / PPL, 16384)), dim3(256), 0,
                           (hipStream_t)stream, x, out, total, H, W, bgr != 0);
      });
    });
  });
  VDN_CHECK_LAUNCH();
  return VDN_OK;
}
