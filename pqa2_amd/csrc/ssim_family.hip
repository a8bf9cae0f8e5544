// libvmaf's float_ssim and float_ms_ssim features (the iqa-derived extractors float_ssim.c / float_ms_ssim.c): luma only,
// f32 filtering, an 11 x 11 Gaussian window (sigma 1.5) over the valid region, l / c / s per pixel.  The definition and its
// unpinned items: tests/ssim_family_ref.py (the CPU restatement the kernels are tested against) and DESIGN.md section 5.
//
// Three kernels, all LDS-tiled (a workgroup owns a 64 x 32 block of the map, a 64 x 16 block of a decimated plane):
//   ssf_map_kernel<T, BOX>  the five filtered moments and the l, c, s, l*c*s sums of one tile of the SSIM map.  T = u8 / u16
//                           reads the caller's planes (scale 0 of MS-SSIM, float_ssim), T = float a pyramid level.  BOX:
//                           float_ssim's f x f box decimation is formed while the tile is loaded (the luma pair is read once,
//                           the map is computed on the decimated samples).
//                           DOWN (MS-SSIM scale 0): the same launch also writes the 9/7-decimated f32 planes of scale 1
//                           from the tile it holds, as VIF scale 0 fuses its decimation (the full-resolution pair is read once).
//   ssf_down_kernel<T>      the 9/7 low-pass + 2:1 decimation between the deeper MS-SSIM scales (half-sample symmetric border).
//   ssf_finalize_kernel     fixed-order sum of the tile partials of a frame, the means, and the MS-SSIM product in double,
//                           into the frame's extension record.
// Moments are formed on samples minus a per-thread offset (a sample inside every window of the thread): variance and
// covariance do not change, but E[x^2] - mu^2 no longer cancels two numbers of ~6.5e4 in f32 where the window is flat.  Each tile's sums are
// reduced in double in a fixed order; no atomics, so a frame's record does not depend on batch, launch or alignment.
#include <array>
#include <cmath>

#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int TW = kSsfTileW, TH = kSsfTileH;  // output tile of the map kernel
constexpr int RG = TH / (kBlock / TW);        // output rows per thread (8)
constexpr int HALO = 4;                       // the tile also holds 4 samples left / above: the 9/7 taps of the fused decimation
constexpr int IW = TW + 10 + HALO, IH = TH + 10 + HALO;   // input tile (11 x 11 window + that halo)
constexpr int DTH = 16;                       // output rows of a decimation tile
constexpr float kC1 = (0.01f * 255.0f) * (0.01f * 255.0f);
constexpr float kC2 = (0.03f * 255.0f) * (0.03f * 255.0f);
constexpr float kC3 = kC2 * 0.5f;

struct MapArgs {
  const void* ref;
  const void* dis;
  int64_t rp_r, fp_r, rp_d, fp_d;  // elements
  int sw, sh;                      // size of the planes read (full resolution when box > 1)
  int w, h;                        // size of the plane the map is formed on
  int box;                         // decimation factor (1: none)
  float scale;                     // sample -> float: inv_scale / box^2
  int tiles_x, n_tiles;            // tiles of the map (partials index)
  int grid_x, grid_tiles;          // tiles of the launch: the map's, or with a fused decimation the union of both tilings
  float g[11];
  double* partials;                // [n_frames][n_tiles][4]
  // fused 9/7 decimation (MS-SSIM scale 0): the next scale's f32 planes, ceil(w/2) x ceil(h/2), 32 x 16 per tile
  float* out_r;
  float* out_d;
  int64_t orp, ofp;                // elements
  int ow, oh, down_tx, down_ty;    // next-scale size; decimation tiles per row / column
};

// half-sample symmetric border: -1 -> 0, n -> n - 1 (clamped for safety; every plane here is >= 11 samples wide)
__device__ __forceinline__ int sym(int i, int n) {
  i = i < 0 ? -1 - i : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);
}

template <typename T> __device__ __forceinline__ float as_f(T v) { return (float)v; }

__device__ __forceinline__ f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

// Sample pair {ref, dis} at (x, y) of the plane the map is formed on; x, y already inside it.  BOX: the mean of the f x f
// block that float_ssim's decimation keeps for (x, y), both planes in one loop (unrolled: eight loads of each plane in
// flight before the first add waits).
template <typename T, bool BOX>
__device__ __forceinline__ f2 sample_pair(const T* __restrict__ pr, const T* __restrict__ pd, const MapArgs& a, int x, int y) {
  if constexpr (!BOX) {
    return f2{as_f(pr[(int64_t)y * a.rp_r + x]), as_f(pd[(int64_t)y * a.rp_d + x])} * a.scale;
  } else {
    const int f = a.box, x0 = x * f - f / 2, y0 = y * f - f / 2;
    unsigned sr = 0, sd = 0;
    for (int j = 0; j < f; ++j) {
      const int yy = sym(y0 + j, a.sh);
      const T* rr = pr + (int64_t)yy * a.rp_r;
      const T* rd = pd + (int64_t)yy * a.rp_d;
#pragma unroll 8
      for (int i = 0; i < f; ++i) {
        const int xx = sym(x0 + i, a.sw);
        sr += (unsigned)rr[xx];
        sd += (unsigned)rd[xx];
      }
    }
    return f2{(float)sr, (float)sd} * a.scale;
  }
}

__constant__ float kLpf97[9] = {0.026748757411f, -0.016864118443f, -0.078223266529f, 0.266864118443f, 0.602949018236f,
                                0.266864118443f,  -0.078223266529f, -0.016864118443f, 0.026748757411f};

template <typename T, bool BOX, bool DOWN>
__global__ __launch_bounds__(kBlock) void ssf_map_kernel(const MapArgs a) {
  __shared__ f2 in[IH][IW];   // {ref, dis} interleaved: one ds_read_b64 per tap
  __shared__ float gk[11];    // the taps again, for the vertical pass's row-dependent index
  __shared__ double red[16];
  __shared__ f2 dz[DOWN ? 2 * (TH / 2) + 7 : 1][DOWN ? TW / 2 : 1];   // fused decimation: horizontal pass
  const int tile = xcd_remap(blockIdx.x, a.grid_tiles);
  const int tx = tile % a.grid_x, ty = tile / a.grid_x;
  const int fr = blockIdx.y;
  const int x0 = tx * TW, y0 = ty * TH;
  const T* __restrict__ pr = (const T*)a.ref + (int64_t)fr * a.fp_r;
  const T* __restrict__ pd = (const T*)a.dis + (int64_t)fr * a.fp_d;
  const int tid = threadIdx.x;
  if (tid < 11) gk[tid] = a.g[tid];
#pragma unroll 4
  for (int i = tid; i < IH * IW; i += kBlock) {
    const int ly = i / IW, lx = i - ly * IW;
    // half-sample symmetric fold: what the decimation needs at the borders; map outputs that reach beyond the plane are masked
    const int x = sym(x0 - HALO + lx, a.w), y = sym(y0 - HALO + ly, a.h);
    in[ly][lx] = sample_pair<T, BOX>(pr, pd, a, x, y);
  }
  __syncthreads();
  if constexpr (DOWN) {
    // the next MS-SSIM scale from the same tile: output (32 tx + c, 16 ty + r) takes rows / columns 2 r .. 2 r + 8 of the tile
    if (tx < a.down_tx && ty < a.down_ty) {
      constexpr int DR = 2 * (TH / 2) + 7, DC = TW / 2;
      for (int i = tid; i < DR * DC; i += kBlock) {
        const int r = i / DC, c = i - r * DC;
        f2 u = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 9; ++k) u = pfma(f2{kLpf97[k], kLpf97[k]}, in[r][2 * c + k], u);
        dz[r][c] = u;
      }
      __syncthreads();
      const int c = tid & (DC - 1), r0 = (tid / DC) * 2;   // 8 groups of 2 output rows
      f2 acc[2] = {};
#pragma unroll
      for (int rr = 0; rr < 11; ++rr) {
        const f2 u = dz[2 * r0 + rr][c];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = rr - 2 * j;
          if (k >= 0 && k < 9) acc[j] = pfma(f2{kLpf97[k], kLpf97[k]}, u, acc[j]);
        }
      }
      const int x = tx * DC + c;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int y = ty * (TH / 2) + r0 + j;
        if (x < a.ow && y < a.oh) {
          a.out_r[(int64_t)fr * a.ofp + (int64_t)y * a.orp + x] = acc[j].x;
          a.out_d[(int64_t)fr * a.ofp + (int64_t)y * a.orp + x] = acc[j].y;
        }
      }
    }
    if (tx >= a.tiles_x || ty >= a.n_tiles / a.tiles_x) return;   // a decimation-only tile (block-uniform)
  }
  // One column and RG consecutive output rows per thread: the RG + 10 input rows are filtered horizontally in registers and
  // accumulated into the RG outputs at once.  The thread's offsets are the samples at the centre of its middle window,
  // which lies inside every one of its RG windows: a flat window gives exactly zero moments.  {ref, dis} travel as a pair
  // through packed FMAs: mean and second moment of both planes in two v_pk ops per tap, the cross term in one v_fma.
  const int cx = tid & (TW - 1), rg = (tid / TW) * RG;
  const f2 o = in[HALO + rg + 5 + RG / 2][HALO + cx + 5];
  f2 am[RG], aq[RG];
  float ac[RG];
#pragma unroll
  for (int j = 0; j < RG; ++j) { am[j] = f2{0.f, 0.f}; aq[j] = f2{0.f, 0.f}; ac[j] = 0.f; }
  // rows stay a loop (a full unroll hoists every LDS read and needs all 256 VGPRs: two waves per SIMD instead of five)
#pragma unroll 1
  for (int rr = 0; rr < RG + 10; ++rr) {
    f2 m = {0.f, 0.f}, q = {0.f, 0.f};
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const f2 d = in[HALO + rg + rr][HALO + cx + k] - o;
      const f2 gd = d * a.g[k];
      m += gd;
      q = pfma(gd, d, q);
      c = fmaf(gd.x, d.y, c);
    }
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int k = rr - j;
      if (k >= 0 && k < 11) {   // wave-uniform
        const float g = gk[k];
        am[j] = pfma(f2{g, g}, m, am[j]);
        aq[j] = pfma(f2{g, g}, q, aq[j]);
        ac[j] = fmaf(g, c, ac[j]);
      }
    }
  }
  const int mw = a.w - 10, mh = a.h - 10;
  float sl = 0.f, sc = 0.f, ss = 0.f, slcs = 0.f;
#pragma unroll
  for (int j = 0; j < RG; ++j) {
    if (x0 + cx < mw && y0 + rg + j < mh) {
      const float mu = am[j].x, mv = am[j].y;
      const float vx = aq[j].x - mu * mu, vy = aq[j].y - mv * mv, cxy = ac[j] - mu * mv;
      const float mx = mu + o.x, my = mv + o.y;
      const float sxsy = __builtin_sqrtf(fmaxf(vx, 0.f) * fmaxf(vy, 0.f));
      const float l = (2.f * (mx * my) + kC1) * fast_rcp((mx * mx + my * my) + kC1);
      const float c = (2.f * sxsy + kC2) * fast_rcp((vx + vy) + kC2);
      const float s = (cxy + kC3) * fast_rcp(sxsy + kC3);
      sl += l; sc += c; ss += s; slcs += l * c * s;
    }
  }
  double v[4] = {(double)sl, (double)sc, (double)ss, (double)slcs};
  block_sum<4>(v, red);
  if (tid == 0) {
    double* out = a.partials + ((int64_t)fr * a.n_tiles + ty * a.tiles_x + tx) * 4;
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; out[3] = v[3];
  }
}

// ---- 9/7 low-pass + 2:1 decimation between MS-SSIM scales ----------------------------------------------------------
constexpr int DIW = 2 * TW + 7, DIH = 2 * DTH + 7;   // input columns / rows of a 64 x 16 output tile (9 taps, stride 2)

struct DownArgs {
  const void* ref;
  const void* dis;
  int64_t rp_r, fp_r, rp_d, fp_d;  // elements
  int w, h;
  float scale;
  float* out_r;
  float* out_d;
  int64_t orp, ofp;                // elements
  int ow, oh, tiles_x, n_tiles;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ssf_down_kernel(const DownArgs a) {
  // {ref, dis} pairs, input columns split by parity: the stride-2 taps of the horizontal pass read consecutive words
  __shared__ f2 in[2][DIH][(DIW + 1) / 2];
  __shared__ f2 hz[DIH][TW];
  const int tile = xcd_remap(blockIdx.x, a.n_tiles);
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  const int fr = blockIdx.y;
  const int x0 = tx * TW, y0 = ty * DTH;
  const T* __restrict__ pr = (const T*)a.ref + (int64_t)fr * a.fp_r;
  const T* __restrict__ pd = (const T*)a.dis + (int64_t)fr * a.fp_d;
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int i = tid; i < DIH * DIW; i += kBlock) {
    const int ly = i / DIW, lx = i - ly * DIW;
    const int x = sym(2 * x0 - 4 + lx, a.w), y = sym(2 * y0 - 4 + ly, a.h);
    in[lx & 1][ly][lx >> 1] = f2{as_f(pr[(int64_t)y * a.rp_r + x]), as_f(pd[(int64_t)y * a.rp_d + x])} * a.scale;
  }
  __syncthreads();
  for (int i = tid; i < DIH * TW; i += kBlock) {
    const int r = i / TW, cx = i - r * TW;
    f2 u = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 9; ++k) u = pfma(f2{kLpf97[k], kLpf97[k]}, in[k & 1][r][cx + (k >> 1)], u);
    hz[r][cx] = u;
  }
  __syncthreads();
  const int cx = tid & (TW - 1), rg = (tid / TW) * 4;   // output rows rg .. rg + 3: input rows 2 rg .. 2 rg + 14
  f2 acc[4] = {};
#pragma unroll
  for (int rr = 0; rr < 15; ++rr) {
    const f2 u = hz[2 * rg + rr][cx];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = rr - 2 * j;
      if (k >= 0 && k < 9) acc[j] = pfma(f2{kLpf97[k], kLpf97[k]}, u, acc[j]);
    }
  }
  const int x = x0 + cx;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = y0 + rg + j;
    if (x < a.ow && y < a.oh) {
      a.out_r[(int64_t)fr * a.ofp + (int64_t)y * a.orp + x] = acc[j].x;
      a.out_d[(int64_t)fr * a.ofp + (int64_t)y * a.orp + x] = acc[j].y;
    }
  }
}

// ---- per-frame epilogue ------------------------------------------------------------------------------------------
__device__ double sum_partials(const double* p, int n_tiles, int comp, double* red) {
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < n_tiles; i += kBlock) acc[0] += p[(int64_t)i * 4 + comp];
  __syncthreads();   // red reuse
  block_sum<1>(acc, red);
  return acc[0];     // valid in thread 0
}

// C pow as MS-SSIM meets it: x^0 = 1, a negative base under a fractional exponent gives NaN (the defined outcome)
__device__ __forceinline__ double cpow(double b, double e) { return e == 0.0 ? 1.0 : pow(b, e); }

__global__ __launch_bounds__(kBlock) void ssf_finalize_kernel(const SsfFinalizeArgs a) {
  __shared__ double red[4];
  const int fr = blockIdx.x, tid = threadIdx.x;
  const int row = (int)(((int64_t)a.slot_base + (int64_t)fr * a.slot_step) % a.capacity);
  double* e = a.ext + (int64_t)row * a.ext_stride;
  const double nan = __builtin_nan("");
  double fs[4] = {nan, nan, nan, nan};
  if (a.fs_part) {
    const double* p = a.fs_part + (int64_t)fr * a.fs_tiles * 4;
    for (int q = 0; q < 4; ++q) fs[q] = sum_partials(p, a.fs_tiles, q, red) * a.fs_norm;
  }
  double lm[kMsScales], cm[kMsScales], sm[kMsScales];
  for (int j = 0; j < kMsScales; ++j) lm[j] = cm[j] = sm[j] = nan;
  if (a.ms_part[0]) {
    for (int j = 0; j < kMsScales; ++j) {
      const double* p = a.ms_part[j] + (int64_t)fr * a.ms_tiles[j] * 4;
      lm[j] = sum_partials(p, a.ms_tiles[j], 0, red) * a.ms_norm[j];
      cm[j] = sum_partials(p, a.ms_tiles[j], 1, red) * a.ms_norm[j];
      sm[j] = sum_partials(p, a.ms_tiles[j], 2, red) * a.ms_norm[j];
    }
  }
  if (tid != 0) return;
  // float_ssim is the mean of l*c*s; its l, c, s means follow
  e[0] = fs[3]; e[1] = fs[0]; e[2] = fs[1]; e[3] = fs[2];
  const double w[kMsScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  double ms = nan;
  if (a.ms_part[0]) {
    ms = 1.0;
    for (int j = 0; j < kMsScales; ++j) ms *= cpow(cm[j], w[j]) * cpow(sm[j], w[j]);
    ms *= cpow(lm[kMsScales - 1], w[kMsScales - 1]);
  }
  e[4] = ms;
  for (int j = 0; j < kMsScales; ++j) { e[5 + j] = lm[j]; e[10 + j] = cm[j]; e[15 + j] = sm[j]; }
  // slots 20.. belong to other features (CIEDE2000): left as they are (NaN from the ring fill where nothing writes them)
}

__global__ __launch_bounds__(64) void ext_nan_kernel(double* ext, int slot_base, int capacity, int stride) {
  const int row = (int)(((int64_t)slot_base + blockIdx.x) % capacity);
  if ((int)threadIdx.x < stride) ext[(int64_t)row * stride + threadIdx.x] = __builtin_nan("");
}

}  // namespace

int ssf_tiles(int w, int h) {
  const int mw = w - 10, mh = h - 10;
  if (mw < 1 || mh < 1) return 0;
  return ((mw + TW - 1) / TW) * ((mh + TH - 1) / TH);
}

int ssf_decimation(int w, int h) {
  const int m = w < h ? w : h;
  const int f = (int)(m / 256.0 + 0.5);
  return f > 1 ? f : 1;
}

hipError_t launch_ssf_map(hipStream_t stream, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames, int src_w, int src_h,
                          int box, float inv_scale, double* partials, MutPlaneRun down_ref, MutPlaneRun down_dis) {
  if (n_frames <= 0) return hipSuccess;
  static const auto taps = [] {   // 11 Gaussian taps, sigma 1.5, unit sum (formed in double, stored as f32)
    std::array<float, 11> t{};
    double g[11], s = 0.0;
    for (int k = 0; k < 11; ++k) { const double x = k - 5; g[k] = exp(-x * x / (2.0 * 1.5 * 1.5)); s += g[k]; }
    for (int k = 0; k < 11; ++k) t[k] = (float)(g[k] / s);
    return t;
  }();
  MapArgs a{};
  a.ref = ref.base; a.dis = dis.base;
  a.rp_r = ref.row_pitch; a.fp_r = ref.frame_pitch; a.rp_d = dis.row_pitch; a.fp_d = dis.frame_pitch;
  a.sw = src_w; a.sh = src_h;
  a.box = box < 1 ? 1 : box;
  a.w = (src_w + a.box - 1) / a.box; a.h = (src_h + a.box - 1) / a.box;
  a.scale = inv_scale / (float)(a.box * a.box);
  a.n_tiles = ssf_tiles(a.w, a.h);
  if (a.n_tiles == 0) return hipErrorInvalidValue;
  a.tiles_x = (a.w - 10 + TW - 1) / TW;
  a.grid_x = a.tiles_x;
  a.grid_tiles = a.n_tiles;
  for (int k = 0; k < 11; ++k) a.g[k] = taps[k];
  a.partials = partials;
  const bool down = down_ref.base != nullptr;
  if (down) {   // fused 2:1 decimation: only for the caller's planes, without box decimation
    if (a.box != 1 || elem == ELEM_F32 || !down_dis.base || down_ref.row_pitch != down_dis.row_pitch ||
        down_ref.frame_pitch != down_dis.frame_pitch)
      return hipErrorInvalidValue;
    a.out_r = (float*)down_ref.base; a.out_d = (float*)down_dis.base;
    a.orp = down_ref.row_pitch; a.ofp = down_ref.frame_pitch;
    a.ow = (a.w + 1) / 2; a.oh = (a.h + 1) / 2;
    a.down_tx = (a.ow + TW / 2 - 1) / (TW / 2);
    a.down_ty = (a.oh + TH / 2 - 1) / (TH / 2);
    const int ty = a.n_tiles / a.tiles_x;
    a.grid_x = a.tiles_x > a.down_tx ? a.tiles_x : a.down_tx;
    a.grid_tiles = a.grid_x * (ty > a.down_ty ? ty : a.down_ty);
  }
  const dim3 grid(a.grid_tiles, n_frames), block(kBlock);
  if (a.box > 1) {
    switch (elem) {
      case ELEM_U8: hipLaunchKernelGGL((ssf_map_kernel<uint8_t, true, false>), grid, block, 0, stream, a); break;
      case ELEM_U16: hipLaunchKernelGGL((ssf_map_kernel<uint16_t, true, false>), grid, block, 0, stream, a); break;
      default: return hipErrorInvalidValue;
    }
  } else if (down) {
    switch (elem) {
      case ELEM_U8: hipLaunchKernelGGL((ssf_map_kernel<uint8_t, false, true>), grid, block, 0, stream, a); break;
      case ELEM_U16: hipLaunchKernelGGL((ssf_map_kernel<uint16_t, false, true>), grid, block, 0, stream, a); break;
      default: return hipErrorInvalidValue;
    }
  } else {
    switch (elem) {
      case ELEM_U8: hipLaunchKernelGGL((ssf_map_kernel<uint8_t, false, false>), grid, block, 0, stream, a); break;
      case ELEM_U16: hipLaunchKernelGGL((ssf_map_kernel<uint16_t, false, false>), grid, block, 0, stream, a); break;
      case ELEM_F32: a.scale = 1.0f; hipLaunchKernelGGL((ssf_map_kernel<float, false, false>), grid, block, 0, stream, a); break;
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

hipError_t launch_ssf_down(hipStream_t stream, Elem elem, PlaneRun ref, PlaneRun dis, int n_frames, int w, int h,
                           float inv_scale, MutPlaneRun out_ref, MutPlaneRun out_dis) {
  if (n_frames <= 0) return hipSuccess;
  DownArgs a{};
  a.ref = ref.base; a.dis = dis.base;
  a.rp_r = ref.row_pitch; a.fp_r = ref.frame_pitch; a.rp_d = dis.row_pitch; a.fp_d = dis.frame_pitch;
  a.w = w; a.h = h;
  a.scale = elem == ELEM_F32 ? 1.0f : inv_scale;
  a.out_r = (float*)out_ref.base; a.out_d = (float*)out_dis.base;
  if (out_ref.row_pitch != out_dis.row_pitch || out_ref.frame_pitch != out_dis.frame_pitch) return hipErrorInvalidValue;
  a.orp = out_ref.row_pitch; a.ofp = out_ref.frame_pitch;
  a.ow = (w + 1) / 2; a.oh = (h + 1) / 2;
  a.tiles_x = (a.ow + TW - 1) / TW;
  a.n_tiles = a.tiles_x * ((a.oh + DTH - 1) / DTH);
  const dim3 grid(a.n_tiles, n_frames), block(kBlock);
  switch (elem) {
    case ELEM_U8: hipLaunchKernelGGL((ssf_down_kernel<uint8_t>), grid, block, 0, stream, a); break;
    case ELEM_U16: hipLaunchKernelGGL((ssf_down_kernel<uint16_t>), grid, block, 0, stream, a); break;
    case ELEM_F32: hipLaunchKernelGGL((ssf_down_kernel<float>), grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_ssf_finalize(hipStream_t stream, const SsfFinalizeArgs& args) {
  if (args.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(ssf_finalize_kernel, dim3(args.n_frames), dim3(kBlock), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_ext_fill_nan(hipStream_t stream, double* ext, int slot_base, int n_rows, int capacity, int stride) {
  if (n_rows <= 0) return hipSuccess;
  if (stride > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ext_nan_kernel, dim3(n_rows), dim3(64), 0, stream, ext, slot_base, capacity, stride);
  return hipGetLastError();
}

}  // namespace pqa
