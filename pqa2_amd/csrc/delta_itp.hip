// Delta E ITP (ITU-R BT.2124) of frame pairs: per luma pixel Y'CbCr code values -> R'G'B' (a 3 x 4 matrix) -> linear display
// light in cd/m2 (the PQ EOTF, the HLG inverse OETF and OOTF, or BT.1886) -> LMS / 10000 (a 3 x 3 matrix) -> PQ inverse EOTF
// -> ICtCp (BT.2100) for the reference and the captured frame, dE = 720 sqrt(dI^2 + dT^2 + dP^2) with T = Ct / 2.  The
// definition, its constants and the measured errors: tests/itp_ref.py and DESIGN.md section 5.
//
// Three kernels:
//   delta_itp_kernel<T, HS, VS, TR>  shaped after ciede_kernel: one thread per chroma sample, the chroma part of the first
//                            matrix once, then the (1 << HS) x (1 << VS) luma pixels under it (chroma by replication); ref and
//                            dis travel as an f2 pair.  A workgroup owns 64 x 4 chroma samples; per thread f32 sums, per tile
//                            doubles in a fixed order, one partial of 8 values per tile.  The transfer is a template argument.
//                            No f64 in the per-pixel path, no scratch, LDS for the reduction only, no atomics.  (As in
//                            ciede_kernel there is no loop over chroma rows and the shift-2 pixel loops stay rolled.)
//   delta_itp_finalize_kernel  a frame's partials, in a fixed order, into out[frame][8] doubles.
//   delta_itp_debug_kernel   the device function on single code triples (pqa_debug_itp).
//
// Issue cost: every power is exp2(k log2 x) on the hardware v_log_f32 / v_exp_f32 (a few ulp); PQ costs 5 transcendentals per
// channel each way (two powers and one reciprocal), so a PQ pixel pair is 60 of them and a square root.
//
// The neutral axis is exact.  In exact arithmetic a neutral sample (Cb = Cr = the matrix's neutral point) decodes to R' = G' =
// B', gives L = M = S (the rows of RGB -> LMS have one sum) and Ct = Cp = 0.  Rounded f32 coefficients lose that by an ulp
// per stage, which would turn a pure luminance difference into chroma noise.  itp_prepare therefore rewrites both matrices
// about the neutral axis:  R' = gy Y + (cu (Cb - u0) + cv (Cr - v0) + o)  and  L = ls G + lr (R - G) + lb (B - G), and where
// the three rows' gy, o or ls agree to within the rounding of the coefficients they came from it gives them one value.  The
// chroma rows of ICtCp are formed from differences, Ct = a (L' - M') + b (S' - M'): a grey has Ct = Cp = 0 exactly.
#include <cmath>

#include "../../include/pqa_vmaf.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int CTW = kCiedeTileW, CTH = kCiedeTileH;   // chroma samples per workgroup tile (64 x 4), as ciede_kernel
static_assert(CTW * CTH == kBlock, "one chroma sample per thread");

// ST 2084
constexpr double kM1 = 2610.0 / 16384.0, kM2 = 2523.0 / 4096.0 * 128.0;
constexpr float kC1 = (float)(3424.0 / 4096.0), kC2 = (float)(2413.0 / 4096.0 * 32.0), kC3 = (float)(2392.0 / 4096.0 * 32.0);
// HLG (BT.2100)
constexpr double kHlgA = 0.17883277, kHlgB = 0.28466892, kHlgC = 0.55991073;
constexpr double kLog2e = 1.4426950408889634;
// LMS' -> (720 I, 360 Ct, 720 Cp); the chroma rows in differences: -13613 = -(6610 + 7003), -17390 = -(17933 - 543)
constexpr float kI = 360.0f;
constexpr float kTa = (float)(360.0 * 6610.0 / 4096.0), kTb = (float)(360.0 * 7003.0 / 4096.0);
constexpr float kPa = (float)(720.0 * 17933.0 / 4096.0), kPb = (float)(720.0 * -543.0 / 4096.0);

__device__ __forceinline__ float hw_log2(float x) { return __builtin_amdgcn_logf(x); }   // v_log_f32
__device__ __forceinline__ float hw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32
__device__ __forceinline__ float hw_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }  // v_sqrt_f32
__device__ __forceinline__ float hw_rcp(float x) { return __builtin_amdgcn_rcpf(x); }    // v_rcp_f32

__device__ __forceinline__ f2 pow2(f2 x, float k) { return f2{hw_exp2(k * hw_log2(x.x)), hw_exp2(k * hw_log2(x.y))}; }   // x^k, x >= 0 (0 -> 0 for k > 0)
__device__ __forceinline__ f2 fma2(f2 a, float s, f2 c) { return f2{fmaf(a.x, s, c.x), fmaf(a.y, s, c.y)}; }
__device__ __forceinline__ f2 max0(f2 v) { return f2{fmaxf(v.x, 0.0f), fmaxf(v.y, 0.0f)}; }
__device__ __forceinline__ f2 clamp01(f2 v) { return f2{fminf(fmaxf(v.x, 0.0f), 1.0f), fminf(fmaxf(v.y, 0.0f), 1.0f)}; }
// 1 / d with one Newton step: the quotient of the PQ inverse is raised to the power 78.8 afterwards
__device__ __forceinline__ float rcp_nr(float d) {
  const float r = hw_rcp(d);
  return fmaf(fmaf(-d, r, 1.0f), r, r);
}

// ST 2084 EOTF of a signal in [0, 1]: luminance / 10000
__device__ __forceinline__ f2 pq_eotf(f2 e) {
  const f2 p = pow2(e, (float)(1.0 / kM2));
  const f2 num = max0(p - f2{kC1, kC1});
  const f2 y = f2{num.x * hw_rcp(fmaf(-kC3, p.x, kC2)), num.y * hw_rcp(fmaf(-kC3, p.y, kC2))};
  return pow2(y, (float)(1.0 / kM1));
}

// ST 2084 inverse EOTF of y = luminance / 10000 >= 0
__device__ __forceinline__ f2 pq_inverse(f2 y) {
  const f2 yp = pow2(y, (float)kM1);
  const f2 v = f2{fmaf(kC2, yp.x, kC1) * rcp_nr(fmaf(kC3, yp.x, 1.0f)), fmaf(kC2, yp.y, kC1) * rcp_nr(fmaf(kC3, yp.y, 1.0f))};
  return pow2(v, (float)kM2);
}

// HLG inverse OETF of a signal >= 0: scene light, 1 at signal 1
__device__ __forceinline__ f2 hlg_inverse_oetf(f2 e) {
  const f2 lo = e * e * (float)(1.0 / 3.0);
  const float k = (float)(kLog2e / kHlgA), c = (float)kHlgC;
  const f2 hi = (f2{hw_exp2((e.x - c) * k), hw_exp2((e.y - c) * k)} + (float)kHlgB) * (float)(1.0 / 12.0);
  return f2{e.x <= 0.5f ? lo.x : hi.x, e.y <= 0.5f ? lo.y : hi.y};
}

struct Itp3 { f2 i, t, p; };   // (720 I, 360 Ct, 720 Cp) of {ref, dis}

// R'G'B' pairs -> ICtCp pairs; the kernel's and pqa_debug_itp's one definition
template <int TR>
__device__ __forceinline__ Itp3 itp_of(f2 R, f2 G, f2 B, const ItpCoef& k) {
  // light on a scale of its own (r, g, b) and what takes it to cd/m2 (sc): the differences from green are formed before the
  // scale, and not fused with it, so that R' = G' = B' gives exact zeros
  f2 r, g, b, sc;
  if (TR == PQA_ITP_PQ) {
    r = pq_eotf(clamp01(R)); g = pq_eotf(clamp01(G)); b = pq_eotf(clamp01(B));
    sc = f2{10000.0f, 10000.0f};
  } else if (TR == PQA_ITP_HLG) {
    r = hlg_inverse_oetf(max0(R)); g = hlg_inverse_oetf(max0(G)); b = hlg_inverse_oetf(max0(B));
    const f2 ys = r * 0.2627f + g * 0.6780f + b * 0.0593f;
    const f2 pw = pow2(ys, k.gamma_m1) * k.peak;   // Lw Ys^(gamma - 1); black stays black whatever the sign of gamma - 1
    sc = f2{ys.x > 0.0f ? pw.x : 0.0f, ys.y > 0.0f ? pw.y : 0.0f};
  } else {
    r = pow2(max0(R), 2.4f); g = pow2(max0(G), 2.4f); b = pow2(max0(B), 2.4f);
    sc = f2{k.peak, k.peak};
  }
  f2 dr, db;
  {
#pragma clang fp contract(off)
    dr = r - g;
    db = b - g;
  }
  g = g * sc; dr = dr * sc; db = db * sc;
  const f2 L = pq_inverse(max0(g * k.ls[0] + dr * k.lr[0] + db * k.lb[0]));
  const f2 M = pq_inverse(max0(g * k.ls[1] + dr * k.lr[1] + db * k.lb[1]));
  const f2 S = pq_inverse(max0(g * k.ls[2] + dr * k.lr[2] + db * k.lb[2]));
  const f2 lm = L - M, sm = S - M;
  return Itp3{(L + M) * kI, lm * kTa + sm * kTb, lm * kPa + sm * kPb};
}

// ---- the frame kernel -------------------------------------------------------------------------------------------
struct ItpArgs {
  const void* ref[3];
  const void* dis[3];
  int64_t fp_r[3], fp_d[3];                     // frame pitches, elements
  int rp_r[3], rp_d[3];                         // row pitches, elements (< 2^31: checked by the launcher)
  int w, h, cw, ch;                             // luma and chroma plane sizes
  int tiles_x, n_tiles;
  ItpCoef k;
  double* partials;                             // [n_frames][n_tiles][kItpSums]
};

template <typename T> __device__ __forceinline__ f2 ld_pair(const T* r, const T* d, int x) { return f2{(float)r[x], (float)d[x]}; }

template <typename T, int HS, int VS, int TR>
__global__ __launch_bounds__(kBlock) void delta_itp_kernel(const ItpArgs a) {
  __shared__ double red[4 * 5];
  __shared__ float red_max[4];
  __shared__ int red_cnt[4][2];
  const int tile = blockIdx.x, fr = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int cx = (tile % a.tiles_x) * CTW + lane;
  const int cy = (tile / a.tiles_x) * CTH + wid;
  const T* ry = (const T*)a.ref[0] + (int64_t)fr * a.fp_r[0];
  const T* ru = (const T*)a.ref[1] + (int64_t)fr * a.fp_r[1];
  const T* rv = (const T*)a.ref[2] + (int64_t)fr * a.fp_r[2];
  const T* dy = (const T*)a.dis[0] + (int64_t)fr * a.fp_d[0];
  const T* du = (const T*)a.dis[1] + (int64_t)fr * a.fp_d[1];
  const T* dv = (const T*)a.dis[2] + (int64_t)fr * a.fp_d[2];
  float s_de = 0.0f, s_i = 0.0f, s_t = 0.0f, s_p = 0.0f, s_ref = 0.0f, mx = 0.0f;
  int above = 0, pixels = 0;
  if (cx < a.cw && cy < a.ch) {
    // chroma part of Y'CbCr -> R'G'B', once per chroma sample
    const f2 U = ld_pair(ru + (int64_t)cy * a.rp_r[1], du + (int64_t)cy * a.rp_d[1], cx) - a.k.u0;
    const f2 V = ld_pair(rv + (int64_t)cy * a.rp_r[2], dv + (int64_t)cy * a.rp_d[2], cx) - a.k.v0;
    const f2 cr = fma2(U, a.k.cu[0], fma2(V, a.k.cv[0], f2{a.k.o[0], a.k.o[0]}));
    const f2 cg = fma2(U, a.k.cu[1], fma2(V, a.k.cv[1], f2{a.k.o[1], a.k.o[1]}));
    const f2 cb = fma2(U, a.k.cu[2], fma2(V, a.k.cv[2], f2{a.k.o[2], a.k.o[2]}));
#pragma unroll VS < 2 ? 2 : 1
    for (int sy = 0; sy < (1 << VS); ++sy) {
      const int y = (cy << VS) + sy;
      if (VS > 0 && y >= a.h) break;
      const T* rrow = ry + (int64_t)y * a.rp_r[0];
      const T* drow = dy + (int64_t)y * a.rp_d[0];
#pragma unroll HS < 2 ? 2 : 1
      for (int sx = 0; sx < (1 << HS); ++sx) {
        const int x = (cx << HS) + sx;
        if (HS > 0 && x >= a.w) break;
        const f2 Y = ld_pair(rrow, drow, x);
        const Itp3 c = itp_of<TR>(fma2(Y, a.k.gy[0], cr), fma2(Y, a.k.gy[1], cg), fma2(Y, a.k.gy[2], cb), a.k);
        float di, dt, dp;   // plain differences, not fused with the products in front of them: identical pixels give exact zeros
        {
#pragma clang fp contract(off)
          di = c.i.x - c.i.y; dt = c.t.x - c.t.y; dp = c.p.x - c.p.y;
        }
        const float i2 = di * di, t2 = dt * dt, p2 = dp * dp;
        const float de = hw_sqrt(i2 + t2 + p2);
        s_de += de; s_i += i2; s_t += t2; s_p += p2; s_ref += c.i.x;
        mx = fmaxf(mx, de);
        above += de > a.k.threshold ? 1 : 0;
        ++pixels;
      }
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {   // the wave's maximum and counts; order does not matter to either
    mx = fmaxf(mx, __shfl_xor(mx, m));
    above += __shfl_xor(above, m);
    pixels += __shfl_xor(pixels, m);
  }
  if (lane == 0) { red_max[wid] = mx; red_cnt[wid][0] = above; red_cnt[wid][1] = pixels; }
  const float in[5] = {s_de, s_i, s_t, s_p, s_ref};
  double out[5];
  block_sum_f32<5>(in, out, red);   // its barrier also covers red_max / red_cnt
  if (threadIdx.x != 0) return;
  double* p = a.partials + ((int64_t)fr * a.n_tiles + tile) * kItpSums;
  p[0] = out[0]; p[1] = out[1]; p[2] = out[2]; p[3] = out[3];
  p[4] = (double)fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
  p[5] = (double)(red_cnt[0][0] + red_cnt[1][0] + red_cnt[2][0] + red_cnt[3][0]);
  p[6] = (double)(red_cnt[0][1] + red_cnt[1][1] + red_cnt[2][1] + red_cnt[3][1]);
  p[7] = out[4];
}

// out[frame][8]: the sums of a frame's partials (a thread takes every kBlock-th tile, then block_sum: one fixed order whatever
// the launch), the maximum, the counts (whole numbers far below 2^53: exact) and the reference's sum of I without its 720
__global__ __launch_bounds__(kBlock) void delta_itp_finalize_kernel(const double* partials, int n_tiles, double* out) {
  __shared__ double red[4 * 7];
  __shared__ double red_max[4];
  const int fr = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double* p = partials + (int64_t)fr * n_tiles * kItpSums;
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double mx = 0.0;
  for (int i = threadIdx.x; i < n_tiles; i += kBlock) {
    const double* q = p + (int64_t)i * kItpSums;
    acc[0] += q[0]; acc[1] += q[1]; acc[2] += q[2]; acc[3] += q[3]; acc[4] += q[5]; acc[5] += q[6]; acc[6] += q[7];
    mx = fmax(mx, q[4]);
  }
  for (int m = 32; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m));
  if (lane == 0) red_max[wid] = mx;
  block_sum<7>(acc, red);
  if (threadIdx.x != 0) return;
  double* o = out + (int64_t)fr * kItpSums;
  o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
  o[4] = fmax(fmax(red_max[0], red_max[1]), fmax(red_max[2], red_max[3]));
  o[5] = acc[4]; o[6] = acc[5];
  o[7] = acc[6] * (1.0 / 720.0);
}

struct ItpDebugArgs {
  ItpCoef k;
  const float* yuv;
  int n;
  float* out;
};

template <int TR>
__global__ __launch_bounds__(64) void delta_itp_debug_kernel(const ItpDebugArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const ItpCoef& k = a.k;
  float* out = a.out;
  const float* q = a.yuv + (int64_t)i * 3;
  const f2 Y{q[0], q[0]}, U{q[1] - k.u0, q[1] - k.u0}, V{q[2] - k.v0, q[2] - k.v0};   // both halves of the pair: the one triple
  const f2 R = fma2(Y, k.gy[0], fma2(U, k.cu[0], fma2(V, k.cv[0], f2{k.o[0], k.o[0]})));
  const f2 G = fma2(Y, k.gy[1], fma2(U, k.cu[1], fma2(V, k.cv[1], f2{k.o[1], k.o[1]})));
  const f2 B = fma2(Y, k.gy[2], fma2(U, k.cu[2], fma2(V, k.cv[2], f2{k.o[2], k.o[2]})));
  const Itp3 c = itp_of<TR>(R, G, B, k);
  out[(int64_t)i * 3 + 0] = c.i.x;
  out[(int64_t)i * 3 + 1] = c.t.x;
  out[(int64_t)i * 3 + 2] = c.p.x;
}

template <typename T, int TR>
hipError_t launch_itp_tt(hipStream_t stream, int hs, int vs, const dim3 grid, const ItpArgs& a) {
  const dim3 block(kBlock);
#define PQA_ITP_CASE(H, V) \
  if (hs == H && vs == V) { hipLaunchKernelGGL((delta_itp_kernel<T, H, V, TR>), grid, block, 0, stream, a); return hipGetLastError(); }
  PQA_ITP_CASE(1, 1) PQA_ITP_CASE(1, 0) PQA_ITP_CASE(0, 0)
  PQA_ITP_CASE(2, 2) PQA_ITP_CASE(2, 1) PQA_ITP_CASE(2, 0) PQA_ITP_CASE(1, 2) PQA_ITP_CASE(0, 1) PQA_ITP_CASE(0, 2)
#undef PQA_ITP_CASE
  return hipErrorInvalidValue;
}

template <typename T>
hipError_t launch_itp_t(hipStream_t stream, int hs, int vs, const dim3 grid, const ItpArgs& a) {
  switch (a.k.transfer) {
    case PQA_ITP_PQ: return launch_itp_tt<T, PQA_ITP_PQ>(stream, hs, vs, grid, a);
    case PQA_ITP_HLG: return launch_itp_tt<T, PQA_ITP_HLG>(stream, hs, vs, grid, a);
    case PQA_ITP_BT1886: return launch_itp_tt<T, PQA_ITP_BT1886>(stream, hs, vs, grid, a);
    default: return hipErrorInvalidValue;
  }
}

// one value for three that agree to within tol (the rounding of the coefficients they were summed from)
void unite(double v[3], double tol) {
  const double lo = fmin(v[0], fmin(v[1], v[2])), hi = fmax(v[0], fmax(v[1], v[2]));
  if (hi - lo <= tol) v[0] = v[1] = v[2] = v[1];
}

}  // namespace

int itp_tiles(int cw, int ch) { return ((cw + CTW - 1) / CTW) * ((ch + CTH - 1) / CTH); }

const char* itp_spec_error(const pqa_itp_spec& sp) {
  if (sp.transfer > PQA_ITP_BT1886) return "unknown transfer";
  for (float v : sp.yuv_to_rgb)
    if (!std::isfinite(v)) return "a coefficient of yuv_to_rgb is not finite";
  for (float v : sp.rgb_to_lms)
    if (!std::isfinite(v)) return "a coefficient of rgb_to_lms is not finite";
  if (sp.transfer != PQA_ITP_PQ && !(std::isfinite(sp.peak) && sp.peak > 0.0f)) return "peak must be positive and finite for HLG and BT.1886";
  if (!(std::isfinite(sp.threshold) && sp.threshold >= 0.0f)) return "threshold must be finite and not negative";
  return nullptr;
}

void itp_prepare(const pqa_itp_spec& sp, ItpCoef* k) {
  const double eps = 1.0 / (1 << 22);   // four f32 roundings
  const float* m = sp.yuv_to_rgb;
  // the neutral chroma point: where the three rows' chroma terms agree (rows R and B against row G)
  const double a00 = (double)m[1] - m[5], a01 = (double)m[2] - m[6], b0 = -((double)m[3] - m[7]);
  const double a10 = (double)m[9] - m[5], a11 = (double)m[10] - m[6], b1 = -((double)m[11] - m[7]);
  const double det = a00 * a11 - a01 * a10;
  double u0 = 0.0, v0 = 0.0;
  if (fabs(det) > 1e-12 * (fabs(a00 * a11) + fabs(a01 * a10)) && det != 0.0) {
    u0 = (b0 * a11 - a01 * b1) / det;
    v0 = (a00 * b1 - b0 * a10) / det;
    if (fabs(u0 - rint(u0)) < 1e-3) u0 = rint(u0);   // samples are whole numbers: Cb - u0 is then exact
    if (fabs(v0 - rint(v0)) < 1e-3) v0 = rint(v0);
    if (!(fabs(u0) < 65536.0 && fabs(v0) < 65536.0)) u0 = v0 = 0.0;
  }
  double gy[3], o[3], otol = 0.0;
  for (int r = 0; r < 3; ++r) {
    gy[r] = m[4 * r];
    o[r] = (double)m[4 * r + 3] + (double)m[4 * r + 1] * u0 + (double)m[4 * r + 2] * v0;
    otol = fmax(otol, fabs((double)m[4 * r + 3]) + fabs((double)m[4 * r + 1] * u0) + fabs((double)m[4 * r + 2] * v0));
  }
  unite(gy, eps * fabs(gy[1]));
  unite(o, eps * otol);
  const float* q = sp.rgb_to_lms;
  double ls[3], ltol = 0.0;
  for (int r = 0; r < 3; ++r) {
    ls[r] = (double)q[3 * r] + q[3 * r + 1] + q[3 * r + 2];
    ltol = fmax(ltol, fabs((double)q[3 * r]) + fabs((double)q[3 * r + 1]) + fabs((double)q[3 * r + 2]));
  }
  unite(ls, eps * ltol);
  k->transfer = (int)sp.transfer;
  k->u0 = (float)u0; k->v0 = (float)v0;
  for (int r = 0; r < 3; ++r) {
    k->gy[r] = (float)gy[r]; k->cu[r] = m[4 * r + 1]; k->cv[r] = m[4 * r + 2]; k->o[r] = (float)o[r];
    k->ls[r] = (float)ls[r]; k->lr[r] = q[3 * r]; k->lb[r] = q[3 * r + 2];
  }
  k->peak = sp.peak;
  k->gamma_m1 = sp.transfer == PQA_ITP_HLG ? (float)(0.2 + 0.42 * log10((double)sp.peak / 1000.0)) : 0.0f;
  k->threshold = sp.threshold;
}

hipError_t launch_delta_itp(hipStream_t stream, Elem elem, const ItpCoef& coef, const PlaneRun ref[3], const PlaneRun dis[3],
                            int n_frames, int w, int h, int hshift, int vshift, double* partials) {
  if (n_frames <= 0) return hipSuccess;
  if (hshift < 0 || hshift > 2 || vshift < 0 || vshift > 2) return hipErrorInvalidValue;
  ItpArgs a{};
  for (int p = 0; p < 3; ++p) {
    if (ref[p].row_pitch >= (1ll << 31) || dis[p].row_pitch >= (1ll << 31)) return hipErrorInvalidValue;
    a.ref[p] = ref[p].base; a.dis[p] = dis[p].base;
    a.rp_r[p] = (int)ref[p].row_pitch; a.fp_r[p] = ref[p].frame_pitch;
    a.rp_d[p] = (int)dis[p].row_pitch; a.fp_d[p] = dis[p].frame_pitch;
  }
  a.w = w; a.h = h;
  a.cw = (w + (1 << hshift) - 1) >> hshift;
  a.ch = (h + (1 << vshift) - 1) >> vshift;
  a.tiles_x = (a.cw + CTW - 1) / CTW;
  a.n_tiles = itp_tiles(a.cw, a.ch);
  a.k = coef;
  a.partials = partials;
  const dim3 grid(a.n_tiles, n_frames);
  switch (elem) {
    case ELEM_U8: return launch_itp_t<uint8_t>(stream, hshift, vshift, grid, a);
    case ELEM_U16: return launch_itp_t<uint16_t>(stream, hshift, vshift, grid, a);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_delta_itp_finalize(hipStream_t stream, const double* partials, int n_tiles, int n_frames, double* out) {
  if (n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(delta_itp_finalize_kernel, dim3(n_frames), dim3(kBlock), 0, stream, partials, n_tiles, out);
  return hipGetLastError();
}

hipError_t launch_delta_itp_debug(hipStream_t stream, const ItpCoef& coef, const float* yuv, int n, float* itp_out) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((n + 63) / 64), block(64);
  const ItpDebugArgs a{coef, yuv, n, itp_out};
  switch (coef.transfer) {
    case PQA_ITP_PQ: hipLaunchKernelGGL((delta_itp_debug_kernel<PQA_ITP_PQ>), grid, block, 0, stream, a); break;
    case PQA_ITP_HLG: hipLaunchKernelGGL((delta_itp_debug_kernel<PQA_ITP_HLG>), grid, block, 0, stream, a); break;
    case PQA_ITP_BT1886: hipLaunchKernelGGL((delta_itp_debug_kernel<PQA_ITP_BT1886>), grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pqa
