// libvmaf's ciede feature (log key ciede2000): per luma pixel YUV -> R'G'B' (BT.709 analog matrix) -> linear sRGB -> XYZ
// (D65) -> CIELAB for the reference and the distorted frame, the CIEDE2000 difference of the pair, the frame mean and
// 45 - 20 log10(mean).  The definition, its constants and its unpinned items: tests/ciede_ref.py and DESIGN.md section 1.
//
// Two kernels:
//   ciede_kernel<T, HS, VS>  one thread per chroma sample: the chroma part of the colour conversion once, then the
//                            (1 << HS) x (1 << VS) luma pixels it covers (chroma upsampled by replication).  A workgroup
//                            owns 64 x 4 chroma samples (a wave one chroma row); per-thread and per-wave sums in f32, the
//                            tile sum in double, one partial per tile.  f32 throughout the per-pixel path, no f64, no scratch.
//                            (No loop over chroma rows: inside a loop the compiler parks the ~50 constants of the colour
//                            conversion in SGPRs and spills them; the shift-2 pixel loops stay rolled for the same reason.)
//   ciede_finalize_kernel    fixed-order sum of a frame's tile partials, mean and score in double, into slots 20 / 21 of
//                            the frame's extension record (and nothing else of the row).
// No atomics: a frame's value does not depend on batch, launch, pitch or alignment.
//
// Approximations and their errors (the combined effect, measured on the MI355X against the f64
// restatement: <= 3.4e-6 * (1 + dE) on 1e5 random Lab pairs, <= 1.6e-7 relative on frame means; DESIGN.md sections 1 and 5):
//   v_log_f32 / v_exp_f32 (hardware log2 / exp2, what the compiler itself emits for f32 log2 / exp2 of normal inputs, a
//     few ulp): x^2.4 = exp2(2.4 log2 x) and cbrt x = exp2(log2 x / 3) -- a few 1e-7 relative (the error of log2 x, up to
//     |log2 x| ~ 7 here, times the exponent).
//   v_sqrt_f32 / v_rsq_f32 / v_rcp_f32: about 1 ulp.
//   atan2: a degree-8 minimax polynomial of atan(t) / t in t^2 on [0, 1] after octant reduction, relative error 4.4e-8
//     (f32 coefficients), returned in turns.
//   v_sin_f32 / v_cos_f32 take turns (no range reduction needed: the mean hue is in [0, 1) turn, 2 d_theta in [0, 1/6]);
//     one sincos of the mean hue gives all four cosines of T through multiple-angle identities (cos 2h, cos 3h, cos 4h and
//     the matching sines).  T and R_T only scale S_H and the rotation term, so their absolute errors of order 1e-6 move
//     dE by about 1e-6 relative at most.
//   Hue: the hue DIFFERENCE is atan2(a1' b2 - b1 a2', a1' a2' + b1 b2) (the angle between the two chroma vectors), not the
//     difference of two hue angles, and dH' = 2 sqrt(C1' C2') sin(dh'/2) is formed without trigonometry:
//     sqrt(2) * cross / sqrt(P + dot) for dot >= 0, sign(cross) * sqrt(2 (P - dot)) otherwise (P = C1' C2').  Neither
//     cancels for small or for near-180-degree differences.  The mean hue is h1' + dh'/2 wrapped into [0, 1) turn, which
//     equals Sharma's rule (eq. 14) wherever |h1' - h2'| != 180 degrees.  At 180 degrees the rule jumps (Sharma pairs 9 / 10:
//     7.1792 vs 7.2195); here the side is decided by the sign of the rounded cross product (products rounded separately,
//     no FMA), i.e. pairs within ~1e-5 degrees of the jump may land on either side.  Identical colours give cross = 0,
//     dot > 0 and an exact 0.
#include <cmath>

#include "../../include/pqa_vmaf.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int CTW = kCiedeTileW, CTH = kCiedeTileH;   // chroma samples per workgroup tile (64 x 4)
static_assert(CTW * CTH == kBlock, "one chroma sample per thread");

// ---- the colour conversion (constants: tests/ciede_ref.py CONST) ----------------------------------------------------
constexpr double kRv = 1.28033, kGu = -0.21482, kGv = -0.38059, kBu = 2.12798;
constexpr float kSrgbThr = 0.04045f;
constexpr float kSrgbA = (float)(1.0 / 1.055), kSrgbB = (float)(0.055 / 1.055), kSrgbLin = (float)(1.0 / 12.92);
// linear sRGB (0..1) -> XYZ / white: the 4-digit D65 matrix, x 100, divided by the white point row by row
constexpr double kWx = 95.047, kWy = 100.0, kWz = 108.883;
constexpr float kM[3][3] = {{(float)(41.24 / kWx), (float)(35.76 / kWx), (float)(18.05 / kWx)},
                            {(float)(21.26 / kWy), (float)(71.52 / kWy), (float)(7.22 / kWy)},
                            {(float)(1.93 / kWz), (float)(11.92 / kWz), (float)(95.05 / kWz)}};
constexpr float kLabEps = 0.008856f, kLabK = 7.787f, kLabC = (float)(16.0 / 116.0);

__device__ __forceinline__ float hw_log2(float x) { return __builtin_amdgcn_logf(x); }   // v_log_f32
__device__ __forceinline__ float hw_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32
__device__ __forceinline__ float hw_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }  // v_sqrt_f32
__device__ __forceinline__ float hw_rsq(float x) { return __builtin_amdgcn_rsqf(x); }    // v_rsq_f32
__device__ __forceinline__ float hw_rcp(float x) { return __builtin_amdgcn_rcpf(x); }    // v_rcp_f32
__device__ __forceinline__ float hw_sin(float t) { return __builtin_amdgcn_sinf(t); }    // sin(2 pi t)
__device__ __forceinline__ float hw_cos(float t) { return __builtin_amdgcn_cosf(t); }    // cos(2 pi t)

// sRGB transfer of a {ref, dis} pair (the x 100 is in kM): the power branch on the hardware log2 / exp2, negative and small
// values take the linear branch
__device__ __forceinline__ f2 srgb_linear(f2 c) {
  const f2 t = c * f2{kSrgbA, kSrgbA} + f2{kSrgbB, kSrgbB};
  const f2 l = c * f2{kSrgbLin, kSrgbLin};
  const float p0 = hw_exp2(2.4f * hw_log2(t.x)), p1 = hw_exp2(2.4f * hw_log2(t.y));
  return f2{c.x > kSrgbThr ? p0 : l.x, c.y > kSrgbThr ? p1 : l.y};
}

// CIELAB f(t) of a pair: cube root above eps (hardware log2 / exp2), the linear segment below it (negative t included)
__device__ __forceinline__ f2 lab_f(f2 t) {
  const f2 l = t * f2{kLabK, kLabK} + f2{kLabC, kLabC};
  const float c0 = hw_exp2(hw_log2(t.x) * (1.0f / 3.0f)), c1 = hw_exp2(hw_log2(t.y) * (1.0f / 3.0f));
  return f2{t.x > kLabEps ? c0 : l.x, t.y > kLabEps ? c1 : l.y};
}

// ---- CIEDE2000 ----------------------------------------------------------------------------------------------------
// atan2(y, x) in turns, (-0.5, 0.5]; atan2(+-0, 0) = +-0.  Octant reduction, then atan(a) = a * P(a^2) on [0, 1]: P is the
// degree-8 minimax polynomial of atan(a) / a in a^2 (relative error 4.4e-8 with these f32 coefficients), pre-scaled by 1/(2 pi).
__device__ __forceinline__ float atan2_turns(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  const float a = mx > 0.0f ? mn * hw_rcp(mx) : 0.0f;
  const float s = a * a;
  constexpr double k = 0.15915494309189535;   // 1 / (2 pi)
  float p = (float)(0.002849890384823084 * k);
  p = fmaf(p, s, (float)(-0.016068635508418083 * k));
  p = fmaf(p, s, (float)(0.04269153252243996 * k));
  p = fmaf(p, s, (float)(-0.0750429630279541 * k));
  p = fmaf(p, s, (float)(0.10640934854745865 * k));
  p = fmaf(p, s, (float)(-0.14203645288944244 * k));
  p = fmaf(p, s, (float)(0.1999261975288391 * k));
  p = fmaf(p, s, (float)(-0.3333307206630707 * k));
  p = fmaf(p, s, (float)(1.0 * k));
  float r = p * a;
  r = ay > ax ? 0.25f - r : r;
  r = x < 0.0f ? 0.5f - r : r;
  return copysignf(r, y);
}

// x^7 / (x^7 + 25^7) for x >= 0
__device__ __forceinline__ float c7_ratio(float x) {
  const float x2 = x * x, x7 = x2 * x2 * x2 * x;
  return x7 * hw_rcp(x7 + 6103515625.0f);
}

// CIEDE2000 (kL = kC = kH = 1) of (L1, a1, b1) and (L2, a2, b2); the kernel's and pqa_debug_ciede2000's one definition.
__device__ __forceinline__ float de00(float L1, float a1, float b1, float L2, float a2, float b2) {
  const float C1 = hw_sqrt(a1 * a1 + b1 * b1), C2 = hw_sqrt(a2 * a2 + b2 * b2);
  const float g1 = 1.0f + 0.5f * (1.0f - hw_sqrt(c7_ratio(0.5f * (C1 + C2))));   // 1 + G
  const float a1p = g1 * a1, a2p = g1 * a2;
  const float C1p = hw_sqrt(a1p * a1p + b1 * b1), C2p = hw_sqrt(a2p * a2p + b2 * b2);
  const bool z1 = a1 == 0.0f && b1 == 0.0f, z2 = a2 == 0.0f && b2 == 0.0f;
  // angle between the chroma vectors; both products rounded (no contraction into an FMA), so identical colours give
  // cross = 0 exactly
  float cross, dot;
  {
#pragma clang fp contract(off)
    cross = a1p * b2 - b1 * a2p;
    dot = a1p * a2p + b1 * b2;
  }
  const float P = C1p * C2p;
  const float dh = (z1 || z2) ? 0.0f : atan2_turns(cross, dot);
  // dH' = 2 sqrt(P) sin(dh / 2), from cross and dot: q = P + |dot|
  const float q = P + fabsf(dot);
  const float rq = hw_rsq(q);
  const float dH = (z1 || z2) ? 0.0f : (dot >= 0.0f ? 1.41421356f * cross * rq : copysignf(1.41421356f * q * rq, cross));
  // mean hue: h1' + dh' / 2 (Sharma eq. 14), or the one defined hue when a chroma is zero (h' = 0 there: h1' + h2')
  float hb = z1 ? atan2_turns(b2, a2p) : atan2_turns(b1, a1p);
  hb = hb < 0.0f ? hb + 1.0f : hb;
  hb += 0.5f * dh;
  hb = hb < 0.0f ? hb + 1.0f : (hb >= 1.0f ? hb - 1.0f : hb);
  // T from one sincos: cos(h - 30), cos 2h, cos(3h + 6), cos(4h - 63)
  const float sh = hw_sin(hb), ch = hw_cos(hb);
  const float c2 = ch * ch - sh * sh, s2 = 2.0f * sh * ch;
  const float c3 = ch * (4.0f * ch * ch - 3.0f), s3 = sh * (3.0f - 4.0f * sh * sh);
  const float c4 = c2 * c2 - s2 * s2, s4 = 2.0f * s2 * c2;
  constexpr double d2r = 3.14159265358979323846 / 180.0;
  const float T = 1.0f - 0.17f * ((float)cos(30 * d2r) * ch + (float)sin(30 * d2r) * sh) + 0.24f * c2 +
                  0.32f * ((float)cos(6 * d2r) * c3 - (float)sin(6 * d2r) * s3) -
                  0.20f * ((float)cos(63 * d2r) * c4 + (float)sin(63 * d2r) * s4);
  // rotation: d_theta = 30 exp(-((h - 275) / 25)^2) degrees, R_T = -sin(2 d_theta) R_C
  const float e = fmaf(hb, 14.4f, -11.0f);   // (360 h - 275) / 25
  const float dtheta_turns = hw_exp2(-1.44269504f * e * e) * (1.0f / 6.0f);   // 2 d_theta / 360
  const float Cbp = 0.5f * (C1p + C2p);
  const float RT = -2.0f * hw_sqrt(c7_ratio(Cbp)) * hw_sin(dtheta_turns);
  const float Lb = 0.5f * (L1 + L2) - 50.0f, l50 = Lb * Lb;
  const float SL = 1.0f + 0.015f * l50 * hw_rsq(20.0f + l50);
  const float SC = 1.0f + 0.045f * Cbp;
  const float SH = 1.0f + 0.015f * Cbp * T;
  const float r = hw_rcp(SL * SC * SH);
  const float tl = (L2 - L1) * (SC * SH) * r, tc = (C2p - C1p) * (SL * SH) * r, th = dH * (SL * SC) * r;
  return hw_sqrt(fmaxf(0.0f, tl * tl + tc * tc + th * th + RT * tc * th));
}

// ---- the frame kernel -------------------------------------------------------------------------------------------
struct CiedeArgs {
  const void* ref[3];
  const void* dis[3];
  int64_t fp_r[3], fp_d[3];                     // frame pitches, elements
  int rp_r[3], rp_d[3];                         // row pitches, elements (< 2^31: checked by the launcher)
  int w, h, cw, ch;                             // luma and chroma plane sizes
  float inv;                                    // 1 / (255 * 2^(bpc - 8))
  int tiles_x, n_tiles;
  double* partials;                             // [n_frames][n_tiles]
};

template <typename T> __device__ __forceinline__ f2 ld_pair(const T* r, const T* d, int x, float inv) {
  return f2{(float)r[x], (float)d[x]} * f2{inv, inv};
}

template <typename T, int HS, int VS>
__global__ __launch_bounds__(kBlock) void ciede_kernel(const CiedeArgs a) {
  __shared__ double red[4];
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
  const f2 half{0.5f, 0.5f};
  float acc = 0.0f;
  if (cx < a.cw && cy < a.ch) {
    // chroma part of Y'UV -> R'G'B', once per chroma sample
    const f2 U = ld_pair(ru + (int64_t)cy * a.rp_r[1], du + (int64_t)cy * a.rp_d[1], cx, a.inv) - half;
    const f2 V = ld_pair(rv + (int64_t)cy * a.rp_r[2], dv + (int64_t)cy * a.rp_d[2], cx, a.inv) - half;
    const f2 cr = V * (float)kRv;
    const f2 cg = U * (float)kGu + V * (float)kGv;
    const f2 cb = U * (float)kBu;
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
        const f2 Y = ld_pair(rrow, drow, x, a.inv);
        const f2 R = srgb_linear(Y + cr), G = srgb_linear(Y + cg), B = srgb_linear(Y + cb);
        const f2 fx = lab_f(R * kM[0][0] + G * kM[0][1] + B * kM[0][2]);
        const f2 fy = lab_f(R * kM[1][0] + G * kM[1][1] + B * kM[1][2]);
        const f2 fz = lab_f(R * kM[2][0] + G * kM[2][1] + B * kM[2][2]);
        const f2 L = fy * 116.0f - 16.0f, A = (fx - fy) * 500.0f, Bb = (fy - fz) * 200.0f;
        acc += de00(L.x, A.x, Bb.x, L.y, A.y, Bb.y);
      }
    }
  }
  const float in[1] = {acc};
  double out[1];
  block_sum_f32<1>(in, out, red);
  if (threadIdx.x == 0) a.partials[(int64_t)fr * a.n_tiles + tile] = out[0];
}

__global__ __launch_bounds__(kBlock) void ciede_finalize_kernel(const CiedeFinalizeArgs a) {
  __shared__ double red[4];
  const int fr = blockIdx.x;
  double acc[1] = {0.0};
  const double* p = a.partials + (int64_t)fr * a.n_tiles;
  for (int i = threadIdx.x; i < a.n_tiles; i += kBlock) acc[0] += p[i];
  block_sum<1>(acc, red);
  if (threadIdx.x != 0) return;
  const int row = (int)(((int64_t)a.slot_base + (int64_t)fr * a.slot_step) % a.capacity);
  double* e = a.ext + (int64_t)row * a.ext_stride;
  const double mean = acc[0] * a.norm;
  e[PQA_EXT_CIEDE_MEAN_DE] = mean;
  e[PQA_EXT_CIEDE2000] = mean > 0.0 ? 45.0 - 20.0 * log10(mean) : __builtin_inf();
}

__global__ __launch_bounds__(64) void ciede_debug_kernel(const float* lab, int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* q = lab + (int64_t)i * 6;
  out[i] = de00(q[0], q[1], q[2], q[3], q[4], q[5]);
}

template <typename T>
hipError_t launch_ciede_t(hipStream_t stream, int hs, int vs, const dim3 grid, const CiedeArgs& a) {
  const dim3 block(kBlock);
#define PQA_CIEDE_CASE(H, V) \
  if (hs == H && vs == V) { hipLaunchKernelGGL((ciede_kernel<T, H, V>), grid, block, 0, stream, a); return hipGetLastError(); }
  PQA_CIEDE_CASE(1, 1) PQA_CIEDE_CASE(1, 0) PQA_CIEDE_CASE(0, 0)
  PQA_CIEDE_CASE(2, 2) PQA_CIEDE_CASE(2, 1) PQA_CIEDE_CASE(2, 0) PQA_CIEDE_CASE(1, 2) PQA_CIEDE_CASE(0, 1) PQA_CIEDE_CASE(0, 2)
#undef PQA_CIEDE_CASE
  return hipErrorInvalidValue;
}

}  // namespace

int ciede_tiles(int cw, int ch) { return ((cw + CTW - 1) / CTW) * ((ch + CTH - 1) / CTH); }

hipError_t launch_ciede(hipStream_t stream, Elem elem, const PlaneRun ref[3], const PlaneRun dis[3], int n_frames, int w,
                        int h, int hshift, int vshift, int bit_depth, double* partials) {
  if (n_frames <= 0) return hipSuccess;
  if (hshift < 0 || hshift > 2 || vshift < 0 || vshift > 2 || bit_depth < 8 || bit_depth > 16) return hipErrorInvalidValue;
  CiedeArgs a{};
  for (int p = 0; p < 3; ++p) {
    if (ref[p].row_pitch >= (1ll << 31) || dis[p].row_pitch >= (1ll << 31)) return hipErrorInvalidValue;
    a.ref[p] = ref[p].base; a.dis[p] = dis[p].base;
    a.rp_r[p] = (int)ref[p].row_pitch; a.fp_r[p] = ref[p].frame_pitch;
    a.rp_d[p] = (int)dis[p].row_pitch; a.fp_d[p] = dis[p].frame_pitch;
  }
  a.w = w; a.h = h;
  a.cw = (w + (1 << hshift) - 1) >> hshift;
  a.ch = (h + (1 << vshift) - 1) >> vshift;
  a.inv = (float)(1.0 / (255.0 * (double)(1 << (bit_depth - 8))));
  a.tiles_x = (a.cw + CTW - 1) / CTW;
  a.n_tiles = ciede_tiles(a.cw, a.ch);
  a.partials = partials;
  const dim3 grid(a.n_tiles, n_frames);
  switch (elem) {
    case ELEM_U8: return launch_ciede_t<uint8_t>(stream, hshift, vshift, grid, a);
    case ELEM_U16: return launch_ciede_t<uint16_t>(stream, hshift, vshift, grid, a);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_ciede_finalize(hipStream_t stream, const CiedeFinalizeArgs& args) {
  if (args.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(ciede_finalize_kernel, dim3(args.n_frames), dim3(kBlock), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_ciede_debug(hipStream_t stream, const float* lab_pairs, int n, float* de_out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ciede_debug_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, lab_pairs, n, de_out);
  return hipGetLastError();
}

}  // namespace pqa
