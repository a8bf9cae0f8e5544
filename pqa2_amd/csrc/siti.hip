// ITU-T P.910 Spatial and Temporal Information as FFmpeg's siti filter computes them (libavfilter/vf_siti.c), on the luma
// of both clips.  The definition, its constants and its unpinned items: tests/siti_ref.py and DESIGN.md section 1.
//
// Two kernels:
//   siti_kernel<T>        one wave per (stripe of kSitiCols columns, segment of kSitiSegRows rows, frame, clip), marching
//                         DOWN its stripe one row at a time (the motion_march.hip scheme, one column per lane):
//                           lane <-> column 62 * stripe - 1 + lane; lanes 0 and 63 only feed their neighbours' taps;
//                           each sample is mapped to full range once, in exact integer arithmetic (a full-range clip: as
//                           it is);
//                           the 3-row Sobel window stays in registers as the column sums s = a + 2b + c and d = a - c,
//                           horizontal neighbours come from the lanes beside: gx = s(x-1) - s(x+1), gy = d(x-1) + 2d + d(x+1);
//                           g = sqrtf(rne_f32(gx^2 + gy^2)) (exact integer sum, correctly rounded square root);
//                           m = y'_t - y'_{t-1} exact; sum m and sum m^2 per lane in int32 (a segment bounds them);
//                           sum g and sum g^2 per lane in double.
//                         Each wave writes {sum g, sum g^2, sum m, sum m^2} (doubles; the m sums are exact integers).
//   siti_finalize_kernel  one workgroup per (frame, clip): the wave partials in a fixed order, SI from the one-pass
//                         moments, TI exactly from the integer sums; into the frame's ext4 row.
// No atomics: a frame's values do not depend on batch, launch, pitch or alignment.
#include <cmath>

#include "../../include/pqa_vmaf.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int kSitiCols = 62;   // output columns per wave (lanes 1..62)

struct SitiArgs {
  const void* cur[2];          // clip 0: distorted, clip 1: reference (frame 0 of the run)
  unsigned pitch[2];           // elements
  int64_t frame_pitch[2];      // elements
  const void* prev0[2];        // frame -1 of each clip (nullptr: a chain start, m = 0 on frame 0)
  unsigned prev0_pitch[2];     // elements
  int full[2];                 // the clip's samples are full range
  int w, h, n_stripes, n_sg, n_seg, n_part;
  double* partials;            // [n_frames][2][n_part][4]
  float* gmap;                 // test hook: the (w - 2) x (h - 2) gradient map of frame 0, clip 0 (nullable)
};

// Horizontal neighbours through ds_bpermute (__shfl_up / __shfl_down): with DPP wave shifts folded into the subtraction
// (v_subrev_u32_dpp wave_shl) the MI355X returned gx = 0 on every pixel, so the shifts stay plain cross-lane reads.
__device__ __forceinline__ int from_left(int v) { return __shfl_up(v, 1, 64); }     // lane l <- l - 1
__device__ __forceinline__ int from_right(int v) { return __shfl_down(v, 1, 64); }  // lane l <- l + 1

// limited -> full range: ((256 f - 1) * clamp(y - 16 f, 0, 219 f)) / (219 f), f = 1 (8 bit) or 4 (10 bit), truncating
template <typename T, bool FULL>
__device__ __forceinline__ int to_full(unsigned v) {
  if constexpr (FULL) {
    return (int)v;
  } else {
    constexpr int f = sizeof(T) == 1 ? 1 : 4;
    const int c = min(max((int)v - 16 * f, 0), 219 * f);
    return (int)((unsigned)((256 * f - 1) * c) / (unsigned)(219 * f));
  }
}

template <typename T, bool FULL>
__device__ __forceinline__ void march(const SitiArgs& a, rsrc_t rc, unsigned pc, rsrc_t rp, unsigned pp, int x, int r0, int r1,
                                      bool own, bool own_g, float* gmap, double (&out)[4]) {
  const int h = a.h;
  const unsigned col = (unsigned)min(max(x, 0), a.w - 1);
  int ra = to_full<T, FULL>(buf_load<T>(rc, col, (unsigned)max(r0 - 1, 0) * pc));
  int rb = to_full<T, FULL>(buf_load<T>(rc, col, (unsigned)r0 * pc));
  int sm = 0, sm2 = 0;        // a segment of kSitiSegRows rows: sum m^2 <= 128 * 1023^2 < 2^31
  double sg = 0.0, sg2 = 0.0;
  for (int y = r0; y < r1; ++y) {
    const int rn = to_full<T, FULL>(buf_load<T>(rc, col, (unsigned)min(y + 1, h - 1) * pc));
    const int q = to_full<T, FULL>(buf_load<T>(rp, col, (unsigned)y * pp));
    const int m = own ? rb - q : 0;
    sm += m;
    sm2 += m * m;
    const int s = ra + 2 * rb + rn, d = ra - rn;
    const int gx = from_left(s) - from_right(s);
    const int gy = from_left(d) + 2 * d + from_right(d);
    const float g = sqrtf((float)(gx * gx + gy * gy));   // the sum is exact (< 2^26); one rounding to f32, then the root
    const bool vg = own_g && y >= 1 && y <= h - 2;
    const double gd = vg ? (double)g : 0.0;
    sg += gd;
    sg2 = fma(gd, gd, sg2);
    if (gmap && vg) gmap[(int64_t)(y - 1) * (a.w - 2) + (x - 1)] = g;
    ra = rb;
    rb = rn;
  }
  out[0] = sg;
  out[1] = sg2;
  out[2] = (double)sm;
  out[3] = (double)sm2;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void siti_kernel(const SitiArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int id = xcd_remap(blockIdx.x, a.n_sg * a.n_seg);
  const int sg = id % a.n_sg, seg = id / a.n_sg;
  const int stripe = sg * 4 + wave;
  const int fr = blockIdx.y, z = blockIdx.z;
  double* __restrict__ part = a.partials + (((int64_t)fr * 2 + z) * a.n_part + (int64_t)id * 4 + wave) * 4;
  if (stripe >= a.n_stripes) {   // idle wave of the last group
    if (lane < 4) part[lane] = 0.0;
    return;
  }
  const T* cur = (const T*)a.cur[z] + (int64_t)fr * a.frame_pitch[z];
  const T* prev = fr > 0 ? cur - a.frame_pitch[z] : (const T*)a.prev0[z];
  unsigned pp = fr > 0 ? a.pitch[z] : a.prev0_pitch[z];
  if (!prev) { prev = cur; pp = a.pitch[z]; }   // a chain start: m = 0
  const rsrc_t rc = make_rsrc(cur, (unsigned)a.h * a.pitch[z] * (unsigned)sizeof(T));
  const rsrc_t rp = make_rsrc(prev, (unsigned)a.h * pp * (unsigned)sizeof(T));
  const int r0 = seg * kSitiSegRows, r1 = min(r0 + kSitiSegRows, a.h);
  const int x = stripe * kSitiCols - 1 + lane;
  const bool own = lane >= 1 && lane <= kSitiCols && x < a.w;
  const bool own_g = own && x >= 1 && x <= a.w - 2;
  float* gmap = (fr == 0 && z == 0) ? a.gmap : nullptr;
  double v[4];
  if (a.full[z]) march<T, true>(a, rc, a.pitch[z], rp, pp, x, r0, r1, own, own_g, gmap, v);
  else march<T, false>(a, rc, a.pitch[z], rp, pp, x, r0, r1, own, own_g, gmap, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) part[k] = v[k];
  }
}

struct SitiFinalizeArgs {
  const double* partials;
  int n_part;
  double n_grad, n_pix;        // (w - 2)(h - 2) and w h
  long long n_pix_i;
  double* ext4;
  int ext_stride, slot_base, capacity;
};

__global__ __launch_bounds__(kBlock) void siti_finalize_kernel(const SitiFinalizeArgs a) {
  __shared__ double lds[4 * 4];
  const int fr = blockIdx.x, z = blockIdx.y;
  const double* p = a.partials + ((int64_t)fr * 2 + z) * a.n_part * 4;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < a.n_part; i += kBlock) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += p[(int64_t)i * 4 + k];
  }
  block_sum<4>(v, lds);
  if (threadIdx.x != 0) return;
  const double mean = v[0] / a.n_grad;
  const double var_g = v[1] / a.n_grad - mean * mean;
  const double si = var_g > 0.0 ? sqrt(var_g) : 0.0;
  // TI exactly: (N sum m^2 - (sum m)^2) / N^2 from the integer sums (every partial and sum is an exact integer < 2^53)
  const long long s1 = (long long)v[2], s2 = (long long)v[3];
  const __int128 num = (__int128)a.n_pix_i * s2 - (__int128)s1 * s1;
  const double ti = sqrt((double)num / (a.n_pix * a.n_pix));
  double* row = a.ext4 + (int64_t)((a.slot_base + fr) % a.capacity) * a.ext_stride;
  row[2 * z] = si;
  row[2 * z + 1] = ti;
}

}  // namespace

int siti_partials(int w, int h) {
  const int n_stripes = (w + kSitiCols - 1) / kSitiCols;
  return ((n_stripes + 3) / 4) * 4 * ((h + kSitiSegRows - 1) / kSitiSegRows);
}

hipError_t launch_siti(hipStream_t stream, Elem elem, const PlaneRun clip[2], const void* const prev0[2],
                       const int64_t prev0_pitch[2], const bool full[2], int n_clips, int n_frames, int w, int h,
                       double* partials, double* ext4, int ext_stride, int slot_base, int capacity, float* gmap) {
  if (elem != ELEM_U8 && elem != ELEM_U16) return hipErrorInvalidValue;
  if (n_frames <= 0) return hipSuccess;
  const int es = elem == ELEM_U16 ? 2 : 1;
  SitiArgs a{};
  for (int z = 0; z < n_clips; ++z) {
    // buffer offsets are 32-bit: one plane (and its predecessor) must span less than 2 GiB
    if ((int64_t)clip[z].row_pitch * h * es >= (1ll << 31) || (int64_t)prev0_pitch[z] * h * es >= (1ll << 31))
      return hipErrorInvalidValue;
    a.cur[z] = clip[z].base;
    a.pitch[z] = (unsigned)clip[z].row_pitch;
    a.frame_pitch[z] = clip[z].frame_pitch;
    a.prev0[z] = prev0[z];
    a.prev0_pitch[z] = (unsigned)prev0_pitch[z];
    a.full[z] = full[z] ? 1 : 0;
  }
  a.w = w; a.h = h;
  a.n_stripes = (w + kSitiCols - 1) / kSitiCols;
  a.n_sg = (a.n_stripes + 3) / 4;
  a.n_seg = (h + kSitiSegRows - 1) / kSitiSegRows;
  a.n_part = a.n_sg * 4 * a.n_seg;
  a.partials = partials;
  a.gmap = gmap;
  const dim3 grid(a.n_sg * a.n_seg, n_frames, n_clips), block(kBlock);
  if (elem == ELEM_U16) hipLaunchKernelGGL((siti_kernel<uint16_t>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((siti_kernel<uint8_t>), grid, block, 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  SitiFinalizeArgs f{};
  f.partials = partials;
  f.n_part = a.n_part;
  f.n_grad = (double)(w - 2) * (double)(h - 2);
  f.n_pix = (double)w * (double)h;
  f.n_pix_i = (long long)w * h;
  f.ext4 = ext4;
  f.ext_stride = ext_stride;
  f.slot_base = slot_base;
  f.capacity = capacity;
  hipLaunchKernelGGL(siti_finalize_kernel, dim3(n_frames, n_clips), dim3(kBlock), 0, stream, f);
  return hipGetLastError();
}

}  // namespace pqa
