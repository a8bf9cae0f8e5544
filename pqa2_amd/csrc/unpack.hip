// Packed capture formats -> the planes the feature kernels read.
//
// A capture card delivers packed 4:2:2 (include/pqa_vmaf.h has the normative layouts):
//   UYVY (8 bit)   macropixel k of a row = the bytes U_k, Y_2k, V_k, Y_2k+1
//   YUYV (8 bit)   the same with the bytes Y_2k, U_k, Y_2k+1, V_k
//   v210 (10 bit)  groups of 6 pixels in four little-endian words of three 10-bit components (bits 0-9, 10-19, 20-29; bits
//                  30-31 undefined):  w0 = U0 Y0 V0,  w1 = Y1 U1 Y2,  w2 = V1 Y3 U2,  w3 = Y4 V2 Y5
// The unpacked planes are the same integers a planar file of the clip holds, so every record downstream is bit-identical.
// Pure byte work, HBM-bound, like ingest.hip: no LDS, no atomics; every packed byte is read once and every output byte
// written once.  A lane takes one span of a row: 32 source bytes (16 pixels) of UYVY / YUYV, which become 16 / 8 / 8 bytes of
// Y / U / V; 64 source bytes (4 groups, 24 pixels) of v210, which become 48 / 24 / 24 bytes -- so a lane's Y store starts 16
// bytes aligned and its U and V stores 8.  PLANES = 1 decodes and stores luma only.
#include "host_packed.h"
#include "ingest.h"
#include "pqa_device.h"

namespace pqa {
namespace {

struct UnpackArgs {
  const uint8_t* src;
  int64_t src_row_pitch, src_frame_pitch;   // bytes
  uint8_t* dst[3];                          // Y, U, V (U, V unused with PLANES = 1)
  int64_t dst_row_pitch[3], dst_frame_pitch[3];
  int w, h, cw;                             // luma samples per row, rows, chroma samples per row = ceil(w / 2)
};

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

constexpr int kLanesX = 64, kRowsPerBlock = 4;   // a workgroup: one wave's width of spans, four rows

template <int FORMAT>
struct Span {   // what one lane takes
  static constexpr int pixels = FORMAT == UNPACK_V210 ? 24 : 16;
  static constexpr int src_bytes = FORMAT == UNPACK_V210 ? 64 : 32;
};

// v_perm_b32: result byte i = byte sel_i of {hi : lo} (0-3 lo, 4-7 hi)
__device__ __forceinline__ unsigned perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
// the 10-bit component at bit `at` of a v210 word (v_bfe_u32); bits 30-31 never reach the result
__device__ __forceinline__ unsigned c10(unsigned word, int at) { return (word >> at) & 0x3ffu; }

// four macropixels (16 bytes) of UYVY / YUYV: 8 Y, 4 U, 4 V
template <int FORMAT, int PLANES>
__device__ __forceinline__ void split8(const u4 v, u2* y, unsigned* u, unsigned* vv) {
  constexpr unsigned ysel = FORMAT == UNPACK_UYVY ? 0x07050301u : 0x06040200u;
  *y = u2{perm(v.y, v.x, ysel), perm(v.w, v.z, ysel)};
  if (PLANES == 3) {
    // two macropixels -> U_a U_b V_a V_b, then the U halves and the V halves of two such words
    constexpr unsigned csel = FORMAT == UNPACK_UYVY ? 0x06020400u : 0x07030501u;
    const unsigned c0 = perm(v.y, v.x, csel), c1 = perm(v.w, v.z, csel);
    *u = perm(c1, c0, 0x05040100u);
    *vv = perm(c1, c0, 0x07060302u);
  }
}

// one group (four words) of v210: 6 Y, 3 U, 3 V
template <int PLANES>
__device__ __forceinline__ void split10(const u4 g, unsigned* y, unsigned* u, unsigned* v) {
  y[0] = c10(g.x, 10); y[1] = c10(g.y, 0); y[2] = c10(g.y, 20); y[3] = c10(g.z, 10); y[4] = c10(g.w, 0); y[5] = c10(g.w, 20);
  if (PLANES == 3) {
    u[0] = c10(g.x, 0); u[1] = c10(g.y, 10); u[2] = c10(g.z, 20);
    v[0] = c10(g.x, 20); v[1] = c10(g.z, 0); v[2] = c10(g.w, 10);
  }
}
__device__ __forceinline__ unsigned pair16(unsigned lo, unsigned hi) { return lo | (hi << 16); }

// VEC: every source row and every destination row starts 16-byte aligned (bases and pitches multiples of 16).  Only spans
// that lie completely inside the row take the wide path; row tails, and every span of a surface that is not aligned, go
// sample by sample (group by group for v210).  No row is read beyond its minimum bytes (4 * cw; 16 * ceil(w / 6)) and no
// destination row is written beyond w / cw samples.
template <int FORMAT, int PLANES, bool VEC>
__global__ __launch_bounds__(kLanesX* kRowsPerBlock) void unpack_kernel(const UnpackArgs a) {
  constexpr int PIX = Span<FORMAT>::pixels;
  const int span = blockIdx.x * kLanesX + threadIdx.x;
  const int x = span * PIX;
  const int y = blockIdx.y * kRowsPerBlock + threadIdx.y, fr = blockIdx.z;
  if (x >= a.w || y >= a.h) return;
  const uint8_t* __restrict__ s = a.src + (int64_t)fr * a.src_frame_pitch + (int64_t)y * a.src_row_pitch + (int64_t)span * Span<FORMAT>::src_bytes;
  uint8_t* __restrict__ dy = a.dst[0] + (int64_t)fr * a.dst_frame_pitch[0] + (int64_t)y * a.dst_row_pitch[0];
  uint8_t* __restrict__ du = PLANES == 3 ? a.dst[1] + (int64_t)fr * a.dst_frame_pitch[1] + (int64_t)y * a.dst_row_pitch[1] : nullptr;
  uint8_t* __restrict__ dv = PLANES == 3 ? a.dst[2] + (int64_t)fr * a.dst_frame_pitch[2] + (int64_t)y * a.dst_row_pitch[2] : nullptr;
  const int cx = x / 2;   // PIX is even: the span's first chroma sample
  const bool full = x + PIX <= a.w;
  if (FORMAT != UNPACK_V210) {
    if (VEC && full) {
      const u4 p = *reinterpret_cast<const u4*>(s), q = *reinterpret_cast<const u4*>(s + 16);
      u2 y0, y1;
      unsigned u0 = 0, u1 = 0, v0 = 0, v1 = 0;
      split8<FORMAT, PLANES>(p, &y0, &u0, &v0);
      split8<FORMAT, PLANES>(q, &y1, &u1, &v1);
      *reinterpret_cast<u4*>(dy + x) = u4{y0.x, y0.y, y1.x, y1.y};
      if (PLANES == 3) {
        *reinterpret_cast<u2*>(du + cx) = u2{u0, u1};
        *reinterpret_cast<u2*>(dv + cx) = u2{v0, v1};
      }
      return;
    }
    const int n = full ? PIX : a.w - x;   // samples of this span; its macropixels: ceil(n / 2)
    constexpr int yo = FORMAT == UNPACK_UYVY ? 1 : 0, uo = FORMAT == UNPACK_UYVY ? 0 : 1;
    for (int k = 0; 2 * k < n; ++k) {
      const uint8_t* m = s + 4 * k;
      dy[x + 2 * k] = m[yo];
      if (2 * k + 1 < n) dy[x + 2 * k + 1] = m[yo + 2];
      if (PLANES == 3) {
        du[cx + k] = m[uo];
        dv[cx + k] = m[uo + 2];
      }
    }
  } else {
    unsigned short* __restrict__ oy = reinterpret_cast<unsigned short*>(dy) + x;
    unsigned short* __restrict__ ou = PLANES == 3 ? reinterpret_cast<unsigned short*>(du) + cx : nullptr;
    unsigned short* __restrict__ ov = PLANES == 3 ? reinterpret_cast<unsigned short*>(dv) + cx : nullptr;
    if (VEC && full) {
      unsigned yy[24], uu[12], vv[12];
#pragma unroll
      for (int g = 0; g < 4; ++g) split10<PLANES>(*reinterpret_cast<const u4*>(s + 16 * g), yy + 6 * g, uu + 3 * g, vv + 3 * g);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        reinterpret_cast<u4*>(oy)[i] = u4{pair16(yy[8 * i], yy[8 * i + 1]), pair16(yy[8 * i + 2], yy[8 * i + 3]),
                                          pair16(yy[8 * i + 4], yy[8 * i + 5]), pair16(yy[8 * i + 6], yy[8 * i + 7])};
      if (PLANES == 3) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          reinterpret_cast<u2*>(ou)[i] = u2{pair16(uu[4 * i], uu[4 * i + 1]), pair16(uu[4 * i + 2], uu[4 * i + 3])};
          reinterpret_cast<u2*>(ov)[i] = u2{pair16(vv[4 * i], vv[4 * i + 1]), pair16(vv[4 * i + 2], vv[4 * i + 3])};
        }
      }
      return;
    }
    const int n = full ? PIX : a.w - x;          // luma samples of this span
    const int cn = full ? PIX / 2 : a.cw - cx;   // chroma samples of this span
    for (int g = 0; 6 * g < n; ++g) {
      const unsigned* wds = reinterpret_cast<const unsigned*>(s + 16 * g);   // rows are 4-byte aligned (the launcher checks)
      unsigned yy[6], uu[3], vv[3];
      split10<PLANES>(u4{wds[0], wds[1], wds[2], wds[3]}, yy, uu, vv);
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (6 * g + i < n) oy[6 * g + i] = (unsigned short)yy[i];
      if (PLANES == 3) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (3 * g + i < cn) {
            ou[3 * g + i] = (unsigned short)uu[i];
            ov[3 * g + i] = (unsigned short)vv[i];
          }
      }
    }
  }
}

template <int FORMAT, int PLANES>
hipError_t launch_planes(hipStream_t stream, const UnpackArgs& a, int n_frames, bool vec) {
  const int spans = (a.w + Span<FORMAT>::pixels - 1) / Span<FORMAT>::pixels;
  const dim3 grid((spans + kLanesX - 1) / kLanesX, (a.h + kRowsPerBlock - 1) / kRowsPerBlock, n_frames), block(kLanesX, kRowsPerBlock);
  if (vec) hipLaunchKernelGGL((unpack_kernel<FORMAT, PLANES, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((unpack_kernel<FORMAT, PLANES, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}

template <int FORMAT>
hipError_t launch_format(hipStream_t stream, const UnpackArgs& a, int n_frames, bool luma_only, bool vec) {
  return luma_only ? launch_planes<FORMAT, 1>(stream, a, n_frames, vec) : launch_planes<FORMAT, 3>(stream, a, n_frames, vec);
}

}  // namespace

hipError_t launch_unpack(hipStream_t stream, int format, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                         void* const dst[3], const int64_t dst_row_pitch[3], const int64_t dst_frame_pitch[3], int w, int h,
                         int n_frames) {
  if (n_frames <= 0 || w <= 0 || h <= 0) return hipSuccess;
  if (n_frames > 65535 || (format != UNPACK_UYVY && format != UNPACK_YUYV && format != UNPACK_V210) || !src || !dst[0])
    return hipErrorInvalidValue;
  const bool luma_only = !dst[1] || !dst[2];
  const int es = format == UNPACK_V210 ? 2 : 1;
  // what the sample-by-sample path itself needs: whole words on the v210 side, whole samples on the plane side
  if (format == UNPACK_V210 && (((uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch) & 3)) return hipErrorInvalidValue;
  if (src_row_pitch < host::packed_min_row_bytes((uint32_t)format, w)) return hipErrorInvalidValue;
  UnpackArgs a{};
  a.src = (const uint8_t*)src; a.src_row_pitch = src_row_pitch; a.src_frame_pitch = src_frame_pitch;
  a.w = w; a.h = h; a.cw = (w + 1) / 2;
  uintptr_t bits = (uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch;
  for (int p = 0; p < (luma_only ? 1 : 3); ++p) {
    a.dst[p] = (uint8_t*)dst[p]; a.dst_row_pitch[p] = dst_row_pitch[p]; a.dst_frame_pitch[p] = dst_frame_pitch[p];
    const uintptr_t b = (uintptr_t)dst[p] | (uintptr_t)dst_row_pitch[p] | (uintptr_t)dst_frame_pitch[p];
    if (b & (uintptr_t)(es - 1)) return hipErrorInvalidValue;
    if (dst_row_pitch[p] < (int64_t)(p ? a.cw : w) * es) return hipErrorInvalidValue;
    bits |= b;
  }
  const bool vec = (bits & 15) == 0;
  switch (format) {
    case UNPACK_UYVY: return launch_format<UNPACK_UYVY>(stream, a, n_frames, luma_only, vec);
    case UNPACK_YUYV: return launch_format<UNPACK_YUYV>(stream, a, n_frames, luma_only, vec);
    default: return launch_format<UNPACK_V210>(stream, a, n_frames, luma_only, vec);
  }
}

}  // namespace pqa
