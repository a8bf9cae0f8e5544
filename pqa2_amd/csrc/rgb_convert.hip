// Packed RGB captures -> the Y'CbCr planes of the other clip's layout (pqa_rgb_convert / pqa_rgb_convert_device; restated in
// tests/rgb_ref.py): unpack, colour matrix, range, depth, chroma subsampling and siting in ONE streaming pass with ONE rounding.
// Byte work bound by HBM, in the family of unpack.hip, ingest.hip and format_convert.hip: integers only, no LDS, no atomics,
// no floating point, no scratch.
//
// Formats (include/pqa_vmaf.h has the normative text): a pixel is 4 bytes.  BGRA / ARGB / RGBA / ABGR hold 8-bit components in
// that byte order, the A byte influences nothing; r210 is one BIG-endian word with R in bits 29-20, G in 19-10, B in 9-0, bits
// 31-30 influence nothing.
//
// Definition (exact integers).  m[3][4] is Q14, column 0 the offset:  A_c(x, y) = m[c][0] + m[c][1] R + m[c][2] G + m[c][3] B.
//     Y(x, y)  = clamp((A_0 + 2^13) >> 14, 0, 2^dst_bits - 1)                                    (>> arithmetic, i.e. floor)
//     C_c(i,k) = clamp((sum_y sum_x w_y w_x A_c + 2^(t-1)) >> t, 0, 2^dst_bits - 1),  t = 14 + log2(S_x S_y),  c = 1, 2
// with the taps of format_convert.hip from a 4:4:4 plane: an axis of shift 0 is the sample itself (S = 1); an axis of shift 1
// takes the luma samples 2i - 1 ... with [2 4 2] (co-sited) or [1 3 3 1] (centred), S = 8, indices folded onto the plane (edge
// replication).  The taps are linear, so the kernels sum w_y w_x R, G, B first and put the matrix behind the sum:
//     sum w A_c = S_x S_y m[c][0] + m[c][1] sum w R + m[c][2] sum w G + m[c][3] sum w B                     -- the same integer.
//
// Why int32 is enough.  The launcher refuses a matrix unless, for every row c,
//     E_c S_x S_y + 2^(t-1) < 2^31,   E_c = max |A_c| over the cube [0, 2^sb - 1]^3
//         = max(|m[c][0] + sum_j max(m[c][j], 0) top|, |m[c][0] + sum_j min(m[c][j], 0) top|),  top = 2^sb - 1
// (host::rgb_matrix_fits, in int64).  Every weight is positive, so sum w A_c lies between S min A_c and S max A_c: the exact sum
// plus the rounding half is inside int32.  The partial sums on the way (S m[c][0] + m[c][1] sum w R ...) may leave int32; they
// are formed in unsigned arithmetic, which wraps, and the last addition lands on the exact value because that value is
// representable.  The tap sums themselves are at most 64 * 1023 < 2^16.
// 24-bit multiply-adds: v_mad_i32_i24 needs both factors inside [-2^23, 2^23).  The sample factor is at most 65472.  The bound
// above does NOT confine a coefficient to 24 bits (offset and gain may cancel: m0 = -2^30, m1 = 2^23 passes at 8 bit), so the
// launcher looks: when all nine gains lie inside (-2^23, 2^23) -- every named matrix, whose largest gain is below 2^17 -- it
// takes the M24 instance, otherwise the instance with full 32-bit multiplies.  The low 32 bits of the products are the same.
//
// Kernels, templated on the source depth (8 / 10), the case (luma only; 4:4:4; 4:2:2 co-sited; 4:2:0 "left") and M24:
//   rows     the fast paths, taken when every base and pitch is a multiple of 16 and the layout is one of the three above.  A
//            lane owns a span of 16 pixels: four 16-byte loads a source row, a 16-byte store of 16 u8 luma samples (two for
//            u16), and for the subsampled layouts an 8-byte store of 8 u8 chroma samples a plane (16 bytes for u16).  The
//            components come out with v_perm_b32 -- the byte order is a selector in a scalar register, not a kernel of its own
//            --, r210 with one v_perm_b32 byte swap and three v_bfe_u32.  The left neighbour of a span ([2 4 2] reaches one
//            pixel back) is one overlapping dword load.  4:2:0 left: a lane's unit is one chroma row, i.e. the luma rows 2i and
//            2i + 1; it walks the source rows 2i - 1 ... 2i + 2 (clamped), adds w_y R, G, B per pixel into registers and
//            writes the two luma rows as it passes them.  Rows 2i - 1 and 2i + 2 are read again by the units above and below
//            (the simplest form: no LDS exchange; the re-reads are measured in tools/rgb_convert_times.py).
//            A span that crosses the end of the row goes sample by sample with the general kernel's functions.
//   general  every other shift / siting pair, every surface that does not allow 16-byte accesses, and the partner the fast
//            paths are tested against (PQA_RGB_GENERIC).  A lane owns one luma sample and, where it has one of that index, one
//            chroma sample a plane, and walks its taps with clamped loads.
// No source row is read beyond 4 * w bytes, no destination row is written beyond its samples.
#include "host_packed.h"
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

struct RgbAxis {
  int shift, n, j0;   // destination sample i takes the source samples (i << shift) + j0 + k, k < n, clamped to the plane
  int w[4];
};

struct RgbArgs {
  const uint8_t* src;
  int64_t src_row_pitch, src_frame_pitch;   // bytes
  uint8_t* dst[3];                          // Y, U, V (U, V null: luma only)
  int64_t dst_row_pitch[3], dst_frame_pitch[3];
  int w, h, cw, ch;
  RgbAxis x, y;
  int m[3][3];       // the gains of R, G, B
  int off[3];        // row 0: m[0][0] + 2^13; rows 1, 2: S_x S_y m[c][0] + 2^(t-1)
  int t;             // 14 + log2(S_x S_y)
  int dmax, d16;     // 2^dst_bits - 1; destination samples are u16
  unsigned sel[3];   // 8-bit formats: the v_perm_b32 selectors of R, G, B (that byte of the pixel, zero-extended)
  int at[3];         //                the byte of R, G, B in a pixel (sample-by-sample path)
};

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

enum { CASE_LUMA = 0, CASE_444 = 1, CASE_422C = 2, CASE_420L = 3 };
constexpr int kLanesX = 64, kRowsPerBlock = 4;   // a workgroup: one wave's width of spans, four units
constexpr int kPix = 16;                         // pixels of a span

// v_perm_b32: result byte i = byte sel_i of {hi : lo} (0-3 lo, 4-7 hi, 12: 0x00)
__device__ __forceinline__ unsigned perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// R, G, B of one pixel word as it was loaded (little-endian)
template <int SB>
__device__ __forceinline__ void rgb_of(const RgbArgs& a, unsigned px, unsigned (&c)[3]) {
  if (SB == 8) {
    c[0] = perm(0, px, a.sel[0]);
    c[1] = perm(0, px, a.sel[1]);
    c[2] = perm(0, px, a.sel[2]);
  } else {
    const unsigned v = perm(0, px, 0x00010203u);   // big-endian word; bits 31-30 never reach a result
    c[0] = (v >> 20) & 0x3ffu;                     // v_bfe_u32
    c[1] = (v >> 10) & 0x3ffu;
    c[2] = v & 0x3ffu;
  }
}

// the pixel at p, sample by sample: any address for the 8-bit formats, r210 words are 4-byte aligned (the launcher checks)
template <int SB>
__device__ __forceinline__ void load_px(const RgbArgs& a, const uint8_t* __restrict__ p, unsigned (&c)[3]) {
  if (SB == 8) {
    c[0] = p[a.at[0]];
    c[1] = p[a.at[1]];
    c[2] = p[a.at[2]];
  } else {
    rgb_of<10>(a, *reinterpret_cast<const unsigned*>(p), c);
  }
}

// off + m[c] . v in wrapping arithmetic (the head of the file: the exact value is inside int32)
template <bool M24>
__device__ __forceinline__ int row_of(const RgbArgs& a, int c, int off, const unsigned (&v)[3]) {
  if (M24)   // v_mad_i32_i24
    return (int)((unsigned)off + (unsigned)__mul24(a.m[c][0], (int)v[0]) + (unsigned)__mul24(a.m[c][1], (int)v[1]) +
                 (unsigned)__mul24(a.m[c][2], (int)v[2]));
  return (int)((unsigned)off + (unsigned)a.m[c][0] * v[0] + (unsigned)a.m[c][1] * v[1] + (unsigned)a.m[c][2] * v[2]);
}
__device__ __forceinline__ unsigned finish(int acc, int t, int dmax) { return (unsigned)clampi(acc >> t, dmax); }

__device__ __forceinline__ void put(uint8_t* __restrict__ row, int x, unsigned v, int d16) {
  if (d16) reinterpret_cast<unsigned short*>(row)[x] = (unsigned short)v;
  else row[x] = (uint8_t)v;
}

// luma sample (x, y) of one frame
template <int SB>
__device__ __forceinline__ void luma_sample(const RgbArgs& a, const uint8_t* __restrict__ sf, uint8_t* __restrict__ dy, int x, int y) {
  unsigned c[3];
  load_px<SB>(a, sf + (int64_t)y * a.src_row_pitch + (int64_t)x * 4, c);
  put(dy + (int64_t)y * a.dst_row_pitch[0], x, finish(row_of<false>(a, 0, a.off[0], c), 14, a.dmax), a.d16);
}

// chroma sample (cx, cy) of both planes of one frame by the definition: every tap, loads clamped
template <int SB>
__device__ __forceinline__ void chroma_sample(const RgbArgs& a, const uint8_t* __restrict__ sf, uint8_t* __restrict__ du,
                                              uint8_t* __restrict__ dv, int cx, int cy) {
  unsigned s[3] = {0, 0, 0};
  for (int ky = 0; ky < a.y.n; ++ky) {
    const uint8_t* __restrict__ row = sf + (int64_t)clampi((cy << a.y.shift) + a.y.j0 + ky, a.h - 1) * a.src_row_pitch;
    for (int kx = 0; kx < a.x.n; ++kx) {
      unsigned c[3];
      load_px<SB>(a, row + (int64_t)clampi((cx << a.x.shift) + a.x.j0 + kx, a.w - 1) * 4, c);
      const unsigned wt = (unsigned)(a.y.w[ky] * a.x.w[kx]);
      s[0] += wt * c[0];
      s[1] += wt * c[1];
      s[2] += wt * c[2];
    }
  }
  put(du + (int64_t)cy * a.dst_row_pitch[1], cx, finish(row_of<false>(a, 1, a.off[1], s), a.t, a.dmax), a.d16);
  put(dv + (int64_t)cy * a.dst_row_pitch[2], cx, finish(row_of<false>(a, 2, a.off[2], s), a.t, a.dmax), a.d16);
}

template <int SB, bool CHROMA>
__global__ __launch_bounds__(kLanesX* kRowsPerBlock) void rgb_general_kernel(const RgbArgs a) {
  const int x = blockIdx.x * kLanesX + threadIdx.x, y = blockIdx.y * kRowsPerBlock + threadIdx.y, fr = blockIdx.z;
  if (x >= a.w || y >= a.h) return;
  const uint8_t* __restrict__ sf = a.src + (int64_t)fr * a.src_frame_pitch;
  luma_sample<SB>(a, sf, a.dst[0] + (int64_t)fr * a.dst_frame_pitch[0], x, y);
  if (CHROMA && x < a.cw && y < a.ch)
    chroma_sample<SB>(a, sf, a.dst[1] + (int64_t)fr * a.dst_frame_pitch[1], a.dst[2] + (int64_t)fr * a.dst_frame_pitch[2], x, y);
}

// N finished samples to x0 ... x0 + N - 1 of a destination row: one packed store (16 u16: two)
template <int N>
__device__ __forceinline__ void store_span(uint8_t* __restrict__ row, int x0, const unsigned (&o)[N], int d16) {
  if (d16) {
    unsigned wd[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i) wd[i] = o[2 * i] | (o[2 * i + 1] << 16);
#pragma unroll
    for (int i = 0; i < N / 8; ++i) reinterpret_cast<u4*>(row + (int64_t)x0 * 2)[i] = u4{wd[4 * i], wd[4 * i + 1], wd[4 * i + 2], wd[4 * i + 3]};
  } else {
    unsigned wd[N / 4];
#pragma unroll
    for (int i = 0; i < N / 4; ++i) wd[i] = o[4 * i] | (o[4 * i + 1] << 8) | (o[4 * i + 2] << 16) | (o[4 * i + 3] << 24);
    if constexpr (N == 16) *reinterpret_cast<u4*>(row + x0) = u4{wd[0], wd[1], wd[2], wd[3]};
    else *reinterpret_cast<u2*>(row + x0) = u2{wd[0], wd[1]};
  }
}

// Launched only on surfaces whose bases and pitches are multiples of 16, with the layout of CASE.
template <int SB, int CASE, bool M24>
__global__ __launch_bounds__(kLanesX* kRowsPerBlock) void rgb_rows_kernel(const RgbArgs a) {
  constexpr bool TAPS = CASE == CASE_422C || CASE == CASE_420L;   // co-sited [2 4 2] along x
  constexpr bool VS = CASE == CASE_420L;                          // centred [1 3 3 1] along y
  constexpr int NR = VS ? 4 : 1;                                  // source rows of a unit
  const int x0 = (blockIdx.x * kLanesX + threadIdx.x) * kPix, u = blockIdx.y * kRowsPerBlock + threadIdx.y, fr = blockIdx.z;
  if (x0 >= a.w || u >= (VS ? a.ch : a.h)) return;
  const uint8_t* __restrict__ sf = a.src + (int64_t)fr * a.src_frame_pitch;
  uint8_t* __restrict__ dy = a.dst[0] + (int64_t)fr * a.dst_frame_pitch[0];
  uint8_t* __restrict__ du = CASE != CASE_LUMA ? a.dst[1] + (int64_t)fr * a.dst_frame_pitch[1] : nullptr;
  uint8_t* __restrict__ dv = CASE != CASE_LUMA ? a.dst[2] + (int64_t)fr * a.dst_frame_pitch[2] : nullptr;
  if (x0 + kPix > a.w) {   // the row's tail: sample by sample
    for (int y = VS ? 2 * u : u; y < (VS ? 2 * u + 2 : u + 1) && y < a.h; ++y)
      for (int x = x0; x < a.w; ++x) luma_sample<SB>(a, sf, dy, x, y);
    if (CASE != CASE_LUMA)
      for (int cx = TAPS ? x0 / 2 : x0; cx < a.cw; ++cx) chroma_sample<SB>(a, sf, du, dv, cx, u);
    return;
  }
  unsigned acc[3][kPix + 1];   // TAPS: sum_y w_y R, G, B of the pixels x0 - 1 ... x0 + 15
#pragma unroll
  for (int p = 0; p <= kPix; ++p) acc[0][p] = acc[1][p] = acc[2][p] = 0;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int j = VS ? 2 * u - 1 + r : u;
    const unsigned wy = VS ? (r == 0 || r == 3 ? 1u : 3u) : 1u;
    const bool luma_row = VS ? (r == 1 || (r == 2 && j < a.h)) : true;   // uniform in a wave
    const uint8_t* __restrict__ row = sf + (int64_t)clampi(j, a.h - 1) * a.src_row_pitch + (int64_t)x0 * 4;
    u4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = reinterpret_cast<const u4*>(row)[i];
    unsigned left = 0;
    if constexpr (TAPS) left = *reinterpret_cast<const unsigned*>(row - (x0 ? 4 : 0));   // pixel x0 - 1, folded onto pixel 0
    unsigned oy[kPix], ou[kPix], ov[kPix];
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      unsigned c[3];
      rgb_of<SB>(a, v[p >> 2][p & 3], c);
      if (luma_row) oy[p] = finish(row_of<M24>(a, 0, a.off[0], c), 14, a.dmax);
      if constexpr (CASE == CASE_444) {
        ou[p] = finish(row_of<M24>(a, 1, a.off[1], c), 14, a.dmax);
        ov[p] = finish(row_of<M24>(a, 2, a.off[2], c), 14, a.dmax);
      }
      if constexpr (TAPS)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k][p + 1] += wy * c[k];
    }
    if constexpr (TAPS) {
      unsigned c[3];
      rgb_of<SB>(a, left, c);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k][0] += wy * c[k];
    }
    if (luma_row) store_span<kPix>(dy + (int64_t)j * a.dst_row_pitch[0], x0, oy, a.d16);
    if constexpr (CASE == CASE_444) {
      store_span<kPix>(du + (int64_t)u * a.dst_row_pitch[1], x0, ou, a.d16);
      store_span<kPix>(dv + (int64_t)u * a.dst_row_pitch[2], x0, ov, a.d16);
    }
  }
  if constexpr (TAPS) {
    unsigned ou[kPix / 2], ov[kPix / 2];
#pragma unroll
    for (int k = 0; k < kPix / 2; ++k) {   // chroma sample x0 / 2 + k sits on pixel x0 + 2 k: acc index 2 k + 1
      const int i = 2 * k;
      const unsigned s[3] = {2 * acc[0][i] + 4 * acc[0][i + 1] + 2 * acc[0][i + 2], 2 * acc[1][i] + 4 * acc[1][i + 1] + 2 * acc[1][i + 2],
                             2 * acc[2][i] + 4 * acc[2][i + 1] + 2 * acc[2][i + 2]};
      ou[k] = finish(row_of<M24>(a, 1, a.off[1], s), a.t, a.dmax);
      ov[k] = finish(row_of<M24>(a, 2, a.off[2], s), a.t, a.dmax);
    }
    store_span<kPix / 2>(du + (int64_t)u * a.dst_row_pitch[1], x0 / 2, ou, a.d16);
    store_span<kPix / 2>(dv + (int64_t)u * a.dst_row_pitch[2], x0 / 2, ov, a.d16);
  }
}

RgbAxis make_axis(int shift, int site) {
  if (shift == 0) return RgbAxis{0, 1, 0, {1, 0, 0, 0}};
  if (site == kSiteCentre) return RgbAxis{1, 4, -1, {1, 3, 3, 1}};
  return RgbAxis{1, 3, -1, {2, 4, 2, 0}};
}

template <int SB, int CASE>
void launch_rows(hipStream_t stream, const RgbArgs& a, int n_frames, bool m24) {
  const int spans = (a.w + kPix - 1) / kPix, units = CASE == CASE_420L ? a.ch : a.h;
  const dim3 grid((spans + kLanesX - 1) / kLanesX, (units + kRowsPerBlock - 1) / kRowsPerBlock, n_frames), block(kLanesX, kRowsPerBlock);
  if (m24) hipLaunchKernelGGL((rgb_rows_kernel<SB, CASE, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((rgb_rows_kernel<SB, CASE, false>), grid, block, 0, stream, a);
}

template <int SB>
void launch_depth(hipStream_t stream, const RgbArgs& a, int n_frames, int rows_case, bool chroma, bool m24) {
  switch (rows_case) {
    case CASE_LUMA: return launch_rows<SB, CASE_LUMA>(stream, a, n_frames, m24);
    case CASE_444: return launch_rows<SB, CASE_444>(stream, a, n_frames, m24);
    case CASE_422C: return launch_rows<SB, CASE_422C>(stream, a, n_frames, m24);
    case CASE_420L: return launch_rows<SB, CASE_420L>(stream, a, n_frames, m24);
    default: break;
  }
  const dim3 grid((a.w + kLanesX - 1) / kLanesX, (a.h + kRowsPerBlock - 1) / kRowsPerBlock, n_frames), block(kLanesX, kRowsPerBlock);
  if (chroma) hipLaunchKernelGGL((rgb_general_kernel<SB, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((rgb_general_kernel<SB, false>), grid, block, 0, stream, a);
}

}  // namespace

hipError_t launch_rgb_convert(hipStream_t stream, int format, const ConvertLayout& dl, bool generic, const int32_t m[12], const void* src,
                              int64_t src_row_pitch, int64_t src_frame_pitch, void* const dst[3], const int64_t dst_row_pitch[3],
                              const int64_t dst_frame_pitch[3], int w, int h, int n_frames) {
  if (n_frames <= 0) return hipSuccess;
  if (n_frames > 65535 || !host::rgb_format((uint32_t)format) || !src || !dst || !dst[0] || !m || w < 1 || w > 8192 || h < 1 || h > 8192 ||
      (dl.bits != 8 && dl.bits != 10) || dl.hshift < 0 || dl.hshift > 1 || dl.vshift < 0 || dl.vshift > 1 ||
      (dl.hsite != kSiteCosited && dl.hsite != kSiteCentre) || (dl.vsite != kSiteCosited && dl.vsite != kSiteCentre) || !dst[1] != !dst[2])
    return hipErrorInvalidValue;
  const int sb = host::rgb_bit_depth((uint32_t)format), es = dl.bits > 8 ? 2 : 1;
  const bool chroma = dst[1] != nullptr;
  if (!host::rgb_matrix_fits(m, sb, dl.hshift, dl.vshift)) return hipErrorInvalidValue;   // what makes int32 legal in the kernels
  if (sb == 10 && (((uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch) & 3)) return hipErrorInvalidValue;
  if (src_row_pitch < host::rgb_min_row_bytes(w)) return hipErrorInvalidValue;
  RgbArgs a{};
  a.src = (const uint8_t*)src; a.src_row_pitch = src_row_pitch; a.src_frame_pitch = src_frame_pitch;
  a.w = w; a.h = h; a.cw = convert_plane_size(w, dl.hshift); a.ch = convert_plane_size(h, dl.vshift);
  uintptr_t bits = (uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch;
  for (int p = 0; p < (chroma ? 3 : 1); ++p) {
    a.dst[p] = (uint8_t*)dst[p]; a.dst_row_pitch[p] = dst_row_pitch[p]; a.dst_frame_pitch[p] = dst_frame_pitch[p];
    const uintptr_t b = (uintptr_t)dst[p] | (uintptr_t)dst_row_pitch[p] | (uintptr_t)dst_frame_pitch[p];
    if (b & (uintptr_t)(es - 1)) return hipErrorInvalidValue;
    if (dst_row_pitch[p] < (int64_t)(p ? a.cw : w) * es) return hipErrorInvalidValue;
    bits |= b;
  }
  a.x = make_axis(dl.hshift, dl.hsite);
  a.y = make_axis(dl.vshift, dl.vsite);
  const int ts = 3 * (dl.hshift + dl.vshift);   // log2(S_x S_y): 8 an axis of shift 1
  a.t = 14 + ts;
  bool m24 = true;
  for (int c = 0; c < 3; ++c) {
    for (int k = 0; k < 3; ++k) {
      a.m[c][k] = m[4 * c + 1 + k];
      if (a.m[c][k] <= -(1 << 23) || a.m[c][k] >= (1 << 23)) m24 = false;
    }
    const int tc = c ? ts : 0;   // rgb_matrix_fits: inside int32
    a.off[c] = (int)((int64_t)m[4 * c] * ((int64_t)1 << tc) + ((int64_t)1 << (13 + tc)));
  }
  a.dmax = (1 << dl.bits) - 1; a.d16 = es == 2;
  host::rgb_byte_order((uint32_t)format, a.at);
  for (int k = 0; k < 3; ++k) a.sel[k] = 0x0c0c0c00u | (unsigned)a.at[k];
  int rows_case = -1;
  if (!generic && (bits & 15) == 0) {
    if (!chroma) rows_case = CASE_LUMA;
    else if (dl.hshift == 0 && dl.vshift == 0) rows_case = CASE_444;
    else if (dl.hshift == 1 && dl.hsite == kSiteCosited && dl.vshift == 0) rows_case = CASE_422C;
    else if (dl.hshift == 1 && dl.hsite == kSiteCosited && dl.vshift == 1 && dl.vsite == kSiteCentre) rows_case = CASE_420L;
  }
  if (sb == 8) launch_depth<8>(stream, a, n_frames, rows_case, chroma, m24);
  else launch_depth<10>(stream, a, n_frames, rows_case, chroma, m24);
  return hipGetLastError();
}

}  // namespace pqa
