// Pixel-format conversion of one kind of plane: chroma layout (the nine (hshift, vshift) pairs), chroma siting and sample depth
// in ONE streaming pass with ONE rounding (pqa_format_convert / pqa_format_convert_device; restated in
// tests/format_convert_ref.py).  Byte work bound by HBM, like unpack.hip and ingest.hip: no LDS, no atomics, no floating point.
//
// Definition (exact integers; include/pqa_vmaf.h repeats it).  The plane belongs to a frame of luma_width x luma_height; a
// plane of shift s has ceil(luma >> s) samples along an axis.  Per axis, positions are in HALF luma samples.  With
// F = 1 << shift:
//     sample k of a plane sits at P(k) = 2 F k + (centre ? F - 1 : 0)          (siting is void where the shift is 0)
//     W = max(F_src, F_dst)
//     destination sample i takes every source sample j with the weight w = 2 W - |P_src(j) - P_dst(i)| where that is
//     positive -- a triangle of half-width W luma samples --, j folded onto clamp(j, 0, n_src - 1) (edge replication).
// The weights of a destination sample sum to S = 2 W^2 / F_src, a power of two of at most 32, over at most 8 taps
// (2 W / F_src candidates j, the first is floor((P_dst(i) - 2 W - offset_src) / (2 F_src)) + 1).  4:2:2 -> 4:2:0 vertically:
// centred [1 3 3 1] / 8 at rows 2i - 1 ... 2i + 2, co-sited [2 4 2] / 8; 4:2:0 centred -> 4:2:2: [1 3] / 4 and [3 1] / 4
// alternating; identity [2] / 2 (shift s: [2 F] / 2 F).  Both axes and the depth change share one rounding:
//     acc = sum_y sum_x w_y w_x s  (at most 1024 * 4095, int32; a source sample above 2^src_bits - 1 is read as that)
//     t = log2(S_x S_y), d = dst_bits - src_bits
//     t > d:  out = min((acc + 2^(t-d-1)) >> (t - d), 2^dst_bits - 1);   otherwise  out = acc << (d - t)
// Identity returns the source; a constant plane c becomes c << d (d < 0: min((c + 2^(-d-1)) >> -d, max)); a plane linear in
// the luma position stays linear in the interior; 10 -> 8 bit of 1023 gives 255.  Triangle and rounding are this library's
// own, not swscale's.
//
// Kernels, templated on the source and destination sample type (u8 / u16):
//   general   any layout pair and siting.  A lane owns one destination sample and walks its taps from the formula above with
//             clamped loads; a source sample may be read several times.  The path of the rare layouts, of every plane whose
//             bases or pitches do not allow 16-byte loads, and the partner the fast paths are tested against
//             (PQA_CONVERT_GENERIC).
//   rows      the fast paths, chosen on the host once per launch, only when both sides' bases and pitches are multiples of
//             16 and the horizontal layout (shift, and siting where it counts) is the same on both sides, so that a column of
//             the source is a column of the destination.  A lane owns a 16-byte column segment of source rows (16 u8 / 8 u16
//             samples) and writes the same samples of the destination rows with one packed store a row (two 16-byte stores
//             when 16 u8 widen to u16).  A horizontal identity is one tap that carries the whole sum: it is left out of acc and t.
//       COPY  equal vertical layout too: a depth change only (the luma of a v210 capture against an 8-bit master, 8 -> 10).
//             One load, the rounding shift, one store.
//       DOWN  vertical 2:1 (4:2:2 -> 4:2:0, the capture case).  Destination row i reads the four source rows from
//             j0 + 2 i on with weights that do not depend on i.  A lane walks down a run of kRun destination rows with the
//             window in registers: two rows are loaded per destination row, each source row once per run (a run's first
//             two rows are its halo, which the run above loads too -- three times out of four a wave of the same
//             workgroup; where that second read is served from was not measured).
//       UP    vertical 1:2 (4:2:0 -> 4:2:2).  Destination rows 2k and 2k + 1 read two source rows each, from j0[parity] + k on,
//             with a weight pair per parity; a lane keeps three rows and loads one per destination row pair.
//       2:1 on both axes (4:4:4 -> 4:2:0) has no fast path: it takes the general kernel.
//       A lane whose segment crosses the end of the row handles its samples one by one with the general kernel's function.
//   kRun = 4 destination rows (DOWN: 8 + 2 source rows; UP: 4 pairs = 8 destination rows from 4 + 2 source rows): a 1080p
//   4:2:2 chroma plane (960 x 1080 -> 960 x 540) is one wave wide, so 8 frames of one plane kind are 8 * 135 = 1080 waves --
//   one for each of the chip's 1024 SIMDs, U and V in one call two -- at the price of 2 halo rows per 8; a run of 8 would halve
//   the halo and leave half the SIMDs idle.  The loop is unrolled, so a run's ten loads are in flight together.
// No source row is read beyond its samples and no destination byte beyond a row's samples is written.
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

struct ConvAxis {
  int sshift, dshift;   // log2 F of the source / destination plane
  int soff, doff;       // (centre ? F - 1 : 0)
  int w2, nt;           // 2 W; candidates j of a destination sample: 2 W / F_src
  int ns, nd;           // samples of the source / destination plane along this axis
};

struct ConvArgs {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_row_pitch, src_frame_pitch, dst_row_pitch, dst_frame_pitch;   // bytes
  ConvAxis x, y;
  int rs, ls;            // out = rs > 0 ? min((acc + 2^(rs-1)) >> rs, dmax) : acc << ls; of the whole definition (general_sample)
  int vrs, vls;          // the same for the rows kernels, whose acc leaves the horizontal identity out
  unsigned smax, dmax;   // 2^bits - 1
  // rows kernels: the vertical weights and first rows by the parity of the destination row (DOWN: [0] only)
  int wv[2][4], j0[2];
};

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

enum { MODE_GENERAL = 0, MODE_COPY = 1, MODE_DOWN = 2, MODE_UP = 3 };
constexpr int kLanesX = 64, kRowsPerBlock = 4;   // a workgroup: one wave's width of lanes, four rows (rows kernels: four runs)
constexpr int kRun = 4;                          // DOWN: destination rows of a run; UP: destination row PAIRS of a run

__device__ __forceinline__ unsigned finish(unsigned acc, int rs, int ls, unsigned dmax) {
  if (rs > 0) {
    const unsigned v = (acc + (1u << (rs - 1))) >> rs;
    return v < dmax ? v : dmax;
  }
  return acc << ls;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the first candidate j of destination sample i along an axis (>> of a negative value: arithmetic, i.e. floor)
__device__ __forceinline__ int first_tap(const ConvAxis& ax, int pd) { return ((pd - ax.w2 - ax.soff) >> (ax.sshift + 1)) + 1; }
__device__ __forceinline__ int tap_weight(const ConvAxis& ax, int j, int pd) {
  const int dlt = (j << (ax.sshift + 1)) + ax.soff - pd;
  return ax.w2 - (dlt < 0 ? -dlt : dlt);
}

// destination sample (x, y) of one frame by the definition: every tap from the formula, loads clamped
template <class SrcT, class DstT>
__device__ __forceinline__ void general_sample(const ConvArgs& a, const uint8_t* __restrict__ sf, uint8_t* __restrict__ df, int x, int y) {
  const int pdx = (x << (a.x.dshift + 1)) + a.x.doff, pdy = (y << (a.y.dshift + 1)) + a.y.doff;
  const int jx0 = first_tap(a.x, pdx), jy0 = first_tap(a.y, pdy);
  unsigned acc = 0;
  for (int ny = 0; ny < a.y.nt; ++ny) {
    const int wy = tap_weight(a.y, jy0 + ny, pdy);
    if (wy <= 0) continue;
    const SrcT* __restrict__ row = reinterpret_cast<const SrcT*>(sf + (int64_t)clampi(jy0 + ny, a.y.ns - 1) * a.src_row_pitch);
    unsigned racc = 0;
    for (int nx = 0; nx < a.x.nt; ++nx) {
      const int wx = tap_weight(a.x, jx0 + nx, pdx);
      if (wx <= 0) continue;
      const unsigned s = row[clampi(jx0 + nx, a.x.ns - 1)];
      racc += (unsigned)wx * (s < a.smax ? s : a.smax);
    }
    acc += (unsigned)wy * racc;
  }
  reinterpret_cast<DstT*>(df + (int64_t)y * a.dst_row_pitch)[x] = (DstT)finish(acc, a.rs, a.ls, a.dmax);
}

template <class SrcT, class DstT>
__global__ __launch_bounds__(kLanesX* kRowsPerBlock) void convert_general_kernel(const ConvArgs a) {
  const int x = blockIdx.x * kLanesX + threadIdx.x, y = blockIdx.y * kRowsPerBlock + threadIdx.y, fr = blockIdx.z;
  if (x >= a.x.nd || y >= a.y.nd) return;
  general_sample<SrcT, DstT>(a, a.src + (int64_t)fr * a.src_frame_pitch, a.dst + (int64_t)fr * a.dst_frame_pitch, x, y);
}

// ---- the rows kernels -------------------------------------------------------------------------------------------------
template <class SrcT>
struct Seg {   // a lane's 16 bytes of a source row
  static constexpr int n = 16 / (int)sizeof(SrcT);
};

// sample k of a loaded segment (v_bfe_u32), clamped to the source depth where the container is wider than the samples
template <class SrcT>
__device__ __forceinline__ unsigned sample_of(const u4 v, int k, unsigned smax) {
  if (sizeof(SrcT) == 1) return (v[k >> 2] >> (8 * (k & 3))) & 0xffu;
  const unsigned s = (v[k >> 1] >> (16 * (k & 1))) & 0xffffu;
  return s < smax ? s : smax;
}

// the N finished samples of a lane to x0 ... x0 + N - 1 of a destination row: one packed store (16 u8 -> u16: two)
template <class DstT, int N>
__device__ __forceinline__ void store_seg(uint8_t* __restrict__ row, int x0, const unsigned (&o)[N]) {
  if (sizeof(DstT) == 1) {
    unsigned wd[N / 4];
#pragma unroll
    for (int i = 0; i < N / 4; ++i) wd[i] = o[4 * i] | (o[4 * i + 1] << 8) | (o[4 * i + 2] << 16) | (o[4 * i + 3] << 24);
    if constexpr (N == 16) *reinterpret_cast<u4*>(row + x0) = u4{wd[0], wd[1], wd[2], wd[3]};
    else *reinterpret_cast<u2*>(row + x0) = u2{wd[0], wd[1]};
  } else {
    unsigned wd[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i) wd[i] = o[2 * i] | (o[2 * i + 1] << 16);
#pragma unroll
    for (int i = 0; i < N / 8; ++i) reinterpret_cast<u4*>(row + (int64_t)x0 * 2)[i] = u4{wd[4 * i], wd[4 * i + 1], wd[4 * i + 2], wd[4 * i + 3]};
  }
}

template <class SrcT>
__device__ __forceinline__ u4 load_row(const ConvArgs& a, const uint8_t* __restrict__ sf, int j, int x0) {
  return *reinterpret_cast<const u4*>(sf + (int64_t)clampi(j, a.y.ns - 1) * a.src_row_pitch + (int64_t)x0 * (int)sizeof(SrcT));
}

// one destination row from NT source rows in registers
template <class SrcT, class DstT, int NT>
__device__ __forceinline__ void emit_row(const ConvArgs& a, uint8_t* __restrict__ df, int y, int x0, const u4 (&r)[NT], const int (&w)[NT]) {
  constexpr int N = Seg<SrcT>::n;
  unsigned o[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    unsigned acc = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc += (unsigned)w[t] * sample_of<SrcT>(r[t], k, a.smax);   // v_mad_u32_u24: both factors below 2^24
    o[k] = finish(acc, a.vrs, a.vls, a.dmax);
  }
  store_seg<DstT, N>(df + (int64_t)y * a.dst_row_pitch, x0, o);
}

// Launched only on planes whose bases and pitches are multiples of 16, with a.x.ns == a.x.nd and a horizontal identity.
template <class SrcT, class DstT, int MODE>
__global__ __launch_bounds__(kLanesX* kRowsPerBlock) void convert_rows_kernel(const ConvArgs a) {
  constexpr int N = Seg<SrcT>::n;
  const int x0 = (blockIdx.x * kLanesX + threadIdx.x) * N, run = blockIdx.y * kRowsPerBlock + threadIdx.y, fr = blockIdx.z;
  constexpr int rows_per_run = MODE == MODE_COPY ? 1 : (MODE == MODE_DOWN ? kRun : 2 * kRun);
  const int y0 = run * rows_per_run;
  if (x0 >= a.x.nd || y0 >= a.y.nd) return;
  const uint8_t* __restrict__ sf = a.src + (int64_t)fr * a.src_frame_pitch;
  uint8_t* __restrict__ df = a.dst + (int64_t)fr * a.dst_frame_pitch;
  if (x0 + N > a.x.nd) {   // the row's tail: sample by sample
    for (int y = y0; y < y0 + rows_per_run && y < a.y.nd; ++y)
      for (int x = x0; x < a.x.nd; ++x) general_sample<SrcT, DstT>(a, sf, df, x, y);
    return;
  }
  if (MODE == MODE_COPY) {
    const u4 r[1] = {load_row<SrcT>(a, sf, y0, x0)};
    const int w[1] = {1};
    emit_row<SrcT, DstT, 1>(a, df, y0, x0, r, w);
  } else if (MODE == MODE_DOWN) {
    const int w[4] = {a.wv[0][0], a.wv[0][1], a.wv[0][2], a.wv[0][3]};
    int j = a.j0[0] + 2 * y0;
    u4 r[4];
    r[0] = load_row<SrcT>(a, sf, j, x0);
    r[1] = load_row<SrcT>(a, sf, j + 1, x0);
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      if (y0 + i < a.y.nd) {   // uniform in a wave
        r[2] = load_row<SrcT>(a, sf, j + 2, x0);
        r[3] = load_row<SrcT>(a, sf, j + 3, x0);
        emit_row<SrcT, DstT, 4>(a, df, y0 + i, x0, r, w);
        r[0] = r[2];
        r[1] = r[3];
        j += 2;
      }
    }
  } else {
    // rows y0 = 2k (even: j0[0] + k, j0[0] + k + 1) and 2k + 1 (odd: j0[1] + k ...), j0[1] - j0[0] = 0 or 1: three rows from j0[0] + k
    const int we[2] = {a.wv[0][0], a.wv[0][1]}, wo[2] = {a.wv[1][0], a.wv[1][1]};
    const bool odd_next = a.j0[1] != a.j0[0];
    int j = a.j0[0] + (y0 >> 1);
    u4 r[3];
    r[0] = load_row<SrcT>(a, sf, j, x0);
    r[1] = load_row<SrcT>(a, sf, j + 1, x0);
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      const int y = y0 + 2 * i;
      if (y < a.y.nd) {
        r[2] = load_row<SrcT>(a, sf, j + 2, x0);
        const u4 e[2] = {r[0], r[1]};
        emit_row<SrcT, DstT, 2>(a, df, y, x0, e, we);
        if (y + 1 < a.y.nd) {
          const u4 o[2] = {odd_next ? r[1] : r[0], odd_next ? r[2] : r[1]};
          emit_row<SrcT, DstT, 2>(a, df, y + 1, x0, o, wo);
        }
        r[0] = r[1];
        r[1] = r[2];
        ++j;
      }
    }
  }
}

int ilog2(int v) {
  int n = 0;
  while ((1 << n) < v) ++n;
  return n;
}

ConvAxis make_axis(int luma, int sshift, int dshift, int ssite, int dsite) {
  ConvAxis ax{};
  const int fs = 1 << sshift, fd = 1 << dshift, w = fs > fd ? fs : fd;
  ax.sshift = sshift; ax.dshift = dshift;
  ax.soff = ssite == kSiteCentre ? fs - 1 : 0;
  ax.doff = dsite == kSiteCentre ? fd - 1 : 0;
  ax.w2 = 2 * w; ax.nt = 2 * w / fs;
  ax.ns = convert_plane_size(luma, sshift); ax.nd = convert_plane_size(luma, dshift);
  return ax;
}
int axis_log2_sum(const ConvAxis& ax) { return 1 + 2 * (ilog2(ax.w2) - 1) - ax.sshift; }   // log2(2 W^2 / F_src)
bool axis_identity(const ConvAxis& ax) { return ax.sshift == ax.dshift && ax.soff == ax.doff; }

template <class SrcT, class DstT>
void launch_typed(hipStream_t stream, const ConvArgs& a, int mode, int n_frames) {
  const dim3 block(kLanesX, kRowsPerBlock);
  if (mode == MODE_GENERAL) {
    const dim3 grid((a.x.nd + kLanesX - 1) / kLanesX, (a.y.nd + kRowsPerBlock - 1) / kRowsPerBlock, n_frames);
    hipLaunchKernelGGL((convert_general_kernel<SrcT, DstT>), grid, block, 0, stream, a);
    return;
  }
  const int seg = Seg<SrcT>::n, lanes = (a.x.nd + seg - 1) / seg;
  const int rows_per_run = mode == MODE_COPY ? 1 : (mode == MODE_DOWN ? kRun : 2 * kRun);
  const int runs = (a.y.nd + rows_per_run - 1) / rows_per_run;
  const dim3 grid((lanes + kLanesX - 1) / kLanesX, (runs + kRowsPerBlock - 1) / kRowsPerBlock, n_frames);
  if (mode == MODE_COPY) hipLaunchKernelGGL((convert_rows_kernel<SrcT, DstT, MODE_COPY>), grid, block, 0, stream, a);
  else if (mode == MODE_DOWN) hipLaunchKernelGGL((convert_rows_kernel<SrcT, DstT, MODE_DOWN>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((convert_rows_kernel<SrcT, DstT, MODE_UP>), grid, block, 0, stream, a);
}

}  // namespace

hipError_t launch_format_convert(hipStream_t stream, const ConvertLayout& sl, const ConvertLayout& dl, int luma_w, int luma_h,
                                 bool generic, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch, void* dst,
                                 int64_t dst_row_pitch, int64_t dst_frame_pitch, int n_frames) {
  if (n_frames <= 0) return hipSuccess;
  auto layout_ok = [](const ConvertLayout& l) {
    return (l.bits == 8 || l.bits == 10 || l.bits == 12) && l.hshift >= 0 && l.hshift <= 2 && l.vshift >= 0 && l.vshift <= 2 &&
           (l.hsite == kSiteCosited || l.hsite == kSiteCentre) && (l.vsite == kSiteCosited || l.vsite == kSiteCentre);
  };
  if (n_frames > 65535 || !src || !dst || !layout_ok(sl) || !layout_ok(dl) || luma_w < 1 || luma_w > 8192 || luma_h < 1 || luma_h > 8192)
    return hipErrorInvalidValue;
  const int ses = sl.bits > 8 ? 2 : 1, des = dl.bits > 8 ? 2 : 1;
  ConvArgs a{};
  a.src = (const uint8_t*)src; a.dst = (uint8_t*)dst;
  a.src_row_pitch = src_row_pitch; a.src_frame_pitch = src_frame_pitch;
  a.dst_row_pitch = dst_row_pitch; a.dst_frame_pitch = dst_frame_pitch;
  a.x = make_axis(luma_w, sl.hshift, dl.hshift, sl.hsite, dl.hsite);
  a.y = make_axis(luma_h, sl.vshift, dl.vshift, sl.vsite, dl.vsite);
  // whole samples on both sides, rows that hold a row
  if ((((uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch) & (uintptr_t)(ses - 1)) ||
      (((uintptr_t)dst | (uintptr_t)dst_row_pitch | (uintptr_t)dst_frame_pitch) & (uintptr_t)(des - 1)) ||
      src_row_pitch < (int64_t)a.x.ns * ses || dst_row_pitch < (int64_t)a.x.nd * des)
    return hipErrorInvalidValue;
  a.smax = (1u << sl.bits) - 1; a.dmax = (1u << dl.bits) - 1;
  const uintptr_t bits = (uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch | (uintptr_t)dst | (uintptr_t)dst_row_pitch |
                         (uintptr_t)dst_frame_pitch;
  int mode = MODE_GENERAL;
  if (!generic && (bits & 15) == 0 && axis_identity(a.x)) {
    if (axis_identity(a.y)) mode = MODE_COPY;
    else if (dl.vshift == sl.vshift + 1) mode = MODE_DOWN;
    else if (dl.vshift + 1 == sl.vshift) mode = MODE_UP;
  }
  // one rounding: t = log2 of the weights' sum (a horizontal identity left out on the rows paths), d the depth change
  const int t = axis_log2_sum(a.x) + axis_log2_sum(a.y), tv = mode == MODE_COPY ? 0 : axis_log2_sum(a.y);
  const int d = dl.bits - sl.bits;
  a.rs = t > d ? t - d : 0;
  a.ls = t > d ? 0 : d - t;
  a.vrs = tv > d ? tv - d : 0;
  a.vls = tv > d ? 0 : d - tv;
  if (mode == MODE_DOWN || mode == MODE_UP) {   // the weights of destination rows 0 and 1 are those of every even / odd row
    for (int par = 0; par < 2; ++par) {
      const int pd = (par << (a.y.dshift + 1)) + a.y.doff;
      const int j = ((pd - a.y.w2 - a.y.soff) >> (a.y.sshift + 1)) + 1;   // as first_tap
      a.j0[par] = mode == MODE_DOWN ? j - 2 * par : j;
      for (int n = 0; n < a.y.nt && n < 4; ++n) {
        const int dl = ((j + n) << (a.y.sshift + 1)) + a.y.soff - pd, w = a.y.w2 - (dl < 0 ? -dl : dl);
        a.wv[par][n] = w > 0 ? w : 0;
      }
    }
  }
  const bool s16 = ses == 2, d16 = des == 2;
  if (!s16 && !d16) launch_typed<uint8_t, uint8_t>(stream, a, mode, n_frames);
  else if (!s16 && d16) launch_typed<uint8_t, uint16_t>(stream, a, mode, n_frames);
  else if (s16 && !d16) launch_typed<uint16_t, uint8_t>(stream, a, mode, n_frames);
  else launch_typed<uint16_t, uint16_t>(stream, a, mode, n_frames);
  return hipGetLastError();
}

}  // namespace pqa
