// Colour-matrix alignment: the cross-plane moments of frame pairs (pqa_colour_moments / pqa_colour_moments_device) and the
// kernel that applies a 3 x 4 integer matrix to a frame (pqa_colour_apply / pqa_colour_apply_device).  Restated in
// tests/colour_ref.py; the solver is pqa2_amd/align.py (best_colour, colour_correction).
//
// Both work on the chroma grid: chroma planes of cw x ch = ceil(w / 2^hs) x ceil(h / 2^vs) samples, s = 2^(hs + vs).  For a
// chroma sample c = (cx, cy), SY(c) is the integer sum of the 2^hs x 2^vs luma samples it covers, luma coordinates clamped to
// the plane (a partial edge block of an odd-sized frame still has s terms: the replication ciede.hip uses for chroma, read
// the other way round).  A sample above top = 2^bits - 1 (a u16 container can hold one) is read as top.
//
// Moments.  z(c) = (1, SYr, Ur, Vr, SYd, Ud, Vd); out[f][28] = the upper triangle of sum_c z z^T, row-major, exact uint64;
// entry 0 counts the samples that entered.  A sample enters only if every captured luma sample under it, Ud and Vd lie in
// [lo, hi] (the capture chain clips after it converts, and clipped samples bias a linear fit); reference samples are never
// masked.
//
// Work.  A workgroup of 256 threads owns a tile of kColTileW x kColTileH = 256 x 32 chroma samples of one frame pair; wave wv
// walks the chroma rows wv, wv + 4, ... of the tile, a lane four neighbouring chroma samples of a row and the luma block
// under them, of both clips.  When every base address and pitch is a multiple of 16 bytes (the host entries stage that way)
// a lane whose four samples and their luma lie inside the planes reads them with one load a row and plane (4 ... 16 bytes);
// every other lane -- the right edge, or the whole launch when something is unaligned -- reads sample by sample with clamped
// coordinates.  Nothing outside a plane is touched either way.
// Sums.  Every component of z is at most M = s * top <= 4 * 4095 = 16380 < 2^15: an int16.  Two samples of a lane are packed
// into one dword per component, and an entry's contribution of the pair is one v_dot2_i32_i16 (27 of them a pair; entry 0 is
// a count).  A dot adds at most 2 M^2 to a lane's int32 partial, so the partials are widened into the lane's uint64 sums
// every `flush` row steps of two pairs, flush = floor(floor((2^31 - 1) / (2 M^2)) / 2) >= 1, worked out by the launcher from
// the bit depth and s: 516 steps at 8 bit 4:2:0, 2 at 12 bit 4:2:0 (2 M^2 = 536 608 800 is a quarter of 2^31).  A wave makes
// at most kColTileH / 4 = 8 steps.  uint64: an entry is at most M^2 a sample, times at most 16384^2 / s samples of a plane
// = 16384^2 * s * top^2 < 2^28 * 2^2 * 2^24 = 2^54.
// Merge.  The 28 (padded to 32) sums of a wave's lanes are reduced by a butterfly that halves the number of values a lane
// keeps at every step (32 exchanges in place of 6 * 28), the four waves meet in LDS, and the workgroup adds its 28 sums to the
// zeroed output with 64-bit integer atomics.  Sums of integers do not depend on order; no floating point anywhere.
//
// Apply.  m[3][4] in Q14, column 0 the offset in Q14 code values; |m[r][0]| < 2^28, |m[r][1..3]| < 2^16 (the entries refuse
// anything else):
//   Y'(x, y) = clamp((m00 + m01 Y(x, y) + m02 U(c) + m03 V(c) + 2^13) >> 14, 0, top),   c = (x >> hs, y >> vs)
//   U'(c)    = clamp((m10 s + m11 SY(c) + s m12 U(c) + s m13 V(c) + s 2^13) >> (14 + hs + vs), 0, top),   V' with row 2
// Luma in int32: |m00| < 2^28 and three products below 2^16 * 2^12 each, plus 2^13, stay below 2^31.  Chroma in int64.  The
// shifts are arithmetic.  A workgroup owns 256 x 16 chroma samples and the luma under them; every input sample is read once
// (a clamped edge sample again by its own lane), every output sample written once, rows and columns outside a plane never.
#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kColLane = 4;                  // chroma samples of a lane and row
constexpr int kColTileW = 64 * kColLane;     // chroma columns of a workgroup
constexpr int kColTileH = 32;                // chroma rows of a workgroup of the moments kernel
constexpr int kColApplyH = 16;               // ... of the apply kernel
constexpr int kColSums = 28;

struct ColClip {
  const void* p[3];
  int64_t rp[3], fp[3];   // elements
};

struct ColMomArgs {
  ColClip ref, dis;
  int w, h, cw, ch;
  unsigned lo, hi, top;
  int flush, vec;
  unsigned long long* out;
};

struct ColApplyArgs {
  ColClip src;
  void* dp[3];
  int64_t drp[3], dfp[3];
  int w, h, cw, ch, top, vec;
  int m[12];
};

// What a lane reads of one clip at one chroma row: four chroma samples, the block sums of the luma under them and its
// smallest and largest sample; KEEP: the luma samples themselves too.
template <int HS, int VS, bool KEEP>
struct ColBlock {
  unsigned u[kColLane], v[kColLane], sy[kColLane], mn[kColLane], mx[kColLane];
  unsigned y[KEEP ? (1 << VS) : 1][KEEP ? (kColLane << HS) : 1];
};

template <typename T>
__device__ __forceinline__ unsigned col_sample(T v, unsigned top) {
  if constexpr (sizeof(T) == 1) return v;
  else return min((unsigned)v, top);
}

template <typename T, int HS, int VS, bool KEEP>
__device__ __forceinline__ void col_load(ColBlock<HS, VS, KEEP>& b, const T* Y, const T* U, const T* V, int64_t yrp, int64_t urp,
                                         int64_t vrp, int cx0, int cy, int w, int h, int cw, bool fast, unsigned top) {
  constexpr int NX = kColLane << HS, NY = 1 << VS;
  const int lx0 = cx0 << HS;
  const T* ur = U + (int64_t)cy * urp;
  const T* vr = V + (int64_t)cy * vrp;
  if (fast) {
    const SampleVec<T, kColLane> uu = *reinterpret_cast<const SampleVec<T, kColLane>*>(ur + cx0);
    const SampleVec<T, kColLane> vv = *reinterpret_cast<const SampleVec<T, kColLane>*>(vr + cx0);
#pragma unroll
    for (int k = 0; k < kColLane; ++k) {
      b.u[k] = col_sample(uu.s[k], top);
      b.v[k] = col_sample(vv.s[k], top);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kColLane; ++k) {
      const int cx = min(cx0 + k, cw - 1);
      b.u[k] = col_sample(ur[cx], top);
      b.v[k] = col_sample(vr[cx], top);
    }
  }
#pragma unroll
  for (int k = 0; k < kColLane; ++k) {
    b.sy[k] = 0u;
    b.mn[k] = 0xffffffffu;
    b.mx[k] = 0u;
  }
#pragma unroll
  for (int j = 0; j < NY; ++j) {
    const int ly = min((cy << VS) + j, h - 1);
    const T* row = Y + (int64_t)ly * yrp;
    unsigned s[NX];
    if (fast) {
      const SampleVec<T, NX> r = *reinterpret_cast<const SampleVec<T, NX>*>(row + lx0);
#pragma unroll
      for (int i = 0; i < NX; ++i) s[i] = col_sample(r.s[i], top);
    } else {
#pragma unroll
      for (int i = 0; i < NX; ++i) s[i] = col_sample(row[min(lx0 + i, w - 1)], top);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int k = i >> HS;
      b.sy[k] += s[i];
      b.mn[k] = min(b.mn[k], s[i]);
      b.mx[k] = max(b.mx[k], s[i]);
      if constexpr (KEEP) b.y[j][i] = s[i];
    }
  }
}

typedef short col_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int col_dot2(int a, int b, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(col_s2, a), __builtin_bit_cast(col_s2, b), acc, false);
}

// index of entry (i, j), i <= j, of the row-major upper triangle of a 7 x 7 matrix
__host__ __device__ constexpr int col_idx(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }

template <typename T, int HS, int VS>
__global__ __launch_bounds__(kBlock) void colour_moments_kernel(const ColMomArgs a) {
  __shared__ unsigned long long red[kBlock / 64][32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.z;
  const int cx0 = blockIdx.x * kColTileW + lane * kColLane;
  const int y0 = blockIdx.y * kColTileH, y1 = min(a.ch, y0 + kColTileH);
  const T* Yr = (const T*)a.ref.p[0] + (int64_t)f * a.ref.fp[0];
  const T* Ur = (const T*)a.ref.p[1] + (int64_t)f * a.ref.fp[1];
  const T* Vr = (const T*)a.ref.p[2] + (int64_t)f * a.ref.fp[2];
  const T* Yd = (const T*)a.dis.p[0] + (int64_t)f * a.dis.fp[0];
  const T* Ud = (const T*)a.dis.p[1] + (int64_t)f * a.dis.fp[1];
  const T* Vd = (const T*)a.dis.p[2] + (int64_t)f * a.dis.fp[2];
  const bool live = cx0 < a.cw;
  const bool fast = a.vec && cx0 + kColLane <= a.cw && ((cx0 + kColLane) << HS) <= a.w;

  int acc[kColSums];
  unsigned long long wide[kColSums];
#pragma unroll
  for (int e = 0; e < kColSums; ++e) {
    acc[e] = 0;
    wide[e] = 0ull;
  }
  int since = 0;
  for (int cy = y0 + wv; cy < y1; cy += kBlock / 64) {
    if (live) {
      ColBlock<HS, VS, false> r, d;
      col_load<T, HS, VS, false>(r, Yr, Ur, Vr, a.ref.rp[0], a.ref.rp[1], a.ref.rp[2], cx0, cy, a.w, a.h, a.cw, fast, a.top);
      col_load<T, HS, VS, false>(d, Yd, Ud, Vd, a.dis.rp[0], a.dis.rp[1], a.dis.rp[2], cx0, cy, a.w, a.h, a.cw, fast, a.top);
      unsigned z[kColLane][7];
#pragma unroll
      for (int k = 0; k < kColLane; ++k) {
        const unsigned least = min(min(d.mn[k], d.u[k]), d.v[k]), most = max(max(d.mx[k], d.u[k]), d.v[k]);
        const bool in = cx0 + k < a.cw && least >= a.lo && most <= a.hi;
        z[k][0] = in ? 1u : 0u;
        z[k][1] = in ? r.sy[k] : 0u;
        z[k][2] = in ? r.u[k] : 0u;
        z[k][3] = in ? r.v[k] : 0u;
        z[k][4] = in ? d.sy[k] : 0u;
        z[k][5] = in ? d.u[k] : 0u;
        z[k][6] = in ? d.v[k] : 0u;
      }
#pragma unroll
      for (int pr = 0; pr < kColLane / 2; ++pr) {
        int P[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) P[j] = (int)(z[2 * pr][j] | (z[2 * pr + 1][j] << 16));
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
          for (int j = i; j < 7; ++j) acc[col_idx(i, j)] = col_dot2(P[i], P[j], acc[col_idx(i, j)]);
      }
    }
    if (++since == a.flush) {   // the same for every lane of the wave
      since = 0;
#pragma unroll
      for (int e = 0; e < kColSums; ++e) {
        wide[e] += (unsigned long long)(unsigned)acc[e];
        acc[e] = 0;
      }
    }
  }

  // Butterfly: at step b a lane keeps one half of its values and sends the other half to its partner lane ^ (1 << b).  After
  // five steps a lane holds ONE value, summed over the 32 lanes that share its bit 5; its index is the 5-bit reversal of the lane.
  unsigned long long v[32];
#pragma unroll
  for (int e = 0; e < 32; ++e) v[e] = e < kColSums ? wide[e] + (unsigned long long)(unsigned)acc[e] : 0ull;
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    const int half = 16 >> b;
    const bool up = (lane >> b) & 1;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const unsigned long long keep = up ? v[i + half] : v[i];
      const unsigned long long send = up ? v[i] : v[i + half];
      v[i] = keep + __shfl_xor(send, 1 << b, 64);
    }
  }
  v[0] += __shfl_xor(v[0], 32, 64);
  const int idx = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
  if (lane < 32) red[wv][idx] = v[0];
  __syncthreads();
  if (tid < kColSums) {
    const unsigned long long sum = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (sum) atomicAdd(a.out + (int64_t)f * kColSums + tid, sum);
  }
}

template <typename T, int HS, int VS>
__global__ __launch_bounds__(kBlock) void colour_apply_kernel(const ColApplyArgs a) {
  constexpr int NX = kColLane << HS, NY = 1 << VS, S = 1 << (HS + VS);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.z;
  const int cx0 = blockIdx.x * kColTileW + lane * kColLane, lx0 = cx0 << HS;
  const int y0 = blockIdx.y * kColApplyH, y1 = min(a.ch, y0 + kColApplyH);
  if (cx0 >= a.cw) return;   // no barrier below
  const T* Ys = (const T*)a.src.p[0] + (int64_t)f * a.src.fp[0];
  const T* Us = (const T*)a.src.p[1] + (int64_t)f * a.src.fp[1];
  const T* Vs = (const T*)a.src.p[2] + (int64_t)f * a.src.fp[2];
  T* Yo = (T*)a.dp[0] + (int64_t)f * a.dfp[0];
  T* Uo = (T*)a.dp[1] + (int64_t)f * a.dfp[1];
  T* Vo = (T*)a.dp[2] + (int64_t)f * a.dfp[2];
  const bool fast = a.vec && cx0 + kColLane <= a.cw && ((cx0 + kColLane) << HS) <= a.w;
  for (int cy = y0 + wv; cy < y1; cy += kBlock / 64) {
    ColBlock<HS, VS, true> b;
    col_load<T, HS, VS, true>(b, Ys, Us, Vs, a.src.rp[0], a.src.rp[1], a.src.rp[2], cx0, cy, a.w, a.h, a.cw, fast, (unsigned)a.top);
#pragma unroll
    for (int j = 0; j < NY; ++j) {
      const int ly = (cy << VS) + j;
      if (ly >= a.h) break;
      SampleVec<T, NX> o;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int k = i >> HS;
        const int t = (a.m[0] + a.m[1] * (int)b.y[j][i] + a.m[2] * (int)b.u[k] + a.m[3] * (int)b.v[k] + 8192) >> 14;
        o.s[i] = (T)min(max(t, 0), a.top);
      }
      T* row = Yo + (int64_t)ly * a.drp[0];
      if (fast) {
        *reinterpret_cast<SampleVec<T, NX>*>(row + lx0) = o;
      } else {
#pragma unroll
        for (int i = 0; i < NX; ++i)
          if (lx0 + i < a.w) row[lx0 + i] = o.s[i];
      }
    }
    SampleVec<T, kColLane> ou, ov;
#pragma unroll
    for (int k = 0; k < kColLane; ++k) {
      const long long sy = (long long)b.sy[k], su = (long long)S * b.u[k], sv = (long long)S * b.v[k];
      const long long tu = ((long long)a.m[4] * S + a.m[5] * sy + a.m[6] * su + a.m[7] * sv + (long long)S * 8192) >> (14 + HS + VS);
      const long long tv = ((long long)a.m[8] * S + a.m[9] * sy + a.m[10] * su + a.m[11] * sv + (long long)S * 8192) >> (14 + HS + VS);
      ou.s[k] = (T)min(max(tu, 0ll), (long long)a.top);
      ov.s[k] = (T)min(max(tv, 0ll), (long long)a.top);
    }
    T* urow = Uo + (int64_t)cy * a.drp[1];
    T* vrow = Vo + (int64_t)cy * a.drp[2];
    if (fast) {
      *reinterpret_cast<SampleVec<T, kColLane>*>(urow + cx0) = ou;
      *reinterpret_cast<SampleVec<T, kColLane>*>(vrow + cx0) = ov;
    } else {
#pragma unroll
      for (int k = 0; k < kColLane; ++k)
        if (cx0 + k < a.cw) {
          urow[cx0 + k] = ou.s[k];
          vrow[cx0 + k] = ov.s[k];
        }
    }
  }
}

bool col_aligned(const void* p, int64_t rp, int64_t fp, int es) {
  return (((uint64_t)(uintptr_t)p | (uint64_t)(rp * es) | (uint64_t)(fp * es)) & 15u) == 0;
}

void col_clip(ColClip* c, const PlaneRun run[3]) {
  for (int p = 0; p < 3; ++p) {
    c->p[p] = run[p].base;
    c->rp[p] = run[p].row_pitch;
    c->fp[p] = run[p].frame_pitch;
  }
}

bool col_shape_ok(Elem elem, int bits, int hs, int vs, int w, int h) {
  return w >= 1 && h >= 1 && w <= 16384 && h <= 16384 && (bits == 8 || bits == 10 || bits == 12) && (elem == ELEM_U8) == (bits == 8) &&
         (elem == ELEM_U8 || elem == ELEM_U16) && hs >= 0 && hs <= 1 && vs >= 0 && vs <= 1;
}

template <typename T>
void launch_mom_t(hipStream_t stream, dim3 grid, int hs, int vs, const ColMomArgs& a) {
  if (hs == 1 && vs == 1) hipLaunchKernelGGL((colour_moments_kernel<T, 1, 1>), grid, dim3(kBlock), 0, stream, a);
  else if (hs == 1) hipLaunchKernelGGL((colour_moments_kernel<T, 1, 0>), grid, dim3(kBlock), 0, stream, a);
  else if (vs == 1) hipLaunchKernelGGL((colour_moments_kernel<T, 0, 1>), grid, dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((colour_moments_kernel<T, 0, 0>), grid, dim3(kBlock), 0, stream, a);
}

template <typename T>
void launch_apply_t(hipStream_t stream, dim3 grid, int hs, int vs, const ColApplyArgs& a) {
  if (hs == 1 && vs == 1) hipLaunchKernelGGL((colour_apply_kernel<T, 1, 1>), grid, dim3(kBlock), 0, stream, a);
  else if (hs == 1) hipLaunchKernelGGL((colour_apply_kernel<T, 1, 0>), grid, dim3(kBlock), 0, stream, a);
  else if (vs == 1) hipLaunchKernelGGL((colour_apply_kernel<T, 0, 1>), grid, dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((colour_apply_kernel<T, 0, 0>), grid, dim3(kBlock), 0, stream, a);
}

}  // namespace

bool colour_shift_ok(int hshift, int vshift) { return hshift >= 0 && hshift <= 1 && vshift >= 0 && vshift <= 1; }

bool colour_matrix_ok(const int32_t m[12]) {
  for (int i = 0; i < 12; ++i) {
    const int64_t lim = i % 4 == 0 ? kColourMaxOffset : kColourMaxGain;
    if (m[i] <= -lim || m[i] >= lim) return false;
  }
  return true;
}

int colour_flush_steps(int bit_depth, int hshift, int vshift) {
  const int64_t M = (int64_t)(((1 << bit_depth) - 1)) << (hshift + vshift);
  return (int)((INT32_MAX / (2 * M * M)) / (kColLane / 2));
}

hipError_t launch_colour_moments(hipStream_t stream, Elem elem, int bit_depth, int hshift, int vshift, const PlaneRun ref[3],
                                 const PlaneRun dis[3], int n_frames, int w, int h, unsigned lo, unsigned hi,
                                 unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  if (!col_shape_ok(elem, bit_depth, hshift, vshift, w, h) || n_frames > 65535) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(out, 0, (size_t)n_frames * kColSums * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  const int es = elem == ELEM_U8 ? 1 : 2;
  ColMomArgs a{};
  col_clip(&a.ref, ref);
  col_clip(&a.dis, dis);
  a.w = w; a.h = h;
  a.cw = (w + (1 << hshift) - 1) >> hshift;
  a.ch = (h + (1 << vshift) - 1) >> vshift;
  a.lo = lo; a.hi = hi; a.top = (1u << bit_depth) - 1u;
  a.flush = colour_flush_steps(bit_depth, hshift, vshift);
  if (a.flush < 1) return hipErrorInvalidValue;   // cannot happen for the shapes above: 2 at 12 bit 4:2:0
  a.vec = 1;
  for (int p = 0; p < 3; ++p)
    a.vec &= col_aligned(ref[p].base, ref[p].row_pitch, ref[p].frame_pitch, es) && col_aligned(dis[p].base, dis[p].row_pitch, dis[p].frame_pitch, es);
  a.out = out;
  const dim3 grid((a.cw + kColTileW - 1) / kColTileW, (a.ch + kColTileH - 1) / kColTileH, n_frames);
  if (elem == ELEM_U8) launch_mom_t<uint8_t>(stream, grid, hshift, vshift, a);
  else launch_mom_t<uint16_t>(stream, grid, hshift, vshift, a);
  return hipGetLastError();
}

hipError_t launch_colour_apply(hipStream_t stream, Elem elem, int bit_depth, int hshift, int vshift, const int32_t m[12],
                               const PlaneRun src[3], const MutPlaneRun dst[3], int n_frames, int w, int h) {
  if (n_frames <= 0) return hipSuccess;
  if (!col_shape_ok(elem, bit_depth, hshift, vshift, w, h) || n_frames > 65535 || !colour_matrix_ok(m)) return hipErrorInvalidValue;
  const int es = elem == ELEM_U8 ? 1 : 2;
  ColApplyArgs a{};
  col_clip(&a.src, src);
  a.w = w; a.h = h;
  a.cw = (w + (1 << hshift) - 1) >> hshift;
  a.ch = (h + (1 << vshift) - 1) >> vshift;
  a.top = (1 << bit_depth) - 1;
  a.vec = 1;
  for (int p = 0; p < 3; ++p) {
    a.dp[p] = dst[p].base; a.drp[p] = dst[p].row_pitch; a.dfp[p] = dst[p].frame_pitch;
    a.vec &= col_aligned(src[p].base, src[p].row_pitch, src[p].frame_pitch, es) && col_aligned(dst[p].base, dst[p].row_pitch, dst[p].frame_pitch, es);
  }
  for (int i = 0; i < 12; ++i) a.m[i] = m[i];
  const dim3 grid((a.cw + kColTileW - 1) / kColTileW, (a.ch + kColApplyH - 1) / kColApplyH, n_frames);
  if (elem == ELEM_U8) launch_apply_t<uint8_t>(stream, grid, hshift, vshift, a);
  else launch_apply_t<uint16_t>(stream, grid, hshift, vshift, a);
  return hipGetLastError();
}

}  // namespace pqa
