// Spatial alignment: shifted-window luma SSE (pqa_shift_sse / pqa_shift_sse_device; restated in tests/spatial_align_ref.py).
//
//   S[j][i] = sum_{y=R}^{H-R-1} sum_{x=R}^{W-R-1} (ref[y][x] - dis[y + dy][x + dx])^2,  dy = j - R,  dx = i - R,  0 <= R <= 16
//
// The reference window is the same for every shift; window pixel (wx, wy) is reference pixel (R + wx, R + wy) and meets
// captured pixel (wx + i, wy + j).  sum (r - d)^2 = sum r^2 + sum d^2 - 2 sum r d, and only the cross term needs the tiling:
//
// Cross term (shift_cross_kernel).  A workgroup of 256 threads owns a tile of 8 strips x 256 rows of the window; a strip is
// four packed words (16 samples at 8 bit, 8 at 10 / 12 bit), so the tile is 128 x 256 or 64 x 256 pixels.  Thread (sx, sy),
// sy = tid & 31, keeps the strip sx of the rows sy, sy + 32, ... sy + 224 in 32 registers.  The captured tile with its halo
// (256 + 2R rows, 32 + nq words a row, nq = ceil((2R + 1) / samples per word)) is read from memory once into LDS; every shift
// is evaluated from there: for each dy and each word offset q a thread reads five words a row and forms the byte-shifted
// operand with v_alignbyte_b32, so one pass yields the four (two) shifts dx = 4q ... 4q + 3 (2q, 2q + 1).  8 bit: centred
// samples x' = x ^ 0x80 and v_dot4_i32_i8.  10 / 12 bit: plain u16 products, plain integer VALU.  The LDS row pitch is an odd
// number of words and the 32 lanes of a half wave read 32 consecutive rows at one x, so a ds_read_b32 (bank = word mod 32,
// conflicts inside a 32-lane half only) meets 32 different banks whatever the byte shift.
// Zero padding: a window pixel outside the window (partial last tiles, row tails) is zero IN THE OPERAND WORD of the reference
// (centred domain at 8 bit), so its product vanishes whatever the captured word holds; captured words beyond the frame are
// zero too and are never read from memory.
// Square terms.  sum r^2 rides along in the cross kernel (one more slot of the partial vector).  sum d^2 over the shifted
// windows: shift_rowsq_kernel makes, for every captured row, the 2R + 1 sliding sums of its squares (row total minus the
// i samples in front and the 2R - i behind); the combine kernel slides vertically.
// Overflow: |r'd'| <= 2^14 at 8 bit, and an i32 may take 131 071 of them: a thread adds 128 per shift (2^21), a wave 8192
// (2^27), and the wave's sum is what is stored (i32).  A u16 product is < 2^24 and a u32 takes 256 of them: a thread adds 64
// (< 2^30), is widened to 64 bit BEFORE the wave reduction, and the wave's sum is stored as int64.  Row sums of squares and
// everything the combine kernel does are 64-bit.
// Determinism: no atomics; one partial vector per (frame, tile, wave), summed by the combine kernel in int64.  Integer sums
// do not depend on order, base address, row pitch or tail.
#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int kStripWords = 4;     // packed words of one row a thread keeps
constexpr int kStripsX = 8;        // strips across a tile
constexpr int kLanesY = 32;        // threads down a tile: one 32-lane half wave reads 32 consecutive LDS rows
constexpr int kRowsPerThread = 8;
constexpr int kTileRows = kLanesY * kRowsPerThread;    // 256
constexpr int kTileWords = kStripsX * kStripWords;     // 32

template <typename T> struct Samp;
template <> struct Samp<uint8_t> { static constexpr int spw = 4; static constexpr unsigned centre = 0x80808080u; using Acc = int; };
template <> struct Samp<uint16_t> { static constexpr int spw = 2; static constexpr unsigned centre = 0u; using Acc = long long; };

// one packed word of the samples x ... x + spw - 1 of a row (centred at 8 bit); samples at or beyond xlim are zero
template <typename T>
__device__ __forceinline__ unsigned load_word(const T* __restrict__ row, int x, int xlim, bool aligned) {
  constexpr int spw = Samp<T>::spw;
  if (x >= xlim) return 0u;
  if (aligned && x + spw <= xlim) return *reinterpret_cast<const unsigned*>(row + x) ^ Samp<T>::centre;
  unsigned wd = 0;
#pragma unroll
  for (int b = 0; b < spw; ++b)
    if (x + b < xlim) wd |= ((unsigned)row[x + b] ^ (Samp<T>::centre & 0xffu)) << (8 * (int)sizeof(T) * b);
  return wd;
}

struct ShiftArgs {
  const void* ref;
  const void* dis;
  int64_t ref_rp, ref_fp, dis_rp, dis_fp;   // elements
  int w, h, R, tiles_x, tiles_y, nq, pitch, nsp;   // pitch: LDS words a row; nsp: slots of a partial vector
  int aligned_ref, aligned_dis;
  void* part;   // [frame][tile][wave][nsp], Acc
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void shift_cross_kernel(const ShiftArgs a) {
  extern __shared__ unsigned tile[];   // (kTileRows + 2R) rows of a.pitch words
  constexpr int spw = Samp<T>::spw;
  using Acc = typename Samp<T>::Acc;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, f = blockIdx.y;
  const int R = a.R, wc = a.w - 2 * R, hc = a.h - 2 * R;
  const int wx0 = tx * kTileWords * spw, wy0 = ty * kTileRows;   // window coordinates of the tile
  const T* pr = (const T*)a.ref + (int64_t)f * a.ref_fp;
  const T* pd = (const T*)a.dis + (int64_t)f * a.dis_fp;

  // the captured tile and its halo: frame rows wy0 ..., frame samples wx0 ...; zero beyond the frame
  const int n_rows = kTileRows + 2 * R, n_words = kTileWords + a.nq + 1;   // n_words <= a.pitch
  for (int row = wv; row < n_rows; row += kBlock / 64) {
    const int y = wy0 + row;
    const T* src = pd + (int64_t)y * a.dis_rp;
    for (int wd = lane; wd < n_words; wd += 64)
      tile[row * a.pitch + wd] = y < a.h ? load_word<T>(src, wx0 + wd * spw, a.w, a.aligned_dis) : 0u;
  }

  // the reference strip: window pixel (wx, wy) = frame pixel (R + wx, R + wy); zero outside the window
  const int sy = tid & (kLanesY - 1), sx = tid / kLanesY;
  unsigned ref[kRowsPerThread][kStripWords];
#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int wy = wy0 + r * kLanesY + sy;
    const T* src = pr + (int64_t)(R + wy) * a.ref_rp;
#pragma unroll
    for (int k = 0; k < kStripWords; ++k)
      ref[r][k] = wy < hc ? load_word<T>(src, R + wx0 + (sx * kStripWords + k) * spw, R + wc, a.aligned_ref) : 0u;
  }
  __syncthreads();

  Acc* part = (Acc*)a.part + (((int64_t)f * gridDim.x + blockIdx.x) * (kBlock / 64) + wv) * a.nsp;
  const int nqs = a.nq * spw;   // shifts a row of the partial vector holds (>= 2R + 1)
  {   // sum r^2
    unsigned s = 0;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r)
#pragma unroll
      for (int k = 0; k < kStripWords; ++k) {
        if constexpr (spw == 4) s = (unsigned)__builtin_amdgcn_sdot4((int)ref[r][k], (int)ref[r][k], (int)s, false);
        else s += (ref[r][k] & 0xffffu) * (ref[r][k] & 0xffffu) + (ref[r][k] >> 16) * (ref[r][k] >> 16);
      }
    const Acc t = wave_sum((Acc)s);
    if (lane == 0) part[(2 * R + 1) * nqs] = t;
  }
  for (int j = 0; j <= 2 * R; ++j) {
    for (int q = 0; q < a.nq; ++q) {
      const unsigned* base = tile + (sy + j) * a.pitch + sx * kStripWords + q;
      if constexpr (spw == 4) {
        int acc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) {
          const unsigned* lrow = base + r * kLanesY * a.pitch;
          unsigned wd[kStripWords + 1];
#pragma unroll
          for (int k = 0; k <= kStripWords; ++k) wd[k] = lrow[k];
#pragma unroll
          for (int k = 0; k < kStripWords; ++k) {
            acc[0] = __builtin_amdgcn_sdot4((int)ref[r][k], (int)wd[k], acc[0], false);
#pragma unroll
            for (int b = 1; b < 4; ++b)
              acc[b] = __builtin_amdgcn_sdot4((int)ref[r][k], (int)__builtin_amdgcn_alignbyte(wd[k + 1], wd[k], b), acc[b], false);
          }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int t = wave_sum(acc[b]);
          if (lane == 0) part[j * nqs + 4 * q + b] = t;
        }
      } else {
        unsigned acc[2] = {0, 0};
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) {
          const unsigned* lrow = base + r * kLanesY * a.pitch;
          unsigned wd[kStripWords + 1];
#pragma unroll
          for (int k = 0; k <= kStripWords; ++k) wd[k] = lrow[k];
#pragma unroll
          for (int k = 0; k < kStripWords; ++k) {
            const unsigned r0 = ref[r][k] & 0xffffu, r1 = ref[r][k] >> 16;
            const unsigned d1 = __builtin_amdgcn_alignbyte(wd[k + 1], wd[k], 2);
            acc[0] += r0 * (wd[k] & 0xffffu) + r1 * (wd[k] >> 16);
            acc[1] += r0 * (d1 & 0xffffu) + r1 * (d1 >> 16);
          }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const long long t = wave_sum((long long)acc[b]);   // widened before the lanes are added
          if (lane == 0) part[j * nqs + 2 * q + b] = t;
        }
      }
    }
  }
}

// rowsq[(f * h + y) * (2R + 1) + i] = sum_{x=i}^{i + W - 2R - 1} d'[y][x]^2 (d' centred at 8 bit); one wave per row
template <typename T>
__global__ __launch_bounds__(kBlock) void shift_rowsq_kernel(const T* __restrict__ dis, int64_t rp, int64_t fp, int w, int h, int R,
                                                             unsigned long long* __restrict__ rowsq) {
  constexpr int c = sizeof(T) == 1 ? 128 : 0;
  const int lane = threadIdx.x & 63, y = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), f = blockIdx.y;
  if (y >= h) return;
  const T* row = dis + (int64_t)f * fp + (int64_t)y * rp;
  unsigned long long s = 0;
  for (int x = lane; x < w; x += 64) {
    const int v = (int)row[x] - c;
    s += (unsigned)(v * v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane <= 2 * R) {
    for (int x = 0; x < lane; ++x) {
      const int v = (int)row[x] - c;
      s -= (unsigned)(v * v);
    }
    for (int x = lane + w - 2 * R; x < w; ++x) {
      const int v = (int)row[x] - c;
      s -= (unsigned)(v * v);
    }
    rowsq[((int64_t)f * h + y) * (2 * R + 1) + lane] = s;
  }
}

// S[f][j][i] = sum r^2 + (sum over rows j ... j + H - 2R - 1 of rowsq[.][i]) - 2 (cross term), all partial vectors in int64
template <typename Acc>
__global__ __launch_bounds__(kBlock) void shift_combine_kernel(const Acc* __restrict__ part, int n_parts, int nsp, int nqs,
                                                               const unsigned long long* __restrict__ rowsq, int h, int R,
                                                               unsigned long long* __restrict__ out) {
  __shared__ long long red[kBlock / 64][64];
  const int j = blockIdx.x, f = blockIdx.y, i = threadIdx.x & 63, g = threadIdx.x >> 6, n = 2 * R + 1;
  long long s = 0;
  if (i < n) {
    for (int y = j + g; y < j + h - 2 * R; y += kBlock / 64) s += (long long)rowsq[((int64_t)f * h + y) * n + i];
    for (int p = g; p < n_parts; p += kBlock / 64) {
      const Acc* v = part + ((int64_t)f * n_parts + p) * nsp;
      s += (long long)v[n * nqs] - 2 * (long long)v[j * nqs + i];
    }
  }
  red[g][i] = s;
  __syncthreads();
  if (g == 0 && i < n) out[((int64_t)f * n + j) * n + i] = (unsigned long long)((red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
}

struct Geom {
  int spw, tiles_x, tiles_y, nq, pitch, nsp;
};

Geom geom(Elem elem, int w, int h, int R) {
  Geom g;
  g.spw = elem == ELEM_U8 ? 4 : 2;
  g.tiles_x = (w - 2 * R + kTileWords * g.spw - 1) / (kTileWords * g.spw);
  g.tiles_y = (h - 2 * R + kTileRows - 1) / kTileRows;
  g.nq = (2 * R + 1 + g.spw - 1) / g.spw;
  g.pitch = (kTileWords + g.nq + 1) | 1;
  g.nsp = (2 * R + 1) * g.nq * g.spw + 4;
  return g;
}

template <typename T>
hipError_t launch_t(hipStream_t stream, const Geom& g, const void* ref, int64_t ref_rp, int64_t ref_fp, const void* dis,
                    int64_t dis_rp, int64_t dis_fp, int n_frames, int w, int h, int R, void* part, unsigned long long* rowsq,
                    unsigned long long* out) {
  using Acc = typename Samp<T>::Acc;
  constexpr int es = sizeof(T);
  ShiftArgs a{};
  a.ref = ref; a.dis = dis; a.ref_rp = ref_rp; a.ref_fp = ref_fp; a.dis_rp = dis_rp; a.dis_fp = dis_fp;
  a.w = w; a.h = h; a.R = R; a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y; a.nq = g.nq; a.pitch = g.pitch; a.nsp = g.nsp;
  // a word load needs a 4-byte address: the tile origin is a whole number of words, the window origin R samples further
  a.aligned_ref = (uintptr_t)ref % 4 == 0 && (ref_rp * es) % 4 == 0 && (ref_fp * es) % 4 == 0 && (R * es) % 4 == 0;
  a.aligned_dis = (uintptr_t)dis % 4 == 0 && (dis_rp * es) % 4 == 0 && (dis_fp * es) % 4 == 0;
  a.part = part;
  const int n_tiles = g.tiles_x * g.tiles_y;
  const size_t lds = (size_t)(kTileRows + 2 * R) * g.pitch * sizeof(unsigned);
  hipLaunchKernelGGL((shift_rowsq_kernel<T>), dim3((h + kBlock / 64 - 1) / (kBlock / 64), n_frames), dim3(kBlock), 0, stream,
                     (const T*)dis, dis_rp, dis_fp, w, h, R, rowsq);
  hipLaunchKernelGGL((shift_cross_kernel<T>), dim3(n_tiles, n_frames), dim3(kBlock), lds, stream, a);
  hipLaunchKernelGGL((shift_combine_kernel<Acc>), dim3(2 * R + 1, n_frames), dim3(kBlock), 0, stream, (const Acc*)part,
                     n_tiles * (kBlock / 64), g.nsp, g.nq * g.spw, rowsq, h, R, out);
  return hipGetLastError();
}

}  // namespace

size_t shift_part_bytes(Elem elem, int w, int h, int R, int n_frames) {
  const Geom g = geom(elem, w, h, R);
  return (size_t)n_frames * g.tiles_x * g.tiles_y * (kBlock / 64) * g.nsp * (elem == ELEM_U8 ? sizeof(int) : sizeof(long long));
}

size_t shift_rowsq_bytes(int h, int R, int n_frames) { return (size_t)n_frames * h * (2 * R + 1) * sizeof(unsigned long long); }

hipError_t launch_shift_sse(hipStream_t stream, Elem elem, const void* ref, int64_t ref_row_pitch, int64_t ref_frame_pitch,
                            const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch, int n_frames, int w, int h, int R,
                            void* part, unsigned long long* rowsq, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  if (R < 0 || R > kShiftMaxRadius || w <= 2 * R || h <= 2 * R) return hipErrorInvalidValue;
  const Geom g = geom(elem, w, h, R);
  if (elem == ELEM_U8)
    return launch_t<uint8_t>(stream, g, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, n_frames, w, h,
                             R, part, rowsq, out);
  if (elem == ELEM_U16)
    return launch_t<uint16_t>(stream, g, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, n_frames, w,
                              h, R, part, rowsq, out);
  return hipErrorInvalidValue;
}

}  // namespace pqa
