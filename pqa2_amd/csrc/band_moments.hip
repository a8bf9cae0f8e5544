// Distortion spectrum: the second moments of the unnormalised Haar octave bands of a frame pair (pqa_band_moments /
// pqa_band_moments_device; restated in tests/spectrum_ref.py; the solver is pqa2_amd/spectrum.py).  With A_0 the plane (a u16
// sample above top = 2^bits - 1 is read as top), for l = 1 ... L, W_l = W >> l, H_l = H >> l, 0 <= i < W_l, 0 <= j < H_l and
// a = A_{l-1}[2j][2i], b = A_{l-1}[2j][2i+1], c = A_{l-1}[2j+1][2i], e = A_{l-1}[2j+1][2i+1]:
//
//   A_l = a + b + c + e     H_l = a - b + c - e     V_l = a + b - c - e     D_l = a - b - c + e
//   out[f][l-1][o][0..2] = sum r_o^2, sum d_o^2, sum r_o d_o     o: 0 H, 1 V, 2 D, 3 A
//
// over the level's W_l * H_l coefficients, exact (the third as int64 in two's complement).  Nothing is divided or rounded.
//
// Work.  A WAVE owns a block of 64 x 64 pixels, which holds the whole support of every coefficient of the six levels that
// starts in it: no halo, no neighbour.  A workgroup of 256 threads is four such blocks, 128 x 128 pixels.  A lane owns 16 bytes
// of R consecutive rows of both planes -- 16 x 4 samples of u8, 8 x 8 of u16 -- by one 16-byte load, four 4-byte loads or sample
// by sample, whichever the base addresses and pitches of BOTH planes allow (load_bytes of plane_scan.h).  A lane whose
// 16 bytes would cross the end of the row reads sample by sample with the index held at the row's last sample, and a row
// below the plane is read as the plane's last row: every address is a real sample's, nothing past a row's last sample is
// touched.  Padding is NOT neutral for a Haar difference (a zero next to a sample is an edge), so nothing that was not
// there reaches a sum: a coefficient (i, j) of level l counts only when i < W_l and j < H_l, that is when its 2^l x 2^l
// support is inside the plane, and a coefficient that counts reads real samples only (its four parents count too).
// Levels 1 ... 2 (u8) or 1 ... 3 (u16) lie inside a lane's own samples and are formed in registers.  The u8 lanes then hold
// four A_2 of one row; lanes l and l ^ 4 hold the rows of a pair and exchange their horizontal sums and differences, each
// forms one coefficient of level 3, and one more move puts A_3 (i, j) on lane 8 j + i, where the u16 lanes have it already.
// From there a level with a G x G grid of parents on lanes G j + i is formed on the lanes below (G / 2)^2 from four cross-lane
// moves a plane.  No LDS holds a sample or a coefficient.
// Widening.  Products are formed in 64 bits (|coefficient| <= top 4^l < 2^24), except a u8 lane's levels 1 and 2: its 16
// coefficients of level 1 are at most 1020 and its 4 of level 2 at most 4080 in magnitude, so a lane's sums stay below
// 16 * 1020^2 < 2^24 and 4 * 4080^2 < 2^27 in int32 and are widened once, before the wave adds them up (a wave's level 2 can
// reach 256 * 4080^2 > 2^32).  Everything a wave, a workgroup and the frame add up is int64: a band sum is at most
// top^2 W H 4^l < 2^62.
// Reduction, in a fixed order and without atomics: the lanes that hold a level's coefficients add their twelve sums with xor
// moves, lane 0 of the wave writes them to LDS, after a barrier a thread per sum adds the four waves and stores the
// workgroup's partial; band_finish_kernel adds the partials of a frame, a wave per sum, and writes every output word once: no
// zeroing.  Integer sums: the result does not depend on order, base address, pitch, load width or launch shape.  No floating
// point anywhere.
#include <type_traits>

#include "plane_scan.h"

namespace pqa {
namespace {

constexpr int kBandBlock = 64;             // pixels a wave covers each way
constexpr int kBandGroup = 2 * kBandBlock; // pixels a workgroup covers each way
constexpr int kBandMaxLevels = 6;
constexpr int kBandWords = 4 * kBandSums;  // sums a level: 12

struct BandArgs : PairPlanes {
  int levels, gx, gy;
  unsigned top;
  long long* part;   // [frame][gy][gx][levels][4][3]
};

// sample k of a lane's row, clamped
template <typename T>
__device__ __forceinline__ int band_sample(const PackedQuad& q, int k, unsigned top) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  const unsigned s = (q.d[k / PER] >> (BITS * (k % PER))) & ((1u << BITS) - 1u);
  return (int)(sizeof(T) == 1 ? s : (s < top ? s : top));
}

// the twelve sums of one level: [o][k], o: H V D A, k: r^2 d^2 r d
template <typename Acc>
__device__ __forceinline__ void band_add(Acc (&acc)[kBandWords], bool on, const int (&r)[4], const int (&d)[4]) {
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const Acc rv = on ? r[o] : 0, dv = on ? d[o] : 0;
    acc[o * 3 + 0] += rv * rv;
    acc[o * 3 + 1] += dv * dv;
    acc[o * 3 + 2] += rv * dv;
    // an empty statement that pins the running sums: left free, the compiler adds up band by band and keeps every
    // coefficient of the level alive until the last band (182 ... 256 VGPRs instead of 105 ... 161)
    asm volatile("" : "+v"(acc[o * 3 + 0]), "+v"(acc[o * 3 + 1]), "+v"(acc[o * 3 + 2]));
  }
}

// H V D A of the four parents a b / c e
__device__ __forceinline__ void band_haar(int a, int b, int c, int e, int (&o)[4]) {
  const int s0 = a + b, t0 = a - b, s1 = c + e, t1 = c - e;
  o[0] = t0 + t1; o[1] = s0 - s1; o[2] = t0 - t1; o[3] = s0 + s1;
}

// level 3 of the u8 lanes: x holds four A_2 of one row, the row's partner is on lane ^ 4 (`low`: this lane holds the lower
// row).  The upper lane forms the coefficient of x[0] x[1], the lower that of x[2] x[3]: each sends the sum and difference of
// the pair the other one forms.
template <int N>
__device__ __forceinline__ void band_pair_rows(const int (&x)[N], bool low, int (&o)[4]) {
  const int s0 = x[0] + x[1], t0 = x[0] - x[1], s1 = x[2] + x[3], t1 = x[2] - x[3];
  const int gs = __shfl_xor(low ? s0 : s1, 4, 64), gt = __shfl_xor(low ? t0 : t1, 4, 64);
  const int ms = low ? s1 : s0, mt = low ? t1 : t0;
  const int ts = low ? gs : ms, bs = low ? ms : gs, tt = low ? gt : mt, bt = low ? mt : gt;   // top / bottom row
  o[0] = tt + bt; o[1] = ts - bs; o[2] = tt - bt; o[3] = ts + bs;
}

// adds the sums over the wave's first `lanes` lanes (a power of two; the others hold zeros or are not read) and leaves the
// level's twelve words in sh on lane 0
template <int LANES>
__device__ __forceinline__ void band_reduce(long long (&acc)[kBandWords], int lane, long long* sh) {
#pragma unroll
  for (int m = 0; m < kBandWords; ++m) {
    long long v = acc[m];
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) sh[m] = v;
  }
}

// a level across the lanes: the G x G parents on lanes G j + i become (G / 2)^2 sums on the lanes below that, in the same order
template <int G>
__device__ __forceinline__ void band_cross(int& ar, int& ad, int lv, int lane, int bx0, int by0, int w, int h, long long* sh) {
  constexpr int G2 = G / 2, N = G2 * G2;
  const int i = lane % G2, j = (lane / G2) % G2, src = 2 * j * G + 2 * i;
  int ro[4], dd[4];
  band_haar(__shfl(ar, src, 64), __shfl(ar, src + 1, 64), __shfl(ar, src + G, 64), __shfl(ar, src + G + 1, 64), ro);
  band_haar(__shfl(ad, src, 64), __shfl(ad, src + 1, 64), __shfl(ad, src + G, 64), __shfl(ad, src + G + 1, 64), dd);
  long long acc[kBandWords];
#pragma unroll
  for (int m = 0; m < kBandWords; ++m) acc[m] = 0;
  band_add<long long>(acc, lane < N && (bx0 >> lv) + i < (w >> lv) && (by0 >> lv) + j < (h >> lv), ro, dd);
  ar = ro[3];
  ad = dd[3];
  band_reduce<N>(acc, lane, sh);
}

// level 1 inside a lane: R packed rows of S samples become R/2 x S/2 sums in r / d; (cx, cy): the lane's first coefficient
// of this level in the plane
template <typename T, typename Acc, int R, int S>
__device__ __forceinline__ void band_lane_first(const PackedQuad (&qr)[R], const PackedQuad (&qd)[R], unsigned top, int (&r)[R / 2][S / 2],
                                                int (&d)[R / 2][S / 2], int cx, int cy, int wl, int hl, long long (&acc)[kBandWords]) {
  Acc part[kBandWords];
#pragma unroll
  for (int m = 0; m < kBandWords; ++m) part[m] = 0;
#pragma unroll
  for (int j = 0; j < R / 2; ++j)
#pragma unroll
    for (int i = 0; i < S / 2; ++i) {
      int ro[4], dd[4];
      band_haar(band_sample<T>(qr[2 * j], 2 * i, top), band_sample<T>(qr[2 * j], 2 * i + 1, top),
                band_sample<T>(qr[2 * j + 1], 2 * i, top), band_sample<T>(qr[2 * j + 1], 2 * i + 1, top), ro);
      band_haar(band_sample<T>(qd[2 * j], 2 * i, top), band_sample<T>(qd[2 * j], 2 * i + 1, top),
                band_sample<T>(qd[2 * j + 1], 2 * i, top), band_sample<T>(qd[2 * j + 1], 2 * i + 1, top), dd);
      band_add<Acc>(part, cx + i < wl && cy + j < hl, ro, dd);
      r[j][i] = ro[3];
      d[j][i] = dd[3];
    }
#pragma unroll
  for (int m = 0; m < kBandWords; ++m) acc[m] = part[m];
}

// a deeper level inside a lane: the W x H parents in the top left of r / d become W/2 x H/2 sums there
template <typename Acc, int W, int H, int RR, int SS>
__device__ __forceinline__ void band_lane_level(int (&r)[RR][SS], int (&d)[RR][SS], int cx, int cy, int wl, int hl,
                                                long long (&acc)[kBandWords]) {
  Acc part[kBandWords];
#pragma unroll
  for (int m = 0; m < kBandWords; ++m) part[m] = 0;
#pragma unroll
  for (int j = 0; j < H / 2; ++j)
#pragma unroll
    for (int i = 0; i < W / 2; ++i) {
      int ro[4], dd[4];
      band_haar(r[2 * j][2 * i], r[2 * j][2 * i + 1], r[2 * j + 1][2 * i], r[2 * j + 1][2 * i + 1], ro);
      band_haar(d[2 * j][2 * i], d[2 * j][2 * i + 1], d[2 * j + 1][2 * i], d[2 * j + 1][2 * i + 1], dd);
      band_add<Acc>(part, cx + i < wl && cy + j < hl, ro, dd);
      r[j][i] = ro[3];
      d[j][i] = dd[3];
    }
#pragma unroll
  for (int m = 0; m < kBandWords; ++m) acc[m] = part[m];
}

// VB: bytes of one load
template <typename T, int VB>
__global__ __launch_bounds__(kBlock) void band_moments_kernel(const BandArgs a) {
  constexpr int S = 16 / (int)sizeof(T);     // samples of a lane's row: 16 / 8
  constexpr int LPR = kBandBlock / S;        // lanes a row of the block: 4 / 8
  constexpr int R = kBandBlock / (64 / LPR);   // rows of a lane: 4 / 8
  using Narrow = typename std::conditional<sizeof(T) == 1, int, long long>::type;
  __shared__ long long sh[kBlock / 64][kBandMaxLevels][kBandWords];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bx0 = (blockIdx.x * 2 + (wv & 1)) * kBandBlock, by0 = (blockIdx.y * 2 + (wv >> 1)) * kBandBlock, f = blockIdx.z;
  for (int i = tid; i < (kBlock / 64) * kBandMaxLevels * kBandWords; i += kBlock) (&sh[0][0][0])[i] = 0;
  __syncthreads();

  if (bx0 < a.w && by0 < a.h) {   // wave-uniform
    const T* pr = (const T*)a.ref + (int64_t)f * a.ref_fp;
    const T* pd = (const T*)a.dis + (int64_t)f * a.dis_fp;
    const int px = bx0 + (lane % LPR) * S, py = by0 + (lane / LPR) * R;   // the lane's first sample
    PackedQuad qr[R], qd[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int y = py + k < a.h ? py + k : a.h - 1;   // a row below the plane: the last one, for no coefficient that counts
      qr[k] = quad_load<T, VB, kTailRepeat>(pr + (int64_t)y * a.ref_rp, px, a.w);
      qd[k] = quad_load<T, VB, kTailRepeat>(pd + (int64_t)y * a.dis_rp, px, a.w);
    }
    const int L = a.levels;
    long long acc[kBandWords];
    int r[R / 2][S / 2], d[R / 2][S / 2];   // A_1 of the lane, then the deeper levels in its top left

    // levels inside the lane
    band_lane_first<T, Narrow, R, S>(qr, qd, a.top, r, d, px >> 1, py >> 1, a.w >> 1, a.h >> 1, acc);
    band_reduce<64>(acc, lane, sh[wv][0]);
    if (L >= 2) {
      band_lane_level<Narrow, S / 2, R / 2, R / 2, S / 2>(r, d, px >> 2, py >> 2, a.w >> 2, a.h >> 2, acc);
      band_reduce<64>(acc, lane, sh[wv][1]);
    }
    int ar = 0, ad = 0;   // A_3 (i, j) of the block on lane 8 j + i
    if (L >= 3) {
#pragma unroll
      for (int m = 0; m < kBandWords; ++m) acc[m] = 0;
      if constexpr (sizeof(T) == 2) {
        band_lane_level<long long, S / 4, R / 4, R / 2, S / 2>(r, d, px >> 3, py >> 3, a.w >> 3, a.h >> 3, acc);
        ar = r[0][0];
        ad = d[0][0];
      } else {
        const bool low = (lane >> 2) & 1;
        int ro[4], dd[4];
        band_pair_rows(r[0], low, ro);
        band_pair_rows(d[0], low, dd);
        const int i3 = (lane & 3) * 2 + (low ? 1 : 0), j3 = lane >> 3;   // the coefficient of level 3 this lane formed
        band_add<long long>(acc, (bx0 >> 3) + i3 < (a.w >> 3) && (by0 >> 3) + j3 < (a.h >> 3), ro, dd);
        const int src = (((lane >> 3) * 2 + (lane & 1)) << 2) + ((lane & 7) >> 1);   // the lane that formed (lane & 7, lane >> 3)
        ar = __shfl(ro[3], src, 64);
        ad = __shfl(dd[3], src, 64);
      }
      band_reduce<64>(acc, lane, sh[wv][2]);
    }
    // levels across the lanes: G x G parents on lanes G j + i
    if (L >= 4) band_cross<8>(ar, ad, 4, lane, bx0, by0, a.w, a.h, sh[wv][3]);
    if (L >= 5) band_cross<4>(ar, ad, 5, lane, bx0, by0, a.w, a.h, sh[wv][4]);
    if (L >= 6) band_cross<2>(ar, ad, 6, lane, bx0, by0, a.w, a.h, sh[wv][5]);
  }
  __syncthreads();

  if (tid < a.levels * kBandWords) {
    const int lv = tid / kBandWords, m = tid % kBandWords;
    long long s = 0;
    for (int k = 0; k < kBlock / 64; ++k) s += sh[k][lv][m];
    a.part[(((int64_t)f * a.gy + blockIdx.y) * a.gx + blockIdx.x) * (a.levels * kBandWords) + tid] = s;
  }
}

// a wave per (sum, frame): adds the workgroups' partials in a fixed order
__global__ __launch_bounds__(64) void band_finish_kernel(const long long* part, int groups, int words, unsigned long long* out) {
  const int m = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
  const long long* p = part + (int64_t)f * groups * words + m;
  long long s = 0;
  for (int g = lane; g < groups; g += 64) s += p[(int64_t)g * words];
  for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) out[(int64_t)f * words + m] = (unsigned long long)s;
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const BandArgs& a, int n_frames) {
  hipLaunchKernelGGL((band_moments_kernel<T, VB>), dim3(a.gx, a.gy, n_frames), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

bool band_levels_ok(int levels) { return levels >= 1 && levels <= kBandMaxLevels; }

size_t band_out_bytes(int levels, int n_frames) {
  return (size_t)(n_frames > 0 ? n_frames : 0) * levels * kBandWords * sizeof(unsigned long long);
}

size_t band_part_bytes(int w, int h, int levels, int n_frames) {
  return band_out_bytes(levels, n_frames) * ((w + kBandGroup - 1) / kBandGroup) * ((h + kBandGroup - 1) / kBandGroup);
}

hipError_t launch_band_moments(hipStream_t stream, Elem elem, int bits, const void* ref, int64_t ref_row_pitch,
                               int64_t ref_frame_pitch, const void* dis, int64_t dis_row_pitch, int64_t dis_frame_pitch,
                               int n_frames, int w, int h, int levels, void* part, unsigned long long* out) {
  if (n_frames <= 0) return hipSuccess;
  BandArgs a{};
  if (!band_levels_ok(levels) ||
      !pair_planes(a, elem, bits, ref, ref_row_pitch, ref_frame_pitch, dis, dis_row_pitch, dis_frame_pitch, w, h))
    return hipErrorInvalidValue;
  a.levels = levels;
  a.gx = (w + kBandGroup - 1) / kBandGroup; a.gy = (h + kBandGroup - 1) / kBandGroup;
  a.top = (1u << bits) - 1u;
  a.part = (long long*)part;
  const hipError_t e = dispatch(elem, load_bytes(elem, a), [&](auto t, auto vb) {
    return launch_v<decltype(t), decltype(vb)::value>(stream, a, n_frames);
  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(band_finish_kernel, dim3(levels * kBandWords, n_frames), dim3(64), 0, stream, (const long long*)part,
                     a.gx * a.gy, levels * kBandWords, out);
  return hipGetLastError();
}

}  // namespace pqa
