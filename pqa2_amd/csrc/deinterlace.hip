// Deinterlacing: a kept field and an interpolated one (pqa_deinterlace / pqa_deinterlace_device; restated in
// tests/deinterlace_ref.py).  The arithmetic follows the filter FFmpeg ships as bwdif (w3fdif taps inside yadif's temporal
// clamp) as this library states it; the edge rule is this library's own and parity with FFmpeg is not pinned.
//
// A clip has `count` planes S_t of w x h samples, h >= 2 (a u16 sample above top = 2^bits - 1 is read as top); S_t with t < 0 is
// S_0 and with t >= count it is S_{count-1}.  An output plane is made from a source frame t and a kept parity p; q = 1 - p;
// P, C, N = S_{t-1}, S_t, S_{t+1}; with `first` the parity of the rows that come first in time, B = P and A = C where
// p == first, otherwise B = C and A = N: the fields of parity q just before and just after the kept one.  row(F, r, k) is row
// min(max(r, k), last_k) of F, last_k the largest row index below h of parity k.  Rows of parity p: O[y] = C[y].  Rows y of
// parity q, every column (every shift is arithmetic: a floor):
//
//   c  = row(C, y-1, p)   e  = row(C, y+1, p)   c3 = row(C, y-3, p)   e3 = row(C, y+3, p)
//   sp = (5077 (c + e) - 981 (c3 + e3)) >> 13
//   intra:     O[y] = clip(sp, 0, top)
//   adaptive:  s(k) = row(B, y+k, q) + row(A, y+k, q), k in {-4, -2, 0, 2, 4};  d = s(0) >> 1
//              td0  = |row(B, y, q) - row(A, y, q)|
//              td1  = (|row(P, y-1, p) - c| + |row(P, y+1, p) - e|) >> 1;  td2 the same with N
//              diff = max(td0 >> 1, td1, td2);  diff == 0: O[y] = d; otherwise
//              bb = (s(-2) >> 1) - c, ff = (s(2) >> 1) - e, dc = d - c, de = d - e
//              diff = max(diff, min(de, dc, max(bb, ff)), -max(de, dc, min(bb, ff)))
//              v = |c - e| > td0 ? (((5570 s(0) - 3801 (s(-2) + s(2)) + 1016 (s(-4) + s(4))) >> 2) + 4309 (c + e) - 213 (c3 + e3)) >> 13 : sp
//              O[y] = clip(clip(v, d - diff, d + diff), 0, top)
//
// int32 bound.  Samples are at most top <= 4095 and s(k) <= 2 top.  5570 s(0) - 3801 (s(-2) + s(2)) + 1016 (s(-4) + s(4)) lies
// in [-3801 * 4 * 4095, (5570 * 2 + 1016 * 4) * 4095]: at most 62 259 240 in magnitude, below 2^26; a quarter of it plus
// 4309 * 2 * 4095 minus up to 213 * 2 * 4095 stays below 2^26; 5077 * 2 * 4095 < 2^26.  Everything else is a sum or difference of
// at most four samples.  No floating point, no LDS, no atomics, no scratch.
//
// Work.  A lane owns 16 bytes of a row (16 u8 / 8 u16 samples), a wave kDeintColBytes = 1024 bytes of it, and marches down a
// band of kDeintBand = 16 rows with the window in registers: the rows y-3 ... y+3 of C (4 pieces of 16 bytes), y-1 and y+1 of P and
// of N, and y-4 ... y+4 of B and of A (5 each): 18 pieces, 72 VGPRs (intra: the 4 of C).  A step is one row pair -- the
// interpolated row y and the kept row beside it, which is c (p == 0) or e (p == 1) of the window -- and loads five new pieces,
// row(C, y+5, p), row(P, y+3, p), row(N, y+3, p), row(B, y+6, q), row(A, y+6, q), BEFORE it computes, so they are in flight under
// the arithmetic of the step, and stores two rows.  The window is filled by five steps of the same loop in front of the band
// that load and do not compute (the loads of P, N and C that nothing would read are left out), so there are five load sites
// and not 23.  Row indices are clamped as row() says, wave-uniformly, so every address is a real row of its own parity.  A
// workgroup is kDeintWaves = 4 waves on bands one below the other; blockIdx.z is the output plane.  A band re-reads the 8 rows
// around it that its neighbours own: 2.5 planes read by the arithmetic, 2.5 * (1 + 8 / 16) by the kernel, the excess mostly
// from L2.  Bands of 16 rows measured 8 ... 28 % faster than bands of 32 on the moving clip (1080p and 2160p, 8 and 10 bit):
// a 1080p 8-bit launch of 8 planes is 1088 waves where 32 rows gave 576 for 1024 SIMDs, and a wave has one step of loads in flight.
// One load is 16 bytes, 4 bytes or one sample, whichever the bases and pitches of BOTH clips allow (plane_scan.h, load_bytes);
// the store takes the same width.  The piece that crosses the end of a row is read and written sample by sample (zeros past the
// end), and a lane that starts past the end reads and writes nothing.
// Still picture.  If, for every lane of the wave, B == A, P == C and N == C on the rows of the step (a comparison of packed
// dwords), then td0 = td1 = td2 = 0 for every sample, so diff == 0 and O[y] = d = row(B, y, q): one ballot decides, the piece of
// B is stored as it is and the taps are skipped.  The test is sufficient, not necessary (diff is also 0 where td0 == 1); a wave
// it does not catch takes the general path, which gives the same integers.  uniform == false: never taken (test partner).
#include "plane_scan.h"

namespace pqa {
namespace {

struct DeintArgs {
  const void* src;
  void* dst;
  int64_t src_rp, src_fp, dst_rp, dst_fp;   // elements
  int w, h, count, t0, first, per;
  unsigned top;
  int uniform;
};

// a piece of u16 samples, none above top (a u8 container cannot hold one)
template <typename T>
__device__ __forceinline__ PackedQuad capped(PackedQuad q, unsigned top) {
  if constexpr (sizeof(T) > 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.d[k] = min(q.d[k] & 0xffffu, top) | (min(q.d[k] >> 16, top) << 16);
  }
  return q;
}

template <typename T>
__device__ __forceinline__ int sample(const PackedQuad& q, int j) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  return (int)((q.d[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1u));
}

__device__ __forceinline__ unsigned differs(const PackedQuad& a, const PackedQuad& b) {
  return (a.d[0] ^ b.d[0]) | (a.d[1] ^ b.d[1]) | (a.d[2] ^ b.d[2]) | (a.d[3] ^ b.d[3]);
}

// the samples x ... x + S - 1 of a destination row that ends before w
template <typename T, int VB>
__device__ __forceinline__ void quad_store(T* row, int x, int w, const PackedQuad& o) {
  constexpr int S = 16 / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  if (x + S <= w && VB == 16) {
    *reinterpret_cast<uint4*>(row + x) = make_uint4(o.d[0], o.d[1], o.d[2], o.d[3]);
  } else if (x + S <= w && VB == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<unsigned*>(row + x + j * PER) = o.d[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < PER; ++s) {
        const int xx = x + j * PER + s;
        if (xx < w) row[xx] = (T)(o.d[j] >> (BITS * s));
      }
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// VB: bytes of one load and of one store; MODE 0 intra, 1 adaptive
template <typename T, int VB, int MODE>
__global__ __launch_bounds__(kBlock) void deinterlace_kernel(const DeintArgs a) {
  constexpr int S = 16 / (int)sizeof(T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = ((int)blockIdx.y * kDeintWaves + wave) * kDeintBand;   // even
  if (y0 >= a.h) return;
  // a lane past the end of the row keeps the wave's ballots whole: it reads as one whose piece is all zeros and stores nothing
  const int x = min(((int)blockIdx.x * 64 + lane) * S, a.w);

  const int t = a.t0 + (int)blockIdx.z / a.per;
  const int p = ((int)blockIdx.z % a.per) ? 1 - a.first : a.first, q = 1 - p;
  const T* const src = (const T*)a.src;
  const T* const C = src + (int64_t)t * a.src_fp;
  const T* const P = src + (int64_t)max(t - 1, 0) * a.src_fp;
  const T* const N = src + (int64_t)min(t + 1, a.count - 1) * a.src_fp;
  const T* const B = p == a.first ? P : C;
  const T* const A = p == a.first ? C : N;
  T* const O = (T*)a.dst + (int64_t)blockIdx.z * a.dst_fp;
  const int last_p = a.h - 1 - ((a.h - 1 - p) & 1), last_q = a.h - 1 - ((a.h - 1 - q) & 1);
  const int top = (int)a.top;

  // row(F, r, k), this lane's piece of it
  const auto piece = [&](const T* F, int r, int k, int last_k) {
    return capped<T>(quad_load<T, VB, kTailZeros>(F + (int64_t)clampi(r, k, last_k) * a.src_rp, x, a.w), a.top);
  };

  PackedQuad c3{}, c{}, e{}, e3{};           // C: rows y-3, y-1, y+1, y+3
  PackedQuad pc{}, pe{}, nc{}, ne{};         // P and N: rows y-1, y+1
  PackedQuad b[5] = {}, f[5] = {};           // B and A: rows y-4 ... y+4
  const int steps = (min(a.h - y0, kDeintBand) + 1) >> 1;
#pragma unroll 1
  for (int i = -5; i < steps; ++i) {
    const int y = y0 + q + 2 * i;            // the interpolated row of this step; the window holds its rows from i == 0 on
    // the rows the next step adds, in flight under this step's arithmetic
    PackedQuad ne3{}, npe{}, nne{}, nb{}, nf{};
    if (i >= -4) ne3 = piece(C, y + 5, p, last_p);
    if constexpr (MODE == 1) {
      if (i >= -2) {
        npe = piece(P, y + 3, p, last_p);
        nne = piece(N, y + 3, p, last_p);
      }
      nb = piece(B, y + 6, q, last_q);
      nf = piece(A, y + 6, q, last_q);
    }
    if (i >= 0) {
      const int yk = y0 + p + 2 * i;         // the kept row of this step: y - 1 (p == 0, always in the plane) or y + 1
      if (yk < a.h) quad_store<T, VB>(O + (int64_t)yk * a.dst_rp, x, a.w, p == 0 ? c : e);
      if (y < a.h) {
        PackedQuad o;
        bool still = false;
        if constexpr (MODE == 1) {
          if (a.uniform) {
            const unsigned moved = differs(b[2], f[2]) | differs(pc, c) | differs(pe, e) | differs(nc, c) | differs(ne, e);
            still = __ballot(moved != 0u) == 0ull;
          }
        }
        if (still) {
          o = b[2];
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) o.d[k] = 0u;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const int vc = sample<T>(c, j), ve = sample<T>(e, j), s3 = sample<T>(c3, j) + sample<T>(e3, j);
            const int sp = (5077 * (vc + ve) - 981 * s3) >> 13;
            int r;
            if constexpr (MODE == 0) {
              r = clampi(sp, 0, top);
            } else {
              const int b0 = sample<T>(b[2], j), a0 = sample<T>(f[2], j);
              const int s0 = b0 + a0, d = s0 >> 1, td0 = abs(b0 - a0);
              const int td1 = (abs(sample<T>(pc, j) - vc) + abs(sample<T>(pe, j) - ve)) >> 1;
              const int td2 = (abs(sample<T>(nc, j) - vc) + abs(sample<T>(ne, j) - ve)) >> 1;
              const int diff0 = max(td0 >> 1, max(td1, td2));
              const int sm2 = sample<T>(b[1], j) + sample<T>(f[1], j), sp2 = sample<T>(b[3], j) + sample<T>(f[3], j);
              const int s4 = sample<T>(b[0], j) + sample<T>(f[0], j) + sample<T>(b[4], j) + sample<T>(f[4], j);
              const int bb = (sm2 >> 1) - vc, ff = (sp2 >> 1) - ve, dc = d - vc, de = d - ve;
              const int hi = max(max(de, dc), min(bb, ff)), lo = min(min(de, dc), max(bb, ff));
              const int diff = max(diff0, max(lo, -hi));
              const int tmp = (((5570 * s0 - 3801 * (sm2 + sp2) + 1016 * s4) >> 2) + 4309 * (vc + ve) - 213 * s3) >> 13;
              const int v = abs(vc - ve) > td0 ? tmp : sp;
              r = diff0 == 0 ? d : clampi(clampi(v, d - diff, d + diff), 0, top);
            }
            constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
            o.d[j / PER] |= (unsigned)r << (BITS * (j % PER));
          }
        }
        quad_store<T, VB>(O + (int64_t)y * a.dst_rp, x, a.w, o);
      }
    }
    // one row pair down
    c3 = c; c = e; e = e3; e3 = ne3;
    if constexpr (MODE == 1) {
      pc = pe; pe = npe; nc = ne; ne = nne;
#pragma unroll
      for (int k = 0; k < 4; ++k) { b[k] = b[k + 1]; f[k] = f[k + 1]; }
      b[4] = nb; f[4] = nf;
    }
  }
}

template <typename T, int VB>
hipError_t launch_v(hipStream_t stream, const DeintArgs& a, int mode, int n_out) {
  const int cols = kDeintColBytes / (int)sizeof(T), rows = kDeintWaves * kDeintBand;
  const dim3 grid((a.w + cols - 1) / cols, (a.h + rows - 1) / rows, n_out);
  if (mode == 0) hipLaunchKernelGGL((deinterlace_kernel<T, VB, 0>), grid, dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((deinterlace_kernel<T, VB, 1>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_deinterlace(hipStream_t stream, Elem elem, int bit_depth, int mode, int first, int per, bool uniform, const void* src,
                              int64_t src_row_pitch, int64_t src_frame_pitch, int count, int t0, int n, void* dst, int64_t dst_row_pitch,
                              int64_t dst_frame_pitch, int w, int h) {
  if (n <= 0) return hipSuccess;
  if (!src || !dst || !scan_shape_ok(elem, bit_depth, w, h) || h < 2 || (mode | first) < 0 || mode > 1 || first > 1 || per < 1 || per > 2 ||
      t0 < 0 || n > 32767 || count < 1 || t0 > count - n)
    return hipErrorInvalidValue;
  const int es = elem == ELEM_U8 ? 1 : 2;
  // whole samples on both sides, rows that hold a row
  if ((((uintptr_t)src | (uintptr_t)src_row_pitch | (uintptr_t)src_frame_pitch | (uintptr_t)dst | (uintptr_t)dst_row_pitch |
        (uintptr_t)dst_frame_pitch) & (uintptr_t)(es - 1)) ||
      src_row_pitch < (int64_t)w * es || dst_row_pitch < (int64_t)w * es)
    return hipErrorInvalidValue;
  DeintArgs a{};
  a.src = src; a.dst = dst;
  a.src_rp = src_row_pitch / es; a.src_fp = src_frame_pitch / es;
  a.dst_rp = dst_row_pitch / es; a.dst_fp = dst_frame_pitch / es;
  a.w = w; a.h = h; a.count = count; a.t0 = t0; a.first = first; a.per = per;
  a.top = (1u << bit_depth) - 1u;
  a.uniform = uniform ? 1 : 0;
  // a lane starts a multiple of 16 bytes into its row
  const int vb = std::min(load_bytes(elem, src, a.src_rp, a.src_fp), load_bytes(elem, dst, a.dst_rp, a.dst_fp));
  return dispatch(elem, vb, [&](auto t, auto v) { return launch_v<decltype(t), decltype(v)::value>(stream, a, mode, n * per); });
}

}  // namespace pqa
