// Exact-integer polyphase resampler (pqa_resample / pqa_resample_device; restated in tests/resample_ref.py; definition and
// bounds: DESIGN.md section 5).  One plane of n_frames frames is resized, or moved by a fraction of a sample, with one
// table-driven separable filter whose coefficients are integers at scale 2^14.
//
// Tables (host, double, resample_table below).  Per destination sample of an axis: `first`, the first source sample it reads,
// and its coefficients q, which sum to exactly 16384; edge replication is folded into the row, so nothing here clamps an
// index for the border's sake.  The device form of a row (resample_plan) starts at first & ~1 and is zero-padded to P pairs of
// int16: a pair is one dword, every pair starts on an even source sample, and a pair sum is one v_dot2c_i32_i16.
//
// Work.  A workgroup of 256 threads owns a destination tile of kRsTileW = 64 columns by th rows (th = 32; the host halves it
// until the tile's source rows fit the LDS, which happens beyond about 10x down).  The rows r0 ... r0 + R - 1 of the source
// that the tile's vertical footprint needs go through the horizontal pass four at a time and wave by wave: the wave copies
// the columns of the tile's horizontal footprint of its four rows into LDS as int16 (8-bit samples are widened here, once;
// 4 samples a load where base and pitches allow it, the host decides), then lane x holds destination column x and
// accumulates the four rows against ONE read of each coefficient pair.  mid = (acc + 2^(b-1)) >> b goes into the LDS tile as
// vertical pairs (rows 2k, 2k + 1 of column x in one dword).  The vertical pass reads that tile: a lane owns four adjacent
// columns of one destination row, one ds_read_b128 brings four vertical pairs, and the four results leave in one store (4 B
// at 8 bit, 8 B above), sixteen lanes covering the tile's row: a wave instruction stores four full tile rows.  Destination
// rows whose address or pitch rules that out are stored sample by sample.  Every source sample is read from HBM once per tile
// that needs it; nothing intermediate leaves the CU.  Integers only, no atomics: the result is independent of scheduling.
// Bounds (the table builder asserts sum |q| < 32768 per row): |acc| < 2^15 (2^b - 1) < 2^27, |mid| < 2^15 (int16),
// |acc2| < 2^30.  Samples above 2^b - 1 (a 16-bit container can hold one) are read as 2^b - 1 so that the bounds hold.
// Rows and columns past the source that only a padding coefficient (zero) meets are read from the last row / column.
#include <cmath>
#include <vector>

#include "kernels.h"
#include "pqa_device.h"

namespace pqa {
namespace {

constexpr int kRsTileW = 64;
constexpr int kRsRowsPerWave = 4;                      // source rows a wave filters against one read of a coefficient pair
constexpr int kRsStage = (kBlock / 64) * kRsRowsPerWave;   // source rows of one round of the horizontal pass
constexpr size_t kRsLdsLimit = 65536;

typedef short short2v __attribute__((ext_vector_type(2)));
typedef int int4v __attribute__((ext_vector_type(4)));

struct RsArgs {
  const void* src;
  void* dst;
  int64_t src_rp, src_fp, dst_rp, dst_fp;   // elements
  int src_w, src_h, dst_w, dst_h;
  int th;            // destination rows of a tile
  int ph, pv;        // coefficient pairs of a row of the horizontal / vertical table
  int wpad;          // dst_w rounded up to kRsTileW: the stride of the horizontal coefficients
  int mid_rows;      // rows of the LDS tile (even, a multiple of kRsStage)
  int sw;            // samples of one staged source row (a multiple of 4)
  int bits;
  int src_vec, dst_vec;   // 4-sample loads / stores are aligned
  const int* first_h;     // [wpad], even
  const int* coef_h;      // [ph][wpad] pairs
  const int* first_v;     // [dst_h], even
  const int* coef_v;      // [dst_h][pv] pairs
  const int* tile_h;      // [tiles across][2]: first source column a tile stages (a multiple of 4), one past its last
  const int* tile_v;      // [tiles down][2]: first source row of a tile (even), number of rows
};

__device__ __forceinline__ int dot2(int samples, int coefs, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, samples), __builtin_bit_cast(short2v, coefs), acc, false);
}
__device__ __forceinline__ int pack2(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }

template <typename T>
__global__ __launch_bounds__(kBlock) void resample_kernel(const RsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int rs_lds[];
  int* mid = rs_lds;                                        // [mid_rows / 2][kRsTileW] vertical pairs
  int* stage = rs_lds + (a.mid_rows / 2) * kRsTileW;        // [kRsStage][sw / 2] horizontal pairs
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * kRsTileW, y0 = blockIdx.y * a.th, y1 = min(a.dst_h, y0 + a.th);
  const int maxv = (1 << a.bits) - 1;
  const T* src = (const T*)a.src + (int64_t)blockIdx.z * a.src_fp;
  T* dst = (T*)a.dst + (int64_t)blockIdx.z * a.dst_fp;

  const int r0 = a.tile_v[2 * blockIdx.y], rows = a.tile_v[2 * blockIdx.y + 1];   // the tile's vertical footprint
  const int sx0 = a.tile_h[2 * blockIdx.x], sx1 = a.tile_h[2 * blockIdx.x + 1];   // and its horizontal one
  const int my_off = (a.first_h[x0 + lane] - sx0) >> 1;                   // this lane's column: its first pair in a staged row
  int* my_stage = stage + wv * kRsRowsPerWave * (a.sw >> 1);

  // ---- horizontal pass: kRsStage source rows a round -------------------------------------------------------------------
  for (int rb = 0; rb < rows; rb += kRsStage) {
    const int rw = rb + wv * kRsRowsPerWave;   // this wave's four rows, relative to r0
#pragma unroll
    for (int j = 0; j < kRsRowsPerWave; ++j) {
      const T* row = src + (int64_t)min(r0 + rw + j, a.src_h - 1) * a.src_rp;
      int* out = my_stage + j * (a.sw >> 1);
      for (int i = lane * 4; sx0 + i < sx1; i += 256) {
        int v[4];
        if (a.src_vec && sx0 + i + 3 < a.src_w) {
          struct alignas(4 * sizeof(T)) Vec { T s[4]; };
          const Vec q = *reinterpret_cast<const Vec*>(row + sx0 + i);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = q.s[e];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = row[min(sx0 + i + e, a.src_w - 1)];
        }
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = min(v[e], maxv);
        }
        *reinterpret_cast<int2*>(out + (i >> 1)) = int2{pack2(v[0], v[1]), pack2(v[2], v[3])};
      }
    }
    __syncthreads();
    int acc[kRsRowsPerWave] = {};
    for (int k = 0; k < a.ph; ++k) {
      const int c = a.coef_h[k * a.wpad + x0 + lane];
#pragma unroll
      for (int j = 0; j < kRsRowsPerWave; ++j) acc[j] = dot2(my_stage[j * (a.sw >> 1) + my_off + k], c, acc[j]);
    }
    const int half = 1 << (a.bits - 1);
#pragma unroll
    for (int j = 0; j < kRsRowsPerWave; j += 2)
      mid[((rw + j) >> 1) * kRsTileW + lane] = pack2((acc[j] + half) >> a.bits, (acc[j + 1] + half) >> a.bits);
    __syncthreads();
  }

  // ---- vertical pass: a lane owns four adjacent columns of a destination row -------------------------------------------
  const int xq = (tid & 15) * 4, x = x0 + xq;
  const int sh = 28 - a.bits, rnd = 1 << (27 - a.bits);
  for (int y = y0 + (tid >> 4); y < y1; y += kBlock / 16) {
    const int* m = mid + ((a.first_v[y] - r0) >> 1) * kRsTileW + xq;
    const int* cv = a.coef_v + (int64_t)y * a.pv;
    int acc[4] = {};
    for (int k = 0; k < a.pv; ++k) {
      const int4v p = *reinterpret_cast<const int4v*>(m + k * kRsTileW);
      const int c = cv[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = dot2(p[e], c, acc[e]);
    }
    struct alignas(4 * sizeof(T)) Vec { T s[4]; } o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o.s[e] = (T)min(max((acc[e] + rnd) >> sh, 0), maxv);
    T* drow = dst + (int64_t)y * a.dst_rp;
    if (a.dst_vec && x + 3 < a.dst_w) {
      *reinterpret_cast<Vec*>(drow + x) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < a.dst_w) drow[x + e] = o.s[e];
    }
  }
}

double rs_sinc(double t) {
  if (t == 0.0) return 1.0;
  const double u = M_PI * t;
  return std::sin(u) / u;
}

double rs_kernel(int filter, double t) {
  const double x = std::fabs(t);
  if (filter == 0) return x < 1.0 ? 1.0 - x : 0.0;
  if (filter == 1) {
    const double A = -0.6;
    if (x <= 1.0) return (A + 2.0) * x * x * x - (A + 3.0) * x * x + 1.0;
    if (x < 2.0) return A * x * x * x - 5.0 * A * x * x + 8.0 * A * x - 4.0 * A;
    return 0.0;
  }
  return x < 3.0 ? rs_sinc(t) * rs_sinc(t / 3.0) : 0.0;
}

}  // namespace

int resample_table(int filter, int n_src, int n_dst, int64_t x0_q16, int64_t ext_q16, ResampleTable* out) {
  if (filter < 0 || filter > 2 || n_src < 1 || n_dst < 1 || ext_q16 <= 0) return -1;
  const double s = filter == 0 ? 1.0 : filter == 1 ? 2.0 : 3.0;
  const double x0 = (double)x0_q16 / 65536.0, ext = (double)ext_q16 / 65536.0;
  const double step = ext / n_dst, stretch = step > 1.0 ? step : 1.0, S = s * stretch;
  if (S > 4.0 * kRsMaxTaps) return -1;   // far beyond the tap limit: refuse before the rows are built
  out->first.assign(n_dst, 0);
  out->taps = 1;
  std::vector<std::vector<int>> rows(n_dst);
  std::vector<double> w;
  std::vector<int> q;
  for (int i = 0; i < n_dst; ++i) {
    const double c = x0 + (i + 0.5) * step - 0.5;
    const int64_t j0 = (int64_t)std::ceil(c - S), j1 = (int64_t)std::floor(c + S);
    const int n = (int)(j1 - j0 + 1);
    w.assign(n, 0.0);
    q.assign(n, 0);
    double sum = 0.0;
    for (int t = 0; t < n; ++t) {
      w[t] = rs_kernel(filter, ((double)(j0 + t) - c) / stretch);
      sum += w[t];
    }
    int total = 0, best = 0;
    for (int t = 0; t < n; ++t) {
      q[t] = (int)std::floor(w[t] / sum * 16384.0 + 0.5);
      total += q[t];
      if (q[t] > q[best]) best = t;   // the first of equals
    }
    q[best] += 16384 - total;
    // edge replication, folded into the row
    const auto fold = [&](int64_t j) { return (int)(j < 0 ? 0 : j > n_src - 1 ? n_src - 1 : j); };
    int lo = fold(j0), hi = fold(j1);
    std::vector<int> r(hi - lo + 1, 0);
    for (int t = 0; t < n; ++t) r[fold(j0 + t) - lo] += q[t];
    while (r.size() > 1 && r.back() == 0) r.pop_back();
    size_t lead = 0;
    while (lead + 1 < r.size() && r[lead] == 0) ++lead;
    r.erase(r.begin(), r.begin() + lead);
    lo += (int)lead;
    int mag = 0;
    for (int v : r) mag += v < 0 ? -v : v;
    if ((int)r.size() > kRsMaxTaps || mag >= 32768) return -1;
    out->first[i] = lo;
    if ((int)r.size() > out->taps) out->taps = (int)r.size();
    rows[i] = std::move(r);
  }
  out->coeff.assign((size_t)n_dst * out->taps, 0);
  for (int i = 0; i < n_dst; ++i)
    for (size_t t = 0; t < rows[i].size(); ++t) out->coeff[(size_t)i * out->taps + t] = (int16_t)rows[i][t];
  return 0;
}

void resample_plan(const ResampleTable& th, const ResampleTable& tv, int dst_w, int dst_h, ResamplePlan* p) {
  p->wpad = (dst_w + kRsTileW - 1) / kRsTileW * kRsTileW;
  // a device row starts at first & ~1: one more tap when first is odd, then whole pairs
  p->ph = (th.taps + 2) / 2;
  p->pv = (tv.taps + 2) / 2;
  p->off_first_h = 0;
  p->off_coef_h = p->off_first_h + (size_t)p->wpad;
  p->off_first_v = p->off_coef_h + (size_t)p->ph * p->wpad;
  p->off_coef_v = p->off_first_v + (size_t)dst_h;
  p->words.assign(p->off_coef_v + (size_t)dst_h * p->pv, 0);
  int* w = p->words.data();
  const auto pairs = [](const ResampleTable& t, int i, int k) {   // pair k of device row i
    const int shift = t.first[i] & 1;
    int v[2];
    for (int e = 0; e < 2; ++e) {
      const int tap = 2 * k + e - shift;
      v[e] = tap >= 0 && tap < t.taps ? t.coeff[(size_t)i * t.taps + tap] : 0;
    }
    return (v[0] & 0xffff) | (int)((unsigned)v[1] << 16);
  };
  for (int x = 0; x < p->wpad; ++x) {
    const int i = x < dst_w ? x : dst_w - 1;   // padding columns: a real `first`, no coefficients
    w[p->off_first_h + x] = th.first[i] & ~1;
    for (int k = 0; k < p->ph; ++k) w[p->off_coef_h + (size_t)k * p->wpad + x] = x < dst_w ? pairs(th, i, k) : 0;
  }
  for (int y = 0; y < dst_h; ++y) {
    w[p->off_first_v + y] = tv.first[y] & ~1;
    for (int k = 0; k < p->pv; ++k) w[p->off_coef_v + (size_t)y * p->pv + k] = pairs(tv, y, k);
  }
  // the footprint of `count` device rows from `from` on: {lowest first, one past the highest sample read}
  const auto span = [&](size_t off_first, int from, int count, int pairs_per_row, int* lo, int* hi) {
    *lo = w[off_first + from];
    *hi = *lo + 2 * pairs_per_row;
    for (int i = from; i < from + count; ++i) {
      const int f = w[off_first + i];
      if (f < *lo) *lo = f;
      if (f + 2 * pairs_per_row > *hi) *hi = f + 2 * pairs_per_row;
    }
  };
  const int ntx = p->wpad / kRsTileW;
  std::vector<int> tile_h((size_t)2 * ntx);
  int sw = 0;
  for (int t = 0; t < ntx; ++t) {
    int lo, hi;
    span(p->off_first_h, t * kRsTileW, kRsTileW, p->ph, &lo, &hi);
    tile_h[2 * t] = lo & ~3;
    tile_h[2 * t + 1] = hi;
    if (hi - (lo & ~3) > sw) sw = hi - (lo & ~3);
  }
  p->sw = (sw + 3) / 4 * 4;
  // tile height: the most source rows any tile spans must fit the LDS beside the staged rows
  std::vector<int> tile_v;
  for (p->th = 32;; p->th /= 2) {
    const int nty = (dst_h + p->th - 1) / p->th;
    tile_v.assign((size_t)2 * nty, 0);
    int rows = 0;
    for (int t = 0; t < nty; ++t) {
      const int y0 = t * p->th, y1 = y0 + p->th < dst_h ? y0 + p->th : dst_h;
      int lo, hi;
      span(p->off_first_v, y0, y1 - y0, p->pv, &lo, &hi);
      tile_v[2 * t] = lo;
      tile_v[2 * t + 1] = hi - lo;
      if (hi - lo > rows) rows = hi - lo;
    }
    p->mid_rows = (rows + kRsStage - 1) / kRsStage * kRsStage;
    p->lds_bytes = (size_t)(p->mid_rows / 2) * kRsTileW * 4 + (size_t)kRsStage * (p->sw / 2) * 4;
    if (p->lds_bytes <= kRsLdsLimit || p->th == 1) break;
  }
  p->off_tile_h = p->words.size();
  p->words.insert(p->words.end(), tile_h.begin(), tile_h.end());
  p->off_tile_v = p->words.size();
  p->words.insert(p->words.end(), tile_v.begin(), tile_v.end());
}

hipError_t launch_resample(hipStream_t stream, Elem elem, int bits, const ResamplePlan& p, const int* dev_words, const void* src,
                           int64_t src_row_pitch, int64_t src_frame_pitch, int src_w, int src_h, void* dst, int64_t dst_row_pitch,
                           int64_t dst_frame_pitch, int dst_w, int dst_h, int n_frames) {
  if (n_frames <= 0) return hipSuccess;
  if ((bits != 8 && bits != 10 && bits != 12) || (elem == ELEM_U8) != (bits == 8) || p.lds_bytes > kRsLdsLimit)
    return hipErrorInvalidValue;
  const int64_t es = elem == ELEM_U8 ? 1 : 2;
  RsArgs a{};
  a.src = src; a.dst = dst;
  a.src_rp = src_row_pitch; a.src_fp = src_frame_pitch; a.dst_rp = dst_row_pitch; a.dst_fp = dst_frame_pitch;
  a.src_w = src_w; a.src_h = src_h; a.dst_w = dst_w; a.dst_h = dst_h;
  a.th = p.th; a.ph = p.ph; a.pv = p.pv; a.wpad = p.wpad; a.mid_rows = p.mid_rows; a.sw = p.sw; a.bits = bits;
  a.src_vec = (((uint64_t)(uintptr_t)src | (uint64_t)(src_row_pitch * es) | (uint64_t)(src_frame_pitch * es)) % (4 * es)) == 0;
  a.dst_vec = (((uint64_t)(uintptr_t)dst | (uint64_t)(dst_row_pitch * es) | (uint64_t)(dst_frame_pitch * es)) % (4 * es)) == 0;
  a.first_h = dev_words + p.off_first_h; a.coef_h = dev_words + p.off_coef_h;
  a.first_v = dev_words + p.off_first_v; a.coef_v = dev_words + p.off_coef_v;
  a.tile_h = dev_words + p.off_tile_h; a.tile_v = dev_words + p.off_tile_v;
  const dim3 grid(p.wpad / kRsTileW, (dst_h + p.th - 1) / p.th, n_frames);
  if (elem == ELEM_U8) hipLaunchKernelGGL(resample_kernel<uint8_t>, grid, dim3(kBlock), p.lds_bytes, stream, a);
  else hipLaunchKernelGGL(resample_kernel<uint16_t>, grid, dim3(kBlock), p.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace pqa
